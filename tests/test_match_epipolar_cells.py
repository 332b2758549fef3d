"""CPU checks of cell-ordered epipolar guided matching (fpc_match_frames_guided_epipolar_cells /
fpc_match_bank_guided_epipolar_cells): the header declares the two calls and states the cull, the binding and the built
library have them, and this file's float64 restatement of the ordered algorithm -- fpc_cell_order's order and boxes
(cell_order / run_boxes of tests/test_match_guided_cells.py), the cull of (strip, tile) pairs by testing a tile's pixel box
against the epipolar lines of the strip's rows, and the selection by (distance, original index) keys through the two
permutations -- never drops a tile that holds a candidate of tests/test_match_epipolar.py's epipolar_gate, and gives exactly
the (match, d1, d2) of its epipolar_frames_rule.  The GPU tests (test_gpu_match_epipolar_cells.py) hold the kernel's tile
counts to these functions and its output to the existing device call.

The cull, as include/fpc.h states it (epipolar_cull): with l = F p, g = l0^2 + l1^2 for a query row and the box
[u0, u1] x [v0, v1] of a train tile, e_lo / e_hi the minimum / maximum of l0 u + l1 v + l2 over the four corners, m = 0 if
e_lo <= 0 <= e_hi else min(|e_lo|, |e_hi|), G = max over the corners of l'0^2 + max over the corners of l'1^2 with
l' = F^T (u, v, 1): the row reaches the tile iff m^2 < radius^2 (g + G).

uniform_scene: the scene of the GPU test of the tile counters -- a 2 000-row key of uniform pixels with a depth each, eight
frames seen from planted cameras (sideways baselines with a rotation of at most a degree: the epipolar lines stay close to the
image rows, which is what the 32-px cell order sorts by), +-1 px noise, descriptors without look-alikes.  UNIFORM_RADII are
the radii the GPU test runs; the condition that the restatement visits at most half of the grid there is asserted here."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import FRAME_H, FRAME_W, KMAT, _rotation
from tests.test_match_epipolar import (ALL_PASS, ALL_SCENES, GPU_VGG_SCENE, OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS,
                                       epipolar_frames_rule, epipolar_gate, fundamental_of, planted_f, scene_of, trains_of)
from tests.test_match_guided_cells import STRIP, cell_order, run_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_match_frames_guided_epipolar_cells", "fpc_match_bank_guided_epipolar_cells")
TWINS = ("fpc_match_frames_guided_cells", "fpc_match_bank_guided_cells")
FRAME = (FRAME_H, FRAME_W)
CULL_RADII = (2.0, 4.0, 16.0, ALL_PASS)
UNIFORM_RADII = (2.0, 8.0)
SIDEWAYS_F = (np.array([0, 0, 0, 0, 0, -1, 0, 1, 0]) / np.sqrt(2.0)).astype(np.float32)      # a pure x-shift: F33 = 0


# ---- the ordered algorithm, restated ----------------------------------------------------------------------------------------
def _lines(f9, qxy):
    f = np.asarray(f9, np.float32).astype(np.float64).reshape(3, 3)
    x, y = np.asarray(qxy, np.float64).reshape(-1, 2)[:, 0], np.asarray(qxy, np.float64).reshape(-1, 2)[:, 1]
    return f, f[0, 0] * x + f[0, 1] * y + f[0, 2], f[1, 0] * x + f[1, 1] * y + f[1, 2], f[2, 0] * x + f[2, 1] * y + f[2, 2]


def epipolar_cull(f9, qxy, boxes, radius, scale=1.0):
    """The box rule of include/fpc.h: can a row of `qxy` have a candidate in the box?  -> bool [len(qxy)][len(boxes)].
    float64 from the fp32 F; `scale` widens or narrows the radius for the GPU test's bounds."""
    nq, nb = len(qxy), len(boxes)
    f, l0, l1, l2 = _lines(f9, qxy)
    if not np.isfinite(f).all() or nq == 0 or nb == 0:
        return np.zeros((nq, nb), bool)
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    cu, cv = b[:, [0, 2, 0, 2]], b[:, [1, 1, 3, 3]]                     # the four corners [nb][4]
    e = l0[:, None, None] * cu[None] + l1[:, None, None] * cv[None] + l2[:, None, None]
    e_lo, e_hi = e.min(2), e.max(2)
    m = np.where((e_lo <= 0) & (0 <= e_hi), 0.0, np.minimum(np.abs(e_lo), np.abs(e_hi)))
    m0 = f[0, 0] * cu + f[1, 0] * cv + f[2, 0]                          # l' = F^T (u, v, 1) at the corners
    m1 = f[0, 1] * cu + f[1, 1] * cv + f[2, 1]
    big = (m0 * m0).max(1) + (m1 * m1).max(1)
    r = float(np.float32(radius)) * scale
    return m * m < (r * r) * ((l0 * l0 + l1 * l1)[:, None] + big[None, :])


def scaled_gate(f9, qxy, txy, radius, scale=1.0):
    """tests/test_match_epipolar.py's epipolar_gate, expression for expression, with the radius scaled in float64
    (epipolar_gate rounds its radius to fp32, which would swallow a scale of 1 +- 1e-9)."""
    f, l0, l1, l2 = _lines(f9, qxy)
    if not np.isfinite(f).all():
        return np.zeros((len(qxy), len(txy)), bool)
    u, v = np.asarray(txy, np.float64).reshape(-1, 2)[None, :, 0], np.asarray(txy, np.float64).reshape(-1, 2)[None, :, 1]
    l0, l1, l2 = l0[:, None], l1[:, None], l2[:, None]
    m0 = f[0, 0] * u + f[1, 0] * v + f[2, 0]
    m1 = f[0, 1] * u + f[1, 1] * v + f[2, 1]
    e = l0 * u + l1 * v + l2
    r = float(np.float32(radius)) * scale
    return e * e < (r * r) * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)


def visited_epipolar_tiles(f9, qxy, txy, radius, frame=FRAME, scale=1.0):
    """-> (perm_q, perm_t, keep bool [strips][tiles]): the (strip, tile) pairs that survive the cull."""
    pq, pt = cell_order(qxy, *frame), cell_order(txy, *frame)
    hit = epipolar_cull(f9, np.asarray(qxy)[pq], run_boxes(txy, pt), radius, scale)
    strips = -(-len(pq) // STRIP)
    keep = np.array([hit[s * STRIP:(s + 1) * STRIP].any(0) for s in range(strips)], bool).reshape(strips, -1)
    return pq, pt, keep


def needed_epipolar_tiles(f9, qxy, txy, radius, frame=FRAME, scale=1.0):
    """bool [strips][tiles]: the (strip, tile) pairs that hold a candidate pair of the gate itself."""
    pq, pt = cell_order(qxy, *frame), cell_order(txy, *frame)
    if scale == 1.0:
        cand = epipolar_gate(f9, np.asarray(qxy)[pq], np.asarray(txy)[pt], radius)[0]
    else:
        cand = scaled_gate(f9, np.asarray(qxy)[pq], np.asarray(txy)[pt], radius, scale)
    ns, nt = -(-len(pq) // STRIP), -(-len(pt) // STRIP)
    pad = np.zeros((ns * STRIP, nt * STRIP), bool)
    pad[:len(pq), :len(pt)] = cand
    return pad.reshape(ns, STRIP, nt, STRIP).any(axis=(1, 3))


def ordered_epipolar_pair_rule(q, t, qxy, txy, f9, radius, cross_check=True, max_dist=0.0, ratio=0.0, frame=FRAME):
    """The ordered algorithm for one (query set, train set): rows through the two permutations, only the tiles that survive
    the cull, nearest / second nearest / column minimum by (distance, ORIGINAL index) keys -> (match, d1, d2, keep)."""
    nq, nt = len(q), len(t)
    m = np.full(nq, -1, np.int32)
    d1, d2 = np.full(nq, np.inf), np.full(nq, np.inf)
    if nq == 0 or nt == 0:
        return m, d1, d2, np.zeros((0, 0), bool)
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    # a pair's distance is a function of the pair: tests/test_match_guided.py's expression, on the original rows
    dd = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * q64 @ t64.T
    dd = np.sqrt(np.maximum(dd, 0.0))
    pq, pt, keep = visited_epipolar_tiles(f9, qxy, txy, radius, frame)
    cand, _ = epipolar_gate(f9, np.asarray(qxy)[pq], np.asarray(txy)[pt], radius)
    seen = np.repeat(np.repeat(keep, STRIP, 0), STRIP, 1)[:nq, :nt]           # pairs of a visited tile, ordered domain
    do = dd[np.ix_(pq, pt)]
    do[~(cand & seen)] = np.inf
    order = np.lexsort((np.broadcast_to(pt[None, :], do.shape), do), axis=1)   # per ordered row: (distance, train index)
    rows = np.arange(nq)
    first = order[:, 0]
    e1 = do[rows, first]
    e2 = do[rows, order[:, 1]] if nt >= 2 else np.full(nq, np.inf)
    colmin = np.lexsort((np.broadcast_to(pq[:, None], do.shape), do), axis=0)[0]     # per ordered column: (distance, query index)
    ok = np.isfinite(e1)
    if cross_check:
        ok &= pq[colmin[first]] == pq
    if max_dist > 0:
        ok &= e1 < max_dist
    if ratio > 0:
        ok &= np.isfinite(e2) & (e1 < ratio * e2)
    m[pq[ok]] = pt[first[ok]]                                                   # outputs at the ORIGINAL query row
    d1[pq], d2[pq] = e1, e2
    return m, d1, d2, keep


def ordered_epipolar_frames_rule(desc, xy, counts, trains, fs, radius, cross_check=True, max_dist=0.0, ratio=0.0, frame=FRAME):
    """epipolar_frames_rule's signature -> (match [n][cap], d1, d2, stats int [n][2]: tiles visited, tile grid)."""
    n, cap = len(counts), desc.shape[1]
    m = np.full((n, cap), -1, np.int32)
    d1, d2 = np.full((n, cap), np.inf), np.full((n, cap), np.inf)
    stats = np.zeros((n, 2), np.int64)
    for f in range(n):
        k = counts[f]
        t, txy = trains[f]
        m[f, :k], d1[f, :k], d2[f, :k], keep = ordered_epipolar_pair_rule(desc[f, :k], t, xy[f, :k], txy,
                                                                          np.asarray(fs[f]).reshape(9), radius, cross_check,
                                                                          max_dist, ratio, frame)
        stats[f] = keep.sum(), keep.size
    return m, d1, d2, stats


# ---- the uniform scene of the GPU test of the tile counters ------------------------------------------------------------------
UNIFORM_CAMERAS = 8


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def uniform_scene(cap, nkey=2000, dim=128):
    """-> dict: key [nkey][D], key_xy int32 [nkey][2] uniform over the frame, desc [8][cap][D], xy int32 [8][cap][2], counts
    [8], fs float32 [8][9] (the planted F of every frame, query pixel -> key line).  Key pixel j has a depth in [2, 8]; frame
    f sees its 3-D point from a camera of a sideways baseline (a little of it along y and z) and a rotation of up to a
    degree, +-1 px of noise; points that leave the frame are replaced by uniform unrelated rows.  Built once, shared:
    callers leave it unchanged."""
    rng = np.random.Generator(np.random.PCG64([41, nkey, dim]))
    key = _unit(rng.normal(size=(nkey, dim)))
    key_xy = np.stack([rng.integers(0, FRAME_W, nkey), rng.integers(0, FRAME_H, nkey)], 1).astype(np.int32)
    depth = rng.uniform(2, 8, nkey)
    pts = (np.concatenate([key_xy.astype(np.float64), np.ones((nkey, 1))], 1) @ np.linalg.inv(KMAT).T) * depth[:, None]
    desc, xy = np.zeros((UNIFORM_CAMERAS, cap, dim), np.float32), np.zeros((UNIFORM_CAMERAS, cap, 2), np.int32)
    counts, fs = np.zeros(UNIFORM_CAMERAS, np.int64), np.zeros((UNIFORM_CAMERAS, 9), np.float32)
    ident = (np.eye(3), np.zeros(3))
    for f in range(UNIFORM_CAMERAS):
        sign = 1.0 if f % 2 else -1.0
        cam = (_rotation(rng.normal(size=3), np.deg2rad(0.125 * f)),
               np.array([sign * (0.3 + 0.05 * f), 0.01 * (f - 3), 0.005 * f]))
        p = (pts @ cam[0].T + cam[1]) @ KMAT.T
        p = np.rint(p[:, :2] / p[:, 2:3]) + rng.integers(-1, 2, (nkey, 2))
        ok = np.flatnonzero((p[:, 0] >= 0) & (p[:, 0] < FRAME_W) & (p[:, 1] >= 0) & (p[:, 1] < FRAME_H))
        extra = max(0, nkey - len(ok) - 7 * f)
        d = np.concatenate([_unit(key[ok] + rng.normal(0, 0.02, (len(ok), dim))), _unit(rng.normal(size=(extra, dim)))])
        q = np.concatenate([p[ok], np.stack([rng.integers(0, FRAME_W, extra), rng.integers(0, FRAME_H, extra)], 1)])
        o = rng.permutation(len(d))
        counts[f] = len(d)
        desc[f, :len(d)], xy[f, :len(d)] = d[o], q[o].astype(np.int32)
        fm = fundamental_of(cam, ident)
        fs[f] = (fm / np.sqrt((fm * fm).sum())).astype(np.float32).reshape(9)
    return dict(key=key, key_xy=key_xy, desc=desc, xy=xy, counts=counts, fs=fs)


@functools.lru_cache(maxsize=None)
def uniform_bounds(cap, radius):
    """(need, upper, grid) int [8] of the uniform scene: the tiles that hold a candidate at a radius scaled by 1 - 1e-9, the
    tiles the restated cull visits at a radius scaled by 1 + 1e-9, strips x tiles."""
    s = uniform_scene(cap)
    counts = s["counts"]
    n = len(counts)
    need = np.array([needed_epipolar_tiles(s["fs"][f], s["xy"][f, :counts[f]], s["key_xy"], radius, scale=1 - 1e-9).sum()
                     for f in range(n)])
    upper = np.array([visited_epipolar_tiles(s["fs"][f], s["xy"][f, :counts[f]], s["key_xy"], radius, scale=1 + 1e-9)[2].sum()
                      for f in range(n)])
    grid = np.array([-(-counts[f] // STRIP) * -(-len(s["key"]) // STRIP) for f in range(n)])
    return need, upper, grid


def _cases(spec):
    """(label, scene, trains, fs, frame) of a spec of ALL_SCENES, for both pairings."""
    s = scene_of(spec)
    frame = (240, 320) if spec is GPU_VGG_SCENE else FRAME                  # the D = 256 context of the GPU tests
    for pairing in (PAIR_KEY, PAIR_PREVIOUS):
        yield pairing, s, trains_of(s["desc"], s["xy"], s["counts"], s["key"], s["key_xy"], pairing), planted_f(s, pairing), frame


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "fpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    for name, twin in zip(NAMES, TWINS):                              # argument for argument the cell-ordered calls
        assert getattr(lib, name).argtypes == getattr(lib, twin).argtypes, name
        args = [re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1) for n in (name, twin)]
        assert re.sub(r"\s+", " ", args[0]).replace("F_dev", "H_dev") == re.sub(r"\s+", " ", args[1]), name
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 and lib.fpc_abi_version() == 4
    assert lib.fpc_pack_layout_revision() == 4                      # symbols were only added
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert lib.fpc_match_frames_guided_epipolar_cells(None, 1, PAIR_KEY, p, p, p, p, 4.0, 1, 0.0, 0.0, p, None,
                                                      p) == FPC_E_INVALID
    assert lib.fpc_match_bank_guided_epipolar_cells(None, 1, p, p, 4.0, 1, 0.0, 0.0, p, None, p) == FPC_E_INVALID
    assert (buf == 0).all()
    from fpc_amd.engine import Engine
    for name in ("match_frames_guided_epipolar_cells_async", "match_frames_guided_epipolar_cells",
                 "match_bank_guided_epipolar_cells_async", "match_bank_guided_epipolar_cells"):
        assert callable(getattr(Engine, name)), name
    # the cull is part of the contract: the header states it
    flat = re.sub(r"[\s*]+", " ", hdr)
    for text in ("e_lo, e_hi = the minimum and the maximum of l0 u + l1 v + l2 over the four corners of the box",
                 "m = 0 if e_lo <= 0 <= e_hi, else min(|e_lo|, |e_hi|)",
                 "G = max over the four corners of l'0^2 + max over the four corners of l'1^2, l' = F^T (u, v, 1)",
                 "the row can reach the tile iff m^2 < radius^2 (g + G)",
                 "a strip visits a tile iff one of its rows can reach it"):
        assert text in flat, text


def test_the_scaled_gate_is_the_gate_and_the_cull_follows_the_radius():
    s = scene_of(ALL_SCENES[2])
    fs = planted_f(s, PAIR_KEY)
    for f, cnt in enumerate(s["counts"]):
        for radius in (2.0, RADIUS, 16.0):
            a = scaled_gate(fs[f], s["xy"][f, :cnt], s["key_xy"], radius)
            np.testing.assert_array_equal(a, epipolar_gate(fs[f], s["xy"][f, :cnt], s["key_xy"], radius)[0])
            lo = scaled_gate(fs[f], s["xy"][f, :cnt], s["key_xy"], radius, scale=1 - 1e-9)
            hi = scaled_gate(fs[f], s["xy"][f, :cnt], s["key_xy"], radius, scale=1 + 1e-9)
            assert not (lo & ~a).any() and not (a & ~hi).any()
            boxes = run_boxes(s["key_xy"], cell_order(s["key_xy"]))
            c = [epipolar_cull(fs[f], s["xy"][f, :cnt], boxes, radius, scale) for scale in (1 - 1e-9, 1.0, 1 + 1e-9)]
            assert not (c[0] & ~c[1]).any() and not (c[1] & ~c[2]).any() and c[1].any() and not c[1].all()


def _assert_no_needed_tile_is_dropped(f9, qxy, txy, radius, frame, label):
    _, _, keep = visited_epipolar_tiles(f9, qxy, txy, radius, frame)
    need = needed_epipolar_tiles(f9, qxy, txy, radius, frame)
    assert need.shape == keep.shape and not (need & ~keep).any(), label
    return need.sum(), keep.sum(), keep.size


@pytest.mark.parametrize("k", range(len(ALL_SCENES)))
def test_the_cull_never_drops_a_tile_that_holds_a_candidate(k):
    checked = kept = total = 0
    for pairing, s, trains, fs, frame in _cases(ALL_SCENES[k]):
        for f, cnt in enumerate(s["counts"]):
            for radius in CULL_RADII:
                need, keep, size = _assert_no_needed_tile_is_dropped(fs[f], s["xy"][f, :cnt], trains[f][1], radius, frame,
                                                                     (k, pairing, f, radius))
                assert radius != ALL_PASS or need == keep == size           # every pair a candidate: every tile
                checked, kept, total = checked + need, kept + keep, total + size
    print("scene %d: %d needed, %d visited of %d" % (k, checked, kept, total))
    assert checked > 100 and kept < total


def test_the_cull_on_the_uniform_scene_and_its_condition():
    """The cull drops no needed tile of the uniform scene, and -- the condition the GPU test puts on its input -- the
    restatement visits at most half of the grid there, at a radius widened by 1e-9."""
    cap = 4800
    s = uniform_scene(cap)
    counts = s["counts"]
    assert 1900 <= counts.min() and counts.max() <= cap and len(set(counts.tolist())) > 1
    for radius in UNIFORM_RADII:
        need, upper, grid = uniform_bounds(cap, radius)
        print("radius %g: needed %.3f, upper %.3f of the grid; per frame %s" %
              (radius, need.sum() / grid.sum(), upper.sum() / grid.sum(), np.round(upper / grid, 3).tolist()))
        assert (need <= upper).all() and 2 * upper.sum() <= grid.sum()
        assert (need > 0).all()
        for f in range(len(counts)):
            _assert_no_needed_tile_is_dropped(s["fs"][f], s["xy"][f, :counts[f]], s["key_xy"], radius, FRAME, (f, radius))
    # the planted pairs are candidates at the smaller radius: +-1 px of noise and half a pixel of rounding
    for f in range(len(counts)):
        cand = epipolar_gate(s["fs"][f], s["xy"][f, :counts[f]], s["key_xy"], UNIFORM_RADII[0])[0]
        assert cand.any(1).mean() > 0.9


def test_the_cull_under_edge_matrices():
    s = scene_of(ALL_SCENES[0])
    rng = np.random.Generator(np.random.PCG64(77))
    qxy = np.stack([rng.integers(-40, FRAME_W + 40, 700), rng.integers(-40, FRAME_H + 40, 700)], 1)
    txy = np.stack([rng.integers(-40, FRAME_W + 40, 900), rng.integers(-40, FRAME_H + 40, 900)], 1)
    good = planted_f(s, PAIR_KEY)[1]
    for bad in (np.zeros(9), np.r_[good[:8], np.nan], np.r_[np.inf, good[1:]]):
        for radius in (RADIUS, ALL_PASS):
            assert not visited_epipolar_tiles(bad, qxy, txy, radius)[2].any()       # nine zeros: 0 < 0; non-finite: nowhere
            assert not needed_epipolar_tiles(bad, qxy, txy, radius).any()
    for radius in CULL_RADII[:3]:
        a, b = visited_epipolar_tiles(good, qxy, txy, radius)[2], visited_epipolar_tiles(-good, qxy, txy, radius)[2]
        np.testing.assert_array_equal(a, b)                                        # the cull is even in F, as the gate
        assert a.any() and not a.all()
        _assert_no_needed_tile_is_dropped(-good, qxy, txy, radius, FRAME, ("-F", radius))
        # a pure x-shift (F33 = 0, l' does not depend on the pixel's own row): the band is a band of image rows
        need, keep, size = _assert_no_needed_tile_is_dropped(SIDEWAYS_F, qxy, txy, radius, FRAME, ("sideways", radius))
        assert 0 < need <= keep < size
    # 100 random matrices of rank 2, epipoles inside and outside the frame, pixels outside the frame included
    some = 0
    for _ in range(100):
        u, _, vt = np.linalg.svd(rng.normal(size=(3, 3)) * [[1, 1, 300], [1, 1, 300], [300, 300, 9e4]])
        fm = (u * [1.0, rng.uniform(0.2, 1.0), 0.0]) @ vt
        f9 = fm.astype(np.float32).reshape(9)
        radius = float(np.exp(rng.uniform(np.log(0.5), np.log(300.0))))
        some += _assert_no_needed_tile_is_dropped(f9, qxy, txy, radius, FRAME, "random")[0]
    assert some > 2000


def _assert_same_rule(s, trains, fs, radius, options, frame, label):
    for cross, md, ratio in options:
        want = epipolar_frames_rule(s["desc"], s["xy"], s["counts"], trains, fs, radius, cross, md, ratio)[:3]
        got = ordered_epipolar_frames_rule(s["desc"], s["xy"], s["counts"], trains, fs, radius, cross, md, ratio, frame)
        for a, b, what in zip(got[:3], want, ("match", "d1", "d2")):
            np.testing.assert_array_equal(a, b, err_msg="%s %s %s" % (label, (cross, md, ratio), what))
    return got[3]


@pytest.mark.parametrize("k", range(len(ALL_SCENES)))
def test_ordered_rule_equals_the_epipolar_rule(k):
    """Table for table.  The small scenes under every option set; the two GPU scenes (eight frames of 820 / 430 rows) under
    the two option sets that between them switch everything on."""
    small = len(scene_of(ALL_SCENES[k])["key"]) < 300
    options = OPTIONS if small else ((True, 0.0, 0.0), (False, 0.7, 0.8))
    for pairing, s, trains, fs, frame in _cases(ALL_SCENES[k]):
        for radius in (RADIUS, 16.0) if small else (RADIUS,):
            stats = _assert_same_rule(s, trains, fs, radius, options, frame, (k, pairing, radius))
            assert (stats[:, 0] <= stats[:, 1]).all()
    # no key under FPC_PAIR_PREVIOUS: frame 0 has no train rows
    s = scene_of(ALL_SCENES[k])
    trains = trains_of(s["desc"], s["xy"], s["counts"], None, None, PAIR_PREVIOUS)
    stats = _assert_same_rule(s, trains, planted_f(s, PAIR_PREVIOUS), RADIUS, options[:1], FRAME, (k, "no key"))
    assert (stats[0] == 0).all()


def test_ordered_rule_on_the_uniform_scene_and_under_edge_matrices():
    cap = 4800
    u = uniform_scene(cap)
    n = 2                                                                   # two of its frames: 2 000 x 2 000 pairs each
    sub = dict(desc=u["desc"][:n], xy=u["xy"][:n], counts=u["counts"][:n])
    trains = trains_of(sub["desc"], sub["xy"], sub["counts"], u["key"], u["key_xy"], PAIR_KEY)
    stats = _assert_same_rule(sub, trains, u["fs"][:n], UNIFORM_RADII[0], ((True, 0.0, 0.0),), FRAME, "uniform")
    assert (2 * stats[:, 0] <= stats[:, 1]).all()
    s = scene_of(ALL_SCENES[0])
    fs = planted_f(s, PAIR_KEY).copy()
    fs[0] = 0
    fs[1, 4] = np.nan
    fs[2] = -fs[2]
    fs[3] = SIDEWAYS_F
    trains = trains_of(s["desc"], s["xy"], s["counts"], s["key"], s["key_xy"], PAIR_KEY)
    for radius in (RADIUS, ALL_PASS):
        stats = _assert_same_rule(s, trains, fs, radius, OPTIONS, FRAME, ("edge", radius))
        assert (stats[:2, 0] == 0).all() and (stats[2:, 0] > 0).all()
