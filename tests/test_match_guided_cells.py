"""CPU checks of cell-ordered guided matching (fpc_cell_order / fpc_match_frames_guided_cells / fpc_match_bank_guided_cells):
the header declares the three calls and the binding and the built library have them, and this file's numpy restatement of
the ordered algorithm -- the order by 32-px cell, the boxes of every run of 64 ordered rows, the cull of (strip, tile) pairs
by box, and the selection by (d^2, original index) keys through the two permutations -- gives exactly the (match, d1, d2) of
tests/test_match_guided.py's guided_frames_rule: on the planted scenes there, and on a crafted scene with exact ties, all
points in one cell, and points outside the frame.  The GPU tests (test_gpu_match_guided_cells.py) hold the kernel's order,
its tile counts and its output to these functions and to the existing device call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_homography_ransac import FRAME_H, FRAME_W
from tests.test_match_guided import (OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS, SCENES, gate, guided_frames_rule, planted_h,
                                     scene_of, trains_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
CELL_SHIFT, STRIP = 5, 64
TRAIN_CHOICES = ((PAIR_KEY, True), (PAIR_PREVIOUS, True), (PAIR_PREVIOUS, False))


# ---- the ordered algorithm, restated ----------------------------------------------------------------------------------------
def cells_of(xy, h=FRAME_H, w=FRAME_W):
    """include/fpc.h's cell of every row: int pixels [k][2] -> int [k]."""
    xy = np.asarray(xy, np.int64).reshape(-1, 2)
    cx_n, cy_n = -(-w // 32), -(-h // 32)
    cx = np.clip(xy[:, 0] >> CELL_SHIFT, 0, cx_n - 1)          # (>> on negative integers is arithmetic in numpy)
    cy = np.clip(xy[:, 1] >> CELL_SHIFT, 0, cy_n - 1)
    return cy * cx_n + cx


def cell_order(xy, h=FRAME_H, w=FRAME_W):
    """The stable order by cell: ascending (cell, original index)."""
    cell = cells_of(xy, h, w)
    return np.lexsort((np.arange(len(cell)), cell))


def run_boxes(xy, perm):
    """[umin, vmin, umax, vmax] of every run of 64 ordered rows, over the actual pixels: int64 [ceil(k / 64)][4]."""
    p = np.asarray(xy, np.int64).reshape(-1, 2)[perm]
    runs = [p[i:i + STRIP] for i in range(0, len(p), STRIP)]
    return np.array([[r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()] for r in runs], np.int64).reshape(-1, 4)


def cull(h9, qxy, boxes, radius, scale=1.0):
    """The box rule: can a row of `qxy` have a candidate in the box?  -> bool [len(qxy)][len(boxes)].  float64 from the fp32
    H, the operation forms of the gate (px - w u); `scale` widens or narrows the radius for the GPU test's bounds."""
    h = np.asarray(h9, np.float32).astype(np.float64).reshape(9)
    nq, nb = len(qxy), len(boxes)
    if not np.isfinite(h).all():
        return np.zeros((nq, nb), bool)
    x, y = np.asarray(qxy, np.float64)[:, 0:1], np.asarray(qxy, np.float64)[:, 1:2]
    b = np.asarray(boxes, np.float64)
    u0, v0, u1, v1 = b[None, :, 0], b[None, :, 1], b[None, :, 2], b[None, :, 3]
    w = h[6] * x + h[7] * y + h[8]
    px, py = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5]
    dx = np.maximum(np.maximum(px - w * u1, -(px - w * u0)), 0.0)
    dy = np.maximum(np.maximum(py - w * v1, -(py - w * v0)), 0.0)
    r = float(np.float32(radius)) * scale
    return (w > 0) & (dx * dx + dy * dy < (r * r) * w * w)


def visited_tiles(h9, qxy, txy, radius, frame=(FRAME_H, FRAME_W), scale=1.0):
    """-> (perm_q, perm_t, keep bool [strips][tiles]): the (strip, tile) pairs that survive the cull."""
    pq, pt = cell_order(qxy, *frame), cell_order(txy, *frame)
    hit = cull(h9, np.asarray(qxy)[pq], run_boxes(txy, pt), radius, scale)
    strips = -(-len(pq) // STRIP)
    keep = np.array([hit[s * STRIP:(s + 1) * STRIP].any(0) for s in range(strips)], bool).reshape(strips, -1)
    return pq, pt, keep


def needed_tiles(h9, qxy, txy, radius, frame=(FRAME_H, FRAME_W), scale=1.0):
    """bool [strips][tiles]: the (strip, tile) pairs that hold a candidate pair of the gate itself."""
    pq, pt = cell_order(qxy, *frame), cell_order(txy, *frame)
    cand, _ = gate(h9, np.asarray(qxy)[pq], np.asarray(txy)[pt], radius * scale)
    ns, nt = -(-len(pq) // STRIP), -(-len(pt) // STRIP)
    pad = np.zeros((ns * STRIP, nt * STRIP), bool)
    pad[:len(pq), :len(pt)] = cand
    return pad.reshape(ns, STRIP, nt, STRIP).any(axis=(1, 3))


def ordered_pair_rule(q, t, qxy, txy, h9, radius, cross_check=True, max_dist=0.0, ratio=0.0, frame=(FRAME_H, FRAME_W)):
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
    pq, pt, keep = visited_tiles(h9, qxy, txy, radius, frame)
    cand, _ = gate(h9, np.asarray(qxy)[pq], np.asarray(txy)[pt], radius)
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


def ordered_frames_rule(desc, xy, counts, trains, hs, radius, cross_check=True, max_dist=0.0, ratio=0.0,
                        frame=(FRAME_H, FRAME_W)):
    """guided_frames_rule's signature -> (match [n][cap], d1, d2, stats int [n][2]: tiles visited, tile grid)."""
    n, cap = len(counts), desc.shape[1]
    m = np.full((n, cap), -1, np.int32)
    d1, d2 = np.full((n, cap), np.inf), np.full((n, cap), np.inf)
    stats = np.zeros((n, 2), np.int64)
    for f in range(n):
        k = counts[f]
        t, txy = trains[f]
        m[f, :k], d1[f, :k], d2[f, :k], keep = ordered_pair_rule(desc[f, :k], t, xy[f, :k], txy, np.asarray(hs[f]).reshape(9),
                                                                 radius, cross_check, max_dist, ratio, frame)
        stats[f] = keep.sum(), keep.size
    return m, d1, d2, stats


# ---- a crafted scene: exact ties, one cell, outside the frame -----------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def crafted_scene(dim=128, cap=None, seed=21):
    """planted_scene's dict with "hs" [4][9] (use these for every pairing).  The key: 150 rows in the frame, 24 exact copies
    of key rows one pixel beside their original (nearest and second nearest tie exactly: the index decides), 12 rows
    outside the frame, some with negative coordinates.  Frame 0: the key's rows with noise under the identity, plus 24
    exact copies of query rows at the same pixel (the column minimum ties).  Frame 1: every point in one cell.  Frame 2:
    the key shifted by (-3, -2) under the opposite translation, the rows outside the frame included.  Frame 3: the key's
    own descriptors, unchanged (d^2 clamps to 0 against a row and its copy)."""
    rng = np.random.Generator(np.random.PCG64([seed, dim]))
    base = _unit(rng.normal(size=(150, dim)))
    flat = rng.permutation((FRAME_W - 2) * FRAME_H)[:150]
    base_xy = np.stack([flat % (FRAME_W - 2), flat // (FRAME_W - 2)], 1)
    dup = rng.permutation(150)[:24]
    out_xy = np.array([[-5, -40], [-1, 10], [700, 500], [-100, 200], [640, 479], [300, -1], [-33, -33], [639, 480],
                       [1000, -7], [-64, 240], [320, 511], [672, 100]])
    key = np.concatenate([base, base[dup], _unit(rng.normal(size=(len(out_xy), dim)))])
    key_xy = np.concatenate([base_xy, base_xy[dup] + [1, 0], out_xy]).astype(np.int32)
    o = rng.permutation(len(key))
    key, key_xy = key[o], key_xy[o]
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    frames = []
    d0 = _unit(key + rng.normal(0, 0.02, key.shape))
    again = rng.permutation(len(key))[:24]
    frames.append((np.concatenate([d0, d0[again]]), np.concatenate([key_xy, key_xy[again]])))
    frames.append((_unit(rng.normal(size=(100, dim))), np.stack([rng.integers(64, 96, 100), rng.integers(32, 64, 100)], 1)))
    frames.append((_unit(key + rng.normal(0, 0.02, key.shape)), key_xy - [3, 2]))
    frames.append((key.copy(), key_xy.copy()))
    hs = np.stack([ident, ident, np.array([1, 0, 3, 0, 1, 2, 0, 0, 1], np.float32), ident])
    shuffled = []
    for d, p in frames:
        o = rng.permutation(len(d))
        shuffled.append((d[o], np.asarray(p)[o].astype(np.int32)))
    cap = cap or max(len(d) for d, _ in shuffled)
    desc, xy = np.zeros((4, cap, dim), np.float32), np.zeros((4, cap, 2), np.int32)
    for f, (d, p) in enumerate(shuffled):
        desc[f, :len(d)], xy[f, :len(d)] = d, p
    return dict(key=key, key_xy=key_xy, desc=desc, xy=xy, counts=np.array([len(d) for d, _ in shuffled]), hs=hs)


def scene_cases(s, hs_of):
    """(label, trains, hs) of the three train-set choices."""
    for pcode, with_key in TRAIN_CHOICES:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        yield (pcode, with_key), trains_of(s["desc"], s["xy"], s["counts"], key, key_xy, pcode), hs_of(pcode)


def _assert_same_rule(s, trains, hs, radius, label):
    for cross, md, ratio in OPTIONS:
        want = guided_frames_rule(s["desc"], s["xy"], s["counts"], trains, hs, radius, cross, md, ratio)[:3]
        got = ordered_frames_rule(s["desc"], s["xy"], s["counts"], trains, hs, radius, cross, md, ratio)
        for a, b, what in zip(got[:3], want, ("match", "d1", "d2")):
            np.testing.assert_array_equal(a, b, err_msg="%s %s %s" % (label, (cross, md, ratio), what))
    return got[3]


# ---- tests ------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = open(os.path.join(ROOT, "include", "fpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    names = ("fpc_cell_order", "fpc_match_frames_guided_cells", "fpc_match_bank_guided_cells")
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(names) <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.fpc_cell_order.argtypes == [vp, vp, vp, ci, ci, vp]
    assert lib.fpc_match_frames_guided_cells.argtypes == [vp, ci, ci, vp, vp, vp, vp, cf, ci, cf, cf, vp, vp, vp]
    assert lib.fpc_match_bank_guided_cells.argtypes == [vp, ci, vp, vp, cf, ci, cf, cf, vp, vp, vp]
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 and lib.fpc_abi_version() == 4
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert lib.fpc_cell_order(None, p, p, 1, 8, p) == FPC_E_INVALID
    assert lib.fpc_match_frames_guided_cells(None, 1, PAIR_KEY, p, p, p, p, 4.0, 1, 0.0, 0.0, p, None, p) == FPC_E_INVALID
    assert lib.fpc_match_bank_guided_cells(None, 1, p, p, 4.0, 1, 0.0, 0.0, p, None, p) == FPC_E_INVALID
    assert (buf == 0).all()
    from fpc_amd.engine import Engine
    for name in ("cell_order_async", "match_frames_guided_cells_async", "match_frames_guided_cells",
                 "match_bank_guided_cells_async", "match_bank_guided_cells"):
        assert callable(getattr(Engine, name)), name
    # the order is part of the contract: the header states it
    for text in ("CX = ceil(W / 32)", "cx = clamp(x >> 5, 0, CX - 1)", "ascending (cell, original index)", "BIT-IDENTICAL"):
        assert text in hdr, text


def test_the_order_and_the_boxes():
    xy = np.array([[0, 0], [31, 31], [32, 0], [-1, -1], [639, 479], [640, 480], [5000, -5000], [0, 32], [33, 1], [-70, 470]])
    assert cells_of(xy).tolist() == [0, 0, 1, 0, 14 * 20 + 19, 14 * 20 + 19, 19, 20, 1, 14 * 20]
    perm = cell_order(xy)
    assert perm.tolist() == [0, 1, 3, 2, 8, 6, 7, 9, 4, 5]                      # stable inside a cell
    np.testing.assert_array_equal(run_boxes(xy, perm), [[-70, -5000, 5000, 480]])
    rng = np.random.Generator(np.random.PCG64(3))
    xy = np.stack([rng.integers(-50, 700, 1000), rng.integers(-50, 530, 1000)], 1)
    perm = cell_order(xy)
    key = cells_of(xy)[perm] * 1000 + perm
    assert (np.diff(key) > 0).all() and sorted(perm.tolist()) == list(range(1000))
    boxes = run_boxes(xy, perm)
    assert boxes.shape == (16, 4)
    last = xy[perm[960:]]
    assert boxes[15].tolist() == [last[:, 0].min(), last[:, 1].min(), last[:, 0].max(), last[:, 1].max()]


@pytest.mark.parametrize("k", range(len(SCENES)))
def test_ordered_rule_equals_the_guided_rule_on_the_planted_scenes(k):
    s = scene_of(k)
    for label, trains, hs in scene_cases(s, lambda pcode: planted_h(s, pcode)):
        stats = _assert_same_rule(s, trains, hs, RADIUS, (k, label))
        assert (stats[:, 0] <= stats[:, 1]).all()


def test_ordered_rule_equals_the_guided_rule_on_the_crafted_scene():
    s = crafted_scene()
    counts = s["counts"]
    assert (cells_of(s["xy"][1, :counts[1]]) == 1 * 20 + 2).all()               # frame 1: one cell
    assert (s["key_xy"].min(0) < 0).all() and s["key_xy"][:, 0].max() >= FRAME_W and s["key_xy"][:, 1].max() >= FRAME_H
    for radius in (4.0, 16.0, 1e4):
        for label, trains, hs in scene_cases(s, lambda pcode: s["hs"]):
            _assert_same_rule(s, trains, hs, radius, (radius, label))
    # the ties are there, and the index decides them: frame 3 against the key, nearest and second nearest both at 0
    trains = trains_of(s["desc"], s["xy"], counts, s["key"], s["key_xy"], PAIR_KEY)
    m, d1, d2, _ = ordered_frames_rule(s["desc"], s["xy"], counts, trains, s["hs"], 4.0, False)
    tied = np.flatnonzero((d1[3, :counts[3]] == d2[3, :counts[3]]) & np.isfinite(d1[3, :counts[3]]))
    assert len(tied) >= 20                                                       # rows whose float64 distances to a key row and to its copy are equal
    for i in tied:
        twins = np.flatnonzero((s["key"] == s["desc"][3, i]).all(1))
        assert len(twins) == 2 and m[3, i] == twins.min()
    mc, _, _, _ = ordered_frames_rule(s["desc"], s["xy"], counts, trains, s["hs"], 4.0, True)
    lost = np.flatnonzero((m[0, :counts[0]] >= 0) & (mc[0, :counts[0]] < 0))
    assert len(lost) >= 20                                                       # copied query rows: the lower index wins


def test_the_cull_never_drops_a_tile_that_holds_a_candidate():
    rng = np.random.Generator(np.random.PCG64(77))
    scenes = [scene_of(k) for k in range(len(SCENES))] + [crafted_scene()]
    checked = 0
    for k, s in enumerate(scenes):
        planted = k < len(SCENES)
        for label, trains, hs in scene_cases(s, (lambda pcode: planted_h(s, pcode)) if planted else (lambda pcode: s["hs"])):
            for f, cnt in enumerate(s["counts"]):
                if len(trains[f][1]) == 0:
                    continue
                for radius in (4.0, RADIUS, 16.0):
                    _, _, keep = visited_tiles(hs[f], s["xy"][f, :cnt], trains[f][1], radius)
                    need = needed_tiles(hs[f], s["xy"][f, :cnt], trains[f][1], radius)
                    assert need.shape == keep.shape and not (need & ~keep).any(), (k, label, f, radius)
                    checked += need.sum()
    assert checked > 1000
    # 200 random H / radius draws: perspective terms large enough that w changes sign inside the frame for some
    qxy = np.stack([rng.integers(-40, FRAME_W + 40, 700), rng.integers(-40, FRAME_H + 40, 700)], 1)
    txy = np.stack([rng.integers(-40, FRAME_W + 40, 900), rng.integers(-40, FRAME_H + 40, 900)], 1)
    some = negative = 0
    for _ in range(200):
        h = np.eye(3) + rng.normal(0, 0.05, (3, 3)) * [[1, 1, 300], [1, 1, 300], [2e-2, 2e-2, 0]]
        h9 = h.astype(np.float32).reshape(9)
        radius = float(np.exp(rng.uniform(np.log(0.5), np.log(300.0))))
        _, _, keep = visited_tiles(h9, qxy, txy, radius)
        need = needed_tiles(h9, qxy, txy, radius)
        assert not (need & ~keep).any()
        some += need.sum()
        w = h9[6] * qxy[:, 0].astype(np.float64) + h9[7] * qxy[:, 1] + h9[8]
        negative += (w <= 0).any()
    assert some > 2000 and negative >= 5
    for bad in (np.zeros(9), np.r_[np.ones(8), np.nan], -np.eye(3).reshape(9)):
        assert not visited_tiles(bad, qxy, txy, 50.0)[2].any()
