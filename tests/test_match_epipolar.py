"""CPU checks of epipolar guided matching (fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar): the header
declares the two calls, the binding and the built library have them, and this file's float64 restatement of the gate of
include/fpc.h -- which the GPU tests (test_gpu_match_epipolar.py) hold the kernel to -- does on planted 3-D scenes what the
call is for: under the planted fundamental matrix it keeps the unguided answer wherever that answer is a candidate, and it
recovers the rows the unguided pass loses to look-alike descriptors off the epipolar line.

Planted scenes (epipolar_scene): the camera model of tests/test_fundamental_ransac.py -- points of the box [-4, 4] x [-3, 3]
x [2, 8] seen by K = KMAT from the key camera (the identity) and from one camera per frame of kind general / sideways /
forward, kept when they project inside every image, every pixel rounded to an integer -- with the descriptors of
tests/test_match_guided.py: nkey unit rows, SHARE of them with a look-alike (the row plus N(0, TWIN_NOISE)), query rows the
key's plus N(0, NOISE), EXTRA unrelated rows per frame, in random order.  A look-alike is a second 3-D point, drawn until in
every image pair the tests use -- (frame f, key) and (frame f, frame f - 1) -- its pixel lies at least FAR = 20 px from the
original's epipolar line and the original's pixel at least FAR from its line, with either of the two as the query row.  Both
point-to-line distances >= 20 px put the Sampson distance at >= 20 / sqrt(2) = 14 px, far outside RADIUS = 3 px.  An original
for which 200 draws find no such point is passed over (its pixel lies near an epipole, through which every line runs).  The
planted F of a camera pair is K^-T [t]x R K^-1 of the relative motion, brought to norm 1 and rounded to fp32; RADIUS = 3 px
holds every rounded planted pair (half a pixel of rounding per coordinate and image: below 1 px in Sampson distance)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import FRAME_H, FRAME_W, KMAT, _rotation, inliers_of, sampson_distance
from tests.test_match_frames import frames_rule
from tests.test_match_guided import (BORDER, EXTRA, NOISE, OPTIONS, PAIR_KEY, PAIR_PREVIOUS, SHARE, TIE, TWIN_NOISE,  # noqa: F401
                                     guided_pair_rule, left_out, planted_truth, recall, trains_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
FAR, RADIUS = 20.0, 3.0
ALL_PASS = 1e6                 # a radius under which the restatement shows every pair of these scenes a candidate
DRAWS = 200                    # look-alike draws per original before it is passed over
NAMES = ("fpc_match_frames_guided_epipolar", "fpc_match_bank_guided_epipolar")
TWINS = ("fpc_match_frames_guided", "fpc_match_bank_guided")


# ---- the rule, restated -----------------------------------------------------------------------------------------------------
def epipolar_gate(f9, qxy, txy, radius):
    """include/fpc.h's gate in float64 from the fp32 F -> (candidate bool [nq][nt], borderline bool [nq][nt])."""
    f = np.asarray(f9, np.float32).astype(np.float64).reshape(3, 3)
    nq, nt = len(qxy), len(txy)
    if not np.isfinite(f).all():
        return np.zeros((nq, nt), bool), np.zeros((nq, nt), bool)
    x, y = np.asarray(qxy, np.float64)[:, 0:1], np.asarray(qxy, np.float64)[:, 1:2]
    u, v = np.asarray(txy, np.float64)[None, :, 0], np.asarray(txy, np.float64)[None, :, 1]
    l0 = f[0, 0] * x + f[0, 1] * y + f[0, 2]                            # l = F p
    l1 = f[1, 0] * x + f[1, 1] * y + f[1, 2]
    l2 = f[2, 0] * x + f[2, 1] * y + f[2, 2]
    m0 = f[0, 0] * u + f[1, 0] * v + f[2, 0]                            # l' = F^T q
    m1 = f[0, 1] * u + f[1, 1] * v + f[2, 1]
    e = l0 * u + l1 * v + l2
    r = float(np.float32(radius))
    lhs, rhs = e * e, (r * r) * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)
    return lhs < rhs, np.abs(lhs - rhs) <= BORDER * rhs


def epipolar_frames_rule(desc, xy, counts, trains, fs, radius, cross_check=True, max_dist=0.0, ratio=0.0):
    """The batched rule, tests/test_match_guided.py's guided_frames_rule with the epipolar gate: desc [n][cap][D], xy
    [n][cap][2], counts [n], trains (trains_of, or the bank's slots per frame), fs [n][9] -> (match [n][cap], d1 [n][cap],
    d2 [n][cap], borderline bool [n][cap]); rows past a frame's count are -1 / +inf."""
    n, cap = len(counts), desc.shape[1]
    m = np.full((n, cap), -1, np.int32)
    d1, d2 = np.full((n, cap), np.inf), np.full((n, cap), np.inf)
    border = np.zeros((n, cap), bool)
    for f in range(n):
        k = counts[f]
        t, txy = trains[f]
        cand, edge = epipolar_gate(np.asarray(fs[f]).reshape(9), xy[f, :k], txy, radius)
        m[f, :k], d1[f, :k], d2[f, :k] = guided_pair_rule(desc[f, :k], t, cand, cross_check, max_dist, ratio)
        border[f, :k] = edge.any(1) if len(t) else False
    return m, d1, d2, border


# ---- planted scenes -----------------------------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _camera(rng, kind):
    """(R, t) of a frame camera, X_cam = R X + t, drawn as tests/test_fundamental_ransac.py's planted_scene draws them (the
    two translations with a random length, so that two frames of one kind differ)."""
    if kind == "general":
        return _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2, 12))), rng.uniform(-0.6, 0.6, 3)
    if kind == "sideways":
        return np.eye(3), np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 0.7), 0, 0])
    assert kind == "forward", kind
    return np.eye(3), np.array([0, 0, -rng.uniform(0.4, 0.8)])


def _pixels(cam, pts):
    p = (pts @ cam[0].T + cam[1]) @ KMAT.T
    return p[:, :2] / p[:, 2:]


def _inside(p):
    return (p[:, 0] >= 0) & (p[:, 0] <= FRAME_W - 1) & (p[:, 1] >= 0) & (p[:, 1] <= FRAME_H - 1)


def fundamental_of(cq, ct):
    """K^-T [t]x R K^-1 of the motion from camera cq (the query image) to camera ct (the train image), float64."""
    r = ct[0] @ cq[0].T
    t = ct[1] - r @ cq[1]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    ki = np.linalg.inv(KMAT)
    return ki.T @ tx @ r @ ki


def _f32(f):
    return (f / np.sqrt((f * f).sum())).astype(np.float32).reshape(9)


def _line_distance(f, p, q):
    """Distance of the pixels q [k][2] (train image) from the epipolar lines F p of the pixels p [k][2] or [2]."""
    l = np.concatenate([np.atleast_2d(p), np.ones((len(np.atleast_2d(p)), 1))], 1) @ f.T
    return np.abs(l[:, 0] * q[:, 0] + l[:, 1] * q[:, 1] + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])


def epipolar_scene(seed, kinds, nkey=200, dim=128, cap=None):
    """-> dict: key [K][D], key_xy int32 [K][2] (K = nkey + SHARE nkey look-alikes), desc [n][cap][D], xy int32 [n][cap][2],
    counts [n], ids [n][cap] (the key row a query row was planted from, -1: unrelated), cams ([0]: the key camera, [1 + f]:
    frame f's)."""
    rng = np.random.Generator(np.random.PCG64([seed, nkey, dim, len(kinds)]))
    ident = (np.eye(3), np.zeros(3))
    cams = [ident] + [_camera(rng, kind) for kind in kinds]
    n = len(kinds)

    def visible(count):
        pts = np.stack([rng.uniform(-4, 4, count), rng.uniform(-3, 3, count), rng.uniform(2, 8, count)], 1)
        pix = [np.rint(_pixels(c, pts)) for c in cams]                  # rint of an inside pixel stays inside
        ok = np.logical_and.reduce([_inside(_pixels(c, pts)) for c in cams])
        return [p[ok] for p in pix]
    pix = visible(40 * nkey)
    assert len(pix[0]) >= nkey, (seed, len(pix[0]))
    pix = [p[:nkey] for p in pix]
    # the image pairs the tests use, (query image, train image): (frame f, key) and (frame f, frame f - 1)
    pairs = [(1 + f, 0) for f in range(n)] + [(1 + f, f) for f in range(1, n)]
    fpair = {ab: fundamental_of(cams[ab[0]], cams[ab[1]]) for ab in pairs}
    ntwin = int(SHARE * nkey)
    twin_of, twin_pix = [], [[] for _ in cams]
    for j in rng.permutation(nkey):
        if len(twin_of) == ntwin:
            break
        cand = visible(8 * DRAWS)
        cand = [c[:DRAWS] for c in cand]
        ok = np.ones(len(cand[0]), bool)
        for (a, b), fm in fpair.items():
            ok &= _line_distance(fm, pix[a][j], cand[b]) >= FAR          # query: the original, train: the look-alike
            ok &= _line_distance(fm.T, cand[b], np.repeat(pix[a][j:j + 1], len(ok), 0)) >= FAR
            ok &= _line_distance(fm, cand[a], np.repeat(pix[b][j:j + 1], len(ok), 0)) >= FAR    # query: the look-alike
            ok &= _line_distance(fm.T, pix[b][j], cand[a]) >= FAR
        hit = np.flatnonzero(ok)
        if len(hit) == 0:
            continue                                                   # near an epipole: passed over
        twin_of.append(j)
        for c in range(len(cams)):
            twin_pix[c].append(cand[c][hit[0]])
    assert len(twin_of) == ntwin, (seed, len(twin_of))
    twin_of = np.array(twin_of)
    pix = [np.concatenate([p, np.array(t)]) for p, t in zip(pix, twin_pix)]
    base = _unit(rng.normal(size=(nkey, dim)))
    twin = _unit(base[twin_of] + rng.normal(0, TWIN_NOISE, (ntwin, dim)))
    key, key_xy = np.concatenate([base, twin]), pix[0].astype(np.int32)
    frames = []
    for f in range(n):
        d = np.concatenate([_unit(key + rng.normal(0, NOISE, key.shape)), _unit(rng.normal(size=(EXTRA, dim)))])
        pxy = np.concatenate([pix[1 + f], np.stack([rng.integers(0, FRAME_W, EXTRA), rng.integers(0, FRAME_H, EXTRA)], 1)])
        ids = np.concatenate([np.arange(len(key)), np.full(EXTRA, -1)])
        o = rng.permutation(len(d))
        frames.append((d[o], pxy[o].astype(np.int32), ids[o]))
    cap = cap or len(key) + EXTRA
    desc, xy = np.zeros((n, cap, dim), np.float32), np.zeros((n, cap, 2), np.int32)
    idt = np.full((n, cap), -1, np.int64)
    for f, (d, p, i) in enumerate(frames):
        assert len(d) <= cap
        desc[f, :len(d)], xy[f, :len(d)], idt[f, :len(d)] = d, p, i
    return dict(key=key, key_xy=key_xy, desc=desc, xy=xy, counts=np.array([len(d) for d, _, _ in frames]), ids=idt, cams=cams,
                twin_of=twin_of)


def planted_f(scene, pairing):
    """The planted F of every frame, query pixel -> train line, as fp32 [n][9] of norm 1."""
    cams = scene["cams"]
    return np.stack([_f32(fundamental_of(cams[1 + f], cams[f] if pairing == PAIR_PREVIOUS and f > 0 else cams[0]))
                     for f in range(len(cams) - 1)])


GENERAL, MIXED = ["general"] * 4, ["general", "sideways", "forward", "general"]
# the GPU tests' scenes (tests/test_gpu_match_epipolar.py): eight cameras; their constants live here so that the premise
# test below covers them
GPU_KINDS = ["general", "sideways", "general", "forward", "general", "general", "sideways", "general"]
GPU_SCENE = dict(seed=11, kinds=GPU_KINDS, nkey=600, cap=1024)
GPU_VGG_SCENE = dict(seed=4, kinds=GPU_KINDS, nkey=300, dim=256, cap=1024)
SCENES = [dict(seed=1, kinds=GENERAL), dict(seed=2, kinds=GENERAL), dict(seed=1, kinds=MIXED), dict(seed=2, kinds=MIXED)]


@functools.lru_cache(maxsize=None)
def _scene(seed, kinds, nkey, dim, cap):
    return epipolar_scene(seed, list(kinds), nkey, dim, cap)


def scene_of(spec):
    """The scene of a spec dict, built once and shared (read-only)."""
    return _scene(spec["seed"], tuple(spec["kinds"]), spec.get("nkey", 200), spec.get("dim", 128), spec.get("cap"))


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
    for name, twin in zip(NAMES, TWINS):                              # argument for argument the homography-gated calls
        assert getattr(lib, name).argtypes == getattr(lib, twin).argtypes, name
        args = [re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1) for n in (name, twin)]
        assert re.sub(r"\s+", " ", args[0]).replace("F_dev", "H_dev") == re.sub(r"\s+", " ", args[1]), name
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 and lib.fpc_abi_version() == 4
    assert lib.fpc_pack_layout_revision() == 4                      # symbols were only added
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert lib.fpc_match_frames_guided_epipolar(None, 1, PAIR_KEY, p, p, p, p, 4.0, 1, 0.0, 0.0, p, None) == FPC_E_INVALID
    assert lib.fpc_match_bank_guided_epipolar(None, 1, p, p, 4.0, 1, 0.0, 0.0, p, None) == FPC_E_INVALID
    assert (buf == 0).all()
    from fpc_amd.engine import Engine
    for name in ("match_frames_guided_epipolar_async", "match_frames_guided_epipolar", "match_bank_guided_epipolar_async",
                 "match_bank_guided_epipolar"):
        assert callable(getattr(Engine, name)), name
    # the gate is part of the contract: the header states it
    for text in ("l  = F p", "l' = F^T q", "e  = q . l = l0 u + l1 v + l2", "e^2 < radius^2 (l0^2 + l1^2 + l'0^2 + l'1^2)",
                 "with radius in the place of reproj_threshold"):
        assert text in hdr, text


def test_gate_is_the_fundamental_calls_inlier_test():
    """The diagonal of the gate is tests/test_fundamental_ransac.py's inliers_of on the same F, pairs and threshold."""
    s = scene_of(SCENES[2])
    rng = np.random.Generator(np.random.PCG64(9))
    for f, cnt in enumerate(s["counts"]):
        fm = planted_f(s, PAIR_KEY)[f]
        rows = np.flatnonzero(s["ids"][f, :cnt] >= 0)
        src = s["xy"][f, rows]
        dst = s["key_xy"][s["ids"][f, rows]].copy()
        swap = rng.permutation(len(rows))[:len(rows) // 3]
        dst[swap] += rng.integers(-6, 7, (len(swap), 2)).astype(np.int32)       # some on, some off the band
        for thr in (0.5, 2.0, RADIUS):
            cand, _ = epipolar_gate(fm, src, dst, thr)
            want = inliers_of(fm.astype(np.float64).reshape(3, 3), src, dst, thr)
            np.testing.assert_array_equal(np.diag(cand), want)
            assert 0 < want.sum() < len(want) or thr == RADIUS
        # the planted F holds the rounded planted pairs well inside the radius
        worst = sampson_distance(fm.astype(np.float64).reshape(3, 3), src.astype(np.float64),
                                 s["key_xy"][s["ids"][f, rows]].astype(np.float64)).max()
        assert worst < 1.5, (f, worst)


ALL_SCENES = SCENES + [GPU_SCENE, GPU_VGG_SCENE]


@pytest.mark.parametrize("k", range(len(ALL_SCENES)))
@pytest.mark.parametrize("pairing", [PAIR_KEY, PAIR_PREVIOUS])
def test_planted_pairs_are_candidates_and_look_alikes_are_not(pairing, k):
    """The premise of the recall tests below and of the GPU comparison, on the restatement alone, for every scene the CPU
    and the GPU tests use."""
    s = scene_of(ALL_SCENES[k])
    fs, truth = planted_f(s, pairing), planted_truth(s, pairing)
    trains = trains_of(s["desc"], s["xy"], s["counts"], s["key"], s["key_xy"], pairing)
    nkey = len(s["key"]) - len(s["twin_of"])
    other = np.full(len(s["key"]), -1)                                   # key row -> its look-alike / its original
    other[s["twin_of"]] = nkey + np.arange(len(s["twin_of"]))
    other[nkey:] = s["twin_of"]
    for f, cnt in enumerate(s["counts"]):
        cand, edge = epipolar_gate(fs[f], s["xy"][f, :cnt], trains[f][1], RADIUS)
        rows = np.flatnonzero(truth[f, :cnt] >= 0)
        assert len(rows) == len(s["key"])
        assert cand[rows, truth[f, rows]].all(), (k, f)                  # every planted pair passes the gate
        assert not edge.any(), (k, f)                                    # no borderline
        # no look-alike is a candidate: the train row planted from the other row of the query row's pair
        ids = s["ids"][f, :cnt]
        tid = np.arange(len(trains[f][1])) if not (pairing == PAIR_PREVIOUS and f > 0) else s["ids"][f - 1, :s["counts"][f - 1]]
        where = {int(v): j for j, v in enumerate(tid) if v >= 0}
        have = np.flatnonzero((ids >= 0) & (other[np.maximum(ids, 0)] >= 0))
        assert len(have) == 2 * len(s["twin_of"])
        assert not cand[have, [where[int(other[ids[r]])] for r in have]].any(), (k, f)
        print("scene %d frame %d: %.1f candidates per row" % (k, f, cand.sum(1).mean()))
        assert cand.sum(1).mean() < 0.05 * len(trains[f][1])            # and the gate is selective
    _, d1, d2, border = epipolar_frames_rule(s["desc"], s["xy"], s["counts"], trains, fs, RADIUS)
    out = left_out(d1, d2, border)
    for f, cnt in enumerate(s["counts"]):
        assert out[f, :cnt].sum() <= 0.01 * cnt, (k, f, out[f, :cnt].sum())


@pytest.mark.parametrize("pairing", [PAIR_KEY, PAIR_PREVIOUS])
def test_guided_keeps_the_unguided_answer_and_raises_recall(pairing):
    total_g = total_u = 0
    for k, spec in enumerate(SCENES):
        s = scene_of(spec)
        desc, xy, counts = s["desc"], s["xy"], s["counts"]
        fs, truth = planted_f(s, pairing), planted_truth(s, pairing)
        trains = trains_of(desc, xy, counts, s["key"], s["key_xy"], pairing)
        ubest, _, _ = frames_rule(desc, counts, s["key"], pairing, False, 0.0, 0.0)          # the nearest row, unchecked
        cands = [epipolar_gate(fs[f], xy[f, :cnt], trains[f][1], RADIUS)[0] for f, cnt in enumerate(counts)]
        for cross, md, ratio in OPTIONS:
            um, ud1, _ = frames_rule(desc, counts, s["key"], pairing, cross, md, ratio)
            gm, gd1, _, _ = epipolar_frames_rule(desc, xy, counts, trains, fs, RADIUS, cross, md, ratio)
            for f, cnt in enumerate(counts):
                cand = cands[f]
                rows = np.flatnonzero(ubest[f, :cnt] >= 0)
                same = rows[cand[rows, ubest[f, rows]]]                 # the unguided winner is a candidate
                assert len(same) > 50
                np.testing.assert_array_equal(gd1[f, same], ud1[f, same])          # ... so it is the guided winner
                if ratio > 0:
                    assert (gm[f, :cnt][cand.sum(1) < 2] == -1).all()   # Lowe's test needs a second CANDIDATE
                    continue
                if not cross:
                    np.testing.assert_array_equal(gm[f, same], um[f, same])
                hit_g, have = recall(gm[f], truth[f])
                hit_u, _ = recall(um[f], truth[f])
                assert hit_g >= hit_u, (k, f, cross, md, ratio)
                total_g, total_u = total_g + hit_g, total_u + hit_u
                if (cross, md) == (True, 0.0):
                    print("scene %d frame %d: recall guided %d, unguided %d of %d" % (k, f, hit_g, hit_u, have))
                    assert hit_g == have                                # every planted pair is recovered
    assert total_g > total_u, (total_g, total_u)


def test_edge_cases_of_the_gate():
    s = scene_of(SCENES[0])
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    n = len(counts)
    for pairing in (PAIR_KEY, PAIR_PREVIOUS):
        trains = trains_of(desc, xy, counts, s["key"], s["key_xy"], pairing)
        fs = planted_f(s, pairing)
        for f, cnt in enumerate(counts):                                # the premise of the identity below
            assert epipolar_gate(fs[f], xy[f, :cnt], trains[f][1], ALL_PASS)[0].all()
        for cross, md, ratio in OPTIONS:
            m, d1, d2, _ = epipolar_frames_rule(desc, xy, counts, trains, fs, ALL_PASS, cross, md, ratio)
            um, ud1, ud2 = frames_rule(desc, counts, s["key"], pairing, cross, md, ratio)
            np.testing.assert_array_equal(m, um)                        # every pair a candidate: fpc_match_frames' rule, exactly
            np.testing.assert_array_equal(d1, ud1)
            np.testing.assert_array_equal(d2, ud2)
        for bad in (np.zeros(9), np.r_[fs[1][:8], np.nan], np.r_[np.inf, fs[1][1:]]):
            g = fs.copy()
            g[1] = bad
            m, d1, _, _ = epipolar_frames_rule(desc, xy, counts, trains, g, RADIUS)
            assert (m[1] == -1).all() and np.isinf(d1[1]).all()         # a failed frame: 0 < 0; a non-finite F: no candidates
            assert (m[[0, 2, 3]] >= 0).any(axis=1).all()
        # the gate is even in F: no sign rule, unlike the homography gate (where -H has w < 0 and passes nowhere)
        g = fs.copy()
        g[1] = -g[1]
        a = epipolar_frames_rule(desc, xy, counts, trains, g, RADIUS)
        b = epipolar_frames_rule(desc, xy, counts, trains, fs, RADIUS)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert (a[0][1] >= 0).sum() > 200
    # no key under FPC_PAIR_PREVIOUS: frame 0 has no train rows
    trains = trains_of(desc, xy, counts, None, None, PAIR_PREVIOUS)
    m, d1, _, _ = epipolar_frames_rule(desc, xy, counts, trains, planted_f(s, PAIR_PREVIOUS), RADIUS)
    assert (m[0] == -1).all() and np.isinf(d1[0]).all() and (m[1:n] >= 0).any()
