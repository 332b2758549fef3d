"""CPU checks of pose-guided matching (fpc_match_frames_guided_pose / fpc_match_bank_guided_pose): the header declares the two
calls, the binding and the built library have them, and this file's float64 restatement of the gate of include/fpc.h --
which the GPU tests (test_gpu_match_pose.py) hold the kernel to -- does on planted 3-D scenes what the call is for: under the
planted pose it recovers the rows the unguided pass loses to look-alike descriptors, INCLUDING those the epipolar gate cannot
recover because the look-alike lies on the same viewing ray of the key camera and so inside the epipolar band.

Planted scenes (pose_scene): the cameras, box and descriptor recipe of tests/test_match_epipolar.py -- points of the box
[-4, 4] x [-3, 3] x [2, 8] seen by K = KMAT from the key camera (the identity) and from one camera per frame, kept when they
project inside every 640 x 480 image, every pixel rounded to an integer; nkey unit rows, SHARE of them with a look-alike (the
row plus N(0, TWIN_NOISE)), query rows the key's plus N(0, NOISE), EXTRA unrelated rows per frame, in random order -- with
the 3-D points kept: the key camera is the identity, so the points are the key's landmarks and cams[1 + f] is frame f's
planted (R, t).  A look-alike is a second landmark on the original's own viewing ray from the key camera, at another depth
of [DEPTH_LO, DEPTH_HI], drawn until its projection lies inside every frame and at least FAR = 20 px from the original's in
every frame.  An original for which DRAWS draws find no such point is passed over (near an epipole of a forward camera the
whole ray projects to almost one pixel).  Both landmarks share the key pixel, hence the epipolar line in every frame: the
epipolar gate holds both.  INVALID of the key's landmarks are marked invalid, three more get non-finite coordinates, and
BEHIND further key rows carry landmarks behind every camera (negative depth), so that those rules have subjects; the rows
behind the cameras stand at the END of the key, so that key[:K] is the scene without them.  RADIUS = 3 px holds every
rounded planted pair (half a pixel of rounding per coordinate: 0.71 px)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import FRAME_H, FRAME_W, KMAT
from tests.test_match_epipolar import (EXTRA, NOISE, SHARE, TWIN_NOISE, _camera, _inside, _pixels, _unit,
                                       epipolar_frames_rule, epipolar_gate, fundamental_of)
from tests.test_match_epipolar import _f32 as _unit_f
from tests.test_match_frames import frames_rule
from tests.test_match_guided import BORDER, OPTIONS, PAIR_KEY, TIE, guided_pair_rule, left_out, recall  # noqa: F401
from tests.test_pnp_ransac import KVEC, inliers_of
from tests.test_pnp_ransac import planted_scene as pnp_planted_scene
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
FAR, RADIUS = 20.0, 3.0
DRAWS = 200                    # look-alike draws per original before it is passed over
DEPTH_LO, DEPTH_HI = 1.5, 12.0  # a look-alike's depth along the original's ray
INVALID, BEHIND = 0.1, 12      # share of the landmarks marked invalid; key rows whose landmark is behind every camera
NAMES = ("fpc_match_frames_guided_pose", "fpc_match_bank_guided_pose")
assert tuple(KMAT[[0, 1, 0, 1], [0, 1, 2, 2]]) == KVEC


# ---- the rule, restated -----------------------------------------------------------------------------------------------------
def pose_gate(r9, t3, kvec, qxy, xyz, valid, radius):
    """include/fpc.h's gate in float64 from the fp32 R and t -> (candidate bool [nq][nt], borderline bool [nq][nt]).  xyz
    float32 [nt][3]; valid bool [nt] or None: a landmark counts when its flag is set and its coordinates are finite."""
    r = np.asarray(r9, np.float32).astype(np.float64).reshape(9)
    t = np.asarray(t3, np.float32).astype(np.float64).reshape(3)
    nq, nt = len(qxy), len(xyz)
    if not (np.isfinite(r).all() and np.isfinite(t).all()) or nt == 0:
        return np.zeros((nq, nt), bool), np.zeros((nq, nt), bool)
    fx, fy, cx, cy = (float(np.float32(v)) for v in kvec)
    p = np.asarray(xyz, np.float32)
    ok = np.isfinite(p).all(1) & (np.ones(nt, bool) if valid is None else np.asarray(valid).astype(bool)[:nt])
    p = np.where(ok[:, None], p, 0).astype(np.float64)
    X, Y, Z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    a = r[0] * X + r[1] * Y + r[2] * Z + t[0]
    b = r[3] * X + r[4] * Y + r[5] * Z + t[1]
    c = r[6] * X + r[7] * Y + r[8] * Z + t[2]
    x, y = np.asarray(qxy, np.float64)[:, 0:1], np.asarray(qxy, np.float64)[:, 1:2]
    ex = fx * a - (x - cx) * c
    ey = fy * b - (y - cy) * c
    rad = float(np.float32(radius))
    lhs, rhs = ex * ex + ey * ey, (rad * rad) * c * c
    live = ok[None, :] & (c > 0)
    return live & (lhs < rhs), live & (np.abs(lhs - rhs) <= BORDER * rhs)


def pose_frames_rule(desc, xy, counts, trains, rs, ts, kvec, radius, cross_check=True, max_dist=0.0, ratio=0.0):
    """The batched rule, tests/test_match_guided.py's guided_pair_rule over the pose gate: desc [n][cap][D], xy [n][cap][2],
    counts [n], trains: per frame (desc [k][D], xyz [k][3], valid [k] or None), rs [n][9], ts [n][3] -> (match [n][cap], d1
    [n][cap], d2 [n][cap], borderline bool [n][cap]); rows past a frame's count are -1 / +inf."""
    n, cap = len(counts), desc.shape[1]
    m = np.full((n, cap), -1, np.int32)
    d1, d2 = np.full((n, cap), np.inf), np.full((n, cap), np.inf)
    border = np.zeros((n, cap), bool)
    for f in range(n):
        k = counts[f]
        t, xyz, valid = trains[f]
        cand, edge = pose_gate(np.asarray(rs[f]).reshape(9), ts[f], kvec, xy[f, :k], xyz, valid, radius)
        m[f, :k], d1[f, :k], d2[f, :k] = guided_pair_rule(desc[f, :k], t, cand, cross_check, max_dist, ratio)
        border[f, :k] = edge.any(1) if len(t) else False
    return m, d1, d2, border


def all_pass_radius(rs, ts, kvec, xy, counts, trains):
    """A radius under which the restatement shows every pair of every frame a candidate -- it depends on the pose: the
    largest reprojection distance of any (row, landmark) pair, doubled -- or None where a landmark is invalid or has
    c <= 0: no radius admits those."""
    fx, fy, cx, cy = kvec
    worst = 0.0
    for f, k in enumerate(counts):
        _, xyz, valid = trains[f]
        if len(xyz) == 0 or k == 0:
            continue
        if valid is not None and not np.asarray(valid).all() or not np.isfinite(xyz).all():
            return None
        r = np.asarray(rs[f], np.float32).astype(np.float64).reshape(3, 3)
        xc = np.asarray(xyz, np.float64) @ r.T + np.asarray(ts[f], np.float32).astype(np.float64)
        if not (xc[:, 2] > 0).all():
            return None
        u, v = fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy
        worst = max(worst, np.hypot(xy[f, :k, 0:1] - u[None], xy[f, :k, 1:2] - v[None]).max())
    return float(np.float32(2.0 * worst + 1.0))


# ---- planted scenes -----------------------------------------------------------------------------------------------------------
def pose_scene(seed, kinds, nkey=200, dim=128, cap=None):
    """-> dict: key [K + BEHIND][D], key_xy int32 [.][2], key_xyz float32 [.][3], key_valid bool [.] (K = nkey + SHARE nkey
    look-alikes; the last BEHIND rows: landmarks behind every camera), desc [n][cap][D], xy int32 [n][cap][2], counts [n],
    ids [n][cap] (the key row a query row was planted from, -1: unrelated), cams ([0]: the key camera, [1 + f]: frame f's),
    twin_of (the original of look-alike K - ntwin + k)."""
    rng = np.random.Generator(np.random.PCG64([seed, nkey, dim, len(kinds), 7]))
    ident = (np.eye(3), np.zeros(3))
    cams = [ident] + [_camera(rng, kind) for kind in kinds]
    n = len(kinds)

    def seen(pts):
        return np.logical_and.reduce([_inside(_pixels(c, pts)) & ((pts @ c[0].T + c[1])[:, 2] > 0.2) for c in cams])
    pts = np.stack([rng.uniform(-4, 4, 40 * nkey), rng.uniform(-3, 3, 40 * nkey), rng.uniform(2, 8, 40 * nkey)], 1)
    pts = pts[seen(pts)][:nkey].astype(np.float32).astype(np.float64)      # (landmarks are fp32: project what is stored)
    assert len(pts) == nkey, (seed, len(pts))
    ntwin = int(SHARE * nkey)
    twin_of, twin_pts = [], []
    for j in rng.permutation(nkey):
        if len(twin_of) == ntwin:
            break
        cand = (pts[j] / pts[j, 2])[None] * rng.uniform(DEPTH_LO, DEPTH_HI, DRAWS)[:, None]     # the original's own ray
        cand = cand.astype(np.float32).astype(np.float64)
        ok = seen(cand)
        for c in cams[1:]:
            ok &= np.hypot(*(_pixels(c, cand) - _pixels(c, pts[j:j + 1])).T) >= FAR
        hit = np.flatnonzero(ok)
        if len(hit) == 0:
            continue                                                   # the ray hardly moves in some frame: passed over
        twin_of.append(j)
        twin_pts.append(cand[hit[0]])
    assert len(twin_of) == ntwin, (seed, len(twin_of))
    twin_of = np.array(twin_of)
    pts = np.concatenate([pts, np.array(twin_pts)])
    pix = [np.rint(_pixels(c, pts)) for c in cams]
    base = _unit(rng.normal(size=(nkey, dim)))
    twin = _unit(base[twin_of] + rng.normal(0, TWIN_NOISE, (ntwin, dim)))
    key = np.concatenate([base, twin])
    K = len(key)
    frames = []
    for f in range(n):
        d = np.concatenate([_unit(key + rng.normal(0, NOISE, key.shape)), _unit(rng.normal(size=(EXTRA, dim)))])
        pxy = np.concatenate([pix[1 + f], np.stack([rng.integers(0, FRAME_W, EXTRA), rng.integers(0, FRAME_H, EXTRA)], 1)])
        ids = np.concatenate([np.arange(K), np.full(EXTRA, -1)])
        o = rng.permutation(len(d))
        frames.append((d[o], pxy[o].astype(np.int32), ids[o]))
    # the landmarks' flags; rows with landmarks behind every camera at the end of the key
    valid = rng.uniform(size=K) >= INVALID
    xyz = pts.astype(np.float32)
    nonfinite = rng.permutation(K)[:3]
    xyz[nonfinite[0], 0], xyz[nonfinite[1], 1], xyz[nonfinite[2], 2] = np.nan, np.inf, -np.inf
    valid[nonfinite[:2]] = True                                        # not finite: invalid whatever the flag says
    back = np.stack([rng.uniform(-4, 4, BEHIND), rng.uniform(-3, 3, BEHIND), -rng.uniform(2, 8, BEHIND)], 1)
    for c in cams:
        assert ((back @ c[0].T + c[1])[:, 2] < 0).all()
    key = np.concatenate([key, _unit(rng.normal(size=(BEHIND, dim)))])
    key_xy = np.concatenate([pix[0], np.stack([rng.integers(0, FRAME_W, BEHIND), rng.integers(0, FRAME_H, BEHIND)], 1)])
    xyz = np.concatenate([xyz, back.astype(np.float32)])
    valid = np.concatenate([valid, np.ones(BEHIND, bool)])
    cap = cap or K + EXTRA
    desc, xy = np.zeros((n, cap, dim), np.float32), np.zeros((n, cap, 2), np.int32)
    idt = np.full((n, cap), -1, np.int64)
    for f, (d, p, i) in enumerate(frames):
        assert len(d) <= cap
        desc[f, :len(d)], xy[f, :len(d)], idt[f, :len(d)] = d, p, i
    return dict(key=key, key_xy=key_xy.astype(np.int32), key_xyz=xyz, key_valid=valid, clean_xyz=pts.astype(np.float32),
                desc=desc, xy=xy, counts=np.array([len(d) for d, _, _ in frames]), ids=idt, cams=cams, twin_of=twin_of, K=K)


def planted_pose(scene):
    """The planted (R [n][9], t [n][3]) of every frame as fp32, X_cam = R X + t."""
    cams = scene["cams"][1:]
    return (np.stack([c[0].reshape(9) for c in cams]).astype(np.float32), np.stack([c[1] for c in cams]).astype(np.float32))


def planted_f(scene):
    """The planted F of every frame against the key, query pixel -> train line, as fp32 [n][9] of norm 1."""
    cams = scene["cams"]
    return np.stack([_unit_f(fundamental_of(cams[1 + f], cams[0])) for f in range(len(cams) - 1)])


def key_train(scene, rows=None, flags=True):
    """The key as every frame's train set: its first `rows` rows (None: all), with or without the flags."""
    k = len(scene["key"]) if rows is None else rows
    return (scene["key"][:k], scene["key_xyz"][:k], scene["key_valid"][:k] if flags else None)


def landmark_ok(scene):
    return scene["key_valid"] & np.isfinite(scene["key_xyz"]).all(1)


GENERAL, MIXED = ["general"] * 4, ["general", "sideways", "forward", "general"]
# the GPU tests' scenes (tests/test_gpu_match_pose.py): eight cameras; their constants live here so that the premise test
# below covers them
GPU_KINDS = ["general", "sideways", "general", "forward", "general", "general", "sideways", "general"]
GPU_SCENE = dict(seed=11, kinds=GPU_KINDS, nkey=600, cap=1024)
GPU_VGG_SCENE = dict(seed=4, kinds=GPU_KINDS, nkey=300, dim=256, cap=1024)
GPU_SLOTS = {2: None, 0: "other", 3: 400}         # bank slot -> the key's first rows (None: all), or 500 unrelated rows
GPU_SLOT_OF = [2, 3, 2, -1, 0, 2, 4, 1]           # frame -> slot; -1, 4: outside the bank; 1: an empty slot
SCENES = [dict(seed=1, kinds=GENERAL), dict(seed=2, kinds=GENERAL), dict(seed=1, kinds=MIXED), dict(seed=2, kinds=MIXED)]


@functools.lru_cache(maxsize=None)
def _scene(seed, kinds, nkey, dim, cap):
    return pose_scene(seed, list(kinds), nkey, dim, cap)


def scene_of(spec):
    """The scene of a spec dict, built once and shared (read-only)."""
    return _scene(spec["seed"], tuple(spec["kinds"]), spec.get("nkey", 200), spec.get("dim", 128), spec.get("cap"))


@functools.lru_cache(maxsize=None)
def other_slot(dim=128):
    """500 unrelated rows with landmarks in front of the cameras, a tenth invalid: the bank's slot of another place."""
    rng = np.random.Generator(np.random.PCG64(5))
    d = _unit(rng.normal(size=(500, dim)))
    xyz = np.stack([rng.uniform(-4, 4, 500), rng.uniform(-3, 3, 500), rng.uniform(2, 8, 500)], 1).astype(np.float32)
    pxy = np.stack([rng.integers(0, FRAME_W, 500), rng.integers(0, FRAME_H, 500)], 1).astype(np.int32)
    return d, pxy, xyz, rng.uniform(size=500) >= INVALID


def gpu_bank_trains(scene):
    """slot -> (desc, xy, xyz, valid) as the GPU test stores them, and the per-frame trains of GPU_SLOT_OF."""
    slots = {}
    for sl, what in GPU_SLOTS.items():
        if what == "other":
            slots[sl] = other_slot(scene["key"].shape[1])
        else:
            k = len(scene["key"]) if what is None else what
            slots[sl] = (scene["key"][:k], scene["key_xy"][:k], scene["key_xyz"][:k], scene["key_valid"][:k])
    empty = (scene["key"][:0], scene["key_xyz"][:0], None)
    return slots, [(slots[v][0], slots[v][2], slots[v][3]) if v in slots else empty for v in GPU_SLOT_OF]


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
    args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1)) for n in NAMES]
    tail = ("const float* R_dev, const float* t_dev, float fx, float fy, float cx, float cy, float radius, int cross_check, "
            "float max_dist, float ratio, int32_t* match_dev, float* dist_dev")
    assert args[0] == ("fpc_ctx* ctx, int n, const float* key_dev, const int32_t* nkey_dev, const float* key_xyz_dev, "
                       "const uint8_t* key_valid_dev, " + tail)
    assert args[1] == "fpc_ctx* ctx, int n, const int32_t* slot_dev, " + tail
    assert len(lib.fpc_match_frames_guided_pose.argtypes) == 18 and len(lib.fpc_match_bank_guided_pose.argtypes) == 15
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 and lib.fpc_abi_version() == 4
    assert lib.fpc_pack_layout_revision() == 4                      # symbols were only added
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    assert lib.fpc_match_frames_guided_pose(None, 1, p, p, p, p, p, p, 500.0, 500.0, 320.0, 240.0, 3.0, 1, 0.0, 0.0, p,
                                            None) == FPC_E_INVALID
    assert lib.fpc_match_bank_guided_pose(None, 1, p, p, p, 500.0, 500.0, 320.0, 240.0, 3.0, 1, 0.0, 0.0, p, None) == FPC_E_INVALID
    assert (buf == 0).all()
    from fpc_amd.engine import Engine
    for name in ("match_frames_guided_pose_async", "match_frames_guided_pose", "match_bank_guided_pose_async",
                 "match_bank_guided_pose"):
        assert callable(getattr(Engine, name)), name
    # the gate is part of the contract: the header states it
    for text in ("a = R0 X + R1 Y + R2 Z + t0,   b = R3 X + R4 Y + R5 Z + t1,   c = R6 X + R7 Y + R8 Z + t2",
                 "ex = fx a - (x - cx) c,        ey = fy b - (y - cy) c", "c > 0 and ex^2 + ey^2 < radius^2 c^2",
                 "with radius in the place of reproj_threshold", "it is not orthonormalised"):
        assert text in hdr, text


def test_gate_is_the_pnp_calls_inlier_test():
    """The diagonal of the gate is tests/test_pnp_ransac.py's inliers_of on the same pose, pairs and threshold, pair for
    pair, on that file's planted scenes (outliers included)."""
    seen = 0
    for i, rho, m in ((0, 0.3, 300), (1, 0.3, 300), (0, 0.6, 40), (1, 0.0, 1100)):
        xy, xyz, planted, r, t = pnp_planted_scene(i, rho, m)
        r32, t32 = r.astype(np.float32), t.astype(np.float32)
        for thr in (0.25, 0.5, 3.0):
            cand, _ = pose_gate(r32.reshape(9), t32, KVEC, xy, xyz, None, thr)
            want = inliers_of(r32.astype(np.float64), t32.astype(np.float64), xy, xyz, KVEC, thr)
            np.testing.assert_array_equal(np.diag(cand), want)
            assert 0 < want.sum() < len(want) or (rho == 0.0 and thr == 3.0)
            seen += want.sum()
        assert inliers_of(r32.astype(np.float64), t32.astype(np.float64), xy, xyz, KVEC, 3.0)[planted].all()
        # an invalid flag, a landmark behind the camera and a non-finite pose pass nowhere
        flags = np.ones(m, bool)
        flags[::3] = False
        assert not np.diag(pose_gate(r32.reshape(9), t32, KVEC, xy, xyz, flags, 3.0)[0])[::3].any()
        mirrored = -xyz.astype(np.float64) - 2 * (t @ r)                  # R X' + t = -(R X + t): behind the camera
        assert not pose_gate(r32.reshape(9), t32, KVEC, xy, mirrored, None, 1e9)[0].any()
        assert not pose_gate(np.r_[r32.reshape(9)[:8], np.nan], t32, KVEC, xy, xyz, None, 3.0)[0].any()
        assert not pose_gate(np.zeros(9), np.zeros(3), KVEC, xy, xyz, None, 1e9)[0].any()        # a failed frame: c = 0
    assert seen > 1000


ALL_SCENES = SCENES + [GPU_SCENE, GPU_VGG_SCENE]


@pytest.mark.parametrize("k", range(len(ALL_SCENES)))
def test_planted_pairs_are_candidates_and_look_alikes_are_not(k):
    """The premise of the recall test below and of the GPU comparison, on the restatement alone, for every scene the CPU and
    the GPU tests use: the planted pair with a valid landmark is a candidate, its look-alike is not, invalid landmarks and
    landmarks behind the cameras are nobody's candidates, and the rows a device comparison may leave out (a near-tie within
    TIE or a borderline pair, left_out) stay within _compare's cap of 1 % of a frame's rows -- for the key as the train set
    and for the GPU test's bank slots."""
    s = scene_of(ALL_SCENES[k])
    rs, ts = planted_pose(s)
    ok, K = landmark_ok(s), s["K"]
    nkey = K - len(s["twin_of"])
    other = np.full(len(s["key"]), -1)                                   # key row -> its look-alike / its original
    other[s["twin_of"]] = nkey + np.arange(len(s["twin_of"]))
    other[nkey:K] = s["twin_of"]
    assert (~ok).sum() > 0.05 * K and ok[K:].all()
    for f, cnt in enumerate(s["counts"]):
        cand, edge = pose_gate(rs[f], ts[f], KVEC, s["xy"][f, :cnt], s["key_xyz"], s["key_valid"], RADIUS)
        ids = s["ids"][f, :cnt]
        rows = np.flatnonzero(ids >= 0)
        assert len(rows) == K
        have = rows[ok[ids[rows]]]
        assert cand[have, ids[have]].all(), (k, f)                       # every planted pair with a valid landmark passes
        assert not edge.any(), (k, f)                                    # no borderline
        assert not cand[:, ~ok].any() and not cand[:, K:].any()          # invalid / behind the camera: nobody's candidate
        twinned = rows[other[ids[rows]] >= 0]
        assert len(twinned) == 2 * len(s["twin_of"])
        assert not cand[twinned, other[ids[twinned]]].any(), (k, f)      # no look-alike is a candidate
        # ... while the epipolar gate under the planted F holds both
        ecand, _ = epipolar_gate(planted_f(s)[f], s["xy"][f, :cnt], s["key_xy"], RADIUS)
        assert ecand[twinned, other[ids[twinned]]].all() and ecand[rows, ids[rows]].all(), (k, f)
        print("scene %d frame %d: %.2f candidates per row (epipolar: %.1f)" % (k, f, cand.sum(1).mean(), ecand.sum(1).mean()))
        assert cand.sum(1).mean() < 0.01 * K                             # and the gate is selective
    trains = [key_train(s)] * len(s["counts"])
    sets = [("key", trains, rs, ts)]
    if "cap" in ALL_SCENES[k] and s["key"].shape[1] == 128:
        sets.append(("bank", gpu_bank_trains(s)[1], rs, ts))
    for tag, tr, r_, t_ in sets:
        _, d1, d2, border = pose_frames_rule(s["desc"], s["xy"], s["counts"], tr, r_, t_, KVEC, RADIUS)
        out = left_out(d1, d2, border)
        for f, cnt in enumerate(s["counts"]):
            assert out[f, :cnt].sum() <= 0.01 * cnt, (k, tag, f, out[f, :cnt].sum())


@pytest.mark.parametrize("k", range(len(ALL_SCENES)))
def test_all_pass_premise_holds_at_the_all_pass_radius(k):
    """Without the flags and the rows behind the cameras (key[:K], valid = None, the finite landmarks) every pair of every
    frame is a candidate at all_pass_radius; with them no radius does that."""
    s = scene_of(ALL_SCENES[k])
    rs, ts = planted_pose(s)
    clean = [(s["key"][:s["K"]], s["clean_xyz"], None)] * len(s["counts"])
    big = all_pass_radius(rs, ts, KVEC, s["xy"], s["counts"], clean)
    assert big is not None and 500 < big < 1e5, big
    for f, cnt in enumerate(s["counts"]):
        assert pose_gate(rs[f], ts[f], KVEC, s["xy"][f, :cnt], s["clean_xyz"], None, big)[0].all(), (k, f)
    assert all_pass_radius(rs, ts, KVEC, s["xy"], s["counts"], [key_train(s)] * len(s["counts"])) is None
    if k == 0:
        for cross, md, ratio in OPTIONS:                                # every pair a candidate: fpc_match_frames' rule
            m, d1, d2, _ = pose_frames_rule(s["desc"], s["xy"], s["counts"], clean, rs, ts, KVEC, big, cross, md, ratio)
            um, ud1, ud2 = frames_rule(s["desc"], s["counts"], s["key"][:s["K"]], PAIR_KEY, cross, md, ratio)
            np.testing.assert_array_equal(m, um)
            np.testing.assert_array_equal(d1, ud1)
            np.testing.assert_array_equal(d2, ud2)


def test_pose_gate_recovers_what_the_epipolar_gate_cannot():
    """Cross-checked, over the planted pairs whose landmark is valid: the unguided rule loses rows to look-alikes; the
    epipolar rule under the planted F at RADIUS cannot recover them (both landmarks lie in the band); the pose rule under the
    planted pose recovers every one."""
    tot = np.zeros(4, np.int64)
    for k, spec in enumerate(SCENES):
        s = scene_of(spec)
        desc, xy, counts = s["desc"], s["xy"], s["counts"]
        rs, ts = planted_pose(s)
        n = len(counts)
        truth = np.where(landmark_ok(s)[np.maximum(s["ids"], 0)], s["ids"], -1)           # (valid landmarks only)
        um, _, _ = frames_rule(desc, counts, s["key"], PAIR_KEY, True, 0.0, 0.0)
        em, _, _, _ = epipolar_frames_rule(desc, xy, counts, [(s["key"], s["key_xy"])] * n, planted_f(s), RADIUS)
        pm, _, _, _ = pose_frames_rule(desc, xy, counts, [key_train(s)] * n, rs, ts, KVEC, RADIUS)
        for f in range(n):
            (hu, have), (he, _), (hp, _) = recall(um[f], truth[f]), recall(em[f], truth[f]), recall(pm[f], truth[f])
            print("scene %d frame %d (%s): recall unguided %d, epipolar %d, pose %d of %d"
                  % (k, f, spec["kinds"][f], hu, he, hp, have))
            assert hu <= he < hp == have, (k, f, hu, he, hp, have)
            tot += (hu, he, hp, have)
            # the pose rule matches nothing to an invalid landmark or one behind the cameras
            got = pm[f, :counts[f]]
            assert landmark_ok(s)[got[got >= 0]].all() and (got < s["K"]).all()
        # the other option sets: Lowe's test needs a second CANDIDATE, and the gate leaves most rows just one
        m, _, _, _ = pose_frames_rule(desc, xy, counts, [key_train(s)] * n, rs, ts, KVEC, RADIUS, False, 0.0, 0.8)
        cand = pose_gate(rs[0], ts[0], KVEC, xy[0, :counts[0]], s["key_xyz"], s["key_valid"], RADIUS)[0]
        assert (m[0, :counts[0]][cand.sum(1) < 2] == -1).all()
    print("total: recall unguided %d, epipolar %d, pose %d of %d" % tuple(tot))
    assert tot[0] < tot[2] and tot[1] < tot[2] == tot[3]


def test_edge_cases_of_the_gate():
    s = scene_of(SCENES[0])
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    rs, ts = planted_pose(s)
    trains = [key_train(s, s["K"])] * len(counts)       # (without the rows behind the cameras: (-R, -t) brings those to the front)
    for bad_r, bad_t in ((np.zeros(9), np.zeros(3)), (np.r_[rs[1][:8], np.nan], ts[1]), (rs[1], np.r_[np.inf, ts[1][1:]]),
                         (-rs[1], -ts[1])):
        r_, t_ = rs.copy(), ts.copy()
        r_[1], t_[1] = bad_r, bad_t
        m, d1, _, _ = pose_frames_rule(desc, xy, counts, trains, r_, t_, KVEC, RADIUS)
        assert (m[1] == -1).all() and np.isinf(d1[1]).all()             # zeros: c = 0; non-finite; (-R, -t): c < 0
        assert ((m[[0, 2, 3]] >= 0).sum(axis=1) > 200).all()
    # R is used as given: 2 R, 2 t is the same camera (the gate is homogeneous in (R, t)), no orthonormalisation
    a = pose_frames_rule(desc, xy, counts, trains, 2 * rs, 2 * ts, KVEC, RADIUS)
    b = pose_frames_rule(desc, xy, counts, trains, rs, ts, KVEC, RADIUS)
    np.testing.assert_array_equal(a[0], b[0])
    # no train rows
    m, d1, _, _ = pose_frames_rule(desc, xy, counts, [(s["key"][:0], s["key_xyz"][:0], None)] * len(counts), rs, ts, KVEC, RADIUS)
    assert (m == -1).all() and np.isinf(d1).all()


def test_pose_kernel_fits_the_guided_budget(code_object):  # noqa: F811
    """match_guided_pose_kernel in the built code object: two workgroups of four waves per CU need <= 256 registers of the
    unified file and <= 80 KiB of LDS; nothing in scratch, no spills."""
    funcs, meta = code_object
    name = "_ZN3fpc24match_guided_pose_kernelENS_15MatchFramesArgsENS_13MatchPoseArgsE"
    assert name in meta, sorted(n for n in meta if "guided" in n)
    m = meta[name]
    print(m)
    assert m["vgpr_count"] <= 256 and m["group_segment_fixed_size"] <= 80 * 1024, m
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert not any(i.startswith("scratch_") for _, i in funcs[name])
    assert {i.split()[0] for _, i in funcs[name] if i.startswith("v_mfma")} == {"v_mfma_f32_32x32x2_f32"}
