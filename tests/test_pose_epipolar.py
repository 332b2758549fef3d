"""CPU checks of the relative-pose stage (fpc_pose_fundamental / fpc_pose_frames / fpc_pose_bank): the header declares it, the
binding binds it, the built library exports it -- and this file's float64 restatement of the rule of include/fpc.h (the
Sampson selection of the pairs, E = K_t^T F K_q, the decomposition through the cyclic Jacobi of E^T E, the four candidates,
the midpoint triangulation, the integer selection), which the GPU tests (test_gpu_pose_epipolar.py) hold the kernel to,
recovers planted camera motions and scene points: exactly from exact pairs, and within measured bars from integer pixels
and the F of the RANSAC restatement."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import (FRAME_H, FRAME_W, KINDS, KMAT, RESEED, _rotation, inliers_of, jacobi, planted_scene,
                                           restated_batch, sampson_terms)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_pose_fundamental", "fpc_pose_frames", "fpc_pose_bank")
RANK = 1e-12                # lambda2 / lambda1 at or below which the frame fails (include/fpc.h)
PARALLEL = 1e-12            # det / ((a.a)(b.b)) at or below which a pair is not in front (include/fpc.h)
KVEC = (500.0, 500.0, 320.0, 240.0)
THR = 2.0                   # the threshold the planted batches' F were estimated with (test_fundamental_ransac.PARAMS)
ROUNDED_SETS = [(0.0, 256), (0.3, 1024)]      # (outlier share, iterations) of the rounded scenes: restated_batch's cases


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def kmat(k):
    fx, fy, cx, cy = k
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def normalised(xy, k):
    fx, fy, cx, cy = k
    xy = np.asarray(xy, np.float64)
    return np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(xy))], 1)


def triangulate(r, t, ph, qh):
    """Midpoint triangulation of every pair under (R, t) -> (front [M], lam [M], mu [M])."""
    a, b = ph @ r.T, qh
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    at, bt = a @ t, b @ t
    det = aa * bb - ab * ab
    with np.errstate(all="ignore"):
        lam = (ab * bt - at * bb) / det
        mu = (aa * bt - ab * at) / det
        front = (det > PARALLEL * (aa * bb)) & (lam > 0) & (mu > 0)
    return front, lam, mu


class Pose:
    """The outputs of the rule for one frame, and what the device comparison needs to know about its thresholds."""

    def __init__(self, m):
        self.R, self.t, self.nfront = np.zeros((3, 3)), np.zeros(3), 0
        self.xyz, self.front = np.zeros((m, 3)), np.zeros(m, bool)
        self.c = -1
        self.near = np.zeros(m, bool)      # pairs whose lam, mu or Sampson distance lies within 1e-9 relative of its threshold

    @property
    def failed(self):
        return not (self.R.any() or self.t.any() or self.nfront or self.xyz.any() or self.front.any())


def pose_rule(src, dst, f, k_query=KVEC, k_train=KVEC, thr=3.0, min_front=8, basis=None):
    """include/fpc.h's rule for one frame in float64: src, dst [M,2], F [3,3] -> Pose.  basis: a function (v1, v2) -> (v1,
    v2) applied to the eigenvector pair before the candidates are built (the invariance test)."""
    src, dst, f = np.asarray(src, np.float64), np.asarray(dst, np.float64), np.asarray(f, np.float64).reshape(3, 3)
    out = Pose(len(src))
    thr = float(np.float32(thr))
    if not f.any() or not np.isfinite(f).all() or len(src) == 0:
        return out
    used = inliers_of(f, src, dst, thr)
    e = kmat(k_train).T @ f @ kmat(k_query)
    mx = np.abs(e).max()
    if not (mx > 0 and mx < 1e300):
        return out
    e = e / mx
    d, v = jacobi(e.T @ e)
    i1 = int(np.argmax(d))                                           # ties: the lowest index
    rest = d.copy()
    rest[i1] = -np.inf
    i2 = int(np.argmax(rest))
    if not d[i2] > RANK * d[i1]:
        return out
    v1, v2 = v[:, i1], v[:, i2]
    if basis is not None:
        v1, v2 = basis(v1, v2)
    v3 = np.cross(v1, v2)
    with np.errstate(all="ignore"):
        u1 = e @ v1
        u1 = u1 / np.sqrt(u1 @ u1)
        u2 = e @ v2
        u2 = u2 - (u1 @ u2) * u1
        u2 = u2 / np.sqrt(u2 @ u2)
    u3 = np.cross(u1, u2)
    s, w = np.outer(u2, v1) - np.outer(u1, v2), np.outer(u3, v3)
    cands = [(s + w, u3), (s + w, -u3), (w - s, u3), (w - s, -u3)]
    if not all(np.isfinite(r).all() and np.isfinite(t).all() for r, t in cands):
        return out
    ph, qh = normalised(src, k_query), normalised(dst, k_train)
    tri = [triangulate(r, t, ph, qh) for r, t in cands]
    counts = [int((used & fr).sum()) for fr, _, _ in tri]
    c = int(np.argmax(counts))                                       # the first maximum: ties go to the lower c
    if counts[c] < min_front:
        return out
    r, t = cands[c]
    fr, lam, mu = tri[c]
    sel = used & fr
    out.R, out.t, out.nfront, out.c = r, t, counts[c], c
    out.front = sel
    xyz = 0.5 * (lam[:, None] * ph + (mu[:, None] * qh - t) @ r)
    out.xyz[sel] = xyz[sel]
    # the neighbourhoods of the thresholds, for the comparison with the device
    e2, g = sampson_terms(f, src, dst)
    with np.errstate(all="ignore"):
        scale = max(np.abs(lam[used & np.isfinite(lam)]).max(initial=0.0), np.abs(mu[used & np.isfinite(mu)]).max(initial=0.0))
        out.near = (np.abs(e2 - thr * thr * g) <= 1e-9 * thr * thr * g) | \
                   (used & ((np.abs(lam) <= 1e-9 * scale) | (np.abs(mu) <= 1e-9 * scale)))
    return out


# ---- planted truth ----------------------------------------------------------------------------------------------------------
def pose_scene(kind, i, rho, npairs=600):
    """planted_scene(kind, i, rho, npairs) -- the same draws, so the same pairs -- with what that function discards:
    -> (src, dst, planted mask, unrounded src, unrounded dst, R, t, the 3-D points [npairs,3] in the first camera's frame)."""
    key = [{"general": 1, "sideways": 2, "forward": 3}[kind], i, int(round(rho * 100))]
    rng = np.random.Generator(np.random.PCG64(key + RESEED.get((kind, i, rho), [])))
    if kind == "general":
        r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2, 12)))
        t = rng.uniform(-0.6, 0.6, 3)
    else:
        r, t = np.eye(3), np.array([0.5, 0, 0] if kind == "sideways" else [0, 0, -0.7])
    pts = np.stack([rng.uniform(-4, 4, 20000), rng.uniform(-3, 3, 20000), rng.uniform(2, 8, 20000)], 1)
    a = pts @ KMAT.T
    b = (pts @ r.T + t) @ KMAT.T
    a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
    ok = np.ones(len(pts), bool)
    for v in (a, b):
        ok &= (v[:, 0] >= 0) & (v[:, 0] <= FRAME_W - 1) & (v[:, 1] >= 0) & (v[:, 1] <= FRAME_H - 1)
    a, b, pts = a[ok][:npairs], b[ok][:npairs], pts[ok][:npairs]
    src, dst, planted, a0, b0 = planted_scene(kind, i, rho, npairs)
    assert np.array_equal(a, a0) and np.array_equal(b, b0)           # the same scene: only the outliers are drawn behind this
    return src, dst, planted, a, b, r, np.asarray(t, np.float64), pts


def pose_batch(rho):
    """planted_batch(rho) of test_fundamental_ransac, scene for scene, with the motions and the points."""
    count = {}
    out = []
    for f, kind in enumerate(KINDS):
        i = count.get(kind, 0)
        count[kind] = i + 1
        out.append(pose_scene(kind, i, rho, 600 - 7 * (f % 5)))
    return out


def exact_f(r, t, k_query=KVEC, k_train=KVEC):
    """K_t^-T [t]x R K_q^-1 of the motion X_train = R X_query + t."""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return np.linalg.inv(kmat(k_train)).T @ tx @ r @ np.linalg.inv(kmat(k_query))


def angle_deg(cosine):
    return float(np.degrees(np.arccos(np.clip(cosine, -1.0, 1.0))))


def pose_errors(r, t, xyz, front, scene):
    """(rotation angle error (deg), angle between t and the planted direction (deg), median relative depth error of the
    planted pairs in front, share of the planted pairs in front)."""
    _, _, planted, _, _, r0, t0, pts = scene
    rot = angle_deg((np.trace(np.asarray(r, np.float64) @ r0.T) - 1.0) / 2.0)
    direction = angle_deg(np.asarray(t, np.float64) @ t0 / np.linalg.norm(t0))
    sel = planted & front
    depth = np.abs(np.asarray(xyz, np.float64)[sel, 2] * np.linalg.norm(t0) - pts[sel, 2]) / pts[sel, 2]
    return rot, direction, float(np.median(depth)) if sel.any() else np.inf, sel.sum() / planted.sum()


# Planted-truth bars on the integer-rounded scenes with the F of the RANSAC rule (threshold 2 px), for restatement and device
# alike: twice the worst value of the restatement over the 28 scenes (14 without outliers at 256 iterations, 14 with a
# share of 0.3 at 1 024), rounded up.  Measured worst values per kind of motion, general / sideways / forward:
#                                    outlier share 0.0              outlier share 0.3
#   rotation angle error (deg)       0.1072 / 0.0000 / 0.0148       0.2086 / 0.0709 / 0.2175       -> bar 0.5
#   angle between t and truth (deg)  0.3214 / 0.0000 / 0.1145       5.0554 / 2.0183 / 1.7519       -> bar 10.5
#   median relative depth error      0.0226 / 0.0066 / 0.0123       0.0277 / 0.0102 / 0.0213       -> bar 0.06
# The 5.06 deg belong to the general scene with the shortest translation (|t| = 0.27, a parallax of a few pixels at integer
# resolution); the next general scene stands at 1.7 deg.  A rotation error above 2 deg or a direction error above 10 deg
# would count as a defect of the rule or of the generator, not as a bar; the worst values are 0.22 and 5.06 deg.
ROT_BAR, DIR_BAR, DEPTH_BAR, FRONT_SHARE = 0.5, 10.5, 0.06, 0.98


def check_planted_pose(r, t, nfront, xyz, front, scene, tag):
    """The planted-truth conditions of one rounded scene, for restatement and device alike -> its three errors."""
    planted = scene[2]
    rot, direction, depth, share = pose_errors(r, t, xyz, front, scene)
    assert nfront == front.sum() and nfront >= FRONT_SHARE * planted.sum(), (tag, nfront, planted.sum())
    assert share >= FRONT_SHARE, (tag, share)
    assert rot <= ROT_BAR, (tag, rot)
    assert direction <= DIR_BAR, (tag, direction)
    assert depth <= DEPTH_BAR, (tag, depth)
    assert abs(np.linalg.det(np.asarray(r, np.float64)) - 1.0) < 1e-5 and abs(np.linalg.norm(t) - 1.0) < 1e-5, tag
    return rot, direction, depth


@functools.lru_cache(maxsize=None)
def restated_poses(rho, iterations):
    """(scenes with their motions, the restated F of every scene, [Pose]) of one rounded case set: computed once, shared
    with the GPU tests.  The F are rounded to fp32, as the device returns them."""
    scenes = pose_batch(rho)
    _, results = restated_batch(rho, iterations)
    fms = [fm.astype(np.float32).astype(np.float64) for fm, _ in results]
    return scenes, fms, [pose_rule(s[0], s[1], fm, thr=THR) for s, fm in zip(scenes, fms)]


# ---- tests ------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_header_binding_and_library_agree():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NAMES + ("fpc_default_pose_params",):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) | {"fpc_default_pose_params"} <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    # argument for argument the fundamental calls, with (F_dev, params) where their params stand and the five outputs
    twins = ("fpc_ransac_fundamental", "fpc_fundamental_frames", "fpc_fundamental_bank")
    tail = "const float* F_dev, const fpc_pose_params* params, float* R_dev, float* t_dev, int32_t* nfront_dev, " \
           "float* xyz_dev, uint8_t* front_dev"
    for name, twin in zip(NAMES, twins):
        args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1)) for n in (name, twin)]
        shared = args[1].split("const fpc_ransac_params*")[0]
        assert args[0] == shared + tail, name
        nshared = len(shared.rstrip(", ").split(","))
        assert getattr(lib, name).argtypes[:nshared] == getattr(lib, twin).argtypes[:nshared], name
        assert len(getattr(lib, name).argtypes) == nshared + 7
    # the struct: the header's fields in the binding's order and types
    body = re.search(r"typedef struct fpc_pose_params \{(.*?)\} fpc_pose_params;", code, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(float|int)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_float if typ == "float" else ctypes.c_int) for n in names.split(",")]
    assert fields == list(_lib.FpcPoseParams._fields_)
    p = _lib.FpcPoseParams()
    assert lib.fpc_default_pose_params(ctypes.byref(p)) == 0
    assert [getattr(p, n) for n, _ in fields] == [500.0, 500.0, 320.0, 240.0, 500.0, 500.0, 320.0, 240.0, 3.0, 8]
    # the constants of the rule are part of the contract: the header states the ones this file restates
    for const in ("lambda2 > %g lambda1" % RANK, "det > %g (a.a)(b.b)" % PARALLEL, "X_train = R X_query + t",
                  "ties go to the lower c", "the index c of a candidate"):
        assert const in hdr, const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4
    assert lib.fpc_abi_version() == 4


def test_null_arguments():
    lib = _lib.load()
    p = _lib.FpcPoseParams()
    assert lib.fpc_default_pose_params(None) == FPC_E_INVALID
    assert lib.fpc_default_pose_params(ctypes.byref(p)) == 0
    buf = np.zeros(64, np.float32)
    d = buf.ctypes.data
    assert lib.fpc_pose_fundamental(None, 1, d, d, d, 8, d, ctypes.byref(p), d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_pose_frames(None, 1, 0, d, d, d, d, ctypes.byref(p), d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_pose_bank(None, 1, d, d, d, ctypes.byref(p), d, d, d, None, None) == FPC_E_INVALID


def test_scene_generator_reproduces_the_planted_scenes():
    for kind, i, rho in (("general", 1, 0.3), ("sideways", 0, 0.0), ("forward", 1, 0.5)):
        src, dst, planted, a, b, r, t, pts = pose_scene(kind, i, rho)
        ref = planted_scene(kind, i, rho)
        for x, y in zip((src, dst, planted, a, b), ref):
            assert np.array_equal(x, y)
        proj = (pts @ r.T + t) @ KMAT.T                                  # the points and the motion are those of the pairs
        assert np.abs(proj[:, :2] / proj[:, 2:] - b).max() < 1e-9
        assert abs(np.linalg.det(r) - 1.0) < 1e-12


EXACT = [("general", 0), ("general", 1), ("general", 2), ("sideways", 0), ("sideways", 1), ("forward", 0), ("forward", 1)]


@pytest.mark.parametrize("kind,i", EXACT)
def test_exact_pairs_give_the_planted_pose_and_points(kind, i):
    """Noise-free, unrounded pairs with the exact F: R and t / |t| to 1e-9, the points to 1e-6 of their distance, at the
    scale |t|."""
    _, _, _, a, b, r, t, pts = pose_scene(kind, i, 0.0)
    assert len(a) == 600
    got = pose_rule(a, b, exact_f(r, t), thr=1.0)
    assert got.nfront == 600 and got.front.all()
    assert np.abs(got.R - r).max() < 1e-9, np.abs(got.R - r).max()
    assert np.abs(got.t - t / np.linalg.norm(t)).max() < 1e-9
    rel = np.linalg.norm(got.xyz * np.linalg.norm(t) - pts, axis=1) / np.linalg.norm(pts, axis=1)
    assert rel.max() < 1e-6, rel.max()
    assert abs(np.linalg.det(got.R) - 1.0) < 1e-12 and abs(np.linalg.norm(got.t) - 1.0) < 1e-12
    # two cameras of different intrinsics: the same motion from the pixels they see
    kq, kt = (430.0, 445.0, 300.0, 250.0), (610.0, 590.0, 335.0, 228.0)
    a2 = (normalised(a, KVEC) @ kmat(kq).T)[:, :2]
    b2 = (normalised(b, KVEC) @ kmat(kt).T)[:, :2]
    got2 = pose_rule(a2, b2, exact_f(r, t, kq, kt), kq, kt, thr=1.0)
    assert got2.nfront == 600 and np.abs(got2.R - r).max() < 1e-9 and np.abs(got2.t - t / np.linalg.norm(t)).max() < 1e-9


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_rounded_scenes_meet_the_planted_truth_bars(rho, iterations):
    scenes, fms, poses = restated_poses(rho, iterations)
    worst = {}
    for f, (scene, fm, got) in enumerate(zip(scenes, fms, poses)):
        assert fm.any(), f
        errs = check_planted_pose(got.R, got.t, got.nfront, got.xyz, got.front, scene, (KINDS[f], f, rho))
        assert not got.front[~inliers_of(fm, scene[0], scene[1], THR)].any()     # only the used pairs can be in front
        assert not got.xyz[~got.front].any() and (got.xyz[got.front, 2] > 0).all()
        worst[KINDS[f]] = tuple(max(x, y) for x, y in zip(worst.get(KINDS[f], (0.0, 0.0, 0.0)), errs))
    for kind, (rot, direction, depth) in worst.items():
        print("rho %.1f %-8s: worst rotation error %.4f deg, direction error %.4f deg, median relative depth error %.5f"
              % (rho, kind, rot, direction, depth))


def test_failure_rules():
    src, dst, planted, a, b, r, t, pts = pose_scene("general", 0, 0.0)
    fm = exact_f(r, t)
    assert not pose_rule(a, b, fm, thr=1.0).failed
    assert pose_rule(a, b, np.zeros((3, 3))).failed                                  # a failed frame of the fundamental calls
    bad = fm.copy()
    bad[1, 1] = np.nan
    assert pose_rule(a, b, bad).failed
    rank1 = np.outer([0.3, -0.2, 1.0], [0.1, 0.4, -1.0])                             # every pair may pass; E has no plane
    assert pose_rule(a, b, rank1, thr=1e9).failed
    assert pose_rule(a[:0], b[:0], fm).failed
    far = b + np.array([0.0, 40.0])                                                  # no pair within the threshold
    assert not inliers_of(fm, a, far, 3.0).any() and pose_rule(a, far, fm).failed
    assert pose_rule(a[:100], b[:100], fm, thr=1.0, min_front=100).nfront == 100
    assert pose_rule(a[:100], b[:100], fm, thr=1.0, min_front=101).failed            # min_front above the count
    # a pure rotation seen under the F of ANOTHER scene.  Being in front of both cameras does not tell a wrong F from a right
    # one (the pairs that pass the Sampson test mostly triangulate in front under one candidate); what fails the frame is
    # how FEW pairs pass: none at 3 px, and at 10 px a handful of the 600, far below a min_front of half the pairs.
    rot = _rotation(np.array([0.2, 1.0, 0.1]), np.deg2rad(6.0))
    rng = np.random.Generator(np.random.PCG64(11))
    cloud = np.stack([rng.uniform(-3, 3, 600), rng.uniform(-2, 2, 600), rng.uniform(4, 8, 600)], 1)
    pa, pb = cloud @ KMAT.T, (cloud @ rot.T) @ KMAT.T
    pa, pb = np.rint(pa[:, :2] / pa[:, 2:]), np.rint(pb[:, :2] / pb[:, 2:])
    assert pose_rule(pa, pb, fm, thr=3.0, min_front=1).failed
    used = inliers_of(fm, pa, pb, 10.0)
    loose = pose_rule(pa, pb, fm, thr=10.0, min_front=1)
    print("pure rotation under a foreign F at 10 px: %d of 600 pairs used, %d in front under the best candidate"
          % (used.sum(), loose.nfront))
    assert 0 < loose.nfront <= used.sum() < 300
    assert pose_rule(pa, pb, fm, thr=10.0, min_front=300).failed


def test_selected_pose_does_not_depend_on_the_eigenvector_basis():
    """lambda1 = lambda2 for a true essential matrix: the basis of the plane is arbitrary.  Swapping v1 and v2 relabels the
    candidates (R_a <-> R_b, u3 <-> -u3) and a rotation within the plane changes nothing; the selected pose is the same."""
    for kind, i in (("general", 0), ("general", 2), ("sideways", 0), ("forward", 1)):
        _, _, _, a, b, r, t, _ = pose_scene(kind, i, 0.0)
        fm = exact_f(r, t)
        base = pose_rule(a, b, fm, thr=1.0)
        swap = pose_rule(a, b, fm, thr=1.0, basis=lambda v1, v2: (v2, v1))
        assert swap.c != base.c                                                  # the label moved ...
        variants = [swap]
        for ang in (0.3, 1.2, 2.9, -2.0):
            c, s = np.cos(ang), np.sin(ang)
            variants.append(pose_rule(a, b, fm, thr=1.0, basis=lambda v1, v2: (c * v1 + s * v2, -s * v1 + c * v2)))
            variants.append(pose_rule(a, b, fm, thr=1.0, basis=lambda v1, v2: (-s * v1 + c * v2, c * v1 + s * v2)))
        for got in variants:                                                     # ... the pose did not
            assert got.nfront == base.nfront == 600
            assert np.abs(got.R - base.R).max() < 1e-9 and np.abs(got.t - base.t).max() < 1e-9
            assert np.abs(got.xyz - base.xyz).max() < 1e-6 * np.abs(base.xyz).max()
    # on an estimated F (lambda1 != lambda2) the swap is still a relabelling
    scenes, fms, poses = restated_poses(*ROUNDED_SETS[0])
    for f in (0, 9, 12):
        swap = pose_rule(scenes[f][0], scenes[f][1], fms[f], thr=THR, basis=lambda v1, v2: (v2, v1))
        assert swap.nfront == poses[f].nfront and np.array_equal(swap.front, poses[f].front)
        assert np.abs(swap.R - poses[f].R).max() < 1e-9 and np.abs(swap.t - poses[f].t).max() < 1e-9
