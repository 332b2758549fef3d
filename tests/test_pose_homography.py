"""CPU checks of the homography-pose stage (fpc_pose_homography / fpc_pose_homography_frames / fpc_pose_homography_bank): the
header declares it, the binding binds it, the built library exports it -- and this file's float64 restatement of the rule of
include/fpc.h (H^ = K_t^-1 H K_q, the cyclic Jacobi of H^T H^, the baseline test, the four candidates of Ma, Soatto, Kosecka
and Sastry, the two counts per candidate, the integer selection), which the GPU tests (test_gpu_pose_homography.py) hold the
kernel to, recovers planted motions, planes and points: exactly from exact pairs, and within measured bars from integer pixels
and the H of the RANSAC restatement."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import _rotation, jacobi, sampson_terms
from tests.test_homography_ransac import FRAME_H, FRAME_W, ransac_rule
from tests.test_homography_ransac import inliers_of as h_inliers_of
from tests.test_pose_epipolar import KVEC, angle_deg, kmat, normalised, triangulate
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_pose_homography", "fpc_pose_homography_frames", "fpc_pose_homography_bank")
FAILED, UNIQUE, TWOFOLD, ROTATION = 0, 1, 2, 3
RANK = 1e-12                # lambda3 / lambda1 at or below which the frame fails (include/fpc.h)
THR = 3.0
MIN_BASELINE = 0.01


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
class PoseH:
    """The outputs of the rule for one frame, and what the device comparison needs to know about its thresholds."""

    def __init__(self, m):
        self.kind = FAILED
        self.R, self.t, self.plane = np.zeros((2, 3, 3)), np.zeros((2, 3)), np.zeros((2, 4))
        self.nfront, self.nplane = np.zeros(2, np.int64), np.zeros(2, np.int64)
        self.xyz, self.front = np.zeros((m, 3)), np.zeros(m, bool)
        self.c = [-1, -1]                  # the candidates of solutions 0 and 1
        self.cands = []                    # the four (R, t, N, d), or None where dropped as non-finite
        self.counts = np.zeros((2, 4), np.int64)      # nplane_c, nfront_c
        self.b = self.l1 = self.l3 = None  # the baseline and the normalised lambda1, lambda3, where the rule got that far
        self.near = np.zeros(m, bool)      # pairs with a test value within 1e-9 relative of its threshold

    @property
    def zeros(self):
        return not (self.R.any() or self.t.any() or self.plane.any() or self.nfront.any() or self.nplane.any()
                    or self.xyz.any() or self.front.any())


def normalised_h(h, kq, kt):
    """K_t^-1 H K_q written out for K = [fx 0 cx; 0 fy cy; 0 0 1]."""
    qfx, qfy, qcx, qcy = kq
    tfx, tfy, tcx, tcy = kt
    g = np.stack([h[:, 0] * qfx, h[:, 1] * qfy, h[:, 0] * qcx + h[:, 1] * qcy + h[:, 2]], 1)
    return np.stack([(g[0] - tcx * g[2]) / tfx, (g[1] - tcy * g[2]) / tfy, g[2]])


def candidate_f(r, t, kq, kt):
    """K_t^-T [t]x R K_q^-1 written out."""
    qfx, qfy, qcx, qcy = kq
    tfx, tfy, tcx, tcy = kt
    e = np.stack([t[1] * r[2] - t[2] * r[1], t[2] * r[0] - t[0] * r[2], t[0] * r[1] - t[1] * r[0]])
    g0, g1 = e[:, 0] / qfx, e[:, 1] / qfy
    g = np.stack([g0, g1, e[:, 2] - g0 * qcx - g1 * qcy], 1)
    f0, f1 = g[0] / tfx, g[1] / tfy
    return np.stack([f0, f1, g[2] - f0 * tcx - f1 * tcy])


def pose_h_rule(src, dst, h, k_query=KVEC, k_train=KVEC, thr=THR, min_front=8, min_baseline=MIN_BASELINE, which=0, basis=None):
    """include/fpc.h's rule for one frame in float64: src, dst [M,2], H [3,3] -> PoseH.  basis: a function (v1, v2) -> (v1,
    v2) applied to the eigenvector pair before v3 and the candidates are built (the invariance test)."""
    src, dst, h = np.asarray(src, np.float64), np.asarray(dst, np.float64), np.asarray(h, np.float64).reshape(3, 3)
    m = len(src)
    out = PoseH(m)
    thr, min_baseline = float(np.float32(thr)), float(np.float32(min_baseline))
    if not h.any() or not np.isfinite(h).all() or m == 0:
        return out
    hn = normalised_h(h, k_query, k_train)
    mx = np.abs(hn).max()
    if not (mx > 0 and mx < 1e300):
        return out
    hn = hn / mx
    d, v = jacobi(hn.T @ hn)
    i1 = int(np.argmax(d))                                           # ties: the lowest index
    rest = d.copy()
    rest[i1] = -np.inf
    i2 = int(np.argmax(rest))
    i3 = 3 - i1 - i2
    if not d[i3] > RANK * d[i1]:
        return out
    l1, l2, l3 = d[i1], d[i2], d[i3]
    hn = hn / np.sqrt(l2)
    l1, l3 = l1 / l2, l3 / l2
    det = hn[0, 0] * (hn[1, 1] * hn[2, 2] - hn[1, 2] * hn[2, 1]) - hn[0, 1] * (hn[1, 0] * hn[2, 2] - hn[1, 2] * hn[2, 0]) \
        + hn[0, 2] * (hn[1, 0] * hn[2, 1] - hn[1, 1] * hn[2, 0])
    if det < 0:
        hn = -hn
    v1, v2 = v[:, i1], v[:, i2]
    if basis is not None:
        v1, v2 = basis(v1, v2)
    v3 = np.cross(v1, v2)
    b = np.sqrt(l1) - np.sqrt(l3)
    out.b, out.l1, out.l3 = b, l1, l3
    if not b > min_baseline:
        with np.errstate(all="ignore"):
            w1 = hn @ v1
            w1 = w1 / np.sqrt(w1 @ w1)
            w2 = hn @ v2
            w2 = w2 - (w1 @ w2) * w1
            w2 = w2 / np.sqrt(w2 @ w2)
        w3 = np.cross(w1, w2)
        r = np.outer(w1, v1) + np.outer(w2, v2) + np.outer(w3, v3)
        if np.isfinite(r).all():
            out.kind, out.R[0] = ROTATION, r
        return out
    a, c, e = np.sqrt(max(0.0, 1.0 - l3)), np.sqrt(max(0.0, l1 - 1.0)), np.sqrt(l1 - l3)
    fs = []
    for sc in (c, -c):
        with np.errstate(all="ignore"):
            u = (a * v1 + sc * v3) / e
            n = np.cross(v2, u)
            w0, w1 = hn @ v2, hn @ u
            w2 = np.cross(w0, w1)
            r = np.outer(w0, v2) + np.outer(w1, u) + np.outer(w2, n)
            tt = (hn - r) @ n
            ln = np.sqrt(tt @ tt)
            t = tt / ln
            f = candidate_f(r, t, k_query, k_train)
            fine = np.isfinite(1.0 / ln) and all(np.isfinite(x).all() for x in (r, t, n, f))
        fs.append(f)
        out.cands += [(r, t, n, 1.0 / ln), (r, -t, -n, 1.0 / ln)] if fine else [None, None]
    ph, qh = normalised(src, k_query), normalised(dst, k_train)
    on = h_inliers_of(h, src, dst, thr)
    tri, support = [None] * 4, [None] * 4
    for ci, cand in enumerate(out.cands):
        if cand is None:
            continue
        tri[ci] = triangulate(cand[0], cand[1], ph, qh)
        e2, g = sampson_terms(fs[ci >> 1], src, dst)
        support[ci] = tri[ci][0] & (e2 < thr * thr * g)
        out.counts[0, ci], out.counts[1, ci] = int((on & tri[ci][0]).sum()), int(support[ci].sum())
    keys = [(int(out.counts[1, ci]) << 32) | (~ci & 0xFFFFFFFF) if out.cands[ci] is not None and out.counts[0, ci] >= min_front
            else 0 for ci in range(4)]
    order = sorted((ci for ci in range(4) if keys[ci]), key=lambda ci: -keys[ci])
    out.kind = FAILED if not order else (UNIQUE if len(order) == 1 else TWOFOLD)
    for j, ci in enumerate(order[:2]):
        r, t, n, dd = out.cands[ci]
        out.c[j] = ci
        out.R[j], out.t[j], out.plane[j, :3], out.plane[j, 3] = r, t, n, dd
        out.nfront[j], out.nplane[j] = out.counts[1, ci], out.counts[0, ci]
    if out.c[which] >= 0:
        ci = out.c[which]
        r, t = out.cands[ci][:2]
        _, lam, mu = tri[ci]
        sel = support[ci]
        out.front = sel
        xyz = 0.5 * (lam[:, None] * ph + (mu[:, None] * qh - t) @ r)
        out.xyz[sel] = xyz[sel]
    # the neighbourhoods of the thresholds, for the comparison with the device
    x, y, uu, vv = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    ex, ey = h[0, 0] * x + h[0, 1] * y + h[0, 2] - w * uu, h[1, 0] * x + h[1, 1] * y + h[1, 2] - w * vv
    near = np.abs(ex * ex + ey * ey - thr * thr * w * w) <= 1e-9 * thr * thr * w * w
    with np.errstate(all="ignore"):
        for ci in range(4):
            if out.cands[ci] is None:
                continue
            e2, g = sampson_terms(fs[ci >> 1], src, dst)
            near |= np.abs(e2 - thr * thr * g) <= 1e-9 * thr * thr * g
            _, lam, mu = tri[ci]
            scale = max(np.abs(lam[np.isfinite(lam)]).max(initial=0.0), np.abs(mu[np.isfinite(mu)]).max(initial=0.0))
            near |= (np.abs(lam) <= 1e-9 * scale) | (np.abs(mu) <= 1e-9 * scale)
    out.near = near
    return out


# ---- planted truth ----------------------------------------------------------------------------------------------------------
KMAT = kmat(KVEC)
SIZES = (8, 40, 200, 1100)
SEEDS = range(5)
# min_front / the homography rule's min_inliers of a scene with M pairs: the defaults (8), and 4 where the list has only 8
# pairs, of which the plane holds 7 at an off-plane share of 0.15.
SMALL = {8: 4}
# A scene whose float64 restatement alone ties on support at share 0.15 is replaced by the scene of another seed, at most
# one in twenty: (M, seed) -> seed.  M = 40, seed 4 is the one: a baseline of 0.12 plane distances, and its 6 off-plane pairs
# all lie within 3 px of the wrong candidate's epipolar lines as well (support 40 against 40); it runs under seed 5.  The
# off-plane pairs of a scene are ceil(0.15 M) -- 2 of 8: a single one would be a share of 0.125.
RESEED = {(40, 4): 5}


def plane_scene(i, share, m, pure_rotation=False):
    """One planted scene of m pairs at VGA, K = KVEC: a plane at depth 4 - 8 tilted 0 - 50 deg, a rotation of 3 - 20 deg, a
    baseline of 0.1 - 0.5 plane distances at >= 20 deg from the plane normal (none with pure_rotation), both cameras on one
    side of the plane; a share of the pairs off the plane, at 0.6 - 0.93 of the plane's depth on their ray.
    -> dict(src, dst (integer pixels), a, b (unrounded), R, T, N, d, pts [m,3], on (the plane's pairs))."""
    rng = np.random.Generator(np.random.PCG64([77, i, int(round(share * 100)), m, int(pure_rotation)]))
    while True:
        tilt = np.deg2rad(rng.uniform(0, 50))
        az = rng.uniform(0, 2 * np.pi)
        n0 = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
        d0 = n0[2] * rng.uniform(4, 8)                                # the plane passes (0, 0, depth)
        r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(3, 20)))
        tdir = rng.normal(size=3)
        tdir /= np.linalg.norm(tdir)
        t = np.zeros(3) if pure_rotation else tdir * rng.uniform(0.1, 0.5) * d0
        ang = angle_deg((r.T @ tdir) @ n0)
        centre = -r.T @ t                                             # the train camera in the query camera's frame
        if not pure_rotation and (not 20.0 <= ang <= 160.0 or not n0 @ centre < 0.9 * d0):
            continue
        px = np.stack([rng.uniform(0, FRAME_W - 1, 30 * m + 600), rng.uniform(0, FRAME_H - 1, 30 * m + 600)], 1)
        rays = normalised(px, KVEC)
        depth = d0 / (rays @ n0)
        noff = int(np.ceil(share * m - 1e-9))
        on = np.ones(len(px), bool)
        on[rng.permutation(len(px))[:int(len(px) * share)]] = False
        scale = np.where(on, 1.0, rng.uniform(0.6, 0.93, len(px)))
        pts = rays * (depth * scale)[:, None]
        q = pts @ r.T + t
        with np.errstate(all="ignore"):
            b = (q @ KMAT.T)[:, :2] / q[:, 2:]
        ok = (depth > 0) & (q[:, 2] > 0) & (b[:, 0] >= 0) & (b[:, 0] <= FRAME_W - 1) & (b[:, 1] >= 0) & (b[:, 1] <= FRAME_H - 1)
        ion, ioff = np.flatnonzero(ok & on), np.flatnonzero(ok & ~on)
        if len(ion) < m - noff or len(ioff) < noff:
            continue
        keep = np.sort(np.concatenate([ion[:m - noff], ioff[:noff]]))
        a, b, pts, on = px[keep], b[keep], pts[keep], on[keep]
        return dict(src=np.rint(a), dst=np.rint(b), a=a, b=b, R=r, T=t, N=n0, d=d0, pts=pts, on=on)


def exact_h(s, kq=KVEC, kt=KVEC):
    """K_t (R + T N^T / d) K_q^-1 of a scene."""
    return kmat(kt) @ (s["R"] + np.outer(s["T"], s["N"]) / s["d"]) @ np.linalg.inv(kmat(kq))


def restated_h(s, m, f=0):
    """The homography restatement's H of the scene's integer pairs, rounded to fp32 as the device returns it."""
    hm, inl = ransac_rule(s["src"], s["dst"], dict(iterations=256, seed=3, min_inliers=SMALL.get(m, 8)), f)
    return hm.astype(np.float32).astype(np.float64), inl


def solution_errors(got, j, s):
    """Solution j of a PoseH-like (R, t, plane) against the planted motion -> (rotation error, angle between t and T, angle
    between N and the planted normal (deg), relative error of d |T| against the planted d)."""
    r, t, pl = np.asarray(got.R[j], np.float64), np.asarray(got.t[j], np.float64), np.asarray(got.plane[j], np.float64)
    tn = np.linalg.norm(s["T"])
    return (angle_deg((np.trace(r @ s["R"].T) - 1.0) / 2.0), angle_deg(t @ s["T"] / tn), angle_deg(pl[:3] @ s["N"]),
            abs(pl[3] * tn - s["d"]) / s["d"])


def depth_error(xyz, front, s):
    """Median relative depth error of the pairs in front, at the planted scale."""
    z = np.asarray(xyz, np.float64)[front, 2] * np.linalg.norm(s["T"])
    return float(np.median(np.abs(z - s["pts"][front, 2]) / s["pts"][front, 2])) if front.any() else np.inf


# Planted-truth bars on the integer-pixel scenes with the H of the RANSAC restatement (3 px), for restatement and device
# alike: twice the worst value of the restatement over the 40 scenes (4 sizes x 5 seeds, off-plane share 0 and 0.15),
# rounded up.  Measured worst values of the planted solution, share 0 / share 0.15:
#   rotation angle error (deg)            0.8788 / 1.3045    -> bar 2.7
#   angle between t and truth (deg)       4.9044 / 7.0818    -> bar 14.2
#   angle between N and truth (deg)       3.8287 / 3.9690    -> bar 8.0
#   relative error of d                   0.04462 / 0.04226  -> bar 0.09
#   median relative depth error           -- / 0.04448       -> bar 0.09
# Every worst value belongs to a scene of 8 pairs (an H through 6 - 8 integer-pixel pairs); from 40 pairs on the worst are
# 0.31 deg, 1.36 deg, 1.09 deg, 0.020 and 0.022.  At share 0 the two survivors tie on support in 9 of the 20 scenes (the
# ambiguity the header describes), at share 0.15 in none after the one replacement of RESEED.
ROT_BAR, DIR_BAR, NRM_BAR, D_BAR, DEPTH_BAR = 2.7, 14.2, 8.0, 0.09, 0.09
# A pure rotation (H = K R K^-1) at integer pixels with the restatement's H: worst rotation error 0.03560 deg over 6 scenes
# -> bar 0.072; its b is at most 1.43e-3 (exact pixels: below 1e-15), the planted baselines' at least 0.1: min_baseline 0.01
# stands a factor of 7 from the one side and of 10 from the other.
PURE_ROT_BAR = 0.072


def within_bars(errs):
    return errs[0] <= ROT_BAR and errs[1] <= DIR_BAR and errs[2] <= NRM_BAR and errs[3] <= D_BAR


def check_planted(got, xyz, front, s, share, tag, min_front=8):
    """The planted-truth conditions of one integer-pixel scene, for restatement and device alike: got has kind, R, t, plane,
    nfront, nplane -> the errors of the planted solution and the depth error (share 0.15: of solution 0)."""
    assert got.kind in (UNIQUE, TWOFOLD), (tag, got.kind)
    if share > 0:
        assert got.nfront[0] > got.nfront[1], (tag, got.nfront)
        errs = solution_errors(got, 0, s)
        assert within_bars(errs), (tag, errs)
        depth = depth_error(xyz, front, s)
        assert depth <= DEPTH_BAR, (tag, depth)
        assert front.sum() == got.nfront[0], (tag, got.nfront)
    else:
        both = [solution_errors(got, j, s) for j in range(2 if got.kind == TWOFOLD else 1)]
        errs, depth = min(both, key=lambda e: e[0] + e[1]), 0.0       # the planted motion is among the returned solutions
        assert within_bars(errs), (tag, both)
    assert got.nplane[0] >= min_front
    for j in range(2 if got.kind == TWOFOLD else 1):
        assert abs(np.linalg.det(np.asarray(got.R[j], np.float64)) - 1.0) < 1e-5, tag
        assert abs(np.linalg.norm(got.t[j]) - 1.0) < 1e-5 and abs(np.linalg.norm(got.plane[j][:3]) - 1.0) < 1e-5, tag
        assert got.plane[j][3] > 0, tag
    return (*errs, depth)


def scene_of(m, seed, share):
    return plane_scene(RESEED.get((m, seed), seed) if share > 0 else seed, share, m)


@functools.lru_cache(maxsize=None)
def restated_scenes(share):
    """[(M, seed, scene, H (fp32 values), PoseH)] of the integer-pixel scenes at one off-plane share: computed once, shared
    with the GPU tests."""
    out = []
    for m in SIZES:
        for seed in SEEDS:
            s = scene_of(m, seed, share)
            hm, _ = restated_h(s, m, f=len(out))
            out.append((m, seed, s, hm, pose_h_rule(s["src"], s["dst"], hm, min_front=SMALL.get(m, 8))))
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_header_binding_and_library_agree():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    default = "fpc_default_pose_homography_params"
    for name in NAMES + (default,):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) | {default} <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    # argument for argument the homography calls, with (H_dev, params) where their params stand and the eight outputs
    twins = ("fpc_ransac_homography", "fpc_homography_frames", "fpc_homography_bank")
    tail = "const float* H_dev, const fpc_pose_homography_params* params, int32_t* kind_dev, float* R_dev, float* t_dev, " \
           "float* plane_dev, int32_t* nfront_dev, int32_t* nplane_dev, float* xyz_dev, uint8_t* front_dev"
    for name, twin in zip(NAMES, twins):
        args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1)) for n in (name, twin)]
        shared = args[1].split("const fpc_ransac_params*")[0]
        assert args[0] == shared + tail, name
        nshared = len(shared.rstrip(", ").split(","))
        assert getattr(lib, name).argtypes[:nshared] == getattr(lib, twin).argtypes[:nshared], name
        assert len(getattr(lib, name).argtypes) == nshared + 10
    body = re.search(r"typedef struct fpc_pose_homography_params \{(.*?)\} fpc_pose_homography_params;", code, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(float|int)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_float if typ == "float" else ctypes.c_int) for n in names.split(",")]
    assert fields == list(_lib.FpcPoseHomographyParams._fields_)
    p = _lib.FpcPoseHomographyParams()
    assert lib.fpc_default_pose_homography_params(ctypes.byref(p)) == 0
    got = [getattr(p, n) for n, _ in fields]
    assert got[:10] == [500.0, 500.0, 320.0, 240.0, 500.0, 500.0, 320.0, 240.0, 3.0, 8] and got[11] == 0
    assert got[10] == np.float32(MIN_BASELINE)
    q = _lib.FpcPoseParams()
    lib.fpc_default_pose_params(ctypes.byref(q))
    assert got[:10] == [getattr(q, n) for n, _ in _lib.FpcPoseParams._fields_]      # fpc_pose_params' defaults
    for word, value in (("FAILED", FAILED), ("UNIQUE", UNIQUE), ("TWOFOLD", TWOFOLD), ("ROTATION", ROTATION)):
        assert re.search(r"FPC_POSE_H_%s = %d\b" % (word, value), code), word
    # the constants of the rule are part of the contract: the header states the ones this file restates
    for const in ("lambda3 > %g lambda1" % RANK, "b = sqrt(lambda1) - sqrt(lambda3)", "(nfront_c << 32) | ~c",
                  "u+- = (a v1 +- c v3) / e", "R = W U^T,      N = v2 x u,      T = (H^ - R) N", "the index c of a candidate",
                  "The twofold ambiguity is a property of planes"):
        assert const in hdr, const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == lib.fpc_abi_version()


def test_null_ctx_and_bad_parameters_are_refused():
    lib = _lib.load()
    assert lib.fpc_default_pose_homography_params(None) == FPC_E_INVALID

    def params(**kw):
        p = _lib.FpcPoseHomographyParams()
        assert lib.fpc_default_pose_homography_params(ctypes.byref(p)) == 0
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    buf = np.zeros(64, np.float32)
    d = buf.ctypes.data
    outs = (d, d, d, d, d, d, None, None)
    assert lib.fpc_pose_homography(None, 1, d, d, d, 8, d, params(), *outs) == FPC_E_INVALID
    assert lib.fpc_pose_homography_frames(None, 1, 0, d, d, d, d, params(), *outs) == FPC_E_INVALID
    assert lib.fpc_pose_homography_bank(None, 1, d, d, d, params(), *outs) == FPC_E_INVALID
    # the parameter check comes before anything of the context is touched: a context that is no context (never read)
    nan, inf = float("nan"), float("inf")
    bad = [dict(q_fx=0.0), dict(q_fy=-1.0), dict(t_fx=0.0), dict(t_fy=nan), dict(q_cx=inf), dict(t_cy=nan),
           dict(reproj_threshold=0.0), dict(reproj_threshold=nan), dict(reproj_threshold=1e19), dict(min_front=0),
           dict(min_baseline=-0.001), dict(min_baseline=nan), dict(min_baseline=inf), dict(which=2), dict(which=-1)]
    fake = ctypes.c_void_p(d)
    for kw in bad:
        assert lib.fpc_pose_homography(fake, 1, d, d, d, 8, d, params(**kw), *outs) == FPC_E_INVALID, kw
        assert lib.fpc_pose_homography_frames(fake, 1, 0, d, d, d, d, params(**kw), *outs) == FPC_E_INVALID, kw
        assert lib.fpc_pose_homography_bank(fake, 1, d, d, d, params(**kw), *outs) == FPC_E_INVALID, kw
    assert lib.fpc_pose_homography(fake, 1, d, d, d, 8, d, None, *outs) == FPC_E_INVALID
    assert not buf.any()


@pytest.mark.parametrize("share", [0.0, 0.15])
def test_exact_pairs_give_the_planted_motion_plane_and_points(share):
    """Unrounded pairs with the exact H: R, t, N and d |T| to 1e-9; with pairs off the plane the planted motion is solution
    0 and its points are the planted ones; without, it is one of the two."""
    for m in SIZES:
        for seed in SEEDS:
            s = plane_scene(seed, share, m)
            got = pose_h_rule(s["a"], s["b"], exact_h(s), thr=1.0, min_front=SMALL.get(m, 8))
            assert got.l1 - 1.0 > 1e-3 and 1.0 - got.l3 > 1e-3, (m, seed, got.l1, got.l3)
            tn = np.linalg.norm(s["T"])
            assert abs(got.b - tn / s["d"]) < 1e-9 and got.b >= 0.1 - 1e-9
            assert got.kind == TWOFOLD, (m, seed, got.kind)       # cheirality leaves the two +T candidates on these scenes
            noff = int((~s["on"]).sum())
            assert noff == int(np.ceil(share * m - 1e-9))
            hit = [j for j in range(2) if np.abs(got.R[j] - s["R"]).max() < 1e-9]
            assert hit == [0] if share > 0 else len(hit) == 1, (m, seed, hit)
            j = hit[0]
            assert np.abs(got.t[j] - s["T"] / tn).max() < 1e-9 and np.abs(got.plane[j, :3] - s["N"]).max() < 1e-9
            assert abs(got.plane[j, 3] * tn - s["d"]) < 1e-9 * s["d"]
            assert m - noff <= got.nplane[j] <= m and got.nfront[j] == m       # (an off-plane pair may lie within 1 px of H)
            if share > 0:
                assert got.nfront[0] > got.nfront[1] and got.front.all()
                rel = np.linalg.norm(got.xyz * tn - s["pts"], axis=1) / np.linalg.norm(s["pts"], axis=1)
                assert rel.max() < 1e-6, rel.max()
            else:
                pts = pose_h_rule(s["a"], s["b"], exact_h(s), thr=1.0, min_front=SMALL.get(m, 8), which=j)
                rel = np.linalg.norm(pts.xyz * tn - s["pts"], axis=1) / np.linalg.norm(s["pts"], axis=1)
                assert pts.front.all() and rel.max() < 1e-6, rel.max()
    # two cameras of different intrinsics: the same motion from the pixels they see
    s = plane_scene(1, 0.15, 200)
    kq, kt = (430.0, 445.0, 300.0, 250.0), (610.0, 590.0, 335.0, 228.0)
    a2, b2 = (normalised(s["a"], KVEC) @ kmat(kq).T)[:, :2], (normalised(s["b"], KVEC) @ kmat(kt).T)[:, :2]
    got = pose_h_rule(a2, b2, exact_h(s, kq, kt), kq, kt, thr=1.0)
    assert got.kind == TWOFOLD and np.abs(got.R[0] - s["R"]).max() < 1e-9 and got.nfront[0] == 200 > got.nfront[1]
    assert np.abs(got.plane[0, :3] - s["N"]).max() < 1e-9


@pytest.mark.parametrize("share", [0.0, 0.15])
def test_integer_pixel_scenes_meet_the_planted_truth_bars(share):
    worst = np.zeros(5)
    ties = 0
    for m, seed, s, hm, got in restated_scenes(share):
        assert hm.any(), (m, seed)
        assert got.l1 - 1.0 > 1e-3 and 1.0 - got.l3 > 1e-3 and got.b > 10 * MIN_BASELINE, (m, seed, got.l1, got.l3, got.b)
        errs = check_planted(got, got.xyz, got.front, s, share, (m, seed, share), SMALL.get(m, 8))
        worst = np.maximum(worst, errs)
        ties += int(got.kind == TWOFOLD and got.nfront[0] == got.nfront[1])
        assert not got.xyz[~got.front].any() and (got.xyz[got.front, 2] > 0).all()
        assert got.near.mean() <= 0.02, (m, seed, got.near.sum())      # the GPU comparison's allowance, met by the rule alone
    print("share %.2f: worst rotation %.4f deg, direction %.4f deg, normal %.4f deg, d %.5f, depth %.5f; %d of %d scenes tie"
          % (share, *worst, ties, len(restated_scenes(share))))
    assert len(RESEED) <= 1


def test_pure_rotation():
    worst = 0.0
    for seed in range(6):
        s = plane_scene(seed, 0.15, 200, pure_rotation=True)
        h0 = exact_h(s)
        for label, src, dst, hm in (("exact", s["a"], s["b"], h0),
                                    ("integer", s["src"], s["dst"], restated_h(s, 200)[0])):
            got = pose_h_rule(src, dst, hm)
            assert got.kind == ROTATION and got.b < MIN_BASELINE / 2, (seed, label, got.kind, got.b)
            err = angle_deg((np.trace(got.R[0] @ s["R"].T) - 1.0) / 2.0)
            if label == "exact":
                assert np.abs(got.R[0] - s["R"]).max() < 1e-9 and got.b < 1e-12
            else:
                worst = max(worst, err)
                assert err <= PURE_ROT_BAR, (seed, err)
            assert abs(np.linalg.det(got.R[0]) - 1.0) < 1e-9
            assert not (got.R[1].any() or got.t.any() or got.plane.any() or got.nfront.any() or got.nplane.any()
                        or got.xyz.any() or got.front.any())
            print("pure rotation %d %-7s: b = %.3e, rotation error %.5f deg" % (seed, label, got.b, err))
    print("pure rotation, integer pixels: worst rotation error %.5f deg" % worst)
    # the planted baselines stand on the other side: b = |T| / d >= 0.1
    for seed in SEEDS:
        s = plane_scene(seed, 0.15, 200)
        assert pose_h_rule(s["a"], s["b"], exact_h(s), thr=1.0).b >= 0.1 - 1e-9
    # min_baseline decides: above a scene's b the same scene is a rotation
    s = plane_scene(0, 0.15, 200)
    b = np.linalg.norm(s["T"]) / s["d"]
    assert pose_h_rule(s["a"], s["b"], exact_h(s), thr=1.0, min_baseline=b * 1.01).kind == ROTATION
    assert pose_h_rule(s["a"], s["b"], exact_h(s), thr=1.0, min_baseline=b * 0.99).kind == TWOFOLD


def _solution_set(got):
    return sorted((tuple(np.round(c[0].ravel(), 9)), tuple(np.round(c[1], 9)), tuple(np.round(c[2], 9))) for c in got.cands)


def test_candidate_set_does_not_depend_on_the_eigenvector_signs():
    """lambda1 > lambda2 > lambda3 on these scenes: v1 and v2 are determined up to their signs (v1 <-> v2, the pose call's
    swap, is no freedom here: the lambdas order them).  Negating v1 swaps c = 0 <-> 1 and 2 <-> 3, negating v2 swaps 0 <-> 3
    and 1 <-> 2; the set of candidates, the counts each one gets and the returned solutions are the same."""
    flips = {"v1": (lambda v1, v2: (-v1, v2), [1, 0, 3, 2]), "v2": (lambda v1, v2: (v1, -v2), [3, 2, 1, 0]),
             "both": (lambda v1, v2: (-v1, -v2), [2, 3, 0, 1])}
    for m, seed in ((200, 0), (200, 3), (1100, 1), (40, 2)):
        s = plane_scene(seed, 0.15, m)
        for src, dst, hm, thr in ((s["a"], s["b"], exact_h(s), 1.0), (s["src"], s["dst"], restated_h(s, m)[0], THR)):
            base = pose_h_rule(src, dst, hm, thr=thr)
            for name, (basis, perm) in flips.items():
                got = pose_h_rule(src, dst, hm, thr=thr, basis=basis)
                for c in range(4):
                    for x, y in zip(got.cands[perm[c]], base.cands[c]):
                        assert np.abs(np.asarray(x) - np.asarray(y)).max() < 1e-9, (name, c)
                    assert (got.counts[:, perm[c]] == base.counts[:, c]).all()
                assert got.c[0] == perm[base.c[0]] and got.kind == base.kind
                assert np.abs(got.R - base.R).max() < 1e-9 and np.abs(got.t - base.t).max() < 1e-9
                assert np.abs(got.plane - base.plane).max() < 1e-9 * max(1.0, np.abs(base.plane).max())
                assert np.array_equal(got.nfront, base.nfront) and np.array_equal(got.front, base.front)
                assert np.abs(got.xyz - base.xyz).max() < 1e-6 * np.abs(base.xyz).max()


def test_failure_rules_which_and_min_front():
    s = plane_scene(2, 0.15, 200)
    a, b, hm = s["a"], s["b"], exact_h(s)
    base = pose_h_rule(a, b, hm, thr=1.0)
    assert base.kind == TWOFOLD and not base.zeros
    for bad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, hm), np.where(np.eye(3) > 0, np.inf, hm)):
        got = pose_h_rule(a, b, bad)
        assert got.kind == FAILED and got.zeros                                      # a zero H, a non-finite H
    rank2 = hm - np.outer(hm @ [0.2, -0.1, 1.0], [0.2, -0.1, 1.0]) / 1.05            # H x = 0 for a pixel x: rank 2
    got = pose_h_rule(a, b, rank2, thr=1e9)
    assert got.kind == FAILED and got.zeros
    assert pose_h_rule(a[:0], b[:0], hm).kind == FAILED
    # which = 1 writes solution 1's points: the other survivor's support, fewer than solution 0's
    other = pose_h_rule(a, b, hm, thr=1.0, which=1)
    assert other.c == base.c and np.array_equal(other.nfront, base.nfront) and np.array_equal(other.R, base.R)
    assert other.front.sum() == base.nfront[1] < base.nfront[0] == base.front.sum()
    assert not np.array_equal(other.xyz, base.xyz) and (other.xyz[other.front, 2] > 0).all()
    # min_front above a candidate's plane count drops it: the planted motion's -T twin keeps no plane pair in front
    top = int(base.nplane.max())
    assert base.counts[0, base.c[0] ^ 1] == 0 and top >= 170 and base.nplane.min() > 8
    assert pose_h_rule(a, b, hm, thr=1.0, min_front=int(base.nplane.min())).kind == TWOFOLD
    got = pose_h_rule(a, b, hm, thr=1.0, min_front=top + 1)
    assert got.kind == FAILED and got.zeros
    # no pair follows H: nothing counts, the frame fails
    got = pose_h_rule(a, b + np.array([0.0, 60.0]), hm, min_front=1)
    assert got.kind == FAILED and got.zeros
    # one survivor: where the second +T candidate's normal turns away from some plane pairs it keeps fewer of them in front,
    # and a min_front between the two counts leaves solution 0 alone -- solution 1 is zeros and which = 1 writes no points
    s1 = plane_scene(0, 0.15, 200)
    two = pose_h_rule(s1["a"], s1["b"], exact_h(s1), thr=1.0)
    assert two.kind == TWOFOLD and two.nplane[1] < two.nplane[0] == 170, two.nplane
    one = pose_h_rule(s1["a"], s1["b"], exact_h(s1), thr=1.0, min_front=int(two.nplane[1]) + 1)
    assert one.kind == UNIQUE and one.c == [two.c[0], -1] and np.array_equal(one.R[0], two.R[0])
    assert not (one.R[1].any() or one.t[1].any() or one.plane[1].any() or one.nfront[1] or one.nplane[1])
    assert np.array_equal(one.front, two.front) and one.front.all()
    none = pose_h_rule(s1["a"], s1["b"], exact_h(s1), thr=1.0, min_front=int(two.nplane[1]) + 1, which=1)
    assert none.kind == UNIQUE and not none.front.any() and not none.xyz.any() and np.array_equal(none.R, one.R)


def test_kernel_uses_no_scratch(code_object):  # noqa: F811
    """pose_homography_kernel in the built code object: nothing in scratch, no spills."""
    _, meta = code_object
    names = [n for n in meta if "pose_homography_kernel" in n]
    assert len(names) == 1, sorted(n for n in meta if "pose" in n)
    m = meta[names[0]]
    print(m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
