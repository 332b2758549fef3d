"""CPU checks of the Sim(3) alignment stage (fpc_ransac_sim3 / fpc_sim3_frames / fpc_sim3_bank): the header declares it, the
binding binds it, the built library exports it -- and this file's float64 restatement of the rule of include/fpc.h (the
integer sampler with 16 draws, the triad solve of three pairs and its degeneracy, the fp32 scoring of the 24-value hypothesis
in both cameras, the integer selection, Horn's quaternion refit through the cyclic Jacobi with its singularity rules and the
monotone guard, the inlier rule and the failure cases), which the GPU tests (test_gpu_sim3_ransac.py) hold the kernels to,
recovers planted similarities.

Planted scenes.  Train points lie in the frustum box DEPTH in front of the train camera at VGA intrinsics; the query points
are s0 R0 X + t0 with a rotation of 5 .. 30 degrees, s0 log-uniform in [0.5, 2] and |t0| = 0.5 .. 1.5 mean depths (in the
query's units), redrawn until every point lies in front of the query camera.  Both sides are then perturbed as triangulated
points are: the point is projected into its OWN camera, the pixel is rounded to an integer (lateral error), and it is put back
on that pixel's ray at a depth with a relative Gaussian error of DEPTH_SIGMA = 0.2 %.  A fraction rho of the pairs gets a
random query point instead.  reproj_threshold is 3 px.

Planted-truth bars.  Measured with this restatement over the case set below (CASE_SETS x CASE_M, scenes 0 and 1 of each): worst
rotation error 0.7073 degrees, worst |s / s0 - 1| 5.746e-03, worst |t - t0| / |t0| 1.261e-02 -- all three at M = 4, where the
four noisy pairs are all there is; from M = 40 on the worst are 0.1902 degrees, 3.141e-03 and 4.489e-03.  The bars
are twice the worst (a different, equally good best sample is allowed): ROT_BAR, SCALE_BAR and TRANS_BAR.  No pair of any
scene lies within 1e-3 px of the threshold under the restatement's model for more than 2 % of a frame's pairs (the cap the
GPU test uses; checked below)."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import jacobi
from tests.test_homography_ransac import mix
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
FRAME_H, FRAME_W = 480, 640
DRAWS, SAMPLE, MAX_ITERATIONS = 16, 3, 4096
DEGENERATE = 1e-12          # sin^2 of the sample triangle's angle at or below which a sample is degenerate (include/fpc.h)
GAP = 1e-12                 # (lambda0 - lambda1) / sqrt(sum |a|^2 sum |b|^2) at or below which a refit is singular
KVEC = (500.0, 500.0, 320.0, 240.0)
DEFAULTS = dict(iterations=1024, reproj_threshold=3.0, seed=0, refits=4, min_inliers=12, fix_scale=0)
NAMES = ("fpc_default_sim3_params", "fpc_ransac_sim3", "fpc_sim3_frames", "fpc_sim3_bank")
FIELDS = ["q_fx", "q_fy", "q_cx", "q_cy", "t_fx", "t_fy", "t_cx", "t_cy", "iterations", "reproj_threshold", "seed", "refits",
          "min_inliers", "fix_scale"]
ROT_BAR = 2 * 0.7073        # degrees: twice the worst the restatement shows on the case set (module docstring)
SCALE_BAR = 2 * 5.746e-03   # |s / s0 - 1|, likewise
TRANS_BAR = 2 * 1.261e-02   # |t - t0| / |t0|, likewise
NEAR_CAP = 0.02             # share of a frame's pairs that may lie within 1e-3 px of the threshold
# the four kernels of csrc/sim3_ransac.h and their LDS bytes
SIM3_KERNELS = {
    "_Z16sim3_pack_kernel8Sim3ArgsPKfS1_PKiiPh": 0,
    "_Z18sim3_gather_kernel8Sim3ArgsPKfPKhPKiS5_Ph8PnpTrain": 16,
    "_Z17sim3_score_kernel8Sim3Args": 32768,
    "_Z17sim3_refit_kernel8Sim3ArgsPfS0_S0_PiPhi": 824,
}


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _draws(seed, f, t, m):
    with np.errstate(over="ignore"):
        base = (np.uint32(f) * np.uint32(MAX_ITERATIONS) + np.asarray(t, np.uint32)) * np.uint32(DRAWS)
        return mix(np.uint32(seed) ^ mix(base[..., None] + np.arange(DRAWS, dtype=np.uint32))) % np.uint32(m)


def all_samples(seed, f, iterations, m):
    """[T,3] indices and [T] validity: the first 3 distinct of the 16 draws of every hypothesis, in draw order."""
    r = _draws(seed, f, np.arange(iterations, dtype=np.uint32), m)
    idx = np.zeros((iterations, SAMPLE), np.int64)
    ok = np.zeros(iterations, bool)
    for t, row in enumerate(r.tolist()):
        got = []
        for v in row:
            if v not in got:
                got.append(v)
                if len(got) == SAMPLE:
                    break
        if len(got) == SAMPLE:
            idx[t], ok[t] = got, True
    return idx, ok


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def triad(p):
    """p [T,3,3] (three points) -> (x, y, z [T,3], ok [T]): x along p1 - p0, z along (p1 - p0) x (p2 - p0), y = z x x."""
    with np.errstate(all="ignore"):
        d1, d2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        n1, n2 = _dot(d1, d1), _dot(d2, d2)
        c = np.cross(d1, d2)
        cc = _dot(c, c)
        ok = cc > (DEGENERATE * n1) * n2
        x = d1 / np.sqrt(n1)[:, None]
        z = c / np.sqrt(cc)[:, None]
        y = np.cross(z, x)
    return x, y, z, ok


def solve3(q, p, fix_scale=0):
    """The minimal solve, batched: q, p [T,3,3] (query and train points of the three pairs) -> (s [T], R [T,3,3], t [T,3],
    ok [T]) with q = s R p + t."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        xq, yq, zq, okq = triad(q)
        xt, yt, zt, okt = triad(p)
        r = (xq[:, :, None] * xt[:, None, :] + yq[:, :, None] * yt[:, None, :]) + zq[:, :, None] * zt[:, None, :]
        qm = ((q[:, 0] + q[:, 1]) + q[:, 2]) / 3.0
        pm = ((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0
        vq = sum(_dot(q[:, k] - qm, q[:, k] - qm) for k in range(3))
        vp = sum(_dot(p[:, k] - pm, p[:, k] - pm) for k in range(3))
        s = np.ones(len(q)) if fix_scale else np.sqrt(vq / vp)
        t = qm - s[:, None] * ((r[:, :, 0] * pm[:, None, 0] + r[:, :, 1] * pm[:, None, 1]) + r[:, :, 2] * pm[:, None, 2])
        ok = okq & okt & (s > 0) & (s < 1e300) & (np.abs(t) < 1e300).all(1) & (np.abs(r) < 1e300).all((1, 2))
    return s, r, t, ok


def hypotheses(s, r, t, ok):
    """The 24 fp32 values of every hypothesis: (A = s R [T,3,3], t [T,3], B = R^T / s [T,3,3], u = -R^T t / s [T,3]) float32
    and ok [T]; a degenerate hypothesis is all zeros."""
    with np.errstate(all="ignore"):
        a = s[:, None, None] * r
        b = np.swapaxes(r, 1, 2) / s[:, None, None]
        u = -((r[:, 0, :] * t[:, None, 0] + r[:, 1, :] * t[:, None, 1]) + r[:, 2, :] * t[:, None, 2]) / s[:, None]
        h = [v.astype(np.float32) for v in (a, t, b, u)]
        ok = ok & np.all([np.isfinite(v).reshape(len(s), -1).all(1) for v in h], 0)
    for v in h:
        v[~ok] = 0.0
    return h, ok


def _fma(a, b, c):
    """fmaf on float32 values: the exact product, one addition in float64, rounded to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def score(h, q, p, kq, kt, thr, chunk=256):
    """The fp32 count of every hypothesis against the pairs q, p [M,3] (float32 values) -> int [T]."""
    a, t, b, u = h
    q32, p32 = np.asarray(q, np.float32), np.asarray(p, np.float32)
    thr = np.float32(thr)
    out = np.zeros(len(a), np.int64)

    def transform(m, v, pt):
        x, y, z = (pt[None, :, k] for k in range(3))
        return [_fma(m[:, i, 2, None], z, _fma(m[:, i, 1, None], y, _fma(m[:, i, 0, None], x, v[:, i, None]))) for i in range(3)]

    def within(y, pt, fx, fy):
        px, py, pz = (pt[None, :, k] for k in range(3))
        ex = np.float32(fx) * _fma(y[0], pz, -(px * y[2]))
        ey = np.float32(fy) * _fma(y[1], pz, -(py * y[2]))
        tw = thr * (y[2] * pz)
        return (y[2] > 0) & (pz > 0) & (_fma(ex, ex, ey * ey) < tw * tw)
    with np.errstate(all="ignore"):
        for c0 in range(0, len(a), chunk):
            sl = slice(c0, c0 + chunk)
            y = transform(a[sl], t[sl], p32)
            w = transform(b[sl], u[sl], q32)
            out[sl] = (within(y, q32, kq[0], kq[1]) & within(w, p32, kt[0], kt[1])).sum(1)
    return out


def inlier_terms(model, q, p, kq, kt):
    """The terms of the header's inlier test under model = (s, R, t): (front bool [M]: every coordinate finite and the four
    depths positive; lhs1, rhs1, lhs2, rhs2 with the pair an inlier iff front and lhs < thr^2 rhs in both cameras)."""
    s, r, t = model
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    kq, kt = [float(np.float32(v)) for v in kq], [float(np.float32(v)) for v in kt]
    with np.errstate(all="ignore"):
        y = s * (p @ r.T) + t
        w = ((q - t) @ r) / s
        fin = np.isfinite(q).all(1) & np.isfinite(p).all(1) & np.isfinite(y).all(1) & np.isfinite(w).all(1)
        front = fin & (y[:, 2] > 0) & (q[:, 2] > 0) & (w[:, 2] > 0) & (p[:, 2] > 0)
        ex, ey = kq[0] * (y[:, 0] * q[:, 2] - q[:, 0] * y[:, 2]), kq[1] * (y[:, 1] * q[:, 2] - q[:, 1] * y[:, 2])
        fx, fy = kt[0] * (w[:, 0] * p[:, 2] - p[:, 0] * w[:, 2]), kt[1] * (w[:, 1] * p[:, 2] - p[:, 1] * w[:, 2])
        return (front, ex * ex + ey * ey, (y[:, 2] * y[:, 2]) * (q[:, 2] * q[:, 2]),
                fx * fx + fy * fy, (w[:, 2] * w[:, 2]) * (p[:, 2] * p[:, 2]))


def inliers_of(model, q, p, kq, kt, thr):
    front, l1, r1, l2, r2 = inlier_terms(model, q, p, kq, kt)
    with np.errstate(all="ignore"):
        return front & (l1 < thr * thr * r1) & (l2 < thr * thr * r2)


def reprojection_errors(model, q, p, kq, kt):
    """Pixels, in the query and in the train camera; inf where the pair is not in front of everything."""
    front, l1, r1, l2, r2 = inlier_terms(model, q, p, kq, kt)
    with np.errstate(all="ignore"):
        return np.where(front, np.sqrt(l1 / r1), np.inf), np.where(front, np.sqrt(l2 / r2), np.inf)


def near_threshold(model, q, p, kq, kt, thr, eps=1e-3):
    e1, e2 = reprojection_errors(model, q, p, kq, kt)
    with np.errstate(all="ignore"):
        return (np.abs(e1 - thr) <= eps) | (np.abs(e2 - thr) <= eps)


def rotation_of(w, x, y, z):
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def horn(q, p, fix_scale=0, rounded=True):
    """Horn's closed form over the pairs q, p [n,3]: -> (s, R, t) with q ~ s R p + t, rounded to fp32 (as float64), or None:
    the refit is singular."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    n = len(q)
    if n < 3:
        return None
    qm, pm = q.sum(0) / n, p.sum(0) / n
    a, b = p - pm, q - qm
    sm = a.T @ b                                                     # row: a's component, column: b's
    va, vb = (a * a).sum(), (b * b).sum()
    if not (va > 0 and vb > 0):
        return None
    (sxx, sxy, sxz), (syx, syy, syz), (szx, szy, szz) = sm
    nm = np.array([[sxx + syy + szz, syz - szy, szx - sxz, sxy - syx],
                   [syz - szy, sxx - syy - szz, sxy + syx, szx + sxz],
                   [szx - sxz, sxy + syx, -sxx + syy - szz, syz + szy],
                   [sxy - syx, szx + sxz, syz + szy, -sxx - syy + szz]])
    lam, v = jacobi(nm)
    top = int(np.argmax(lam))                                        # ties: the lowest index
    second = max(lam[i] for i in range(4) if i != top)
    if not lam[top] - second > GAP * np.sqrt(va * vb):
        return None
    quat = v[:, top] / np.sqrt((v[:, top] ** 2).sum())
    r = rotation_of(*quat)
    s = 1.0 if fix_scale else np.sqrt(vb / va)
    t = qm - s * (r @ pm)
    if not rounded:
        return s, r, t
    s, r, t = float(_f32(s)), _f32(r), _f32(t)
    if not (0 < s < 3e38 and (np.abs(r) < 3e38).all() and (np.abs(t) < 3e38).all()):
        return None
    return s, r, t


Sim3 = collections.namedtuple("Sim3", "s R t ninliers mask failed best_t near first trace")


def _failed(m, best_t=-1, first=None, trace=()):
    return Sim3(0.0, np.zeros((3, 3)), np.zeros(3), 0, np.zeros(m, bool), True, best_t, np.zeros(m, bool), first, tuple(trace))


def sim3_rule(q, p, params, f, kq=KVEC, kt=KVEC, guard=True):
    """The whole rule for frame index f: q, p [M,3] (float32 values; query and train points) -> Sim3.  `near`: the pairs within
    1e-3 px of the threshold under the returned model; `first`: the best sample's fp32 model; `trace`: per refit
    ("singular", n) or ("kept" / "refused", count before, count of the refitted model).  guard=False drops the monotone
    guard (for the tests that show what it is for)."""
    prm = dict(DEFAULTS, **params)
    thr = float(np.float32(prm["reproj_threshold"]))
    q, p = _f32(q).reshape(-1, 3), _f32(p).reshape(-1, 3)
    m = len(q)
    if m < SAMPLE:
        return _failed(m)
    idx, ok = all_samples(prm["seed"], f, prm["iterations"], m)
    s, r, t, ok = solve3(q[idx], p[idx], prm["fix_scale"])
    h, ok = hypotheses(s, r, t, ok)
    counts = np.where(ok, score(h, q, p, kq, kt, thr), 0)
    if counts.max() <= 0:
        return _failed(m)
    best = int(np.argmax(counts))                                    # the largest count, ties to the lower t
    model = (float(_f32(s[best])), _f32(r[best]), _f32(t[best]))
    if not (0 < model[0] < 3e38):
        return _failed(m, best)
    first, trace = model, []
    for _ in range(prm["refits"]):
        inl = inliers_of(model, q, p, kq, kt, thr)
        nxt = horn(q[inl], p[inl], prm["fix_scale"])
        if nxt is None:
            trace.append(("singular", int(inl.sum())))
            break
        after = int(inliers_of(nxt, q, p, kq, kt, thr).sum())
        if guard and after < inl.sum():
            trace.append(("refused", int(inl.sum()), after))
            break
        trace.append(("kept", int(inl.sum()), after))
        model = nxt
    inl = inliers_of(model, q, p, kq, kt, thr)
    if inl.sum() < prm["min_inliers"]:
        return _failed(m, best, first, trace)
    near = near_threshold(model, q, p, kq, kt, thr)
    return Sim3(model[0], model[1], model[2], int(inl.sum()), inl, False, best, near, first, tuple(trace))


# ---- planted scenes -------------------------------------------------------------------------------------------------------
CASE_SETS = [(0.0, 256), (0.3, 1024), (0.6, 4096)]                  # (outlier fraction, iterations)
# M = 3 and 4 stand at rho = 0 only and 12 not at rho = 0.6: a frame needs 3 inliers, and a sample of three noisy pairs whose
# model keeps fewer than 3 pairs within 3 px in both cameras fails the frame.  Every (rho, M) uses scenes 0 and 1.
CASE_M = {0.0: [3, 4, 12, 40, 200, 1100], 0.3: [12, 40, 200, 1100], 0.6: [40, 200, 1100]}
PARAMS = dict(reproj_threshold=3.0, seed=7, refits=4, min_inliers=3)          # (3: the frames of 3 and 4 pairs can pass)
DEPTH = (4.0, 12.0)                                                  # the box: mean depth 8, spread 8
DEPTH_SIGMA = 0.002                                                  # relative depth error of a triangulated point


def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def as_triangulated(x, rng, sigma, kvec=KVEC):
    """Points in a camera's frame, perturbed as triangulated points are: the pixel rounded to an integer, the depth with a
    relative Gaussian error sigma."""
    fx, fy, cx, cy = kvec
    px = np.round(np.stack([fx * x[:, 0] / x[:, 2] + cx, fy * x[:, 1] / x[:, 2] + cy], 1))
    z = x[:, 2] * (1.0 + sigma * rng.normal(size=len(x)))
    return np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)


def planted_scene(i, rho, m, sigma=DEPTH_SIGMA, kvec=KVEC):
    """-> (q float32 [m,3], p float32 [m,3], planted bool [m], s0, R0, t0): see the module docstring."""
    fx, fy, cx, cy = kvec
    rng = np.random.default_rng(1000 * i + 10 * m + int(round(10 * rho)) + 77)
    r0 = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(5.0, 30.0)))
    s0 = float(np.exp(rng.uniform(np.log(0.5), np.log(2.0))))
    px = np.stack([rng.uniform(8, FRAME_W - 8, m), rng.uniform(8, FRAME_H - 8, m)], 1)
    z = rng.uniform(DEPTH[0], DEPTH[1], m)
    xt = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
    while True:
        d = rng.normal(size=3)
        t0 = d / np.linalg.norm(d) * rng.uniform(0.5, 1.5) * 0.5 * (DEPTH[0] + DEPTH[1]) * s0
        xq = s0 * (xt @ r0.T) + t0
        if xq[:, 2].min() > s0:                                      # every point in front of the query camera
            break
    q, p = as_triangulated(xq, rng, sigma, kvec), as_triangulated(xt, rng, sigma, kvec)
    planted = np.ones(m, bool)
    nout = int(round(rho * m))
    if nout:
        out = rng.choice(m, nout, replace=False)
        zo = rng.uniform(DEPTH[0], DEPTH[1], nout) * s0
        q[out] = np.stack([(rng.uniform(0, FRAME_W, nout) - cx) / fx * zo, (rng.uniform(0, FRAME_H, nout) - cy) / fy * zo, zo], 1)
        planted[out] = False
    return q.astype(np.float32), p.astype(np.float32), planted, s0, r0, t0


def planted_batch(rho):
    """The frames of one case set: two scenes of every M."""
    return [planted_scene(i, rho, m) for m in CASE_M[rho] for i in (0, 1)]


def sim3_errors(s, r, t, scene):
    """(rotation angle in degrees, |s / s0 - 1|, |t - t0| / |t0|) of a model against the scene's planted one."""
    s0, r0, t0 = scene[3], scene[4], scene[5]
    cosang = (np.trace(np.asarray(r, np.float64) @ r0.T) - 1.0) / 2.0
    return (np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))), abs(float(s) / s0 - 1.0),
            np.linalg.norm(np.asarray(t, np.float64) - t0) / np.linalg.norm(t0))


def check_planted(s, r, t, mask, scene, tag):
    """The planted-truth bars on one frame -> (rotation error, scale error, translation error)."""
    rot, sc, tr = sim3_errors(s, r, t, scene)
    assert rot <= ROT_BAR and sc <= SCALE_BAR and tr <= TRANS_BAR, (tag, rot, sc, tr)
    assert abs(np.linalg.det(np.asarray(r, np.float64)) - 1.0) < 1e-5 and s > 0, tag
    planted = scene[2]
    assert not mask[~planted].sum() > 0.1 * max(1, (~planted).sum()), tag        # an outlier is an inlier only by chance
    return rot, sc, tr


@functools.lru_cache(maxsize=None)
def restated_batch(rho, iterations):
    scenes = planted_batch(rho)
    return scenes, [sim3_rule(s[0], s[1], dict(PARAMS, iterations=iterations), f) for f, s in enumerate(scenes)]


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpc.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct fpc_sim3_params \{[^}]*float q_fx, q_fy, q_cx, q_cy;[^}]*float t_fx, t_fy, t_cx, t_cy;"
                     r"[^}]*int iterations;[^}]*float reproj_threshold;[^}]*uint32_t seed;[^}]*int refits;[^}]*int min_inliers;"
                     r"[^}]*int fix_scale;[^}]*\} fpc_sim3_params;", hdr)
    assert [n for n, _ in _lib.FpcSim3Params._fields_] == FIELDS
    assert ctypes.sizeof(_lib.FpcSim3Params) == 56
    assert re.search(r"#define FPC_ABI_VERSION 4\b", hdr) and lib.fpc_abi_version() == 4 == _lib.ABI_VERSION
    p = _lib.FpcSim3Params()
    assert lib.fpc_default_sim3_params(ctypes.byref(p)) == 0
    assert (p.q_fx, p.q_fy, p.q_cx, p.q_cy) == KVEC and (p.t_fx, p.t_fy, p.t_cx, p.t_cy) == KVEC
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert lib.fpc_default_sim3_params(None) == FPC_E_INVALID


def test_null_context_is_refused():
    lib = _lib.load()
    p = _lib.FpcSim3Params()
    lib.fpc_default_sim3_params(ctypes.byref(p))
    buf = (ctypes.c_float * 64)()
    b = ctypes.addressof(buf)
    pp = ctypes.byref(p)
    assert lib.fpc_ransac_sim3(None, 1, b, b, b, 1, pp, b, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_sim3_frames(None, 1, b, b, b, b, b, b, pp, b, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_sim3_bank(None, 1, b, b, b, b, pp, b, b, b, b, b) == FPC_E_INVALID


def test_sim3_kernels_keep_their_lds_and_stay_out_of_scratch(code_object):  # noqa: F811
    """The four kernels of csrc/sim3_ransac.h in the built code object: nothing in scratch, no spills, the LDS sizes DESIGN.md
    section 7 records -- the score kernel's is the 1 024-record stage alone -- and registers that leave the score kernel its
    four waves per SIMD."""
    funcs, meta = code_object
    for name, lds in SIM3_KERNELS.items():
        assert name in meta, name
        m = meta[name]
        print(name, m)
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == lds, (name, m)
        assert not any(i.startswith("scratch_") for _, i in funcs[name]), name
    assert meta["_Z17sim3_score_kernel8Sim3Args"]["vgpr_count"] <= 128


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_sampler_is_distinct_reproducible_and_keyed():
    idx, ok = all_samples(7, 3, 64, 40)
    assert ok.all() and all(len(set(row)) == SAMPLE for row in idx.tolist()) and idx.max() < 40
    again, _ = all_samples(7, 3, 64, 40)
    np.testing.assert_array_equal(idx, again)
    assert (all_samples(8, 3, 64, 40)[0] != idx).any() and (all_samples(7, 4, 64, 40)[0] != idx).any()
    idx3, ok3 = all_samples(7, 0, 256, 3)                           # three pairs: a sample is a permutation of all of them
    assert ok3.any() and all(sorted(row) == [0, 1, 2] for row in idx3[ok3].tolist())
    assert not all_samples(7, 0, 16, 2)[1].any()
    # the index uses DRAWS = 16: the first draw of hypothesis t is mix(seed ^ mix((f * 4096 + t) * 16)) % M
    with np.errstate(over="ignore"):
        want = mix(np.uint32(7) ^ mix(np.uint32((3 * 4096 + 5) * 16))) % np.uint32(40)
    assert idx[5, 0] == want


def _exact_triples(i):
    rng = np.random.default_rng(40 + i)
    p = rng.uniform(-3, 3, (3, 3)) + np.array([0, 0, 8.0])
    r0 = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(5, 30)))
    s0, t0 = float(rng.uniform(0.5, 2.0)), rng.normal(size=3) * 4
    return s0 * (p @ r0.T) + t0, p, s0, r0, t0


def test_noise_free_triples_are_recovered():
    for i in range(8):
        q, p, s0, r0, t0 = _exact_triples(i)
        s, r, t, ok = solve3(q[None], p[None])
        assert ok[0]
        assert abs(s[0] / s0 - 1) < 1e-12 and np.abs(r[0] - r0).max() < 1e-12 and np.abs(t[0] - t0).max() < 1e-11 * 8
        assert abs(np.linalg.det(r[0]) - 1.0) < 1e-12
        s1, r1, t1, ok1 = solve3(q[None], p[None], fix_scale=1)
        assert ok1[0] and s1[0] == 1.0
        np.testing.assert_allclose(r1[0], r0, atol=1e-12)


def test_horn_equals_the_triad_on_three_points():
    for i in range(8):
        q, p, s0, r0, t0 = _exact_triples(i)
        s, r, t = horn(q, p, rounded=False)
        st, rt, tt, ok = solve3(q[None], p[None])
        assert ok[0] and abs(s / st[0] - 1) < 1e-9
        np.testing.assert_allclose(r, rt[0], atol=1e-9)
        np.testing.assert_allclose(t, tt[0], atol=1e-8)
        assert horn(q, p, fix_scale=1)[0] == 1.0
    # ... and on many exact pairs Horn recovers the planted similarity
    rng = np.random.default_rng(3)
    p = rng.uniform(-3, 3, (50, 3)) + np.array([0, 0, 8.0])
    _, _, s0, r0, t0 = _exact_triples(1)
    s, r, t = horn(s0 * (p @ r0.T) + t0, p, rounded=False)
    assert abs(s / s0 - 1) < 1e-12 and np.abs(r - r0).max() < 1e-12 and np.abs(t - t0).max() < 1e-10


def test_collinear_samples_and_collinear_inliers():
    line = np.array([[0.0, 0, 5], [1, 0.5, 6], [2, 1.0, 7]])
    other = np.array([[0.0, 0, 5], [1, 0.5, 6], [0, 1.0, 7]])
    assert not solve3(line[None], other[None])[3][0] and not solve3(other[None], line[None])[3][0]
    assert not solve3(np.repeat(line[:1], 3, 0)[None], other[None])[3][0]           # three equal points
    assert solve3(other[None], other[None])[3][0]
    assert not solve3(np.where(np.eye(3, dtype=bool), np.nan, other)[None], other[None])[3][0]
    # Horn over collinear pairs: the rotation about the line is free, lambda0 = lambda1
    u = np.linspace(0, 4, 30)[:, None]
    pl = np.array([0.5, -0.2, 6.0]) + u * np.array([0.6, 0.3, 0.5])
    _, _, s0, r0, t0 = _exact_triples(2)
    assert horn(s0 * (pl @ r0.T) + t0, pl) is None
    assert horn(pl[:2], pl[:2]) is None and horn(np.repeat(pl[:1], 5, 0), pl[:5]) is None
    # a scene whose pairs all lie on one line but for one point 1e-6 of its length off it: a sample with that point is not
    # degenerate (sin^2 ~ 1e-11 > 1e-12) and every pair is its inlier; the first refit is singular (the gap is that one
    # point's 1e-11 shared among 30 pairs: below 1e-12 of the spread), the model stays the best sample's and the refits end
    ps = np.concatenate([pl, pl[10:11] + 5e-6 * np.array([0.3, -0.6, 0.0])])
    qs = s0 * (ps @ r0.T) + t0
    res = sim3_rule(qs, ps, dict(PARAMS, iterations=256), 0)
    assert not res.failed and res.ninliers == len(ps)
    assert res.trace == (("singular", len(ps)),)
    assert res.s == res.first[0] and (res.R == res.first[1]).all() and (res.t == res.first[2]).all()
    # the line alone, as fp32 rounds it: a few samples of neighbouring points pass the degeneracy test on their rounding
    # errors; the refit is singular all the same
    res = sim3_rule(s0 * (pl @ r0.T) + t0, pl, dict(PARAMS, iterations=256), 0)
    assert res.failed or res.trace == (("singular", res.ninliers),)
    # exactly collinear in fp32 (quarter-integer coordinates, q = 2 p + (1, 2, 3)): every sample is degenerate, the frame fails
    pe = np.arange(30)[:, None] * np.array([0.25, 0.5, 0.25]) + np.array([0.0, -2.0, 6.0])
    assert sim3_rule(2.0 * pe + np.array([1.0, 2.0, 3.0]), pe, dict(PARAMS, iterations=256), 0).failed


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_restatement_recovers_planted_similarities(rho, iterations):
    scenes, results = restated_batch(rho, iterations)
    worst, late = np.zeros(3), np.zeros(3)
    for f, (scene, res) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not res.failed, (rho, f, m)
        errs = check_planted(res.s, res.R, res.t, res.mask, scene, (rho, f, m))
        worst = np.maximum(worst, errs)
        if m >= 40:
            late = np.maximum(late, errs)
        assert res.ninliers == res.mask.sum() >= PARAMS["min_inliers"]
        assert res.near.sum() <= NEAR_CAP * m, (rho, f, res.near.sum())            # the GPU test's cap holds here
        # the guard: the returned count is never below the best sample's
        assert res.ninliers >= inliers_of(res.first, scene[0], scene[1], KVEC, KVEC, 3.0).sum()
        print("rho %.1f frame %2d M %4d: rotation %.4f deg, scale %.3e, translation %.3e, %d inliers of %d planted, trace %s"
              % (rho, f, m, *errs, res.ninliers, scene[2].sum(), res.trace))
    print("rho %.1f: worst rotation %.4f deg, scale %.3e, translation %.3e; from M = 40 on %.4f deg, %.3e, %.3e"
          % (rho, *worst, *late))


def test_restatement_failure_rules():
    q, p, _, _, _, _ = planted_scene(0, 0.0, 40)
    params = dict(PARAMS, iterations=256)
    assert sim3_rule(q[:2], p[:2], params, 0).failed                                 # fewer than 3 pairs
    res = sim3_rule(q, p, dict(params, min_inliers=41), 0)                           # inliers end below min_inliers
    assert res.failed and res.s == 0 and not res.R.any() and not res.t.any() and res.ninliers == 0 and not res.mask.any()
    assert not sim3_rule(q, p, dict(params, min_inliers=3), 0).failed
    assert sim3_rule(np.repeat(q[:1], 50, 0), np.repeat(p[:1], 50, 0), params, 0).failed     # one pair repeated
    # a pair with a non-finite coordinate is a pair, and never an inlier
    bad = q.copy()
    bad[3, 1], bad[9, 2] = np.nan, np.inf
    res = sim3_rule(bad, p, params, 0)
    assert not res.failed and not res.mask[[3, 9]].any() and res.ninliers >= 30
    # points behind either camera are never inliers: the mirror images of the first ten pairs, appended
    res = sim3_rule(np.concatenate([q, -q[:10]]), np.concatenate([p, -p[:10]]), params, 0)
    assert not res.failed and not res.mask[40:].any()


def test_fix_scale_returns_exactly_one():
    q, p, _, s0, r0, t0 = planted_scene(1, 0.0, 200)
    rigid = (q / np.float32(s0)).astype(np.float32)                                  # both sets at one scale
    res = sim3_rule(rigid, p, dict(PARAMS, iterations=256, fix_scale=1), 0)
    assert not res.failed and res.s == 1.0 and res.first[0] == 1.0
    rot, _, tr = sim3_errors(1.0, res.R, res.t * s0, (None, None, None, 1.0, r0, t0))
    assert rot <= ROT_BAR and tr <= TRANS_BAR
    free = sim3_rule(rigid, p, dict(PARAMS, iterations=256), 0)
    assert free.s != 1.0 and abs(free.s - 1.0) <= SCALE_BAR


# Found by a search over seeds at a relative depth error of 1 %, where a least-squares fit over the inliers loses pairs the
# best sample had about as often as not: scene (i, M) whose first refit the guard refuses.
GUARD_SCENE = (4, 200)
GUARD_SIGMA = 0.01


def test_the_guard_fires_on_a_planted_case_and_never_lowers_the_count():
    i, m = GUARD_SCENE
    q, p, _, _, _, _ = planted_scene(i, 0.0, m, sigma=GUARD_SIGMA)
    params = dict(PARAMS, iterations=256)
    res = sim3_rule(q, p, params, 0)
    free = sim3_rule(q, p, params, 0, guard=False)
    assert any(step[0] == "refused" for step in res.trace), res.trace
    refused = [step for step in res.trace if step[0] == "refused"][0]
    assert refused[2] < refused[1] == res.ninliers
    assert free.ninliers < res.ninliers, (free.ninliers, res.ninliers)               # what the guard is for
    assert res.ninliers >= inliers_of(res.first, q, p, KVEC, KVEC, 3.0).sum()
    for j in range(6):                                                               # never below the best sample's count
        q, p, _, _, _, _ = planted_scene(j, 0.3, 100, sigma=GUARD_SIGMA)
        r2 = sim3_rule(q, p, params, j)
        if not r2.failed:
            assert r2.ninliers >= inliers_of(r2.first, q, p, KVEC, KVEC, 3.0).sum()
            counts = [step[1] for step in r2.trace if step[0] != "singular"]
            assert counts == sorted(counts)
