"""CPU checks of the two-view bundle adjustment (fpc_refine_pose / fpc_refine_pose_frames / fpc_refine_pose_bank): the header
declares it, the binding binds it, the built library exports it -- and this file's float64 restatement of the rule of
include/fpc.h (`refine_rule`: the members by midpoint triangulation, the cost from the fp32 state, the gauge basis, the
per-member blocks, Marquardt's damping, the Schur complement down to 5 x 5, the step, accept / reject), which the GPU tests
(test_gpu_refine_pose.py) hold the kernel to, never raises the cost, halves the direction error the linear pose leaves on
the scenes with outliers, and reaches the fp32 floor on exact pairs."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import KINDS, _rotation
from tests.test_pose_epipolar import (EXACT, KVEC, PARALLEL, ROUNDED_SETS, THR, kmat, normalised, pose_errors, pose_scene,
                                      restated_poses, triangulate)
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_refine_pose", "fpc_refine_pose_frames", "fpc_refine_pose_bank")
SINGULAR, TMIN, STOP, LAMBDA_MIN, LAMBDA_MAX = 1e-14, 1e-12, 1e-6, 1e-10, 1e6         # include/fpc.h
KERNEL = "_Z18refine_pose_kernel6HfArgs10RefineArgsPKfS2_PfS3_PiS3_PhS3_i"


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def reprojects(k, px, y, thr):
    """The PnP inlier test of include/fpc.h for the points y [M,3] of a camera's frame against the pixels px [M,2] -> (passes
    [M], the margin e^2 - thr^2 c^2 relative to thr^2 c^2)."""
    fx, fy, cx, cy = k
    ex = fx * y[:, 0] - (px[:, 0] - cx) * y[:, 2]
    ey = fy * y[:, 1] - (px[:, 1] - cy) * y[:, 2]
    e2, lim = ex * ex + ey * ey, thr * thr * y[:, 2] * y[:, 2]
    with np.errstate(all="ignore"):
        return (y[:, 2] > 0) & (e2 < lim), np.abs(e2 - lim) / lim


def project(k, y):
    fx, fy, cx, cy = k
    return np.stack([fx * y[:, 0] / y[:, 2] + cx, fy * y[:, 1] / y[:, 2] + cy], 1)


def cost(r, t, x, src, dst, kq, kt):
    """C of the state (R, t, X [m,3]) over the members' pixels; +inf with a depth that is not > 0."""
    xc = x @ r.T + t
    with np.errstate(all="ignore"):
        if not ((x[:, 2] > 0).all() and (xc[:, 2] > 0).all()):
            return np.inf
        return float((((project(kq, x) - src) ** 2).sum(1) + ((project(kt, xc) - dst) ** 2).sum(1)).sum())


def gauge(t):
    k = int(np.argmin(np.abs(t)))                                     # ties: the lowest index
    b1 = np.cross(t, np.eye(3)[k])
    b1 = b1 / np.sqrt(b1 @ b1)
    b2 = np.cross(t, b1)
    return np.stack([b1, b2 / np.sqrt(b2 @ b2)], 1)                  # [3,2]


def jac(k, y):
    """J_p(Y) [m,2,3]."""
    fx, fy = k[0], k[1]
    j = np.zeros((len(y), 2, 3))
    j[:, 0, 0], j[:, 0, 2] = fx / y[:, 2], -fx * y[:, 0] / y[:, 2] ** 2
    j[:, 1, 1], j[:, 1, 2] = fy / y[:, 2], -fy * y[:, 1] / y[:, 2] ** 2
    return j


def skew(y):
    s = np.zeros((len(y), 3, 3))
    s[:, 0, 1], s[:, 0, 2], s[:, 1, 0], s[:, 1, 2], s[:, 2, 0], s[:, 2, 1] = -y[:, 2], y[:, 1], y[:, 2], -y[:, 0], -y[:, 1], y[:, 0]
    return s


def adjugate_inverse(u):
    """[m,3,3] symmetric -> (adj / det [m,3,3], det [m])."""
    c = np.empty_like(u)
    c[:, 0, 0] = u[:, 1, 1] * u[:, 2, 2] - u[:, 1, 2] * u[:, 1, 2]
    c[:, 0, 1] = c[:, 1, 0] = u[:, 0, 2] * u[:, 1, 2] - u[:, 0, 1] * u[:, 2, 2]
    c[:, 0, 2] = c[:, 2, 0] = u[:, 0, 1] * u[:, 1, 2] - u[:, 0, 2] * u[:, 1, 1]
    c[:, 1, 1] = u[:, 0, 0] * u[:, 2, 2] - u[:, 0, 2] * u[:, 0, 2]
    c[:, 1, 2] = c[:, 2, 1] = u[:, 0, 1] * u[:, 0, 2] - u[:, 0, 0] * u[:, 1, 2]
    c[:, 2, 2] = u[:, 0, 0] * u[:, 1, 1] - u[:, 0, 1] * u[:, 0, 1]
    det = u[:, 0, 0] * c[:, 0, 0] + u[:, 0, 1] * c[:, 0, 1] + u[:, 0, 2] * c[:, 0, 2]
    with np.errstate(all="ignore"):
        return c / det[:, None, None], det


def solve_pivoting(s, b, tiny):
    """Gaussian elimination with partial pivoting of S x = b (the first largest pivot); None: a pivot at or below `tiny`."""
    n = len(b)
    m = np.concatenate([s, b[:, None]], 1).astype(np.float64)
    for c in range(n):
        pr = c + int(np.argmax(np.abs(m[c:, c])))
        if not abs(m[pr, c]) > tiny:
            return None
        if pr != c:
            m[[c, pr]] = m[[pr, c]]
        for i in range(c + 1, n):
            m[i, c:] -= (m[i, c] / m[c, c]) * m[c, c:]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (m[i, n] - m[i, i + 1:n] @ x[i + 1:]) / m[i, i]
    return x


def exp_so3(w):
    """E of the PnP refit."""
    th2 = float(w @ w)
    a, b = 1.0, 0.5
    if not th2 < 1e-16:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * wx + b * (np.outer(w, w) - th2 * np.eye(3))


class Refined:
    """The outputs of the rule for one frame, the path it took, and what the device comparison needs to know."""

    def __init__(self, m):
        self.R, self.t, self.nfront = np.zeros((3, 3)), np.zeros(3), 0
        self.xyz, self.front, self.stats = np.zeros((m, 3)), np.zeros(m, bool), np.zeros(4)
        self.member = np.zeros(m, bool)
        self.near = np.zeros(m, bool)      # pairs within 1e-9 relative of a membership threshold
        self.edge = np.zeros(m, bool)      # members within 0.1 px of the threshold in the final front test
        self.costs, self.path, self.lambdas = [], [], []   # C at the start and behind every attempt; accepted?; lambda used

    @property
    def failed(self):
        return not (self.R.any() or self.t.any() or self.nfront or self.xyz.any() or self.front.any() or self.stats.any())


def refine_rule(src, dst, r_in, t_in, k_query=KVEC, k_train=KVEC, thr=3.0, min_parallax_deg=1.0, iterations=8, lambda0=1e-3,
                min_front=8):
    """include/fpc.h's rule for one frame in float64: src, dst [M,2], the input pose (rounded to fp32 here) -> Refined."""
    src, dst = f32(src).reshape(-1, 2), f32(dst).reshape(-1, 2)
    r, t = f32(r_in).reshape(3, 3), f32(t_in).reshape(3)
    out = Refined(len(src))
    thr, lam = float(np.float32(thr)), float(np.float32(lambda0))
    with np.errstate(all="ignore"):
        tlen = np.sqrt(t @ t)
    if not r.any() or not np.isfinite(r).all() or not np.isfinite(t).all() or not tlen > 0 or len(src) == 0:
        return out
    t = f32(t / tlen)
    kq, kt = tuple(float(np.float32(v)) for v in k_query), tuple(float(np.float32(v)) for v in k_train)
    # ---- the members ----
    ph, qh = normalised(src, kq), normalised(dst, kt)
    front, la, mu = triangulate(r, t, ph, qh)
    a = ph @ r.T
    aa, bb, ab = (a * a).sum(1), (qh * qh).sum(1), (a * qh).sum(1)
    det = aa * bb - ab * ab
    deg = float(np.float32(min_parallax_deg))
    par = np.sin(deg * (3.14159265358979323846 / 180.0)) ** 2 if deg > 0 else PARALLEL
    with np.errstate(all="ignore"):
        x = 0.5 * (la[:, None] * ph + (mu[:, None] * qh - t) @ r)
        x = np.where(np.isfinite(x), x, 0.0)
        pq, mq = reprojects(kq, src, x, thr)
        pt, mt = reprojects(kt, dst, x @ r.T + t, thr)
        xs = f32(x)
        member = front & (det > par * aa * bb) & pq & pt & (xs[:, 2] > 0)
        scale = max(np.abs(la[np.isfinite(la)]).max(initial=0.0), np.abs(mu[np.isfinite(mu)]).max(initial=0.0))
        out.near = (np.abs(det - par * aa * bb) <= 1e-9 * par * aa * bb) | (np.abs(la) <= 1e-9 * scale) | \
                   (np.abs(mu) <= 1e-9 * scale) | (mq <= 1e-9) | (mt <= 1e-9)
    out.member = member
    m = int(member.sum())
    if m < min_front:
        return out
    p, q, xs = src[member], dst[member], xs[member]
    c = c0 = cost(r, t, xs, p, q, kq, kt)
    out.costs.append(c)
    made = accepted = 0
    for _ in range(iterations):
        made += 1
        out.lambdas.append(lam)
        step = _attempt(r, t, xs, p, q, kq, kt, lam)
        cn = cost(*step, p, q, kq, kt) if step is not None else np.inf
        if step is not None and cn < c:
            gain, before = c - cn, c
            (r, t, xs), c = step, cn
            accepted += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            out.path.append(True)
            out.costs.append(c)
            if gain <= STOP * before:
                break
        else:
            lam = min(10.0 * lam, LAMBDA_MAX)
            out.path.append(False)
            out.costs.append(c)
    # ---- the result ----
    xc = xs @ r.T + t
    pq, _ = reprojects(kq, p, xs, thr)
    pt, _ = reprojects(kt, q, xc, thr)
    keep = pq & pt
    with np.errstate(all="ignore"):
        eq = np.sqrt(((project(kq, xs) - p) ** 2).sum(1))
        et = np.sqrt(((project(kt, xc) - q) ** 2).sum(1))
    out.edge[np.flatnonzero(member)] = (np.abs(eq - thr) <= 0.1) | (np.abs(et - thr) <= 0.1)
    if keep.sum() < min_front:
        return out
    out.R, out.t, out.nfront = r, t, int(keep.sum())
    idx = np.flatnonzero(member)[keep]
    out.front[idx] = True
    out.xyz[idx] = xs[keep]
    out.stats = np.array([np.sqrt(c0 / (2.0 * m)), np.sqrt(c / (2.0 * m)), made, accepted])
    return out


def _attempt(r, t, x, p, q, kq, kt, lam):
    """One attempt at the state (R, t, X) -> the stepped state (R', t', X'), rounded to fp32, or None: rejected."""
    b = gauge(t)
    xc = x @ r.T + t
    rq, rt = project(kq, x) - p, project(kt, xc) - q
    jq, jp = jac(kq, x), jac(kt, xc)
    jt = jp @ r
    jc = np.concatenate([-jp @ skew(xc), jp @ b], 2)                                 # [m,2,5]
    u = np.einsum("mki,mkj->mij", jq, jq) + np.einsum("mki,mkj->mij", jt, jt)
    w = np.einsum("mki,mkj->mij", jc, jt)                                            # [m,5,3]
    gx = np.einsum("mki,mk->mi", jq, rq) + np.einsum("mki,mk->mi", jt, rt)
    us = u + lam * u * np.eye(3)
    ui, det = adjugate_inverse(us)
    if not (np.isfinite(det).all() and (det > 0).all()):
        return None
    aa = np.einsum("mki,mkj->ij", jc, jc)
    gc = np.einsum("mki,mk->i", jc, rt)
    y = w @ ui                                                                       # W U*^-1
    s = aa + lam * aa * np.eye(5) - np.einsum("mik,mjk->ij", y, w)
    rhs = gc - np.einsum("mik,mk->i", y, gx)
    if not np.isfinite(s).all() or not np.isfinite(rhs).all():
        return None
    d = solve_pivoting(s, -rhs, SINGULAR * np.abs(np.diag(s)).max())
    if d is None:
        return None
    e = exp_so3(d[:3])
    rn = e @ r
    tn = e @ t + b @ d[3:]
    n = np.sqrt(tn @ tn)
    if not n > TMIN:
        return None
    sc = 1.0 / n
    dx = -np.einsum("mij,mj->mi", ui, gx + np.einsum("mij,i->mj", w, d))
    with np.errstate(all="ignore"):
        return f32(rn), f32(sc * tn), f32(sc * (x + dx))


# ---- shared with the GPU tests ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refined_poses(rho, iterations):
    """(scenes, the restated linear poses, [Refined]) of one rounded case set: the refinement starts from restated_poses' R, t
    (rounded to fp32, as the device returns them) with the threshold their F was estimated with.  Computed once."""
    scenes, _, poses = restated_poses(rho, iterations)
    return scenes, poses, [refine_rule(s[0], s[1], po.R, po.t, thr=THR) for s, po in zip(scenes, poses)]


def turned_start(r, t):
    """The planted pose turned 0.3 degrees in R and 2 degrees in t, about axes orthogonal to t."""
    d = t / np.linalg.norm(t)
    axis = np.cross(d, np.eye(3)[int(np.argmin(np.abs(d)))])
    return _rotation(axis, np.deg2rad(0.3)) @ r, _rotation(np.cross(d, axis), np.deg2rad(2.0)) @ d


# Planted-truth bars of the refined pose on the integer-rounded scenes, for restatement and device alike: twice the worst
# value of the restatement over the 28 scenes, rounded up.  Measured worst values per kind of motion, general / sideways /
# forward (test_pose_epipolar.py has the linear pose's in the same layout):
#                                    outlier share 0.0              outlier share 0.3
#   rotation angle error (deg)       0.0978 / 0.0000 / 0.0000       0.2761 / 0.0396 / 0.0198       -> bar 0.6
#   angle between t and truth (deg)  0.2067 / 0.0000 / 0.1235       3.4693 / 0.7003 / 0.1667       -> bar 7.0
#   median relative depth error      0.0195 / 0.0066 / 0.0107       0.0576 / 0.0090 / 0.0110       -> bar 0.12
# Mean direction error over the 14 scenes: 0.089 -> 0.089 deg without outliers (the level of the pixel rounding), 1.257 ->
# 0.618 deg with them (a share of 0.49); worst 5.06 -> 3.47 deg, the general scene with the shortest translation; the
# scenes at 2.02 and 1.75 deg end at 0.00 and 0.06 deg.  Rms reprojection error 0.20 - 0.23 -> 0.20 - 0.21 px without
# outliers.  On the seven EXACT scenes the final rms is 7.2e-6 .. 1.0e-5 px: the fp32 floor of the state.
ROT_BAR, DIR_BAR, DEPTH_BAR = 0.6, 7.0, 0.12
MEAN_DIRECTION_SHARE = 0.75          # outlier set: mean direction error after <= this share of the mean before


def check_refined_pose(r, t, nfront, xyz, front, stats, scene, tag):
    """The planted-truth conditions of one rounded scene, for restatement and device alike -> its three errors."""
    rot, direction, depth, _ = pose_errors(r, t, xyz, front, scene)
    assert nfront == front.sum() and nfront >= 8, (tag, nfront)
    assert rot <= ROT_BAR, (tag, rot)
    assert direction <= DIR_BAR, (tag, direction)
    assert depth <= DEPTH_BAR, (tag, depth)
    assert abs(np.linalg.det(np.asarray(r, np.float64)) - 1.0) < 1e-5 and abs(np.linalg.norm(t) - 1.0) < 1e-5, tag
    assert stats[1] <= stats[0] and 1 <= stats[3] <= stats[2] <= 8, (tag, stats)
    return rot, direction, depth


def exact_case(kind, i):
    """Unrounded pixels cast to fp32 and the turned start of one EXACT scene -> (src, dst, R_start, t_start, scene)."""
    scene = pose_scene(kind, i, 0.0)
    _, _, _, a, b, r, t, _ = scene
    return a.astype(np.float32), b.astype(np.float32), *turned_start(r, t), scene


def check_exact(r, t, stats, scene, tag):
    """Final rms <= 1e-4 px (the fp32 state resolves 1e-5), rotation and direction within 0.05 degrees (arccos near 1 resolves
    no better)."""
    rot, direction, _, _ = pose_errors(r, t, np.zeros((len(scene[0]), 3)), np.zeros(len(scene[0]), bool), scene)
    assert stats[1] <= 1e-4, (tag, stats)
    assert rot <= 0.05 and direction <= 0.05, (tag, rot, direction)
    return rot, direction


# ---- tests ------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_header_binding_and_library_agree():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NAMES + ("fpc_default_refine_params",):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) | {"fpc_default_refine_params"} <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    # argument for argument the pose calls, with (R_in_dev, t_in_dev, params) where their (F_dev, params) stand, and stats
    twins = ("fpc_pose_fundamental", "fpc_pose_frames", "fpc_pose_bank")
    tail = "const float* R_in_dev, const float* t_in_dev, const fpc_refine_params* params, float* R_dev, float* t_dev, " \
           "int32_t* nfront_dev, float* xyz_dev, uint8_t* front_dev, float* stats_dev"
    for name, twin in zip(NAMES, twins):
        args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % n, code, flags=re.S).group(1)) for n in (name, twin)]
        shared = args[1].split("const float* F_dev")[0]
        assert args[0] == shared + tail, name
        nshared = len(shared.rstrip(", ").split(","))
        assert getattr(lib, name).argtypes[:nshared] == getattr(lib, twin).argtypes[:nshared], name
        assert len(getattr(lib, name).argtypes) == nshared + 9
    body = re.search(r"typedef struct fpc_refine_params \{(.*?)\} fpc_refine_params;", code, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(float|int)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_float if typ == "float" else ctypes.c_int) for n in names.split(",")]
    assert fields == list(_lib.FpcRefineParams._fields_)
    p = _lib.FpcRefineParams()
    assert lib.fpc_default_refine_params(ctypes.byref(p)) == 0
    assert [getattr(p, n) for n, _ in fields] == [500.0, 500.0, 320.0, 240.0, 500.0, 500.0, 320.0, 240.0, 3.0, 1.0, 8,
                                                   float(np.float32(1e-3)), 8]
    # the constants of the rule are part of the contract: the header states the ones this file restates
    for const in ("1e-14 of the largest diagonal entry", "|t'| not > 1e-12", "max(lambda / 10, 1e-10)", "min(10 lambda, 1e6)",
                  "C - C' <= 1e-6 C", "accepted iff C' < C", "sqrt(C / (2 m))", "X_train = R X_query + t",
                  "bundle adjustment over more than two views"):
        assert const in hdr, const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4
    assert lib.fpc_abi_version() == 4


def test_null_arguments():
    lib = _lib.load()
    p = _lib.FpcRefineParams()
    assert lib.fpc_default_refine_params(None) == FPC_E_INVALID
    assert lib.fpc_default_refine_params(ctypes.byref(p)) == 0
    buf = np.zeros(64, np.float32)
    d = buf.ctypes.data
    assert lib.fpc_refine_pose(None, 1, d, d, d, 8, d, d, ctypes.byref(p), d, d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_refine_pose_frames(None, 1, 0, d, d, d, d, d, ctypes.byref(p), d, d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_refine_pose_bank(None, 1, d, d, d, d, ctypes.byref(p), d, d, d, d, None, None) == FPC_E_INVALID


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_rounded_scenes_never_rise_and_meet_the_planted_truth_bars(rho, iterations):
    scenes, poses, refined = refined_poses(rho, iterations)
    worst, before, after = {}, [], []
    for f, (scene, po, got) in enumerate(zip(scenes, poses, refined)):
        tag = (KINDS[f], f, rho)
        assert not got.failed, tag
        assert all(b <= a for a, b in zip(got.costs, got.costs[1:])), (tag, got.costs)      # C never rises
        assert all((b < a) == acc for a, b, acc in zip(got.costs, got.costs[1:], got.path)), tag
        assert got.stats[2] == len(got.path) and got.stats[3] == sum(got.path), tag
        m = got.member.sum()
        assert np.isclose(got.stats[0], np.sqrt(got.costs[0] / (2 * m))) and np.isclose(got.stats[1], np.sqrt(got.costs[-1] / (2 * m)))
        assert not got.front[~got.member].any() and not got.xyz[~got.front].any() and (got.xyz[got.front, 2] > 0).all()
        errs = check_refined_pose(got.R, got.t, got.nfront, got.xyz, got.front, got.stats, scene, tag)
        worst[KINDS[f]] = tuple(max(x, y) for x, y in zip(worst.get(KINDS[f], (0.0, 0.0, 0.0)), errs))
        before.append(pose_errors(po.R, po.t, po.xyz, po.front, scene)[1])
        after.append(errs[1])
        print("rho %.1f frame %2d %-8s: direction %.4f -> %.4f deg, rms %.4f -> %.4f px, %d attempts, %d accepted, %d members"
              % (rho, f, KINDS[f], before[-1], after[-1], got.stats[0], got.stats[1], got.stats[2], got.stats[3], m))
    for kind, (rot, direction, depth) in worst.items():
        print("rho %.1f %-8s: worst rotation error %.4f deg, direction error %.4f deg, median relative depth error %.5f"
              % (rho, kind, rot, direction, depth))
    print("rho %.1f: mean direction error %.4f -> %.4f deg, worst %.4f -> %.4f deg"
          % (rho, np.mean(before), np.mean(after), max(before), max(after)))
    if rho > 0:                                                                      # the point of the feature
        assert np.mean(after) <= MEAN_DIRECTION_SHARE * np.mean(before), (np.mean(before), np.mean(after))


@pytest.mark.parametrize("kind,i", EXACT)
def test_exact_pairs_reach_the_fp32_floor(kind, i):
    src, dst, r0, t0, scene = exact_case(kind, i)
    got = refine_rule(src, dst, r0, t0, thr=8.0, iterations=8)
    assert not got.failed and got.nfront >= 500, got.nfront
    rot, direction = check_exact(got.R, got.t, got.stats, scene, (kind, i))
    print("%-8s %d: rms %.3e -> %.3e px, rotation %.4f deg, direction %.4f deg, %d attempts, %d accepted, %d members"
          % (kind, i, got.stats[0], got.stats[1], rot, direction, got.stats[2], got.stats[3], got.member.sum()))


def test_failure_rules():
    src, dst, r0, t0, scene = exact_case("general", 0)
    good = refine_rule(src, dst, r0, t0, thr=8.0)
    assert not good.failed
    assert refine_rule(src, dst, np.zeros((3, 3)), t0, thr=8.0).failed                # a failed frame of the pose calls
    bad = t0.copy()
    bad[1] = np.nan
    assert refine_rule(src, dst, r0, bad, thr=8.0).failed
    bad = r0.copy()
    bad[2, 0] = np.inf
    assert refine_rule(src, dst, bad, t0, thr=8.0).failed
    assert refine_rule(src, dst, r0, np.zeros(3), thr=8.0).failed                     # |t| = 0
    assert refine_rule(src[:0], dst[:0], r0, t0, thr=8.0).failed
    # fewer members than min_front
    few = refine_rule(src[:20], dst[:20], r0, t0, thr=8.0, min_front=1)
    assert 8 <= few.nfront == few.member.sum() <= 20
    assert refine_rule(src[:20], dst[:20], r0, t0, thr=8.0, min_front=few.nfront).nfront == few.nfront
    assert refine_rule(src[:20], dst[:20], r0, t0, thr=8.0, min_front=few.nfront + 1).failed
    # the scale of t_in does not matter
    twice = refine_rule(src, dst, r0, 2.0 * t0, thr=8.0)
    assert np.array_equal(twice.R, good.R) and np.array_equal(twice.xyz, good.xyz)
    # iterations = 1: one attempt
    one = refine_rule(src, dst, r0, t0, thr=8.0, iterations=1)
    assert one.stats[2] == 1 and one.stats[3] == 1 and one.costs[1] < one.costs[0]
    # lambda at its upper clamp: under a damping of 1e30 the step is below what the fp32 state resolves, C' = C, the attempt
    # is rejected, and 10 lambda is clamped to 1e6
    scenes, poses, _ = refined_poses(*ROUNDED_SETS[0])
    s, po = scenes[0], poses[0]
    heavy = refine_rule(s[0], s[1], po.R, po.t, thr=THR, lambda0=1e30, iterations=2)
    assert not heavy.path[0] and heavy.lambdas == [float(np.float32(1e30)), LAMBDA_MAX]
    # lambda at its lower clamp: accepted steps from 1e-10 stay there
    low = refine_rule(s[0], s[1], po.R, po.t, thr=THR, lambda0=1e-10)
    assert low.path[:2] == [True, True] and low.lambdas[:3] == [float(np.float32(1e-10)), LAMBDA_MIN, LAMBDA_MIN]
    assert all(b <= a for a, b in zip(low.costs, low.costs[1:]))
    # a pose turned so far that fewer than min_front pairs are members fails
    far = refine_rule(src, dst, _rotation(np.array([0.3, 1.0, 0.2]), np.deg2rad(40.0)) @ r0, t0, thr=8.0, min_front=50)
    assert far.member.sum() < 50 and far.failed


def test_a_call_without_an_accepted_attempt_returns_the_input_pose_and_its_midpoints():
    """Marquardt's steps find a gain from any start that has members at all (a pose turned 8 degrees, with 3 members left of
    600, still converges), so the start that nothing improves is made by the damping: one attempt at lambda 1e30 moves the
    state by less than fp32 resolves.  The output is the input pose, t normalised, with the members' midpoints."""
    scenes, poses, _ = refined_poses(*ROUNDED_SETS[1])
    for f in (1, 8, 12):
        s, po = scenes[f], poses[f]
        got = refine_rule(s[0], s[1], po.R, 3.0 * po.t, thr=THR, lambda0=1e30, iterations=1)
        assert got.path == [False] and list(got.stats[2:]) == [1, 0] and got.stats[0] == got.stats[1] > 0
        r, t = f32(po.R), f32(f32(3.0 * po.t) / np.linalg.norm(f32(3.0 * po.t)))
        assert np.array_equal(got.R, r) and np.array_equal(got.t, t)
        ph, qh = normalised(f32(s[0]), KVEC), normalised(f32(s[1]), KVEC)
        _, la, mu = triangulate(r, t, ph, qh)
        mid = f32(0.5 * (la[:, None] * ph + (mu[:, None] * qh - t) @ r))
        assert got.nfront == got.member.sum() == got.front.sum() > 300
        assert np.array_equal(got.xyz[got.front], mid[got.front]) and not got.xyz[~got.front].any()


def test_code_object_keeps_the_kernel_out_of_scratch(code_object):  # noqa: F811
    _, meta = code_object
    assert KERNEL in meta, [k for k in meta if "refine" in k]
    m = meta[KERNEL]
    assert m["private_segment_fixed_size"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
