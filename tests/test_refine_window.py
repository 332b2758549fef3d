"""CPU checks of the local bundle adjustment (fpc_refine_window / fpc_refine_window_frames / fpc_refine_window_bank): the
header declares it, the binding binds it, the built library exports it -- and this file's float64 restatement of the rule of
include/fpc.h (`window_rule`: live frames, membership by integer minimum, the cost from the fp32 state, the per-observation
blocks, Marquardt's damping, the Schur complement down to 6 x (kept frames), the solve, the step with the depth-sum gauge,
accept / reject), which the GPU tests (test_gpu_refine_window.py) hold the kernels to, never raises the cost, lowers the pose
and point errors of planted box scenes, and reaches the fp32 floor on exact pixels.

Measured on the restatement (the scene set of `scene_set`, 12 box scenes of 1, 2, 3, 6 frames plus two 16-frame windows per
outlier share; pixels rounded to integers; start 0.12 degrees / 1 % off):
    share 0.0, 1 - 6 frames: mean rotation error 0.1200 -> 0.0411 deg, median point error 0.0730 -> 0.0260
    share 0.3, 1 - 6 frames: mean rotation error 0.1200 -> 0.0551 deg, median point error 0.0733 -> 0.0282
    16 frames: rotation 0.1200 -> 0.0175 (share 0.3: 0.0223) deg, median point error 0.0766 -> 0.0067 (0.0720 -> 0.0091)
    rms reprojection error 0.88 - 1.56 -> 0.19 - 0.38 px, 3 - 5 accepted attempts of 4 - 8
(DESIGN.md section 7 has the table.)  n = 1 against refine_rule: see test_one_frame_minimises_the_two_view_cost."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import _rotation
from tests.test_refine_pose import adjugate_inverse, exp_so3, f32, jac, project, refine_rule, reprojects, skew
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_refine_window", "fpc_refine_window_frames", "fpc_refine_window_bank")
SINGULAR, STOP, LAMBDA_MIN, LAMBDA_MAX = 1e-14, 1e-6, 1e-10, 1e6         # include/fpc.h
MAX_FRAMES, CHUNK, NONE = 16, 64, 0x7f7f7f7f
KVEC = (500.0, 500.0, 320.0, 240.0)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def ordered_sum(terms, descending=False):
    """Sum over axis 0, one term after the other (np.cumsum is sequential), ascending or descending."""
    terms = np.asarray(terms, np.float64)
    if len(terms) == 0:
        return np.zeros(terms.shape[1:])
    return np.cumsum(terms[::-1] if descending else terms, axis=0)[-1]


def chunked_sum(terms, rows, descending=False):
    """The kernels' order: the terms of every chunk of 64 key rows one after the other, then the chunks' sums one after the
    other (terms [J, ...] of the key rows `rows`, ascending)."""
    chunks = np.unique(rows // CHUNK)
    parts = np.stack([ordered_sum(terms[rows // CHUNK == c], descending) for c in chunks]) if len(chunks) else terms[:0]
    return ordered_sum(parts, descending)


def solve_pivoting(s, b, tiny):
    """Gaussian elimination with partial pivoting of S x = b as rw_solve_kernel does it (the first largest pivot, factors
    formed with the pivot's reciprocal); None: a pivot at or below `tiny`."""
    n = len(b)
    m = np.concatenate([s, b[:, None]], 1).astype(np.float64)
    for c in range(n):
        pr = c + int(np.argmax(np.abs(m[c:, c])))
        if not abs(m[pr, c]) > tiny:
            return None
        if pr != c:
            m[[c, pr]] = m[[pr, c]]
        fct = m[c + 1:, c] * (1.0 / m[c, c])
        m[c + 1:, c + 1:] = m[c + 1:, c + 1:] - fct[:, None] * m[c, c + 1:][None, :]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        acc = m[i, n]
        for j in range(i + 1, n):
            acc = acc - m[i, j] * x[j]
        x[i] = acc / m[i, i]
    return x


class Window:
    """The outputs of the rule, the path it took, and what the device comparison needs to know."""

    def __init__(self, n, cap, stride):
        self.R, self.t, self.nobs = np.zeros((n, 3, 3)), np.zeros((n, 3)), np.zeros(n, np.int64)
        self.xyz, self.kind = np.zeros((cap, 3)), np.zeros(cap, np.uint8)
        self.obs, self.stats = np.zeros((n, stride), bool), np.zeros(4)
        self.live, self.kept = np.zeros(n, bool), np.zeros(n, bool)
        self.active = np.zeros(cap, bool)
        self.tab = np.full((n, cap), NONE, np.int64)
        self.near = False                  # an observation or landmark within 1e-9 relative of a membership threshold
        self.edge = np.zeros(cap, bool)    # active landmarks with a final test within 0.1 px of the threshold
        self.costs, self.path, self.lambdas = [], [], []
        self.failed = True


def _cost(r, t, x, act, kpix, mf, mj, mp, kq, kt, descending=False):
    """C of the state: per active landmark the key term, then its members in ascending frame order; chunked over the rows."""
    with np.errstate(all="ignore"):
        y = np.einsum("mij,mj->mi", r[mf], x[mj]) + t[mf]
        if not ((x[act, 2] > 0).all() and (y[:, 2] > 0).all()):
            return np.inf
        per = np.zeros(len(x))
        per[act] = ((project(kt, x[act]) - kpix[act]) ** 2).sum(1)
        np.add.at(per, mj, ((project(kq, y) - mp) ** 2).sum(1))
        return float(chunked_sum(per[act], act, descending))


def window_rule(xy, idx, nobs, key_xy, key_xyz, r_in, t_in, key_valid=None, nkey=None, k_query=KVEC, k_train=KVEC, thr=3.0,
                iterations=8, lambda0=1e-3, min_obs=6, cap=None, takes_part=None, descending=False):
    """include/fpc.h's rule in float64.  xy [n,S,2], idx [n,S], nobs [n]: the observations; key_xy [P,2], key_xyz [P,3],
    key_valid [P] or None, nkey (None: P): the key; the input poses (rounded to fp32 here).  takes_part [n] (None: every
    frame): the bank variant's slot test.  descending: every sum over landmarks runs the other way (the fallback margin of the
    device comparison).  -> Window."""
    xy, idx = f32(xy), np.asarray(idx, np.int64)
    n, stride = idx.shape
    key_xy, key_xyz = f32(key_xy).reshape(-1, 2), np.asarray(key_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    cap = len(key_xyz) if cap is None else cap
    nk = min(max(len(key_xyz) if nkey is None else int(nkey), 0), cap)
    r, t = f32(r_in).reshape(n, 3, 3), f32(t_in).reshape(n, 3)
    out = Window(n, cap, stride)
    thr, lam = float(np.float32(thr)), float(np.float32(lambda0))
    kq, kt = tuple(float(np.float32(v)) for v in k_query), tuple(float(np.float32(v)) for v in k_train)
    # ---- live frames, eligible landmarks ----
    live = np.array([bool(r[f].any()) and bool(np.isfinite(r[f]).all() and np.isfinite(t[f]).all()) for f in range(n)])
    if takes_part is not None:
        live &= np.asarray(takes_part, bool)
    r, t = np.where(live[:, None, None], r, 0.0), np.where(live[:, None], t, 0.0)
    valid = np.zeros(cap, bool)
    with np.errstate(all="ignore"):
        valid[:nk] = np.isfinite(key_xyz[:nk]).all(1) & (np.ones(nk, bool) if key_valid is None else np.asarray(key_valid)[:nk] != 0)
    x = np.zeros((cap, 3))
    x[valid] = key_xyz[:cap][valid]
    kpix = np.zeros((cap, 2))
    kpix[:nk] = key_xy[:nk]
    with np.errstate(all="ignore"):
        eligible, margin = reprojects(kt, kpix, x, thr)
    eligible &= valid
    out.near = bool((margin[valid] <= 1e-9).any())
    out.live = live
    # ---- membership: the lowest passing row of every (frame, landmark) ----
    tab = out.tab
    for f in np.flatnonzero(live):
        m = min(max(int(nobs[f]), 0), stride)
        j = idx[f, :m]
        rows = np.flatnonzero((j >= 0) & (j < nk))
        rows = rows[eligible[j[rows]]]
        with np.errstate(all="ignore"):
            ok, margin = reprojects(kq, xy[f, rows], x[j[rows]] @ r[f].T + t[f], thr)
        out.near |= bool((margin <= 1e-9).any())
        np.minimum.at(tab[f], j[rows[ok]], rows[ok])
    kept = live & ((tab != NONE).sum(1) >= min_obs)
    tab[~kept] = NONE
    out.kept = kept
    active = eligible & (tab != NONE).any(0)
    out.active = active
    out.xyz[valid] = x[valid]
    out.kind[valid] = 2
    if not kept.any():
        return out                                                     # failed: the map passes through as kind 2
    out.failed = False
    act = np.flatnonzero(active)
    mj, mf = np.nonzero((tab != NONE).T)                               # members, by landmark and then by frame
    mp = xy[mf, tab[mf, mj]]
    z0 = float(ordered_sum(x[act, 2], descending))
    pos = np.cumsum(kept) - 1                                          # the frame's place in the reduced system
    nkept, dim = int(kept.sum()), 6 * int(kept.sum())
    c = c0 = _cost(r, t, x, act, kpix, mf, mj, mp, kq, kt, descending)
    out.costs.append(c)
    made = accepted = 0
    for _ in range(iterations):
        made += 1
        out.lambdas.append(lam)
        step = _attempt(r, t, x, act, kpix, mf, mj, mp, kq, kt, lam, z0, kept, pos, dim, descending)
        cn = _cost(*step, act, kpix, mf, mj, mp, kq, kt, descending) if step is not None else np.inf
        if step is not None and cn < c:
            gain, before = c - cn, c
            (r, t, x), c = step, cn
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
    with np.errstate(all="ignore"):
        passes, _ = reprojects(kt, kpix[act], x[act], thr)
        ek = np.sqrt(((project(kt, x[act]) - kpix[act]) ** 2).sum(1))
        y = np.einsum("mij,mj->mi", r[mf], x[mj]) + t[mf]
        seen, _ = reprojects(kq, mp, y, thr)
        eo = np.sqrt(((project(kq, y) - mp) ** 2).sum(1))
    out.edge[act] = np.abs(ek - thr) <= 0.1
    np.logical_or.at(out.edge, mj, np.abs(eo - thr) <= 0.1)
    out.kind[act] = np.where(passes, 1, 0)
    out.xyz[act] = np.where(passes[:, None], x[act], 0.0)
    seen &= out.kind[mj] == 1
    out.obs[mf[seen], tab[mf[seen], mj[seen]]] = True
    out.nobs = np.bincount(mf[seen], minlength=n)
    out.R, out.t = np.where(kept[:, None, None], r, 0.0), np.where(kept[:, None], t, 0.0)
    count = len(mf) + len(act)
    out.stats = np.array([np.sqrt(c0 / count), np.sqrt(c / count), made, accepted])
    return out


def _attempt(r, t, x, act, kpix, mf, mj, mp, kq, kt, lam, z0, kept, pos, dim, descending):
    """One attempt at the state -> the stepped state (R', t', X'), rounded to fp32, or None: rejected."""
    na = len(act)
    row = np.full(len(x), -1)
    row[act] = np.arange(na)
    ma = row[mj]                                                       # the member's landmark among the active ones
    y = np.einsum("mij,mj->mi", r[mf], x[mj]) + t[mf]
    jp = jac(kq, y)
    jx = jp @ r[mf]                                                    # [M,2,3]
    jc = np.concatenate([-jp @ skew(y), jp], 2)                        # [M,2,6]
    res = project(kq, y) - mp
    jk = jac(kt, x[act])
    rk = project(kt, x[act]) - kpix[act]
    u = np.einsum("mki,mkj->mij", jk, jk)
    g = np.einsum("mki,mk->mi", jk, rk)
    np.add.at(u, ma, np.einsum("mki,mkj->mij", jx, jx))               # (in member order: ascending frames per landmark)
    np.add.at(g, ma, np.einsum("mki,mk->mi", jx, res))
    ui, det = adjugate_inverse(u + lam * u * np.eye(3))
    if not (np.isfinite(det).all() and (det > 0).all()):
        return None
    w = np.einsum("mki,mkj->mij", jc, jx)                              # [M,6,3]
    # per landmark, dense over the kept frames: W (stacked), J_c^T J_c (block diagonal), J_c^T r
    wd, ad, gd = np.zeros((na, dim, 3)), np.zeros((na, dim, dim)), np.zeros((na, dim))
    jcjc, jcr = np.einsum("mki,mkj->mij", jc, jc), np.einsum("mki,mk->mi", jc, res)
    for i in range(6):
        wd[ma, pos[mf] * 6 + i] = w[:, i]
        gd[ma, pos[mf] * 6 + i] = jcr[:, i]
        for k in range(6):
            ad[ma, pos[mf] * 6 + i, pos[mf] * 6 + k] = jcjc[:, i, k]
    yd = wd @ ui                                                       # W U*^-1
    s = chunked_sum(ad - np.einsum("jak,jbk->jab", yd, wd), act, descending)
    da = chunked_sum(np.einsum("jaa->ja", ad), act, descending)
    rhs = chunked_sum(gd - np.einsum("jak,jk->ja", yd, g), act, descending)
    s = s + lam * np.diag(da)
    if not np.isfinite(s).all() or not np.isfinite(rhs).all():
        return None
    d = solve_pivoting(s, -rhs, SINGULAR * np.abs(np.diag(s)).max())
    if d is None:
        return None
    rn, tn = r.copy(), t.copy()
    delta = np.zeros((len(r), 6))
    for f in np.flatnonzero(kept):
        delta[f] = d[pos[f] * 6:pos[f] * 6 + 6]
        e = exp_so3(delta[f, :3])
        rn[f], tn[f] = e @ r[f], e @ t[f] + delta[f, 3:]
    h = np.zeros((na, 3))
    np.add.at(h, ma, np.einsum("mij,mi->mj", w, delta[mf]))
    xs = x[act] - np.einsum("mij,mj->mi", ui, g + h)
    with np.errstate(all="ignore"):
        sc = z0 / float(ordered_sum(xs[:, 2], descending))
    if not (np.isfinite(sc) and sc > 0):
        return None
    xn = x.copy()
    xn[act] = f32(sc * xs)
    return f32(rn), np.where(kept[:, None], f32(sc * tn), tn), xn


# ---- planted scenes, shared with the GPU tests ------------------------------------------------------------------------------
class Scene:
    pass


def box_scene(seed, frames, share=0.0, landmarks=120, rounded=True, coplanar=False, size=(640, 480), k=KVEC, stride=None,
              depth_noise=0.02):
    """`landmarks` points at depth 3 - 8 seen from the key camera (the origin) and from `frames` cameras around it; pixels
    rounded to integers; a share of every frame's observations replaced by pixels drawn anywhere in the image (wrong
    matches); the start: every pose 0.12 degrees and 1 % in t off, every landmark 2 % (1 sigma) off along its ray."""
    rng = np.random.RandomState(seed)
    fx, fy, cx, cy = k
    px = np.stack([rng.uniform(20, size[0] - 20, landmarks), rng.uniform(20, size[1] - 20, landmarks)], 1)
    z = rng.uniform(3.0, 8.0, landmarks)
    if coplanar:
        z = 5.0 + 0.002 * (px[:, 0] - cx) + 0.001 * (px[:, 1] - cy)
    x = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
    sc = Scene()
    sc.k, sc.x_true, sc.frames = k, x, frames
    sc.key_xy = np.round(px) if rounded else px
    stride = landmarks if stride is None else stride
    sc.xy, sc.idx, sc.nobs = np.zeros((frames, stride, 2)), np.full((frames, stride), -1, np.int64), np.zeros(frames, np.int64)
    sc.r_true, sc.t_true = np.zeros((frames, 3, 3)), np.zeros((frames, 3))
    sc.r0, sc.t0 = np.zeros((frames, 3, 3)), np.zeros((frames, 3))
    sc.wrong = np.zeros((frames, stride), bool)
    for f in range(frames):
        axis = rng.normal(size=3)
        sc.r_true[f] = _rotation(axis, np.deg2rad(rng.uniform(1.0, 5.0)))
        d = rng.normal(size=3) * (1.0, 1.0, 0.4)
        sc.t_true[f] = d / np.linalg.norm(d) * rng.uniform(0.4, 0.9)
        y = x @ sc.r_true[f].T + sc.t_true[f]
        p = np.stack([fx * y[:, 0] / y[:, 2] + cx, fy * y[:, 1] / y[:, 2] + cy], 1)
        seen = np.flatnonzero((p[:, 0] >= 0) & (p[:, 0] <= size[0] - 1) & (p[:, 1] >= 0) & (p[:, 1] <= size[1] - 1))
        seen = rng.permutation(seen)[:stride]
        m = len(seen)
        wrong = rng.uniform(size=m) < share
        p = p[seen]
        p[wrong] = np.stack([rng.uniform(0, size[0] - 1, wrong.sum()), rng.uniform(0, size[1] - 1, wrong.sum())], 1)
        sc.xy[f, :m], sc.idx[f, :m], sc.nobs[f], sc.wrong[f, :m] = (np.round(p) if rounded else p), seen, m, wrong
        sc.r0[f] = _rotation(rng.normal(size=3), np.deg2rad(0.12)) @ sc.r_true[f]
        sc.t0[f] = 1.01 * sc.t_true[f]
    sc.x0 = x * (1.0 + depth_noise * rng.normal(size=landmarks))[:, None]
    return sc


def run_scene(sc, **kw):
    return window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, k_query=sc.k, k_train=sc.k, **kw)


def scene_errors(sc, r, t, xyz, kind):
    """(mean rotation error over the frames with a pose, degrees; median point error over the refined landmarks)."""
    rot = []
    for f in range(sc.frames):
        if np.asarray(r[f]).any():
            a = np.asarray(r[f], np.float64).reshape(3, 3) @ sc.r_true[f].T        # (small angles: arccos of the trace resolves 0.03 deg)
            v = 0.5 * np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]])
            rot.append(np.degrees(np.arcsin(min(1.0, float(np.linalg.norm(v))))))
    sel = np.asarray(kind) == 1
    err = np.linalg.norm(np.asarray(xyz, np.float64)[:len(sel)][sel] - sc.x_true[sel[:len(sc.x_true)]], axis=1) if sel.any() else np.zeros(1)
    return float(np.mean(rot)) if rot else 0.0, float(np.median(err))


FRAME_COUNTS = (1, 2, 3, 6)


def scene_set(share):
    """The 12 box scenes of 1, 2, 3 and 6 frames (three seeds each) and two 16-frame windows."""
    return [box_scene(100 * n + s, n, share) for n in FRAME_COUNTS for s in range(3)] + [box_scene(1600 + s, 16, share) for s in range(2)]


@functools.lru_cache(maxsize=None)
def refined_set(share):
    """(scenes, [Window]) of one outlier share, computed once (the GPU tests compare against the same objects)."""
    scenes = scene_set(share)
    return scenes, [run_scene(sc) for sc in scenes]


def check_costs(got, tag):
    assert not got.failed, tag
    assert all(b <= a for a, b in zip(got.costs, got.costs[1:])), (tag, got.costs)          # C never rises
    assert all((b < a) == acc for a, b, acc in zip(got.costs, got.costs[1:], got.path)), tag
    assert got.stats[2] == len(got.path) and got.stats[3] == sum(got.path) >= 1, (tag, got.stats)
    assert got.stats[1] < got.stats[0], (tag, got.stats)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_header_binding_and_library_agree():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    extra = ("fpc_default_window_params", "fpc_window_reserve")
    for name in NAMES + extra:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        nargs = len(re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1).split(","))
        assert len(getattr(lib, name).argtypes) == nargs, name
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES + extra) <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    # the three calls end alike: the input poses, the parameters, the seven outputs
    tail = "const float* R_in_dev, const float* t_in_dev, const fpc_window_params* params, float* R_dev, float* t_dev, " \
           "int32_t* nobs_dev, float* xyz_dev, uint8_t* kind_dev, uint8_t* obs_dev, float* stats_dev"
    for name in NAMES:
        args = re.sub(r"\s+", " ", re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1))
        assert args.endswith(tail), name
    body = re.search(r"typedef struct fpc_window_params \{(.*?)\} fpc_window_params;", code, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(float|int)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_float if typ == "float" else ctypes.c_int) for n in names.split(",")]
    assert fields == list(_lib.FpcWindowParams._fields_)
    p = _lib.FpcWindowParams()
    assert lib.fpc_default_window_params(ctypes.byref(p)) == 0
    assert [getattr(p, n) for n, _ in fields] == [500.0, 500.0, 320.0, 240.0, 500.0, 500.0, 320.0, 240.0, 3.0, 8,
                                                   float(np.float32(1e-3)), 6]
    assert int(re.search(r"#define FPC_WINDOW_MAX_FRAMES (\d+)", hdr).group(1)) == _lib.WINDOW_MAX_FRAMES == MAX_FRAMES
    for const in ("1e-14 of\n *    the largest diagonal entry", "max(lambda / 10, 1e-10)", "min(10 lambda, 1e6)", "C - C' <= 1e-6 C",
                  "accepted iff C' < C", "sqrt(C / (members + active))", "s = Z0 / sum_j X_j'[2]",
                  "larger windows (more than 16 frames)", "robust kernels", "several key frames' landmarks"):
        assert const in hdr, const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4
    assert lib.fpc_abi_version() == 4


def test_null_and_bad_arguments_are_refused():
    lib = _lib.load()
    p = _lib.FpcWindowParams()
    assert lib.fpc_default_window_params(None) == FPC_E_INVALID
    assert lib.fpc_default_window_params(ctypes.byref(p)) == 0
    assert lib.fpc_window_reserve(None, None) == FPC_E_INVALID
    buf = np.zeros(64, np.float32)
    d = buf.ctypes.data
    pp = ctypes.byref(p)
    assert lib.fpc_refine_window(None, 1, d, d, d, 8, d, d, None, d, d, d, pp, d, d, d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_refine_window_frames(None, 1, d, d, d, None, d, d, d, pp, d, d, d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_refine_window_bank(None, 1, d, None, d, d, d, pp, d, d, d, d, d, None, None) == FPC_E_INVALID


@pytest.mark.parametrize("share", (0.0, 0.3))
def test_box_scenes_never_rise_and_move_towards_the_planted_truth(share):
    scenes, refined = refined_set(share)
    before, after = [], []
    for i, (sc, got) in enumerate(zip(scenes, refined)):
        tag = (share, i, sc.frames)
        check_costs(got, tag)
        assert got.kept.all() and 3 <= got.stats[3] + 0 and got.stats[2] <= 8, (tag, got.stats)
        kind0 = np.where(got.active, 1, 0)
        b, a = scene_errors(sc, sc.r0, sc.t0, sc.x0, kind0), scene_errors(sc, got.R, got.t, got.xyz, got.kind)
        before.append(b)
        after.append(a)
        print("share %.1f scene %2d, %2d frames: rms %.3f -> %.3f px, rotation %.4f -> %.4f deg, median point error %.4f -> %.4f, "
              "%d attempts, %d accepted, %d members, %d active" % (share, i, sc.frames, got.stats[0], got.stats[1], b[0], a[0],
                                                                    b[1], a[1], got.stats[2], got.stats[3],
                                                                    (got.tab != NONE).sum(), got.active.sum()))
    before, after = np.array(before), np.array(after)
    small = slice(0, 12)
    for name, sel in (("1 - 6 frames", small), ("16 frames", slice(12, None))):
        print("share %.1f, %s: mean rotation error %.4f -> %.4f deg, mean of the median point errors %.4f -> %.4f"
              % (share, name, before[sel, 0].mean(), after[sel, 0].mean(), before[sel, 1].mean(), after[sel, 1].mean()))
    assert after[small, 0].mean() < before[small, 0].mean() and after[small, 1].mean() < before[small, 1].mean()
    assert after[12:, 0].mean() < before[12:, 0].mean() and after[12:, 1].mean() < before[12:, 1].mean()


def test_coplanar_scenes_meet_the_cost_conditions():
    for n in (1, 3, 6):
        for share in (0.0, 0.3):
            got = run_scene(box_scene(7000 + n, n, share, coplanar=True))
            check_costs(got, ("coplanar", n, share))


@pytest.mark.parametrize("frames", (1, 3, 16))
def test_exact_pixels_reach_the_fp32_floor(frames):
    sc = box_scene(4000 + frames, frames, rounded=False)
    got = run_scene(sc, thr=8.0, iterations=16)
    check_costs(got, ("exact", frames))
    rot, point = scene_errors(sc, got.R, got.t, got.xyz, got.kind)
    print("exact, %d frames: rms %.3e -> %.3e px, rotation %.5f deg, median point error %.2e, %d attempts"
          % (frames, got.stats[0], got.stats[1], rot, point, got.stats[2]))
    # the fp32 state resolves 1e-5 px at these depths and focal lengths (refine_rule's floor: 7e-6 .. 1e-5)
    assert got.stats[1] <= 1e-4, got.stats
    assert rot <= 0.05, rot


def test_failure_rules():
    sc = box_scene(11, 3)
    good = run_scene(sc)
    assert not good.failed and good.kept.all()
    # a dead frame: zeros out, the others refined as if it were not there
    r0 = sc.r0.copy()
    r0[1] = 0.0
    dead = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, r0, sc.t0)
    assert list(dead.kept) == [True, False, True] and not dead.R[1].any() and not dead.t[1].any() and dead.nobs[1] == 0
    assert not dead.obs[1].any() and dead.R[0].any()
    alone = window_rule(sc.xy[[0, 2]], sc.idx[[0, 2]], sc.nobs[[0, 2]], sc.key_xy, sc.x0, sc.r0[[0, 2]], sc.t0[[0, 2]])
    assert np.array_equal(alone.R, dead.R[[0, 2]]) and np.array_equal(alone.xyz, dead.xyz)
    bad = sc.t0.copy()
    bad[2, 1] = np.nan
    assert list(window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, bad).kept) == [True, True, False]
    # a slot mismatch is a dead frame
    other = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, takes_part=[True, False, True])
    assert np.array_equal(other.R, dead.R) and np.array_equal(other.xyz, dead.xyz)
    # a frame below min_obs is dropped
    nobs = sc.nobs.copy()
    nobs[0] = 5
    few = window_rule(sc.xy, sc.idx, nobs, sc.key_xy, sc.x0, sc.r0, sc.t0)
    assert list(few.kept) == [False, True, True] and not few.R[0].any() and few.nobs[0] == 0
    # no kept frame: the call fails and the map passes through as kind 2
    none = window_rule(sc.xy, sc.idx, np.minimum(sc.nobs, 5), sc.key_xy, sc.x0, sc.r0, sc.t0)
    assert none.failed and not none.R.any() and not none.t.any() and not none.nobs.any() and not none.stats.any()
    assert (none.kind == 2).all() and np.array_equal(none.xyz, f32(sc.x0))
    # two rows on one landmark: the lowest passing one is the observation
    xy, idx = sc.xy.copy(), sc.idx.copy()
    idx[0, 7] = idx[0, 3]                                              # row 7 names row 3's landmark, with another pixel
    dup = window_rule(xy, idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0)
    assert dup.tab[0, idx[0, 3]] == 3 and not dup.obs[0, 7]
    xy[0, 3] += 50.0                                                   # ... and when row 3 fails the test, row 7 may pass
    xy[0, 7] = sc.xy[0, 3]
    dup = window_rule(xy, idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0)
    assert dup.tab[0, idx[0, 3]] == 7 and not dup.obs[0, 3]
    # an invalid landmark: kind 0, zeros, and its observations are no members
    valid = np.ones(len(sc.x0), np.uint8)
    valid[5] = 0
    x0 = sc.x0.copy()
    x0[9, 1] = np.inf
    inv = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, x0, sc.r0, sc.t0, key_valid=valid)
    assert inv.kind[5] == 0 and inv.kind[9] == 0 and not inv.xyz[[5, 9]].any() and (inv.tab[:, [5, 9]] == NONE).all()
    # a landmark behind the key camera: valid but not eligible -> kind 2, unchanged
    x0 = sc.x0.copy()
    x0[4] = -x0[4]
    behind = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, x0, sc.r0, sc.t0)
    assert behind.kind[4] == 2 and np.array_equal(behind.xyz[4], f32(x0[4])) and (behind.tab[:, 4] == NONE).all()
    # nkey below the rows: the rows behind it are none
    short = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, nkey=100)
    assert not short.kind[100:].any() and not short.xyz[100:].any() and (short.tab[:, 100:] == NONE).all()
    # a call without an accepted attempt returns the rounded inputs
    heavy = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, lambda0=1e30, iterations=2)
    assert not heavy.path[0] and heavy.lambdas == [float(np.float32(1e30)), LAMBDA_MAX]
    heavy = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, lambda0=1e30, iterations=1)
    assert heavy.path == [False] and list(heavy.stats[2:]) == [1, 0]
    assert np.array_equal(heavy.R, f32(sc.r0)) and np.array_equal(heavy.t, f32(sc.t0)) and heavy.stats[0] == heavy.stats[1]
    assert np.array_equal(heavy.xyz[heavy.kind > 0], f32(sc.x0)[heavy.kind > 0])
    # the gauge: the depth sum of the active landmarks stays what it was
    assert abs(good.xyz[good.active, 2].sum() / f32(sc.x0)[good.active, 2].sum() - 1.0) < 1e-6


# What refine_rule reaches when it is started from this rule's answer differs from this rule's final rms by at most 4.3e-7
# (relative; 8.1e-9 .. 4.3e-7 on the four starts below) -- the level of the fp32 state -- so the margin between the two
# restatements run from one start is set to 1e-5 relative: some twenty times that, and far below the 1e-2 another minimum
# would show.  (Observed between the two from one start: 4e-7 at the most.)
ONE_FRAME_MARGIN = 1e-5


@pytest.mark.parametrize("seed", (1, 2, 3, 4))
def test_one_frame_minimises_the_two_view_cost(seed):
    sc = box_scene(500 + seed, 1, landmarks=200)
    m = int(sc.nobs[0])
    src, dst = sc.key_xy[sc.idx[0, :m]], sc.xy[0, :m]                    # refine_rule's query is the key, its train the frame
    t0 = sc.t0[0] / np.linalg.norm(sc.t0[0])
    start = refine_rule(src, dst, sc.r0[0], t0, thr=3.0, lambda0=1e30, iterations=1, min_parallax_deg=0.0)   # its midpoints
    assert start.path == [False] and start.front.sum() > 100
    two = refine_rule(src, dst, sc.r0[0], t0, thr=3.0, iterations=16, min_parallax_deg=0.0)
    mem = np.flatnonzero(start.member)
    x0 = np.zeros((len(sc.x0), 3))
    x0[sc.idx[0, mem]] = start.xyz[mem]
    valid = np.zeros(len(x0), np.uint8)
    valid[sc.idx[0, mem]] = 1
    got = window_rule(sc.xy, sc.idx, sc.nobs, sc.key_xy, x0, start.R[None], start.t[None], key_valid=valid, iterations=16)
    assert (got.tab != NONE).sum() == got.active.sum() == len(mem)     # the same members
    assert abs(got.stats[0] - two.stats[0]) <= 1e-9 * two.stats[0]     # the same start
    back = refine_rule(src, dst, got.R[0], got.t[0], thr=3.0, iterations=16, min_parallax_deg=0.0)
    print("seed %d: rms %.6f -> window %.8f, two-view %.8f, two-view from the window's answer %.8f (relative %.2e)"
          % (seed, got.stats[0], got.stats[1], two.stats[1], back.stats[1], abs(back.stats[1] - got.stats[1]) / got.stats[1]))
    assert abs(got.stats[1] - two.stats[1]) <= ONE_FRAME_MARGIN * two.stats[1], (got.stats, two.stats)


def test_descending_sums_bound_the_order_dependence():
    """The fallback margin of the device comparison: the restatement with every landmark sum run the other way."""
    scenes, refined = refined_set(0.0)
    worst = np.zeros(3)
    for sc, up in zip(scenes, refined):
        down = run_scene(sc, descending=True)
        assert down.path == up.path
        both = (up.kind == 1) & (down.kind == 1)
        rel = np.linalg.norm(up.xyz[both] - down.xyz[both], axis=1) / np.linalg.norm(up.xyz[both], axis=1)
        worst = np.maximum(worst, (np.abs(up.R - down.R).max(), np.abs(up.t - down.t).max(), rel.max()))
    print("ascending against descending: worst |dR| %.3e, |dt| %.3e, relative |dX| %.3e" % tuple(worst))
    assert (worst <= ORDER_MARGIN).all(), worst


# Ascending against descending sums on the 14 scenes without outliers: the same path and the same fp32 outputs, value for value
# -- worst |dR|, |dt| and relative |dX| are all 0.  The order changes the fp64 sums in their last bits (1e-16), and an fp32
# rounding of the state moves only where a value lies that close to a rounding boundary (about one entry in 1e8).  The device
# comparison's fallback bound is four times these: zero, that is the restatement's own fp32 values.
ORDER_MARGIN = np.array([0.0, 0.0, 0.0])


def test_code_object_keeps_the_kernels_out_of_scratch(code_object):  # noqa: F811
    _, meta = code_object
    names = [k for k in meta if re.match(r"_Z\d+rw_[a-z]+_kernel", k)]
    assert len(names) == 16, names          # init, members, resolve for three sources; finish, cost, decide, build, solve, step, final
    for k in names:
        m = meta[k]
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["group_segment_fixed_size"] <= 160 << 10, (k, m)
