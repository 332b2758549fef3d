"""CPU checks of the minimal-sample absolute pose (fpc_ransac_p3p / fpc_p3p_frames / fpc_p3p_bank): the header declares it, the
binding binds it, the built library exports it -- and this file's float64 restatement of the rule of include/fpc.h (the
sampler's first 4 distinct of 32 draws, Grunert's quartic from the first three pairs, Ferrari's roots through the resolvent
cubic with two Newton steps each, the two triads, the fourth pair's choice among the candidates; then the DLT rule's own
scoring, selection and Gauss-Newton refits, with 4 in the place of 6), which the GPU tests (test_gpu_p3p_ransac.py) hold the
kernels to.  Everything the two rules share is imported from tests/test_pnp_ransac.py, not written again.

Two families of planted scenes: the box family is test_pnp_ransac.planted_scene unchanged; the planar family is the same
generator with the depths taken from a plane through depth 8 tilted 0 .. 40 degrees from fronto-parallel.  Both use the plain
seeds 0 and 1 for every (rho, M): no seed was searched.

Planted-truth bars.  Measured with this restatement over the case set below (CASE_SETS x CASE_M, both families, 44 scenes):
M = 4 and 5 (the four or five rounded pixels are all there is): worst rotation error 0.6550 degrees, worst relative
translation error 1.930e-02; from M = 40 on: 0.0745 degrees and 2.041e-03.  The bars are twice the worst (a different,
equally good best sample is allowed): ROT_BAR_FEW / TRANS_BAR_FEW and ROT_BAR / TRANS_BAR.  At most one outlier sat inside an
inlier mask.

Root finder.  Over the quartics of 400 samples whose roots np.roots separates by more than 1e-3 (398 of them, 920 real roots),
the stated Ferrari + Newton procedure and np.roots disagree by at most 7.639e-11 relative to max(1, |v|) on the real roots
(measured); ROOT_BAR is 1e-9."""
import collections
import functools

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_pnp_ransac import (DEFAULTS, DEPTH, FRAME_H, FRAME_W, KVEC, _draws, _f32, _rotation, camera_points,
                                   gauss_newton_step, header_text, hypotheses, inliers_of, planted_scene, pnp_rule,
                                   pose_errors, reprojection_error, score)

import re

FPC_E_INVALID = -1
SAMPLE = 4
LEADING = 1e-12             # |A4| / max |A_i| at or below which the leading coefficient vanishes (include/fpc.h)
CLOSE = 2e-6                # relative bar on the squared side lengths a candidate reproduces
TRIAD = 1e-12               # sin^2 of the triangle's angle at its first point at or below which a triad is degenerate
NEWTON = 2
NAMES = ("fpc_ransac_p3p", "fpc_p3p_frames", "fpc_p3p_bank")
ROT_BAR, TRANS_BAR = 2 * 0.0745, 2 * 2.041e-03              # M >= 40: twice the worst of the restatement (module docstring)
ROT_BAR_FEW, TRANS_BAR_FEW = 2 * 0.6550, 2 * 1.930e-02      # M < 6, likewise
ROOT_BAR = 1e-9


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def all_samples4(seed, f, iterations, m):
    """[T,4] indices and [T] validity: the first 4 distinct of the 32 draws of every hypothesis, in draw order."""
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


def triad(p0, p1, p2):
    """x = (p1 - p0) / |p1 - p0|, z = c / |c| with c = (p1 - p0) x (p2 - p0), y = z x x -> ([T,3] x, y, z, ok)."""
    with np.errstate(all="ignore"):
        d1, d2 = p1 - p0, p2 - p0
        n1, n2 = _dot(d1, d1), _dot(d2, d2)
        c = np.cross(d1, d2)
        cc = _dot(c, c)
        ok = cc > (TRIAD * n1) * n2
        x, z = d1 / np.sqrt(n1)[:, None], c / np.sqrt(cc)[:, None]
        return x, np.cross(z, x), z, ok


def grunert(xy, xyz, kvec):
    """The first three pairs of every sample -> (the quartic's coefficients A4 .. A0 [T,5], the quantities the candidates
    need, ok [T])."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in kvec)
    with np.errstate(all="ignore"):
        xh, yh = (xy[:, :3, 0] - cx) / fx, (xy[:, :3, 1] - cy) / fy
        n = np.sqrt((xh * xh + yh * yh) + 1.0)
        f = np.stack([xh / n, yh / n, 1.0 / n], -1)                                   # [T,3,3] unit bearings
        x = xyz[:, :3]
        e, g, h = x[:, 1] - x[:, 2], x[:, 0] - x[:, 2], x[:, 0] - x[:, 1]
        a2, b2, c2 = _dot(e, e), _dot(g, g), _dot(h, h)
        ok = (a2 > 0) & (b2 > 0) & (c2 > 0)
        ca, cb, cg = _dot(f[:, 1], f[:, 2]), _dot(f[:, 0], f[:, 2]), _dot(f[:, 0], f[:, 1])
        q, r, ab, cbq = (a2 - c2) / b2, (a2 + c2) / b2, a2 / b2, c2 / b2
        a4 = (q - 1.0) * (q - 1.0) - 4.0 * cbq * (ca * ca)
        a3 = 4.0 * ((q * (1.0 - q) * cb - (1.0 - r) * ca * cg) + 2.0 * cbq * (ca * ca) * cb)
        a2c = 2.0 * (((((q * q - 1.0) + 2.0 * (q * q) * (cb * cb)) + 2.0 * ((b2 - c2) / b2) * (ca * ca))
                      - 4.0 * r * ca * cb * cg) + 2.0 * ((b2 - a2) / b2) * (cg * cg))
        a1 = 4.0 * ((-q * (1.0 + q) * cb + 2.0 * ab * (cg * cg) * cb) - (1.0 - r) * ca * cg)
        a0 = (1.0 + q) * (1.0 + q) - 4.0 * ab * (cg * cg)
        coef = np.stack([a4, a3, a2c, a1, a0], 1)
        amax = np.abs(coef).max(1)
        ok = ok & (np.abs(a4) > LEADING * amax) & (amax < 1e300)
    return coef, dict(f=f, a2=a2, b2=b2, c2=c2, ca=ca, cb=cb, cg=cg, q=q), ok


def ferrari(coef):
    """The stated root finder: coef [T,5] (A4 .. A0) -> (v [T,4] in the header's candidate order, real [T,4]): the monic
    quartic is depressed (v = y - b3 / 4), the resolvent cubic's largest real root m comes from Cardano's formula (one real
    root) or the cosine formula (three) and two Newton steps, the two quadratics y^2 -+ s y + (e +- h) give the candidates,
    and each takes two Newton steps on the monic quartic."""
    with np.errstate(all="ignore"):
        b3, b2, b1, b0 = (coef[:, k] / coef[:, 0] for k in (1, 2, 3, 4))
        p = b2 - 0.375 * (b3 * b3)
        qq = (b1 - 0.5 * (b3 * b2)) + 0.125 * ((b3 * b3) * b3)
        rr = ((b0 - 0.25 * (b3 * b1)) + 0.0625 * ((b3 * b3) * b2)) - 0.01171875 * ((b3 * b3) * (b3 * b3))
        c2, c1, c0 = p, 0.25 * (p * p) - rr, -0.125 * (qq * qq)
        pp = c1 - (c2 * c2) / 3.0
        qc = ((2.0 * ((c2 * c2) * c2)) / 27.0 - (c2 * c1) / 3.0) + c0
        disc = 0.25 * (qc * qc) + ((pp * pp) * pp) / 27.0
        sd = np.sqrt(np.maximum(disc, 0.0))
        z1 = np.cbrt(-0.5 * qc + sd) + np.cbrt(-0.5 * qc - sd)
        rho = np.sqrt(np.maximum(-pp / 3.0, 0.0))
        arg = np.minimum(1.0, np.maximum(-1.0, (-0.5 * qc) / ((rho * rho) * rho)))
        z3 = (2.0 * rho) * np.cos(np.arccos(arg) / 3.0)
        z = np.where(disc > 0, z1, np.where(rho > 0, z3, 0.0))
        m = z - c2 / 3.0
        for _ in range(NEWTON):
            gm, dm = ((m + c2) * m + c1) * m + c0, (3.0 * m + 2.0 * c2) * m + c1
            mn = m - gm / dm
            m = np.where(np.abs(mn) < 1e300, mn, m)
        good = (m > 0) & (m < 1e300)
        s = np.sqrt(2.0 * m)
        h, e = qq / (2.0 * s), 0.5 * p + m
        da, db = 2.0 * m - 4.0 * (e + h), 2.0 * m - 4.0 * (e - h)
        vs, real = [], []
        for k in range(4):
            d = da if k < 2 else db
            sq = np.sqrt(np.maximum(d, 0.0))
            v = 0.5 * ((s if k < 2 else -s) + (-sq if k & 1 else sq)) - 0.25 * b3
            for _ in range(NEWTON):
                fv = (((v + b3) * v + b2) * v + b1) * v + b0
                dv = ((4.0 * v + 3.0 * b3) * v + 2.0 * b2) * v + b1
                vn = v - fv / dv
                v = np.where(np.abs(vn) < 1e300, vn, v)
            vs.append(v)
            real.append(good & (d >= 0))
    return np.stack(vs, 1), np.stack(real, 1)


def solve_p3p(xy, xyz, kvec):
    """The minimal solve, batched: xy [T,4,2], xyz [T,4,3] -> (R [T,3,3], t [T,3], ok [T]) in float64."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in kvec)
    xy, xyz = np.asarray(xy, np.float64), np.asarray(xyz, np.float64)
    n = len(xy)
    coef, w, ok = grunert(xy, xyz, kvec)
    xt, yt, zt, tok = triad(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    ok = ok & tok
    vs, real = ferrari(coef)
    f, q, ca, cb, cg = w["f"], w["q"], w["ca"], w["cb"], w["cg"]
    best_e = np.full(n, np.inf)
    have = np.zeros(n, bool)
    rbest, tbest = np.zeros((n, 3, 3)), np.zeros((n, 3))
    with np.errstate(all="ignore"):
        for k in range(4):
            v = vs[:, k]
            good = ok & real[:, k] & (v > 0)
            u = ((((q - 1.0) * v) * v - ((2.0 * q) * cb) * v) + (1.0 + q)) / (2.0 * (cg - v * ca))
            good &= (u > 0) & (u < 1e300)
            ww = (1.0 + v * v) - (2.0 * v) * cb
            good &= ww > 0
            s0 = np.sqrt(w["b2"] / ww)
            c0, c1, c2 = s0[:, None] * f[:, 0], (u * s0)[:, None] * f[:, 1], (v * s0)[:, None] * f[:, 2]
            d01, d12 = _dot(c0 - c1, c0 - c1), _dot(c1 - c2, c1 - c2)
            good &= (np.abs(d01 - w["c2"]) <= CLOSE * w["c2"]) & (np.abs(d12 - w["a2"]) <= CLOSE * w["a2"])
            xq, yq, zq, qok = triad(c0, c1, c2)
            good &= qok
            r = (xq[:, :, None] * xt[:, None, :] + yq[:, :, None] * yt[:, None, :]) + zq[:, :, None] * zt[:, None, :]
            t = c0 - np.einsum("nij,nj->ni", r, xyz[:, 0])
            pc = np.einsum("nij,nj->ni", r, xyz[:, 3]) + t
            ex = fx * (pc[:, 0] / pc[:, 2]) - (xy[:, 3, 0] - cx)
            ey = fy * (pc[:, 1] / pc[:, 2]) - (xy[:, 3, 1] - cy)
            err = ex * ex + ey * ey
            take = good & (pc[:, 2] > 0) & (err < 1e300) & (~have | (err < best_e))      # ties keep the lower k
            rbest[take], tbest[take], best_e[take] = r[take], t[take], err[take]
            have |= take
    fin = (np.abs(rbest) < 1e300).all((1, 2)) & (np.abs(tbest) < 1e300).all(1)
    return rbest, tbest, have & fin


P3p = collections.namedtuple("P3p", "R t ninliers mask failed best_t near first")


def _failed(m, best_t=-1, first=None):
    return P3p(np.zeros((3, 3)), np.zeros(3), 0, np.zeros(m, bool), True, best_t, np.zeros(m, bool), first)


def p3p_rule(xy, xyz, params, f, kvec=KVEC):
    """The whole rule for frame index f: xy [M,2], xyz [M,3] (float32 values) -> P3p.  `near`: the pairs within 1e-3 px of
    the threshold under the returned pose; `first`: the best sample's pose before the refits."""
    p = dict(DEFAULTS, **params)
    thr = float(np.float32(p["reproj_threshold"]))
    xy, xyz = _f32(xy).reshape(-1, 2), _f32(xyz).reshape(-1, 3)
    m = len(xy)
    if m < SAMPLE:
        return _failed(m)
    idx, ok = all_samples4(p["seed"], f, p["iterations"], m)
    r, t, sok = solve_p3p(xy[idx], xyz[idx], kvec)
    ok = ok & sok
    pm = np.concatenate([r, t[:, :, None]], 2)
    pm[~ok] = 0.0
    p32, ok = hypotheses(pm, ok, xyz[idx[:, 0]], kvec)
    counts = np.where(ok, score(p32, xy, xyz, thr), 0)
    if counts.max() <= 0:
        return _failed(m)
    best = int(np.argmax(counts))                                    # the largest count, ties to the lower t
    pose = (_f32(r[best]), _f32(t[best]))
    if not (np.abs(pose[0]) < 3e38).all() or not (np.abs(pose[1]) < 3e38).all():
        return _failed(m, best)
    first = pose
    for _ in range(p["refits"]):
        inl = inliers_of(pose[0], pose[1], xy, xyz, kvec, thr)
        if inl.sum() < SAMPLE:
            break
        nxt = gauss_newton_step(pose[0], pose[1], xy, xyz, inl, kvec)
        if nxt is None:
            break
        pose = nxt
    inl = inliers_of(pose[0], pose[1], xy, xyz, kvec, thr)
    if inl.sum() < p["min_inliers"]:
        return _failed(m, best, first)
    near = np.abs(reprojection_error(pose[0], pose[1], xy, xyz, kvec) - thr) <= 1e-3
    return P3p(pose[0], pose[1], int(inl.sum()), inl, False, best, near, first)


# ---- planted scenes -------------------------------------------------------------------------------------------------------
CASE_SETS = [(0.0, 64), (0.3, 256), (0.6, 1024)]                    # (outlier fraction, iterations): a quarter of the DLT's
CASE_M = {0.0: [4, 5, 40, 300, 1100], 0.3: [40, 300, 1100], 0.6: [40, 300, 1100]}
SCENE_IDS = (0, 1)                                                   # every (rho, M), both families
FAMILIES = ("box", "planar")
PARAMS = dict(reproj_threshold=3.0, seed=7, refits=4, min_inliers=4)          # (4: the frames of 4 and 5 pairs can pass)
PLANE_DEPTH = 0.5 * (DEPTH[0] + DEPTH[1])                            # the plane passes through (0, 0, 8)
PLANE_TILT = 40.0                                                    # degrees from fronto-parallel, at most


def planar_scene(i, rho, m, kvec=KVEC):
    """planted_scene with the depths taken from a plane: the same seed, the same draws of the pose and of the pixels, then a
    tilt of 0 .. 40 degrees about a random in-plane direction instead of the box's depths.  The landmarks (in their own
    frame) lie on one plane up to their fp32 rounding."""
    fx, fy, cx, cy = kvec
    rng = np.random.default_rng(1000 * i + 10 * m + int(round(10 * rho)))
    r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(5.0, 30.0)))
    d = rng.normal(size=3)
    t = d / np.linalg.norm(d) * rng.uniform(0.5, 1.5) * PLANE_DEPTH
    px = np.stack([rng.uniform(8, FRAME_W - 8, m), rng.uniform(8, FRAME_H - 8, m)], 1)
    tilt, phi = np.deg2rad(rng.uniform(0.0, PLANE_TILT)), rng.uniform(0.0, 2.0 * np.pi)
    nrm = np.array([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)])
    ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(m)], 1)
    z = PLANE_DEPTH * nrm[2] / (ray @ nrm)                           # n . (z ray) = n . (0, 0, 8)
    assert (z > 1.0).all()
    xc = ray * z[:, None]
    xyz = ((xc - t) @ r).astype(np.float32)                          # X = R^T (X_c - t)
    xc = camera_points(r, t, xyz)
    xy = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1))
    planted = np.ones(m, bool)
    nout = int(round(rho * m))
    if nout:
        out = rng.choice(m, nout, replace=False)
        xy[out] = np.stack([rng.integers(0, FRAME_W, nout), rng.integers(0, FRAME_H, nout)], 1)
        planted[out] = False
    return xy.astype(np.float32), xyz, planted, r, t


def planted_batch(family, rho):
    """The frames of one case set: two scenes of every M."""
    make = planted_scene if family == "box" else planar_scene
    return [make(i, rho, m) for m in CASE_M[rho] for i in SCENE_IDS]


def bars(m):
    return (ROT_BAR, TRANS_BAR) if m >= 40 else (ROT_BAR_FEW, TRANS_BAR_FEW)


def check_planted_pose(r, t, mask, scene, tag):
    """The planted-truth bars on one frame (test_pnp_ransac.check_planted_pose with this file's bars; the mask conditions
    are its own) -> (rotation error, translation error)."""
    rot, tr = pose_errors(r, t, scene)
    rot_bar, trans_bar = bars(len(scene[0]))
    assert rot <= rot_bar and tr <= trans_bar, (tag, rot, tr)
    assert abs(np.linalg.det(np.asarray(r, np.float64)) - 1.0) < 1e-5, tag
    planted = scene[2]
    assert not mask[~planted].sum() > 0.1 * max(1, (~planted).sum()), tag        # an outlier is an inlier only by chance
    assert mask[planted].sum() >= 0.9 * planted.sum(), (tag, mask[planted].sum(), planted.sum())
    return rot, tr


@functools.lru_cache(maxsize=None)
def restated_batch(family, rho, iterations):
    scenes = planted_batch(family, rho)
    return scenes, [p3p_rule(s[0], s[1], dict(PARAMS, iterations=iterations), f) for f, s in enumerate(scenes)]


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    for name, twin in zip(NAMES, ("fpc_ransac_pnp", "fpc_pnp_frames", "fpc_pnp_bank")):      # the twins' argument lists
        args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1)) for n in (name, twin)]
        assert args[0] == args[1], name
        assert getattr(lib, name).argtypes == getattr(lib, twin).argtypes, name
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+4\b", header_text())
    assert lib.fpc_abi_version() == 4


def test_null_context_is_refused():
    import ctypes
    lib = _lib.load()
    p = _lib.FpcPnpParams()
    lib.fpc_default_pnp_params(ctypes.byref(p))
    p.min_inliers = 4
    buf = (ctypes.c_float * 64)()
    b = ctypes.addressof(buf)
    pp = ctypes.byref(p)
    assert lib.fpc_ransac_p3p(None, 1, b, b, b, 1, pp, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_p3p_frames(None, 1, b, b, b, b, pp, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_p3p_bank(None, 1, b, b, pp, b, b, b, b) == FPC_E_INVALID


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_sampler_takes_the_first_four_of_the_dlt_draws():
    from tests.test_pnp_ransac import all_samples
    idx, ok = all_samples4(7, 3, 64, 40)
    assert ok.all() and all(len(set(row)) == SAMPLE for row in idx.tolist()) and idx.max() < 40
    idx6, ok6 = all_samples(7, 3, 64, 40)                            # the same 32 draws: the DLT's sample begins with this one
    np.testing.assert_array_equal(idx[ok6], idx6[ok6][:, :4])
    assert (all_samples4(8, 3, 64, 40)[0] != idx).any() and (all_samples4(7, 4, 64, 40)[0] != idx).any()
    idx4, ok4 = all_samples4(7, 0, 256, 4)                           # four pairs: a sample is a permutation of all of them
    assert ok4.any() and all(sorted(row) == list(range(4)) for row in idx4[ok4].tolist())
    assert not all_samples4(7, 0, 16, 3)[1].any()


def _exact_samples(make, count, m=4):
    """Noise-free (unrounded) samples of `m` pairs with their planted poses."""
    out = []
    for i in range(count):
        _, xyz, _, r, t = make(i, 0.0, m)
        xc = camera_points(r, t, xyz)
        xy = np.stack([500.0 * xc[:, 0] / xc[:, 2] + 320.0, 500.0 * xc[:, 1] / xc[:, 2] + 240.0], 1)   # not rounded
        out.append((xy, xyz.astype(np.float64), r, t))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_minimal_solve_is_exact_on_noise_free_samples(family):
    make = planted_scene if family == "box" else planar_scene
    samples = _exact_samples(make, 40)
    r, t, ok = solve_p3p(np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples]), KVEC)
    assert ok.all()
    for k, (_, _, r0, t0) in enumerate(samples):
        np.testing.assert_allclose(r[k], r0, atol=1e-6)
        np.testing.assert_allclose(t[k], t0, rtol=1e-6, atol=1e-6)
        assert abs(np.linalg.det(r[k]) - 1.0) < 1e-12


def test_root_finder_agrees_with_np_roots():
    samples = _exact_samples(planted_scene, 200) + _exact_samples(planar_scene, 200)
    xy, xyz = np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples])
    rng = np.random.default_rng(0)
    xy = np.round(xy + rng.normal(size=xy.shape))                    # the quartics of perturbed, rounded pixels as well
    coef, _, ok = grunert(xy, xyz, KVEC)
    vs, real = ferrari(coef)
    worst, used, nroots = 0.0, 0, 0
    for k in np.flatnonzero(ok):
        want = np.roots(coef[k])
        gaps = np.abs(want[:, None] - want[None, :])[np.triu_indices(4, 1)]
        if gaps.min() <= 1e-3:                                       # (a near-double root: either finder may split it)
            continue
        used += 1
        want_real = np.sort(want[np.abs(want.imag) == 0].real)
        got = np.sort(vs[k][real[k]])
        assert len(got) == len(want_real), (k, got, want)
        nroots += len(got)
        if len(got):
            worst = max(worst, (np.abs(got - want_real) / np.maximum(1.0, np.abs(want_real))).max())
    print("root finder: %d quartics, %d real roots, worst relative difference from np.roots %.3e" % (used, nroots, worst))
    assert used >= 300 and nroots >= 2 * used
    assert worst <= ROOT_BAR


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_restatement_recovers_planted_poses(family, rho, iterations):
    scenes, results = restated_batch(family, rho, iterations)
    worst = {False: np.zeros(2), True: np.zeros(2)}
    for f, (scene, res) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not res.failed, (family, rho, f, m)
        errs = check_planted_pose(res.R, res.t, res.mask, scene, (family, rho, f, m))
        worst[m >= 40] = np.maximum(worst[m >= 40], errs)
        assert res.ninliers == res.mask.sum() >= PARAMS["min_inliers"]
        assert res.mask[~scene[2]].sum() <= 1
        print("%s rho %.1f frame %2d M %4d: rotation %.4f deg, translation %.3e, %d inliers of %d planted"
              % (family, rho, f, m, *errs, res.ninliers, scene[2].sum()))
    print("%s rho %.1f: worst rotation %.4f deg, worst relative translation %.3e (M >= 40); %.4f deg, %.3e (M < 6)"
          % (family, rho, *worst[True], *worst[False]))


def test_the_dlt_rule_fails_on_planar_scenes_where_this_rule_passes():
    """The reason for the second model: on the planar family the 6-point DLT rule fails every scene (with its own, four
    times larger, iteration budget), and the minimal-sample rule recovers every one."""
    for (rho, iterations), dlt_iterations in zip(CASE_SETS, (256, 1024, 4096)):
        scenes, results = restated_batch("planar", rho, iterations)
        for f, (scene, res) in enumerate(zip(scenes, results)):
            m = len(scene[0])
            assert not res.failed, (rho, f, m)
            if m < 6:
                continue
            dlt = pnp_rule(scene[0], scene[1], dict(PARAMS, iterations=dlt_iterations, min_inliers=6), f)
            assert dlt.failed and not dlt.R.any() and dlt.ninliers == 0, (rho, f, m)


def test_restatement_failure_rules():
    xy, xyz, _, r, t = planar_scene(0, 0.0, 40)
    params = dict(PARAMS, iterations=64)
    assert p3p_rule(xy[:3], xyz[:3], params, 0).failed                               # fewer than 4 pairs
    assert not p3p_rule(xy[:4], xyz[:4], params, 0).failed
    res = p3p_rule(xy, xyz, dict(params, min_inliers=41), 0)                         # inliers end below min_inliers
    assert res.failed and not res.R.any() and not res.t.any() and res.ninliers == 0 and not res.mask.any()
    assert not p3p_rule(xy, xyz, dict(params, min_inliers=40), 0).failed
    # collinear landmarks: every triad is degenerate
    rng = np.random.default_rng(5)
    s = rng.integers(-192, 193, 60) / 64.0                           # (exact in fp32: the cross products are exactly zero)
    line = np.stack([s, 0.5 * s + 0.25, 2.0 + 0.125 * s], 1).astype(np.float32)
    xc = camera_points(r, np.array([0, 0, 8.0]), line)
    pix = np.round(np.stack([500.0 * xc[:, 0] / xc[:, 2] + 320.0, 500.0 * xc[:, 1] / xc[:, 2] + 240.0], 1))
    assert p3p_rule(pix, line, params, 0).failed
    # coincident landmarks: one pair repeated, and four pairs of which three are equal (any three of them hold two equal
    # ones; with only two equal a sample whose fourth pair is the repeated one is a valid sample)
    assert p3p_rule(np.repeat(xy[:1], 50, 0), np.repeat(xyz[:1], 50, 0), params, 0).failed
    assert p3p_rule(xy[[0, 1, 1, 1]], xyz[[0, 1, 1, 1]], params, 0).failed
    # every landmark behind the camera: the mirror images X' with R X' + t = -(R X + t) show the same pixels.  (A box scene:
    # the mirror image of a PLANAR set is a rotation of it, which has a pose in front of the camera.  Three mirrored points
    # always have one, so a sample may count itself and a chance pair or two: the floor here is 8.)
    bxy, bxyz, _, br, bt = planted_scene(0, 0.0, 40)
    behind = ((-camera_points(br, bt, bxyz) - bt) @ br).astype(np.float32)
    assert p3p_rule(bxy, behind, dict(params, min_inliers=8), 0).failed
    assert not p3p_rule(bxy, bxyz, dict(params, min_inliers=8), 0).failed


def test_landmarks_behind_the_camera_are_never_inliers():
    xy, xyz, _, r, t = planted_scene(1, 0.0, 40)
    behind = ((-camera_points(r, t, xyz[:10]) - t) @ r).astype(np.float32)
    res = p3p_rule(np.concatenate([xy, xy[:10]]), np.concatenate([xyz, behind]), dict(PARAMS, iterations=64), 0)
    assert not res.failed and res.mask[:40].sum() >= 36 and not res.mask[40:].any()
    assert (camera_points(res.R, res.t, behind)[:, 2] < 0).all()


def test_no_refits_returns_the_best_samples_rounded_pose():
    xy, xyz, _, _, _ = planar_scene(2, 0.0, 300)
    res = p3p_rule(xy, xyz, dict(PARAMS, iterations=64, refits=0), 0)
    assert not res.failed
    np.testing.assert_array_equal(res.R, res.first[0])
    np.testing.assert_array_equal(res.t, res.first[1])
    np.testing.assert_array_equal(res.R, _f32(res.R))                                # fp32 values
    sv = np.linalg.svd(res.R, compute_uv=False)
    assert np.abs(sv - 1.0).max() < 1e-6 and abs(np.linalg.det(res.R) - 1.0) < 1e-6   # a rotation without a polar step
    more = p3p_rule(xy, xyz, dict(PARAMS, iterations=64, refits=4), 0)
    assert more.best_t == res.best_t and more.ninliers >= res.ninliers
