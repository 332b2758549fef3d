"""CPU checks of the RANSAC homography stage (fpc_ransac_homography / fpc_homography_frames): the header declares it, the
binding binds it, the built library exports it -- and this file's float64 restatement of the rule of include/fpc.h (the
integer sampler, the exact 4-point homography, the oriented scoring, the integer selection, the Hartley-normalised
least-squares refit), which the GPU tests (test_gpu_homography_ransac.py) hold the kernels to, recovers planted
homographies.  The planted truth is tests/golden/f10_sample_homography.npz: homographies drawn by the reference's own
sample_homography for a 480 x 640 frame.  OpenCV is not available to this build, so nothing here is compared against
cv2.findHomography."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
FRAME_H, FRAME_W = 480, 640
DRAWS, MAX_ITERATIONS, COLLINEAR = 16, 4096, 0.5
DEFAULTS = dict(iterations=1024, reproj_threshold=3.0, seed=0, refits=2, min_inliers=8)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def mix(a):
    a = np.asarray(a, np.uint32).copy()
    with np.errstate(over="ignore"):
        a ^= a >> np.uint32(16)
        a *= np.uint32(0x7feb352d)
        a ^= a >> np.uint32(15)
        a *= np.uint32(0x846ca68b)
        a ^= a >> np.uint32(16)
    return a


def sample_indices(seed, f, t, m):
    """The sample of hypothesis t of frame f over m pairs: 4 distinct indices in draw order, or None (degenerate)."""
    with np.errstate(over="ignore"):
        base = (np.uint32(f) * np.uint32(MAX_ITERATIONS) + np.uint32(t)) * np.uint32(DRAWS)
        r = mix(np.uint32(seed) ^ mix(base + np.arange(DRAWS, dtype=np.uint32))) % np.uint32(m)
    idx = []
    for v in r.tolist():
        if v not in idx:
            idx.append(v)
            if len(idx) == 4:
                return idx
    return None


def _all_samples(seed, f, iterations, m):
    """[T,4] indices and [T] validity, vectorised over t (the same draws as sample_indices)."""
    with np.errstate(over="ignore"):
        base = (np.uint32(f) * np.uint32(MAX_ITERATIONS) + np.arange(iterations, dtype=np.uint32)) * np.uint32(DRAWS)
        r = mix(np.uint32(seed) ^ mix(base[:, None] + np.arange(DRAWS, dtype=np.uint32)[None, :])) % np.uint32(m)
    idx = np.zeros((iterations, 4), np.int64)
    ok = np.zeros(iterations, bool)
    for t, row in enumerate(r.tolist()):
        got = []
        for v in row:
            if v not in got:
                got.append(v)
                if len(got) == 4:
                    break
        if len(got) == 4:
            idx[t], ok[t] = got, True
    return idx, ok


def solve4(src, dst):
    """The homography through 4 pairs, batched: src, dst [T,4,2] -> (H [T,3,3] scaled to max|h| = 1 with w > 0 at the
    first point, ok [T]).  Projective-basis closed form; degenerate when three src or three dst points are collinear
    (doubled triangle area < 0.5), H is non-finite, or |h8| <= 1e-12."""
    def basis(p):
        ph = np.concatenate([p, np.ones(p.shape[:2] + (1,))], 2)                  # [T,4,3]
        c12, c20, c01 = np.cross(ph[:, 1], ph[:, 2]), np.cross(ph[:, 2], ph[:, 0]), np.cross(ph[:, 0], ph[:, 1])
        lam = np.stack([(c12 * ph[:, 3]).sum(1), (c20 * ph[:, 3]).sum(1), (c01 * ph[:, 3]).sum(1)], 1)
        det = (c01 * ph[:, 2]).sum(1)
        good = (np.abs(lam) >= COLLINEAR).all(1) & (np.abs(det) >= COLLINEAR)
        return ph, (c12, c20, c01), lam, good
    ps, cs, ls, gs = basis(np.asarray(src, np.float64))
    pd, _, ld, gd = basis(np.asarray(dst, np.float64))
    adj = np.stack([cs[0] * (ls[:, 1] * ls[:, 2])[:, None], cs[1] * (ls[:, 2] * ls[:, 0])[:, None],
                    cs[2] * (ls[:, 0] * ls[:, 1])[:, None]], 1)                    # rows of adj(A)
    b = (pd[:, :3] * ld[:, :, None]).transpose(0, 2, 1)                            # columns m_i q_i
    with np.errstate(all="ignore"):
        h = b @ adj
        mx = np.abs(h).max((1, 2))
        ok = gs & gd & (mx > 0) & (mx < 1e300)
        w0 = (h[:, 2] * ps[:, 0]).sum(1)
        h = h * (np.where(w0 < 0, -1.0, 1.0) / np.where(ok, mx, 1.0))[:, None, None]
        ok &= np.isfinite(h).all((1, 2)) & (np.abs(h[:, 2, 2]) > 1e-12)
    return h, ok


def inliers_of(h, src, dst, thr):
    """|H.src - dst| < thr without the division (the plain, sign-free test of the header), float64."""
    x, y, u, v = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    ex = h[0, 0] * x + h[0, 1] * y + h[0, 2] - w * u
    ey = h[1, 0] * x + h[1, 1] * y + h[1, 2] - w * v
    return ex * ex + ey * ey < thr * thr * w * w


def _f32(h):
    return h.astype(np.float32).astype(np.float64)


def refit(src, dst):
    """Hartley-normalised (RMS distance sqrt(2)) least squares with h8 = 1 in the normalised frame -> H with H[2,2] = 1
    rounded to fp32 values, or None (zero spread / singular)."""
    n = len(src)
    cs, cd = src.mean(0), dst.mean(0)
    vs, vd = ((src - cs) ** 2).sum(1).mean(), ((dst - cd) ** 2).sum(1).mean()
    if n < 4 or not vs > 1e-12 or not vd > 1e-12:
        return None
    ss, sd = np.sqrt(2.0 / vs), np.sqrt(2.0 / vd)
    p, q = (src - cs) * ss, (dst - cd) * sd
    x, y, u, v = p[:, 0], p[:, 1], q[:, 0], q[:, 1]
    z, o = np.zeros(n), np.ones(n)
    a = np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y], 1)])
    rhs = np.concatenate([u, v])
    ata = a.T @ a
    if np.linalg.matrix_rank(ata, tol=1e-10 * n) < 8:
        return None
    hn = np.append(np.linalg.solve(ata, a.T @ rhs), 1.0).reshape(3, 3)
    ts = np.array([[ss, 0, -ss * cs[0]], [0, ss, -ss * cs[1]], [0, 0, 1]])
    tdi = np.array([[1 / sd, 0, cd[0]], [0, 1 / sd, cd[1]], [0, 0, 1]])
    h = tdi @ hn @ ts
    if not np.isfinite(h).all() or not abs(h[2, 2]) > 1e-12 * np.abs(h).max():
        return None
    return _f32(h / h[2, 2])


def ransac_rule(src, dst, params, f):
    """include/fpc.h's rule for frame f in float64: src, dst [M,2] -> (H [3,3] with H[2,2] = 1, or zeros on failure;
    inlier mask bool [M])."""
    p = dict(DEFAULTS, **params)
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    m, thr = len(src), float(np.float32(p["reproj_threshold"]))
    fail = np.zeros((3, 3)), np.zeros(m, bool)
    if m < 4:
        return fail
    idx, ok = _all_samples(p["seed"], f, p["iterations"], m)
    h, good = solve4(src[idx], dst[idx])
    good &= ok
    if not good.any():
        return fail
    h32 = _f32(h)                                                    # the hypotheses are applied in fp32 on the device
    x, y, u, v = src[:, 0][None], src[:, 1][None], dst[:, 0][None], dst[:, 1][None]
    w = h32[:, 2, 0:1] * x + h32[:, 2, 1:2] * y + h32[:, 2, 2:3]
    ex = h32[:, 0, 0:1] * x + h32[:, 0, 1:2] * y + h32[:, 0, 2:3] - w * u
    ey = h32[:, 1, 0:1] * x + h32[:, 1, 1:2] * y + h32[:, 1, 2:3] - w * v
    count = ((w > 0) & (ex * ex + ey * ey < thr * thr * w * w)).sum(1) * good
    best = int(np.argmax(count))                                     # the first maximum: ties go to the lower t
    if count[best] == 0:
        return fail
    cur = _f32(h[best] / h[best, 2, 2])
    for _ in range(p["refits"]):
        inl = inliers_of(cur, src, dst, thr)
        new = refit(src[inl], dst[inl]) if inl.sum() >= 4 else None
        if new is None:
            break
        cur = new
    inl = inliers_of(cur, src, dst, thr)
    if inl.sum() < p["min_inliers"]:
        return fail
    return cur, inl


# ---- planted truth ----------------------------------------------------------------------------------------------------------
def project(h, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(h, np.float64).T
    with np.errstate(all="ignore"):
        return q[:, :2] / q[:, 2:]


CORNERS = np.array([[0, 0], [FRAME_W - 1, 0], [0, FRAME_H - 1], [FRAME_W - 1, FRAME_H - 1]], np.float64)


def corner_error(h, truth):
    """The largest distance between the frame's four corners under h and under the truth (inf for a failed frame)."""
    if not np.any(h):
        return np.inf
    return float(np.sqrt(((project(h, CORNERS) - project(truth, CORNERS)) ** 2).sum(1)).max())


_F10 = None


def planted_case(name, i, rho, npairs=600):
    """F10 homography `name`[i] as planted truth: integer src pixels, dst = round(H.src) kept when inside the frame, the
    first `npairs` of them; a share rho of the dst points replaced by uniform random pixels.
    -> (truth [3,3], src [npairs,2], dst [npairs,2], planted-inlier mask)."""
    global _F10
    if _F10 is None:
        _F10 = np.load(os.path.join(ROOT, "tests", "golden", "f10_sample_homography.npz"))
        assert [int(v) for v in _F10["shape"]] == [FRAME_H, FRAME_W]
    truth = np.append(_F10[name][i].astype(np.float64), 1.0).reshape(3, 3)
    rng = np.random.Generator(np.random.PCG64([{"defaults": 1, "preprocess": 2}[name], i, int(round(rho * 100))]))
    src = np.stack([rng.integers(0, FRAME_W, 20000), rng.integers(0, FRAME_H, 20000)], 1).astype(np.float64)
    dst = project(truth, src)
    ok = np.isfinite(dst).all(1) & (dst[:, 0] >= 0) & (dst[:, 0] <= FRAME_W - 1) & (dst[:, 1] >= 0) & (dst[:, 1] <= FRAME_H - 1)
    assert ok.sum() >= npairs, (name, i, int(ok.sum()))
    src, dst = src[ok][:npairs], np.rint(dst[ok][:npairs])
    nout = int(rho * npairs)
    out = rng.permutation(npairs)[:nout]
    dst[out] = np.stack([rng.integers(0, FRAME_W, nout), rng.integers(0, FRAME_H, nout)], 1)
    planted = np.ones(npairs, bool)
    planted[out] = False
    return truth, src, dst, planted


# (rho, iterations): rho = 0.7 leaves 0.3^4 * 256 ~ 2 all-inlier samples at T = 256, too few to rely on; at T = 2048 the
# chance of none is ~ e^-16 per case
CASE_SETS = [(0.0, 256), (0.5, 256), (0.7, 2048)]
CASE_NAMES = [(name, i) for name in ("defaults", "preprocess") for i in range(16)]
CORNER_BAR = 1.5            # px; the restatement's own error on these cases (integer-rounded dst: <= 0.71 px per point)


# ---- tests ------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_header_binding_and_library_agree():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("fpc_default_ransac_params", "fpc_ransac_homography", "fpc_homography_frames"):
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    assert {"fpc_default_ransac_params", "fpc_ransac_homography", "fpc_homography_frames"} <= exported
    m = re.search(r"typedef struct fpc_ransac_params \{(.*?)\} fpc_ransac_params;", code, flags=re.S)
    fields = re.findall(r"(int|float|uint32_t)\s+([a-z_]+);", m.group(1))
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.FpcRansacParams._fields_)
    # the sampler's constants are part of the contract: the header states them
    for const in ("0x7feb352d", "0x846ca68b", "(f * 4096 + t) * 16 + k"):
        assert const in hdr, const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4


def test_defaults_and_null_arguments():
    lib = _lib.load()
    p = _lib.FpcRansacParams()
    assert lib.fpc_default_ransac_params(ctypes.byref(p)) == 0
    assert (p.iterations, p.reproj_threshold, p.seed, p.refits, p.min_inliers) == (1024, 3.0, 0, 2, 8)
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert lib.fpc_default_ransac_params(None) == FPC_E_INVALID
    buf = np.zeros(64, np.float32)
    d = buf.ctypes.data
    assert lib.fpc_ransac_homography(None, 1, d, d, d, 4, ctypes.byref(p), d, d, None) == FPC_E_INVALID
    assert lib.fpc_homography_frames(None, 1, 0, d, d, d, ctypes.byref(p), d, d, None) == FPC_E_INVALID


def test_sampler_is_distinct_reproducible_and_keyed():
    seen = set()
    for m in (4, 5, 37, 600, 12288):
        for f in (0, 1, 31):
            for t in (0, 1, 255, 4095):
                for seed in (0, 7, 0xffffffff):
                    idx = sample_indices(seed, f, t, m)
                    if idx is None:                                  # only a tiny m can exhaust the 16 draws
                        assert m <= 5
                        continue
                    assert len(set(idx)) == 4 and all(0 <= v < m for v in idx)
                    assert idx == sample_indices(seed, f, t, m)
                    if m == 12288:
                        seen.add(tuple(idx))
    assert len(seen) == 3 * 4 * 3                                    # every (f, t, seed) drew its own sample
    idx, ok = _all_samples(7, 3, 300, 600)
    for t in (0, 17, 299):
        assert ok[t] and list(idx[t]) == sample_indices(7, 3, t, 600)
    # a pinned value: the hash itself, restated from the header
    a = 12345
    a ^= a >> 16; a = (a * 0x7feb352d) & 0xffffffff; a ^= a >> 15; a = (a * 0x846ca68b) & 0xffffffff; a ^= a >> 16   # noqa: E702
    assert int(mix(12345)) == a
    # m = 4: most hypotheses find all four within 16 draws
    assert sum(sample_indices(0, 0, t, 4) is not None for t in range(256)) > 200


def test_four_point_solve_is_exact_and_flags_degenerate_samples():
    rng = np.random.Generator(np.random.PCG64(9))
    truth = np.array([[1.1, 0.05, 12.0], [-0.03, 0.95, -7.0], [1e-4, -2e-4, 1.0]])
    src = rng.uniform(0, 600, (50, 4, 2))
    dst = np.stack([project(truth, s) for s in src])
    h, ok = solve4(src, dst)
    assert ok.sum() >= 45                                            # (a random triple can be collinear to within the bar)
    h, src, dst = h[ok], src[ok], dst[ok]
    np.testing.assert_allclose(h / h[:, 2:3, 2:3], np.broadcast_to(truth, h.shape), rtol=0, atol=1e-7)
    assert ((h[:, 2] * np.concatenate([src[:, 0], np.ones((len(src), 1))], 1)).sum(1) > 0).all()
    # agreement with a direct 8 x 8 solve of the DLT equations
    s, d = src[0], dst[0]
    a = np.array([r for (x, y), (u, v) in zip(s, d) for r in ([x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y])])
    ref = np.append(np.linalg.solve(a, d.reshape(-1)), 1).reshape(3, 3)
    np.testing.assert_allclose(h[0] / h[0, 2, 2], ref, rtol=0, atol=1e-7)
    col = src[:3].copy()
    col[:, 2] = (col[:, 0] + col[:, 1]) / 2                          # three collinear src points
    assert not solve4(col, dst[:3])[1].any()
    assert not solve4(src[:3], np.repeat(dst[:3, :1], 4, 1))[1].any()   # identical dst points


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_restatement_recovers_planted_homographies(rho, iterations):
    worst = {}
    for f, (name, i) in enumerate(CASE_NAMES):
        truth, src, dst, planted = planted_case(name, i, rho)
        assert len(src) == 600 and planted.sum() == 600 - int(rho * 600)
        h, inl = ransac_rule(src, dst, dict(iterations=iterations, reproj_threshold=3.0, seed=7, refits=2), f)
        err = corner_error(h, truth)
        worst[name] = max(worst.get(name, 0.0), err)
        assert err <= CORNER_BAR, (name, i, rho, err)
        assert inl[planted].all(), (name, i, rho, int((~inl[planted]).sum()))
        assert h[2, 2] == 1.0
    print("rho %.1f T %d: worst 4-corner error %s" % (rho, iterations, {k: round(v, 3) for k, v in worst.items()}))


def test_restatement_failure_rules():
    truth, src, dst, _ = planted_case("defaults", 0, 0.0)
    p = dict(iterations=64, seed=1)
    for m in (0, 3):
        h, inl = ransac_rule(src[:m], dst[:m], p, 0)
        assert not h.any() and not inl.any()
    h, inl = ransac_rule(src[:4], dst[:4], dict(p, min_inliers=4), 0)
    assert inl.all() and corner_error(h, truth) < 50                 # 4 rounded points pin H only loosely
    assert not ransac_rule(src[:4], dst[:4], p, 0)[0].any()          # the default min_inliers = 8
    same = np.repeat(src[:1], 50, 0)
    assert not ransac_rule(same, same, p, 0)[0].any()                # every sample is degenerate
    h, inl = ransac_rule(src[:100], dst[:100], dict(p, min_inliers=101), 0)
    assert not h.any() and not inl.any()
    h0, _ = ransac_rule(src, dst, dict(p, refits=0), 0)
    assert corner_error(h0, truth) < 10 and h0[2, 2] == 1.0
    # the frame index and the seed are part of the key; the inlier set of a clean case is not
    a = ransac_rule(src, dst, dict(p, refits=0), 0)[0]
    assert not np.array_equal(a, ransac_rule(src, dst, dict(p, refits=0), 1)[0])
    assert not np.array_equal(a, ransac_rule(src, dst, dict(p, refits=0, seed=2), 0)[0])
    assert np.array_equal(a, ransac_rule(src, dst, dict(p, refits=0), 0)[0])
