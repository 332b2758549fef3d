"""CPU checks of the minimal-sample relative pose (fpc_ransac_essential / fpc_essential_frames / fpc_essential_bank): the
header declares it, the binding binds it, the built library exports it -- and this file's float64 restatement of the rule of
include/fpc.h, which the GPU tests (test_gpu_essential_ransac.py) hold the kernels to: the sampler's first 6 distinct of 32
draws; the bearings; the full-pivot elimination of the 5 x 9 system and its four null vectors; the ten cubic constraints
expanded over the header's 20 monomials; Gauss-Jordan with row pivoting; B(z) and its determinant of degree 10; the real
roots by derivative interlacing (fixed bisections and guarded Newton steps inside a Cauchy bound); the null vector of B(z);
the sixth pair's choice; the fundamental rule's fp32 Sampson count and selection; the guarded Gauss-Newton refits on the
essential manifold.  Every operation stands in the order the device performs it (contraction off), with fp32 roundings
where the device rounds.  The sampler, the Sampson terms, the Jacobi routine and the pose rule are imported from
tests/test_fundamental_ransac.py and tests/test_pose_epipolar.py, not written again.

Planted scenes (two families, three outlier shares, PLANTED_M pairs, plain seeds: none was searched): `box` has its points
at depths 4 .. 8, `planar` has them on a plane through depth 6 tilted up to 40 degrees.  Both cameras are K = (500, 500, 320,
240), the motion is a rotation of 2 .. 10 degrees and a baseline of 0.5, the pixels are rounded to integers, and a share rho
of the train pixels is replaced by uniform ones.

Measured with this restatement (printed by the tests below; DESIGN.md section 7 quotes them):
  completeness, 300 noise-free box samples: the sixth pair picks the true E in 293 with the stated root rule and in 293 with
    numpy.roots in its place.  planar: a pick with zero residual on all six pairs (the true E or its plane twin) in 287
    samples, numpy.roots 286, none of numpy.roots' missing; 276 of the 300 samples hold two different such candidates.
  planted scenes, pose through the float64 restatement of fpc_pose_*, against the planted motion or (planar) its plane twin,
    worst rotation / translation-direction error in degrees per (family, outlier share):
        box     0.0: 0.1667 /  0.7299    0.3: 2.5519 / 21.1706    0.6: 0.5814 /  7.2739
        planar  0.0: 0.4760 /  4.1002    0.3: 1.3172 / 16.8627    0.6: 1.9934 / 19.8010
    -> ROT_WORST, DIR_WORST (box, 0.3, the second frame of 36 pairs: 25 planted pairs at integer pixels and two outliers
    inside the mask); the GPU test's bars are twice these.
  iterations at which every planted frame succeeds (not failed, at least 90 % of the planted pairs in the mask): ITERATIONS
    below.  At 0.6 the box frames need the 1 024 (512 keeps 36 of 48 planted pairs on one frame); the 8-point restatement
    on the same frames needs 4 096 (at 2 048 it keeps 15 of 24 on one frame, at 1 024 39 of 80), and it fails every exactly
    planar list at any budget."""
import collections
import ctypes
import functools
import re

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import (KEEP, _draws, _f32, header_text, inliers_of, jacobi,
                                           ransac_rule as fundamental_rule, sampson_terms, unit)
from tests.test_pose_epipolar import KVEC, RANK, angle_deg, kmat, pose_rule
from tests.test_pose_homography import pose_h_rule
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

FPC_E_INVALID = -1
SAMPLE, SOLVED = 6, 5
PIVOT5 = 1e-10              # last pivot / first pivot of the 5 x 9 elimination below which a sample is degenerate
PIVOT10 = 1e-12             # a Gauss-Jordan pivot at or below this share of the first one: degenerate
BISECT, NEWTON = 40, 3      # trips of every bracket of the root walk
DOUBLINGS = 64              # trips of the search for the root bound
SINGULAR = 1e-14            # pivot floor of the refit's 5 x 5 solve, of the largest diagonal entry (refine_pose.h's)
TMIN = 1e-12
DEFAULTS = dict(iterations=1024, reproj_threshold=3.0, seed=0, refits=2, min_inliers=8)
NAMES = ("fpc_ransac_essential", "fpc_essential_frames", "fpc_essential_bank")
TWINS = ("fpc_ransac_fundamental", "fpc_fundamental_frames", "fpc_fundamental_bank")

# ---- polynomials in (x, y, z, 1): variables 0 .. 3; a product's coefficient array is indexed by the sorted variable tuple ---
QUAD = [(i, j) for i in range(4) for j in range(i, 4)]
QIDX = {m: k for k, m in enumerate(QUAD)}
# the header's monomial order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
CUBIC = [(0, 0, 0), (1, 1, 1), (0, 0, 1), (0, 1, 1), (0, 0, 2), (0, 0, 3), (1, 1, 2), (1, 1, 3), (0, 1, 2), (0, 1, 3),
         (0, 2, 2), (0, 2, 3), (0, 3, 3), (1, 2, 2), (1, 2, 3), (1, 3, 3), (2, 2, 2), (2, 2, 3), (2, 3, 3), (3, 3, 3)]
CIDX = {m: k for k, m in enumerate(CUBIC)}


def mul11(a, b, q=None, sub=False):
    """q <- q +- a b, linear x linear -> the 10 quadratic coefficients; the products accumulate in the order i, j"""
    q = [0.0] * 10 if q is None else q
    for i in range(4):
        for j in range(4):
            k = QIDX[(min(i, j), max(i, j))]
            q[k] = q[k] - a[i] * b[j] if sub else q[k] + a[i] * b[j]
    return q


def mul21(q, a, c=None, sub=False):
    """c <- c +- q a, quadratic x linear -> the 20 cubic coefficients in the header's order; the products accumulate in the
    order k, l"""
    c = [0.0] * 20 if c is None else c
    for k, (i, j) in enumerate(QUAD):
        for l in range(4):
            m = CIDX[tuple(sorted((i, j, l)))]
            c[m] = c[m] - q[k] * a[l] if sub else c[m] + q[k] * a[l]
    return c


def zmul(a, b, out=None, sub=False):
    """out <- out +- a b, polynomials in z, ascending powers; the products accumulate in the order i, j"""
    out = [0.0] * (len(a) + len(b) - 1) if out is None else out
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] = out[i + j] - a[i] * b[j] if sub else out[i + j] + a[i] * b[j]
    return out


def horner(c, z):
    """c ascending; v = v z + c_i from the leading coefficient down, every operation rounded"""
    v = c[-1]
    for k in range(len(c) - 2, -1, -1):
        v = v * z + c[k]
    return v


# ---- the minimal solve ------------------------------------------------------------------------------------------------------
def all_samples6(seed, f, iterations, m):
    """[T,6] indices and [T] validity: the first 6 distinct of the 32 draws of every hypothesis, in draw order."""
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


def bearings(xy, k):
    fx, fy, cx, cy = (float(np.float32(v)) for v in k)
    return (xy[..., 0] - cx) / fx, (xy[..., 1] - cy) / fy


def null_basis(a):
    """Full-pivot elimination of a [T,5,9] (the 8-point's pivot order and tie rule) -> (the four null vectors [T,4,9]: free
    unknown k = 1, the other three 0, in the order of the columns 5 .. 8 after the pivoting; ok [T])."""
    a = np.array(a, np.float64)
    n = len(a)
    ar = np.arange(n)
    perm = np.tile(np.arange(9), (n, 1))
    first = last = None
    with np.errstate(all="ignore"):
        for c in range(5):
            sub = np.abs(a[:, c:, c:]).reshape(n, -1)
            k = sub.argmax(1)
            last = sub[ar, k]
            first = last if c == 0 else first
            pr, pc = c + k // (9 - c), c + k % (9 - c)
            tmp = a[ar, c].copy(); a[ar, c] = a[ar, pr]; a[ar, pr] = tmp                      # noqa: E702
            tmp = a[ar, :, c].copy(); a[ar, :, c] = a[ar, :, pc]; a[ar, :, pc] = tmp          # noqa: E702
            tmp = perm[ar, c].copy(); perm[ar, c] = perm[ar, pc]; perm[ar, pc] = tmp          # noqa: E702
            fct = a[:, c + 1:, c] / a[:, c, c][:, None]
            a[:, c + 1:, c + 1:] -= fct[:, :, None] * a[:, c:c + 1, c + 1:]
        ok = (first > 0) & (last >= PIVOT5 * first)
        out = np.zeros((n, 4, 9))
        for k in range(4):
            y = np.zeros((n, 9))
            y[:, 5 + k] = 1.0
            for i in range(4, -1, -1):
                acc = np.zeros(n)
                for j in range(i + 1, 5):
                    acc = acc + a[:, i, j] * y[:, j]
                acc = acc + a[:, i, 5 + k]
                y[:, i] = -acc / a[:, i, i]
            out[ar[:, None], k, perm] = y
    return out, ok


def constraints(basis):
    """basis [T,4,9] -> the 10 x 20 matrix [T,10,20]: row 0 det E, rows 1 .. 9 the entries of (E E^T - tr(E E^T) / 2) E in
    row-major order, over the header's monomials."""
    e = [[[basis[:, v, 3 * r + c] for v in range(4)] for c in range(3)] for r in range(3)]
    m0 = mul11(e[1][2], e[2][1], mul11(e[1][1], e[2][2]), sub=True)
    m1 = mul11(e[1][2], e[2][0], mul11(e[1][0], e[2][2]), sub=True)
    m2 = mul11(e[1][1], e[2][0], mul11(e[1][0], e[2][1]), sub=True)
    rows = [mul21(m2, e[0][2], mul21(m1, e[0][1], mul21(m0, e[0][0]), sub=True))]
    g = {}
    for i in range(3):
        for j in range(i, 3):
            g[(i, j)] = g[(j, i)] = mul11(e[i][2], e[j][2], mul11(e[i][1], e[j][1], mul11(e[i][0], e[j][0])))
    tr = [(x + y) + z for x, y, z in zip(g[(0, 0)], g[(1, 1)], g[(2, 2)])]
    for i in range(3):
        g[(i, i)] = [x - 0.5 * y for x, y in zip(g[(i, i)], tr)]
    for i in range(3):
        for j in range(3):
            rows.append(mul21(g[(i, 2)], e[2][j], mul21(g[(i, 1)], e[1][j], mul21(g[(i, 0)], e[0][j]))))
    return np.stack([np.stack([np.broadcast_to(v, basis.shape[:1]) for v in r], -1) for r in rows], 1)


def gauss_jordan(a, fault=None):
    """Gauss-Jordan of the left 10 x 10 block of a [T,10,20] with row pivoting (largest magnitude of the column at or below
    the diagonal, ties to the lowest row) -> (the right block [T,10,10], ok [T])."""
    a = np.array(a, np.float64)
    n = len(a)
    ar = np.arange(n)
    ok = np.ones(n, bool)
    first = None
    with np.errstate(all="ignore"):
        for c in range(10):
            col = np.abs(a[:, c:, c])
            k = col.argmax(1)
            pv = col[ar, k]
            first = pv if c == 0 else first
            ok &= pv > PIVOT10 * first
            pr = c + k
            tmp = a[ar, c].copy(); a[ar, c] = a[ar, pr]; a[ar, pr] = tmp                      # noqa: E702
            a[:, c, c + 1:] = a[:, c, c + 1:] / a[:, c, c][:, None]
            for i in range(10):
                if i != c:
                    a[:, i, c + 1:] = a[:, i, c + 1:] - a[:, i, c][:, None] * a[:, c, c + 1:]
    return a[:, :, 10:], ok


def bz_rows(r):
    """the right block [T,10,10] -> B(z): three rows of three polynomials in z (ascending), from <x^2 z> - z <x^2>,
    <y^2 z> - z <y^2>, <xyz> - z <xy>"""
    rows = []
    for a, b in ((4, 5), (6, 7), (8, 9)):
        ra, rb = r[:, a], r[:, b]
        rows.append(([ra[:, 2], ra[:, 1] - rb[:, 2], ra[:, 0] - rb[:, 1], -rb[:, 0]],
                     [ra[:, 5], ra[:, 4] - rb[:, 5], ra[:, 3] - rb[:, 4], -rb[:, 3]],
                     [ra[:, 9], ra[:, 8] - rb[:, 9], ra[:, 7] - rb[:, 8], ra[:, 6] - rb[:, 7], -rb[:, 6]]))
    return rows


def det_bz(b):
    c0 = zmul(b[1][2], b[2][1], zmul(b[1][1], b[2][2]), sub=True)
    c1 = zmul(b[1][2], b[2][0], zmul(b[1][0], b[2][2]), sub=True)
    c2 = zmul(b[1][1], b[2][0], zmul(b[1][0], b[2][1]), sub=True)
    return zmul(b[0][2], c2, zmul(b[0][1], c1, zmul(b[0][0], c0), sub=True))


FACT = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0]


def real_roots(p, skip=None):
    """The root walk of include/fpc.h: p a list of 11 arrays [T] (ascending) -> (roots [T,10] ascending, valid [T,10],
    ok [T]).  bound: the first power of two B = 1, 2, 4, .. 2^64 with |p_10| B^10 > sum_(i < 10) |p_i| B^i (Cauchy's
    polynomial, by Horner; none: degenerate).  For d = 1 .. 10 the polynomial P_d = p^(10 - d) (coefficient i: p_(i + 10 - d)
    (i + 10 - d)! / i!) has the break points -bound, the d - 1 roots of level d - 1, bound; every one of its d intervals is
    walked: a change of the sign (v > 0) between its ends is bisected BISECT times, the midpoint of what is left takes
    NEWTON Newton steps, each kept only inside the interval; an interval without a change hands its upper end on, not
    valid."""
    n = len(p[0])
    with np.errstate(all="ignore"):
        ca = [-np.abs(p[i]) for i in range(10)] + [np.abs(p[10])]
        bound = np.ones(n)
        for _ in range(DOUBLINGS):
            bound = np.where(horner(ca, bound) > 0, bound, 2.0 * bound)
        ok = horner(ca, bound) > 0                                   # (false for NaN, and for roots beyond 2^64)
        brk = [-bound, bound]
        valid = []
        for d in range(1, 11):
            k = 10 - d
            c = [p[i + k] * (FACT[i + k] / FACT[i]) for i in range(d + 1)]
            dc = [c[i + 1] * float(i + 1) for i in range(d)]
            nxt, valid = [-bound], []
            for j in range(d):
                lo, hi = brk[j], brk[j + 1]
                flo, fhi = horner(c, lo), horner(c, hi)
                change = (flo > 0) != (fhi > 0)
                for _ in range(BISECT):
                    mid = 0.5 * (lo + hi)
                    same = (horner(c, mid) > 0) == (flo > 0)
                    lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
                r = 0.5 * (lo + hi)
                for _ in range(NEWTON):
                    rn = r - horner(c, r) / horner(dc, r)
                    r = np.where((rn >= lo) & (rn <= hi), rn, r)
                if skip is not None and d == 10 and j == skip:
                    change = np.zeros(n, bool)
                nxt.append(np.where(change, r, brk[j + 1]))
                valid.append(change)
            nxt.append(bound)
            brk = nxt
    return np.stack(brk[1:-1], 1), np.stack(valid, 1), ok


def f_of_e(e, kq, kt):
    """K_t^-T E K_q^-1, e: 9 arrays (row-major) -> 9 arrays"""
    qfx, qfy, qcx, qcy = (float(np.float32(v)) for v in kq)
    tfx, tfy, tcx, tcy = (float(np.float32(v)) for v in kt)
    g = []
    for i in range(3):
        g += [e[3 * i] / qfx, e[3 * i + 1] / qfy, e[3 * i + 2] - (e[3 * i] * (qcx / qfx) + e[3 * i + 1] * (qcy / qfy))]
    f = [g[j] / tfx for j in range(3)] + [g[3 + j] / tfy for j in range(3)]
    f += [g[6 + j] - ((tcx / tfx) * g[j] + (tcy / tfy) * g[3 + j]) for j in range(3)]
    return f


def sampson9(f, x, y, u, v):
    l0, l1, l2 = f[0] * x + f[1] * y + f[2], f[3] * x + f[4] * y + f[5], f[6] * x + f[7] * y + f[8]
    e = u * l0 + v * l1 + l2
    m0, m1 = f[0] * u + f[3] * v + f[6], f[1] * u + f[4] * v + f[7]
    return e, ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1


def candidates(src, dst, kq=KVEC, kt=KVEC, roots=None, fault=None):
    """src, dst [T,>=5,2] -> (E [T,10,9] of every candidate root, valid [T,10], ok [T]).  roots: a function p [11] -> real
    roots replacing the stated walk (numpy.roots, the completeness test).  fault: 'coefficient' | 'root' plants one."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    with np.errstate(all="ignore"):
        x, y = bearings(src[:, :SOLVED], kq)
        u, v = bearings(dst[:, :SOLVED], kt)
        a = np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], -1)
        basis, ok = null_basis(a)
        cm = constraints(basis)
        if fault == "coefficient":
            cm[:, 3, 7] *= 1.001
        right, gok = gauss_jordan(cm)
        ok = ok & gok
        b = bz_rows(right)
        p = det_bz(b)
        if roots is None:
            z, valid, rok = real_roots(p, skip=3 if fault == "root" else None)
            ok = ok & rok
        else:
            z, valid = np.zeros((n, 10)), np.zeros((n, 10), bool)
            for k in range(n):
                got = roots(np.array([c[k] for c in p]))
                z[k, :len(got)], valid[k, :len(got)] = got, True
        es = np.zeros((n, 10, 9))
        for j in range(10):
            zj = z[:, j]
            bv = [[horner(poly, zj) for poly in row] for row in b]
            n0 = bv[0][1] * bv[1][2] - bv[0][2] * bv[1][1]
            n1 = bv[0][2] * bv[1][0] - bv[0][0] * bv[1][2]
            n2 = bv[0][0] * bv[1][1] - bv[0][1] * bv[1][0]
            xx, yy = n0 / n2, n1 / n2
            valid[:, j] &= (np.abs(xx) < 1e300) & (np.abs(yy) < 1e300)
            for q in range(9):
                es[:, j, q] = ((xx * basis[:, 0, q] + yy * basis[:, 1, q]) + zj * basis[:, 2, q]) + basis[:, 3, q]
    return es, valid & ok[:, None], ok


def solve5(src, dst, kq=KVEC, kt=KVEC, roots=None, fault=None):
    """The minimal solve, batched: src, dst [T,6,2] -> (E [T,9], F [T,9] = K_t^-T E K_q^-1, ok [T]): the candidate with the
    smallest Sampson error (squared, in pixels through F) of the sixth pair; ties go to the lower root."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    es, valid, _ = candidates(src, dst, kq, kt, roots, fault)
    best = np.full(n, np.inf)
    have = np.zeros(n, bool)
    eb, fb = np.zeros((n, 9)), np.zeros((n, 9))
    with np.errstate(all="ignore"):
        for j in range(10):
            e = [es[:, j, q] for q in range(9)]
            f = f_of_e(e, kq, kt)
            r, g = sampson9(f, src[:, 5, 0], src[:, 5, 1], dst[:, 5, 0], dst[:, 5, 1])
            err = (r * r) / g
            take = valid[:, j] & (err < 1e300) & (~have | (err < best))
            best[take] = err[take]
            eb[take], fb[take] = es[take, j], np.stack(f, 1)[take]
            have |= take
    return eb, fb, have


def hypotheses(f, ok):
    """F [T,9] scaled to max |f| = 1 (what is rounded to fp32 and counted) -> (F [T,9], ok)"""
    with np.errstate(all="ignore"):
        mx = np.abs(f).max(1)
        ok = ok & (mx > 0) & (mx < 1e300)
        f = f / np.where(ok, mx, 1.0)[:, None]
        ok = ok & (np.abs(f) <= 1.0).all(1)
    f[~ok] = 0.0
    return f, ok


# ---- the refit: one guarded Gauss-Newton step on the essential manifold -----------------------------------------------------
def decompose(f, kq, kt):
    """pose_epipolar's decomposition of F (fp32 values), candidate 0 -> (R, t) or None"""
    e = kmat(kt).T @ f.reshape(3, 3) @ kmat(kq)
    mx = np.abs(e).max()
    if not (mx > 0 and mx < 1e300):
        return None
    e = e / mx
    d, v = jacobi(e.T @ e)
    i1 = int(np.argmax(d))
    rest = d.copy()
    rest[i1] = -np.inf
    i2 = int(np.argmax(rest))
    if not d[i2] > RANK * d[i1]:
        return None
    v1, v2 = v[:, i1], v[:, i2]
    v3 = np.cross(v1, v2)
    with np.errstate(all="ignore"):
        u1 = e @ v1
        u1 = u1 / np.sqrt(u1 @ u1)
        u2 = e @ v2
        u2 = u2 - (u1 @ u2) * u1
        u2 = u2 / np.sqrt(u2 @ u2)
    u3 = np.cross(u1, u2)
    r = (np.outer(u2, v1) - np.outer(u1, v2)) + np.outer(u3, v3)
    if not (np.isfinite(r).all() and np.isfinite(u3).all()):
        return None
    return r, u3


def tangent_basis(t):
    """refine_pose.h's rp_basis"""
    k = int(np.argmin(np.abs(t)))                                    # ties: the lowest index
    b1 = np.cross(t, np.eye(3)[k])
    b1 = b1 / np.sqrt(b1 @ b1)
    b2 = np.cross(t, b1)
    return b1, b2 / np.sqrt(b2 @ b2)


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def f_from_pose(r, t, kq, kt):
    e = skew(t) @ r
    return np.array(f_of_e(list(e.reshape(-1)), kq, kt))


def gauss_newton_step(f, src, dst, inl, kq, kt, guard=True):
    """One step from the fp32 F over the pairs `inl` -> the new unit fp32 F, or None.  The state is candidate 0 of the
    decomposition; the residual is e / sqrt(g) in pixels; the Jacobian holds g fixed; the update is R' = Q(omega) R with Q
    the rotation of the unit quaternion (1, omega / 2) / |.|, t' = (Q t + B eta) / |.|."""
    dec = decompose(f, kq, kt)
    if dec is None:
        return None
    r, t = dec
    b1, b2 = tangent_basis(t)
    fu = f_from_pose(r, t, kq, kt)
    s, d = src[inl], dst[inl]
    with np.errstate(all="ignore"):
        e, g = sampson9(fu, s[:, 0], s[:, 1], d[:, 0], d[:, 1])
        sg = np.sqrt(g)
        res = e / sg
        px, py = bearings(s, kq)
        qx, qy = bearings(d, kt)
        ph, qh = np.stack([px, py, np.ones_like(px)], 1), np.stack([qx, qy, np.ones_like(qx)], 1)
        a = ph @ r.T
        c = np.cross(t, a)
        jw = np.cross(c, qh)
        aq = np.cross(a, qh)
        jac = np.concatenate([jw, (aq @ b1)[:, None], (aq @ b2)[:, None]], 1) / sg[:, None]
        sm = jac.T @ jac
        rhs = -(jac.T @ res)
        tiny = SINGULAR * np.diag(sm).max()
        sol = solve_partial(sm, rhs, tiny)
        if sol is None:
            return None
        h = 0.5 * sol[:3]
        nq = np.sqrt(1.0 + h @ h)
        w, (v0, v1, v2) = 1.0 / nq, h / nq
        q = np.array([[1 - 2 * (v1 * v1 + v2 * v2), 2 * (v0 * v1 - w * v2), 2 * (v0 * v2 + w * v1)],
                      [2 * (v0 * v1 + w * v2), 1 - 2 * (v0 * v0 + v2 * v2), 2 * (v1 * v2 - w * v0)],
                      [2 * (v0 * v2 - w * v1), 2 * (v1 * v2 + w * v0), 1 - 2 * (v0 * v0 + v1 * v1)]])
        tn = q @ t + (b1 * sol[3] + b2 * sol[4])
        nt = np.sqrt(tn @ tn)
        if not nt > TMIN:
            return None
        new = unit(f_from_pose(q @ r, tn / nt, kq, kt).reshape(3, 3))
    return None if new is None else new.reshape(-1)


def solve_partial(a, b, tiny):
    """ransac_parts.h's solve_lds: partial pivoting, a pivot at or below tiny fails"""
    n = len(b)
    m = np.concatenate([np.array(a, np.float64), np.array(b, np.float64)[:, None]], 1)
    for c in range(n):
        pr = c + int(np.argmax(np.abs(m[c:, c])))
        if not abs(m[pr, c]) > tiny:
            return None
        m[[c, pr]] = m[[pr, c]]
        ip = 1.0 / m[c, c]
        for i in range(c + 1, n):
            m[i, c:] -= (m[i, c] * ip) * m[c, c:]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (m[i, n] - m[i, i + 1:n] @ x[i + 1:]) / m[i, i]
    return x


def unit_e(f, kq, kt):
    """E_dev of the returned F: K_t^T F K_q, Frobenius norm 1, fp32, the largest-magnitude element positive"""
    e = unit(kmat(kt).T @ f.reshape(3, 3) @ kmat(kq))
    return np.zeros(9) if e is None else e.reshape(-1)


Essential = collections.namedtuple("Essential", "F E ninliers mask failed best_t first accepted")


def _failed(m, best_t=-1):
    return Essential(np.zeros(9), np.zeros(9), 0, np.zeros(m, bool), True, best_t, None, 0)


def essential_rule(src, dst, params, f, kq=KVEC, kt=KVEC, fault=None):
    """The whole rule for frame index f: src, dst [M,2] (float32 values) -> Essential.  fault: 'coefficient', 'root' or
    'guard' plants a fault in that stage."""
    p = dict(DEFAULTS, **params)
    thr = float(np.float32(p["reproj_threshold"]))
    src, dst = _f32(src).reshape(-1, 2), _f32(dst).reshape(-1, 2)
    m = len(src)
    if m < SAMPLE:
        return _failed(m)
    idx, ok = all_samples6(p["seed"], f, p["iterations"], m)
    _, fs, sok = solve5(src[idx], dst[idx], kq, kt, fault=fault)
    hyp, ok = hypotheses(fs, ok & sok)
    e2, g = sampson_terms(_f32(hyp).reshape(-1, 3, 3), src, dst)
    counts = (e2 < thr * thr * g).sum(1) * ok
    if counts.max() <= 0:
        return _failed(m)
    best = int(np.argmax(counts))                                    # the largest count, ties to the lower t
    cur = unit(fs[best].reshape(3, 3))
    if cur is None:
        return _failed(m, best)
    cur = cur.reshape(-1)
    first, accepted = cur, 0
    inl = inliers_of(cur.reshape(3, 3), src, dst, thr)
    for _ in range(p["refits"]):
        if inl.sum() < SAMPLE:
            break
        new = gauss_newton_step(cur, src, dst, inl, kq, kt)
        if new is None:
            break
        ninl = inliers_of(new.reshape(3, 3), src, dst, thr)
        if fault != "guard" and ninl.sum() < inl.sum():
            break
        cur, inl, accepted = new, ninl, accepted + 1
    if inl.sum() < p["min_inliers"]:
        return _failed(m, best)
    return Essential(cur, unit_e(cur, kq, kt), int(inl.sum()), inl, False, best, first, accepted)


# ---- planted scenes -------------------------------------------------------------------------------------------------------
FRAME_H, FRAME_W = 480, 640
FAMILIES = ("box", "planar")
ITERATIONS = {0.0: 256, 0.3: 256, 0.6: 1024}       # at which every planted frame succeeds (measured; the module docstring)
CASE_SETS = sorted(ITERATIONS.items())
# pairs per frame: 24 planted pairs at the least (24 is the issue's floor; below it a frame at rho = 0.6 would hold 10 planted
# pairs against a min_inliers of 8), 200 at the most
PLANTED_M = {0.0: (24, 60, 200), 0.3: (36, 90, 200), 0.6: (60, 120, 200)}
SCENE_IDS = (0, 1)
PARAMS = dict(reproj_threshold=2.0, seed=7, refits=2, min_inliers=8)
DEPTH, PLANE_DEPTH, PLANE_TILT, BASELINE = (4.0, 8.0), 6.0, 40.0, 0.5
# worst errors of the restatement's pose over the 36 planted frames (test_restatement_recovers_planted_poses prints them);
# the GPU test allows twice these: the fp32 F and the fp32 accept decisions
ROT_WORST, DIR_WORST = 2.5519, 21.1706
ROT_BAR, DIR_BAR = 2 * ROT_WORST, 2 * DIR_WORST


def _rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    k = skew(axis)
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def exact_scene(family, i, m, k=KVEC, offplane=0.0):
    """m unrounded pairs of one motion (a rotation of 2 .. 10 degrees, a baseline of 0.5): query pixels uniform in the frame,
    depths 4 .. 8 (box) or on a plane through depth 6 tilted 0 .. 40 degrees (planar; a share `offplane` of the points is
    pulled 0.5 .. 1.5 in front of it) -> (src, dst, R, t, plane (n, d) in the query camera's frame or None)."""
    fx, fy, cx, cy = k
    rng = np.random.default_rng([{"box": 1, "planar": 2}[family], i, m])
    while True:
        r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 10.0)))
        d = rng.normal(size=3)
        t = BASELINE * d / np.linalg.norm(d)
        px = np.stack([rng.uniform(8, FRAME_W - 8, 4 * m), rng.uniform(8, FRAME_H - 8, 4 * m)], 1)
        ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(len(px))], 1)
        tilt, phi = np.deg2rad(rng.uniform(0.0, PLANE_TILT)), rng.uniform(0.0, 2.0 * np.pi)
        nrm = np.array([np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi), np.cos(tilt)])
        z = rng.uniform(*DEPTH, len(px))
        if family == "planar":
            z = PLANE_DEPTH * nrm[2] / (ray @ nrm)
            lift = rng.uniform(0.5, 1.5, len(px)) * (rng.uniform(size=len(px)) < offplane)
            z = z - lift
        xq = ray * z[:, None]
        xt = xq @ r.T + t
        q = np.stack([fx * xt[:, 0] / xt[:, 2] + cx, fy * xt[:, 1] / xt[:, 2] + cy], 1)
        ok = (z > 1.0) & (xt[:, 2] > 1.0) & (q[:, 0] >= 0) & (q[:, 0] <= FRAME_W - 1) & (q[:, 1] >= 0) & (q[:, 1] <= FRAME_H - 1)
        if ok.sum() >= m:
            return px[ok][:m], q[ok][:m], r, t, ((nrm, PLANE_DEPTH * nrm[2]) if family == "planar" else None)


def planted_scene(family, i, rho, m, offplane=0.0):
    """exact_scene rounded to integer pixels, a share rho of the train pixels replaced by uniform ones
    -> (src, dst (float32), planted mask, R, t, plane)."""
    src, dst, r, t, plane = exact_scene(family, i, m, offplane=offplane)
    rng = np.random.default_rng([9, {"box": 1, "planar": 2}[family], i, m, int(round(100 * rho))])
    src, dst = np.rint(src), np.rint(dst)
    planted = np.ones(m, bool)
    nout = int(round(rho * m))
    if nout:
        out = rng.choice(m, nout, replace=False)
        dst[out] = np.stack([rng.integers(0, FRAME_W, nout), rng.integers(0, FRAME_H, nout)], 1)
        planted[out] = False
    return src.astype(np.float32), dst.astype(np.float32), planted, r, t, plane


def planted_batch(family, rho):
    """The frames of one case set: two scenes of every M (6 frames)."""
    return [planted_scene(family, i, rho, m) for m in PLANTED_M[rho] for i in SCENE_IDS]


@functools.lru_cache(maxsize=None)
def restated_batch(family, rho, iterations):
    scenes = planted_batch(family, rho)
    return scenes, [essential_rule(s[0], s[1], dict(PARAMS, iterations=iterations), f) for f, s in enumerate(scenes)]


def truths(scene):
    """The motions that explain the planted pairs: (R, t) as planted and, for a planar scene, its plane twin -- the other
    (R, +-t) among the candidates of the float64 restatement of fpc_pose_homography on the planted homography
    K (R + t n^T / d) K^-1.  The twin fits the pairs as an essential matrix whether or not its points lie in front of both
    cameras, so it is taken from the candidates, before their cheirality test, and its t counts up to sign."""
    r0, t0, plane = scene[3], scene[4], scene[5]
    out = [(r0, t0 / np.linalg.norm(t0), False)]
    if plane is not None:
        h = kmat(KVEC) @ (r0 + np.outer(t0, plane[0]) / plane[1]) @ np.linalg.inv(kmat(KVEC))
        sel = scene[2]
        got = pose_h_rule(scene[0][sel], scene[1][sel], h, thr=PARAMS["reproj_threshold"])
        for cand in got.cands[::2]:
            if cand is not None and pose_distance(cand[0], cand[1], out[0])[0] > 1e-3:
                out.append((cand[0], cand[1], True))
    return out


def pose_distance(r, t, truth):
    r0, t0, free_sign = truth
    c = np.asarray(t, np.float64) @ t0
    return (angle_deg((np.trace(np.asarray(r, np.float64) @ r0.T) - 1.0) / 2.0), angle_deg(abs(c) if free_sign else c))


def pose_errors(r, t, scene):
    """(rotation angle error, angle between t and the planted direction), degrees, against the nearest of truths(scene)"""
    return min((pose_distance(r, t, tr) for tr in truths(scene)), key=lambda e: e[0] / ROT_WORST + e[1] / DIR_WORST)


def restated_pose(scene, res, thr=PARAMS["reproj_threshold"]):
    return pose_rule(scene[0], scene[1], _f32(res.F).reshape(3, 3), thr=thr)


def same_e(e, e0, bar=1e-6):
    e, e0 = np.asarray(e, np.float64).reshape(-1), np.asarray(e0, np.float64).reshape(-1)
    e, e0 = e / np.linalg.norm(e), e0 / np.linalg.norm(e0)
    return min(np.linalg.norm(e - e0), np.linalg.norm(e + e0)) < bar


def exact_samples(family, count):
    s = [exact_scene(family, 100 + i, SAMPLE) for i in range(count)]    # (plain seeds 100 ..: apart from the planted scenes')
    return (np.stack([v[0] for v in s]), np.stack([v[1] for v in s]),
            np.stack([(skew(v[3]) @ v[2]).reshape(-1) for v in s]))


# "Zero residual" of a noise-free sample, Sampson distance in pixels: three orders below the 0.29 px a rounded pixel is off by
# and six above the 1e-10 px a well-conditioned sample leaves.  (Not 1e-6: planar sample 65 has a cluster of seven roots
# within 0.3, its two finders agree on the chosen root to six digits and leave 1.14e-6 and 0.92e-6 px -- the same answer on
# either side of such a bar.)
ZERO_PX = 1e-4


def np_roots(p):
    r = np.roots(p[::-1])
    return np.sort(r[np.abs(r.imag) <= 1e-9 * np.maximum(1.0, np.abs(r))].real)[:10]


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    lib = _lib.load()
    for name in NAMES + ("fpc_default_essential_params",):
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    for name, twin in zip(NAMES, TWINS):         # the twins' argument lists with the new struct and E_dev behind F_dev
        args = [re.sub(r"\s+", " ", re.search(r"\bint %s\s*\(([^)]*)\)" % n, hdr).group(1)) for n in (name, twin)]
        assert args[0] == args[1].replace("fpc_ransac_params", "fpc_essential_params").replace("float* F_dev,",
                                                                                               "float* F_dev, float* E_dev,"), name
        want = list(getattr(lib, twin).argtypes)
        k = want.index(ctypes.POINTER(_lib.FpcRansacParams))
        want[k] = ctypes.POINTER(_lib.FpcEssentialParams)
        want.insert(k + 2, ctypes.c_void_p)
        assert list(getattr(lib, name).argtypes) == want, name
    assert re.search(r"#define\s+FPC_ABI_VERSION\s+4\b", header_text())
    assert lib.fpc_abi_version() == 4
    body = re.search(r"typedef struct fpc_essential_params \{(.*?)\} fpc_essential_params;", hdr, re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [f[0] for f in _lib.FpcEssentialParams._fields_]
    assert fields[:5] == [f[0] for f in _lib.FpcRansacParams._fields_]
    assert fields[5:] == [f[0] for f in _lib.FpcPoseParams._fields_[:8]]


def test_defaults_and_null_arguments():
    lib = _lib.load()
    p = _lib.FpcEssentialParams()
    assert lib.fpc_default_essential_params(None) == FPC_E_INVALID
    assert lib.fpc_default_essential_params(ctypes.byref(p)) == 0
    assert (p.iterations, p.reproj_threshold, p.seed, p.refits, p.min_inliers) == (1024, 3.0, 0, 2, 8)
    assert (p.q_fx, p.q_fy, p.q_cx, p.q_cy, p.t_fx, p.t_fy, p.t_cx, p.t_cy) == (500.0, 500.0, 320.0, 240.0) * 2
    assert DEFAULTS == {k: getattr(p, k) for k in DEFAULTS}
    buf = (ctypes.c_float * 64)()
    b = ctypes.addressof(buf)
    pp = ctypes.byref(p)
    assert lib.fpc_ransac_essential(None, 1, b, b, b, 1, pp, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_essential_frames(None, 1, 0, b, b, b, pp, b, b, b, b) == FPC_E_INVALID
    assert lib.fpc_essential_bank(None, 1, b, b, pp, b, b, b, b) == FPC_E_INVALID


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_sampler_takes_the_first_six_of_the_eight_point_draws():
    from tests.test_fundamental_ransac import _all_samples
    idx, ok = all_samples6(7, 3, 64, 40)
    assert ok.all() and all(len(set(row)) == SAMPLE for row in idx.tolist()) and idx.max() < 40
    idx8, ok8 = _all_samples(7, 3, 64, 40)
    np.testing.assert_array_equal(idx[ok8], idx8[ok8][:, :6])
    assert (all_samples6(8, 3, 64, 40)[0] != idx).any() and (all_samples6(7, 4, 64, 40)[0] != idx).any()
    assert not all_samples6(7, 0, 16, 5)[1].any()


def test_monomial_tables_and_constraints_vanish_on_a_true_essential_matrix():
    assert len(set(CUBIC)) == 20 and all(tuple(sorted(m)) == m for m in CUBIC)
    src, dst, es = exact_samples("box", 20)
    x, y = bearings(src[:, :SOLVED], KVEC)
    u, v = bearings(dst[:, :SOLVED], KVEC)
    basis, ok = null_basis(np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], -1))
    assert ok.all()
    cm = constraints(basis)
    for k in range(len(src)):
        e0 = es[k]
        coef, *_ = np.linalg.lstsq(basis[k].T, e0, rcond=None)          # the true E in the basis: (x, y, z, w)
        assert np.abs(basis[k].T @ coef - e0).max() < 1e-9 * np.abs(e0).max()
        xv = np.append(coef[:3] / coef[3], 1.0)
        mono = np.array([xv[a] * xv[b] * xv[c] for a, b, c in CUBIC])
        assert np.abs(cm[k] @ mono).max() <= 1e-8 * (np.abs(cm[k]) * np.abs(mono)).sum(1).max(), k


@pytest.mark.parametrize("family", FAMILIES)
def test_completeness_of_the_solve(family):
    """300 seeded noise-free samples.  general: the sixth pair picks the true E at least as often as with numpy.roots in
    the place of the root walk, minus 3.  planar: the pick has zero residual on all six pairs (the true E or its plane
    twin) in every sample where the numpy.roots pick has; and the ambiguity is shown: two different candidates, both with
    zero residual on all six pairs."""
    src, dst, es = exact_samples(family, 300)
    e1, f1, ok1 = solve5(src, dst)
    e2, f2, ok2 = solve5(src, dst, roots=np_roots)

    def residual(f, k):
        ee, g = sampson_terms(f[k].reshape(3, 3), src[k], dst[k])
        return float(np.sqrt(ee / g).max())
    true1 = np.array([ok1[k] and same_e(e1[k], es[k]) for k in range(300)])
    true2 = np.array([ok2[k] and same_e(e2[k], es[k]) for k in range(300)])
    zero1 = np.array([ok1[k] and residual(f1, k) < ZERO_PX for k in range(300)])
    zero2 = np.array([ok2[k] and residual(f2, k) < ZERO_PX for k in range(300)])
    print("%s: true E picked %d of 300 (root walk), %d (numpy.roots); zero residual on six pairs %d / %d"
          % (family, true1.sum(), true2.sum(), zero1.sum(), zero2.sum()))
    if family == "box":
        assert true1.sum() >= true2.sum() - 3
        assert true1.sum() >= 280
    else:
        assert (zero1 | ~zero2).all(), np.flatnonzero(~zero1 & zero2)
        es_all, valid, _ = candidates(src, dst)
        twofold = 0
        for k in range(300):
            good = []
            for j in np.flatnonzero(valid[k]):
                f = np.array(f_of_e(list(es_all[k, j]), KVEC, KVEC))
                ee, g = sampson_terms(f.reshape(3, 3), src[k], dst[k])
                if np.sqrt(ee / g).max() < ZERO_PX and not any(same_e(es_all[k, j], es_all[k, i], 1e-4) for i in good):
                    good.append(j)
            twofold += len(good) >= 2
        print("planar: %d of 300 samples have two different candidates with zero residual on all six pairs" % twofold)
        assert twofold >= 150


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_restatement_recovers_planted_poses(family, rho, iterations):
    scenes, results = restated_batch(family, rho, iterations)
    worst = np.zeros(2)
    for f, (scene, res) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not res.failed, (family, rho, f, m)
        pose = restated_pose(scene, res)
        assert not pose.failed, (family, rho, f, m)
        errs = pose_errors(pose.R, pose.t, scene)
        worst = np.maximum(worst, errs)
        planted = scene[2]
        assert res.ninliers == res.mask.sum() >= PARAMS["min_inliers"]
        assert res.mask[planted].sum() >= 0.9 * planted.sum(), (family, rho, f)
        # (a uniform pixel lies within 2 px of a given epipolar line with a chance near 4 x 800 / (640 x 480) = 1 %, and the
        # selection prefers the models it happens to agree with: a tenth of the outliers and two are allowed inside)
        assert res.mask[~planted].sum() <= 2 + 0.1 * (~planted).sum(), (family, rho, f)
        assert abs(np.sqrt((res.F * res.F).sum()) - 1.0) < 1e-6 and res.F[np.argmax(np.abs(res.F))] > 0
        sv = np.linalg.svd(res.E.reshape(3, 3), compute_uv=False)
        assert sv[2] <= 1e-6 * sv[0] and abs(sv[0] - sv[1]) <= 1e-5 * sv[0]          # on the essential manifold, in fp32
        print("%s rho %.1f frame %d M %3d: rotation %.4f deg, direction %.4f deg, %d inliers of %d planted, %d refits kept"
              % (family, rho, f, m, *errs, res.ninliers, planted.sum(), res.accepted))
    print("%s rho %.1f T %d: worst rotation %.4f deg, worst direction %.4f deg" % (family, rho, iterations, *worst))
    assert worst[0] <= ROT_WORST + 1e-4 and worst[1] <= DIR_WORST + 1e-4          # the constants are the measured worst


def test_the_eight_point_rule_on_the_same_scenes():
    """Beside ITERATIONS: the 8-point restatement at the same budgets, same threshold, min_inliers 8.  Exactly planar pairs
    (unrounded, no outlier) fail at ANY budget -- every sample is degenerate -- where this rule returns a full mask."""
    for name, (src, dst) in exact_planar_lists().items():
        f8, m8 = fundamental_rule(src, dst, dict(PARAMS, iterations=1024), 0)
        assert not f8.any() and not m8.any(), name
        res = essential_rule(src, dst, dict(PARAMS, iterations=64), 0)
        assert not res.failed and res.mask.all(), name
    fails = {}
    for family in FAMILIES:
        for rho, iterations in CASE_SETS:
            scenes, results = restated_batch(family, rho, iterations)
            bad = 0
            for f, s in enumerate(scenes):
                f8, m8 = fundamental_rule(s[0], s[1], dict(PARAMS, iterations=iterations), f)
                bad += (not f8.any()) or m8[s[2]].sum() < KEEP * s[2].sum()
            fails[(family, rho)] = bad
            assert not any(r_.failed for r_ in results)
    print("8-point restatement, frames of 6 that fail or keep under 98 %% of the planted pairs at this rule's budgets:", fails)


def exact_planar_lists():
    """Pair lists that follow a homography EXACTLY (integers and quarters, exact in fp32) and hold no outlier: a grid of 50
    query pixels under an image shift (a sideways motion in front of a fronto-parallel plane) and under a zoom of 1.25
    about the principal point (a forward motion towards it)."""
    g = np.stack(np.meshgrid(np.arange(40.0, 600.0, 56.0), np.arange(40.0, 440.0, 80.0)), -1).reshape(-1, 2)
    return {"shift": (g, g + [24.0, -8.0]), "zoom": (g, [320.0, 240.0] + 1.25 * (g - [320.0, 240.0]))}


# T = 128: established below -- the 8-point restatement keeps fewer than KEEP (its own tests' 0.98) of the planted pairs on 4
# of the 6 frames (at 32 .. 256 alike: it settles on the plane's pairs), this rule on none
GAP = dict(offplane=0.15, rho=0.5, m=200, iterations=128, frames=6)


@functools.lru_cache(maxsize=None)
def gap_batch():
    """A plane with 15 % of the points off it and 50 % outliers, at a budget where the 8-point restatement fails on at least
    one frame and this rule on none (established here, used by the GPU test)."""
    scenes = [planted_scene("planar", 10 + i, GAP["rho"], GAP["m"], offplane=GAP["offplane"]) for i in range(GAP["frames"])]
    params = dict(PARAMS, iterations=GAP["iterations"])
    ours = [essential_rule(s[0], s[1], params, f) for f, s in enumerate(scenes)]
    theirs = [fundamental_rule(s[0], s[1], params, f) for f, s in enumerate(scenes)]
    return scenes, ours, theirs


def test_the_gap_on_a_mostly_planar_scene():
    scenes, ours, theirs = gap_batch()
    lost = 0
    for f, (s, a, (f8, m8)) in enumerate(zip(scenes, ours, theirs)):
        planted = s[2]
        assert not a.failed and a.mask[planted].sum() >= KEEP * planted.sum(), f
        lost += (not f8.any()) or m8[planted].sum() < KEEP * planted.sum()
        print("frame %d: essential %d inliers of %d planted; 8-point %d" % (f, a.ninliers, planted.sum(), m8[planted].sum()))
    assert lost >= 1


def test_restatement_failure_rules():
    src, dst, _, _, _, _ = planted_scene("box", 0, 0.0, 60)
    params = dict(PARAMS, iterations=64)
    assert essential_rule(src[:5], dst[:5], params, 0).failed                        # fewer than 6 pairs
    assert not essential_rule(src[:6], dst[:6], dict(params, min_inliers=6), 0).failed
    res = essential_rule(src, dst, dict(params, min_inliers=61), 0)
    assert res.failed and not res.F.any() and not res.E.any() and res.ninliers == 0 and not res.mask.any()
    assert essential_rule(np.repeat(src[:1], 50, 0), np.repeat(dst[:1], 50, 0), params, 0).failed   # all pairs identical
    res = essential_rule(src, dst, dict(params, refits=0), 0)
    np.testing.assert_array_equal(res.F, res.first)
    more = essential_rule(src, dst, dict(params, refits=4), 0)
    assert more.best_t == res.best_t and more.ninliers >= res.ninliers               # the guard: never fewer inliers


@pytest.mark.parametrize("fault", ["coefficient", "root", "guard"])
def test_a_planted_fault_in_each_stage_is_caught(fault):
    """One constraint coefficient off by 1e-3, one root skipped, the monotone guard removed: each changes what the comparison
    of test_gpu_essential_ransac.py compares (the chosen E of exact samples, the returned F or mask of planted frames)."""
    src, dst, es = exact_samples("box", 100)
    e0, _, ok0 = solve5(src, dst)
    if fault != "guard":
        e1, _, ok1 = solve5(src, dst, fault=fault)
        changed = sum(ok0[k] != ok1[k] or (ok0[k] and not same_e(e0[k], e1[k], 1e-9)) for k in range(100))
        hit0 = sum(ok0[k] and same_e(e0[k], es[k]) for k in range(100))
        hit1 = sum(ok1[k] and same_e(e1[k], es[k]) for k in range(100))
        print("%s: %d of 100 picks change; true E picked %d -> %d" % (fault, changed, hit0, hit1))
        assert changed >= 5 and hit1 < hit0
        return
    differ = 0
    for family in FAMILIES:
        for rho, iterations in CASE_SETS:
            scenes, results = restated_batch(family, rho, iterations)
            for f, (s, r0) in enumerate(zip(scenes, results)):
                r1 = essential_rule(s[0], s[1], dict(PARAMS, iterations=iterations, refits=4), f, fault="guard")
                r2 = essential_rule(s[0], s[1], dict(PARAMS, iterations=iterations, refits=4), f)
                assert r2.ninliers >= r0.ninliers or r2.accepted <= r0.accepted
                differ += not np.array_equal(r1.F, r2.F)
    print("guard removed: %d of 36 frames return another F at 4 refits" % differ)
    assert differ >= 1


def test_kernels_use_no_scratch_and_two_workgroups_fit_a_cu(code_object):  # noqa: F811
    """The built code object: nothing in scratch, no spills; the score kernel's systems take 80 KiB, half of a CU's LDS."""
    _, meta = code_object
    for kernel, lds in (("essential_score_kernel", 80 << 10), ("essential_refit_kernel", 4 << 10)):
        names = [n for n in meta if kernel in n]
        assert len(names) == 1, sorted(n for n in meta if "essential" in n)
        m = meta[names[0]]
        print(kernel, m)
        # (SGPRs that do not fit are kept in VGPR lanes, not in memory: the scratch size is the condition)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m
        assert m["group_segment_fixed_size"] <= lds and m["vgpr_count"] <= 512, m
