"""CPU checks of batched descriptor matching (fpc_match_frames / fpc_first_within_frames): the entry points refuse a NULL
context, and this file's float64 restatement of the batched rule -- which the GPU tests (test_gpu_match_frames.py) hold
the kernel to -- agrees with the oracle's pairwise matcher, plus Lowe's ratio test on planted cases."""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

FPC_E_INVALID = -1
PAIR_KEY, PAIR_PREVIOUS = 0, 1


def pair_rule(q, t, cross_check=True, max_dist=0.0, ratio=0.0, gram=None):
    """One pair in float64 -> (match int32[nq], d1 float64[nq], d2 float64[nq]).  Nearest / second-nearest train row in
    (distance, index) order; a row with no train rows: -1, +inf; fewer than two train rows: d2 = +inf and the ratio test
    fails.  Non-finite descriptor rows (include/fpc.h): a pair whose distance is NaN or +inf is no minimum of its row or
    column and no second best -- it is masked to +inf here, and +inf never wins; a row without a finite distance is
    -1 / +inf.  (The library decides "finite" on its fp32 d^2; rows that hold a NaN or an Inf are non-finite in both.)
    gram: the float64 products q t^T by another routine than the matrix product -- tests/test_match_edges.py passes an
    einsum, whose dot products all run through one loop, so that bit-equal rows give bit-equal distances (a blocked GEMM
    need not)."""
    nq, nt = len(q), len(t)
    m = np.full(nq, -1, np.int32)
    d1, d2 = np.full(nq, np.inf), np.full(nq, np.inf)
    if nq == 0 or nt == 0:
        return m, d1, d2
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        qt = q64 @ t64.T if gram is None else gram(q64, t64)
        dd = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * qt
        dd = np.sqrt(np.maximum(dd, 0.0))
    dd[~np.isfinite(dd)] = np.inf
    order = np.argsort(dd, axis=1, kind="stable")            # equal distances keep the lower index first
    rows = np.arange(nq)
    best = order[:, 0]
    d1 = dd[rows, best]
    if nt >= 2:
        d2 = dd[rows, order[:, 1]]
    ok = np.isfinite(d1)
    if cross_check:
        ok &= np.argmin(dd, axis=0)[best] == rows              # argmin: the first (lowest) row on ties
    if max_dist > 0:
        ok &= d1 < max_dist
    if ratio > 0:
        ok &= np.isfinite(d2) & (d1 < ratio * d2)              # (fewer than two finite distances: d2 = +inf)
    m[ok] = best[ok]
    return m, d1, d2


def frames_rule(desc, counts, key, pairing, cross_check=True, max_dist=0.0, ratio=0.0):
    """The batched rule: desc [n][cap][D], counts [n], key [k][D] or None -> (match [n][cap], d1 [n][cap],
    d2 [n][cap]); rows past a frame's count are -1 / +inf."""
    n, cap = len(counts), desc.shape[1]
    m = np.full((n, cap), -1, np.int32)
    d1, d2 = np.full((n, cap), np.inf), np.full((n, cap), np.inf)
    for f in range(n):
        q = desc[f, :counts[f]]
        if pairing == PAIR_PREVIOUS and f > 0:
            t = desc[f - 1, :counts[f - 1]]
        else:
            t = key if key is not None else desc[f, :0]
        mf, a, b = pair_rule(q, t, cross_check, max_dist, ratio)
        m[f, :counts[f]], d1[f, :counts[f]], d2[f, :counts[f]] = mf, a, b
    return m, d1, d2


def _unit(rng, k, dim=128):
    v = rng.normal(size=(k, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    m = np.zeros(8, np.int32)
    assert lib.fpc_match_frames(None, 1, PAIR_KEY, None, None, 1, 0.0, 0.0, m.ctypes.data, None) == FPC_E_INVALID
    assert lib.fpc_match_frames(None, 1, PAIR_PREVIOUS, None, None, 0, 0.0, 0.7, m.ctypes.data, None) == FPC_E_INVALID
    assert lib.fpc_first_within_frames(None, 1, None, None, ctypes.c_float(0.8), m.ctypes.data) == FPC_E_INVALID


@pytest.mark.parametrize("pairing", [PAIR_KEY, PAIR_PREVIOUS])
def test_restatement_agrees_with_the_oracle_at_ratio_zero(pairing):
    from oracle import oracle
    rng = np.random.Generator(np.random.PCG64(11))
    cap, n = 40, 5
    counts = np.array([33, 0, 17, 40, 1])
    desc = np.stack([_unit(rng, cap) for _ in range(n)])
    key = _unit(rng, 29)
    for cross, md in ((True, 0.0), (False, 0.0), (True, 1.3)):
        m, d1, _ = frames_rule(desc, counts, key, pairing, cross, md)
        for f in range(n):
            t = desc[f - 1, :counts[f - 1]] if pairing == PAIR_PREVIOUS and f > 0 else key
            om, od = oracle.match(desc[f, :counts[f]], t, cross, md)
            np.testing.assert_array_equal(m[f, :counts[f]], om)
            if len(t):
                np.testing.assert_allclose(d1[f, :counts[f]], od, rtol=1e-6)
            else:                                                 # (the batched rule's distance is +inf there)
                assert np.isinf(d1[f, :counts[f]]).all()
            assert (m[f, counts[f]:] == -1).all() and np.isinf(d1[f, counts[f]:]).all()
    # frame 0 of PREVIOUS pairing without a key has nothing to match against
    m, d1, _ = frames_rule(desc, counts, None, PAIR_PREVIOUS)
    assert (m[0] == -1).all() and np.isinf(d1[0]).all()


def test_ratio_test_of_the_restatement():
    rng = np.random.Generator(np.random.PCG64(5))
    t = _unit(rng, 50)
    q = t[[3, 7, 7, 20]] + rng.normal(0, 0.01, (4, 128)).astype(np.float32)
    m, d1, d2 = pair_rule(q, t, cross_check=False, ratio=0.8)
    assert list(m[[0, 1, 3]]) == [3, 7, 20] and (d1 < 0.8 * d2)[[0, 1, 3]].all()
    # the ratio test only removes matches
    m0, _, _ = pair_rule(q, t, cross_check=False)
    assert ((m == m0) | (m == -1)).all()
    # a planted duplicate of the nearest row: best and second best tie, the lower index is the best, the test fails
    td = np.concatenate([t[:10], t[3:4], t[10:]])               # row 3 repeated at index 10
    m, d1, d2 = pair_rule(q[:1], td, cross_check=False, ratio=0.99)
    assert m[0] == -1 and d1[0] == d2[0]
    m, _, _ = pair_rule(q[:1], td, cross_check=False)
    assert m[0] == 3
    # one train row: no second-nearest, the test fails; without it the row matches
    assert pair_rule(q[:1], t[3:4], cross_check=False, ratio=0.8)[0][0] == -1
    assert pair_rule(q[:1], t[3:4], cross_check=False)[0][0] == 0
