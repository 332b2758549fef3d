"""The bf16 key-frame bank on the GPU (fpc_bank_create_ex with FPC_BANK_BF16, include/fpc.h): storage, fpc_match_bank,
fpc_match_bank_guided and the chain through fpc_homography_bank, against a float64 restatement on the SAME bf16-rounded
rows (tests/test_match_bank_bf16.py's rounding).

Inputs.  The query sets come from Engine.get_points(prob_map, desc_map): one isolated peak per chosen 8 x 8 cell, a
descriptor map of independent random unit vectors per cell (the detector's synthetic-weight descriptors have near-duplicate
rows and cannot carry index comparisons).  The results are read back and the slots are built from them on the host as
tests/test_match_bank.py's planted() does -- half of a frame's rows + N(0, 0.02) noise, renormalised, then unrelated random
rows -- with pixels that are the frame's own under an integer translation, and stored with bank_store_rows.  Counts cover
the strip's edges: a frame without rows, a frame and a slot of one row (the ratio test must fail), 63 / 64 / 65 rows, a slot
truncated by `rows`, an empty slot.  D = 128, and D = 256 through the VGG arch.

Tolerance on d^2 (derived, not measured).  Products of bf16 values are exact in fp32, so the device's d^2 differs from the
float64 value on the same rounded rows only by the fp32 accumulation of D terms in the dot product and in each norm:
    tol = 8 D 2^-24 max(1, |q~|^2) max(1, |t~|^2)          (6.1e-5 at D = 128 on unit rows)
(dist is returned as sqrtf(d^2); squaring it back costs 2^-23 d^2 < 5e-7, far inside.)  A row is DECIDABLE for an option set
when, in the restatement, neither the first-to-second gap, nor the max_dist threshold, nor the ratio comparison, nor the cross
check's column gap lies within 2 tol of flipping; undecidable rows are left out of index and score comparisons and must be at
most 2 % of all (frame, slot, row) triples.  Everything else is exact.  Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_match_bank import _expect_best
from tests.test_match_bank_bf16 import BANK_BF16, OPTIONS, bf16_bits, bf16_round

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
CAP = 512
ROWS = 400                                       # the bank's rows: the slot of frame 7 (450 rows) is truncated
SLOTS = 12
COUNTS = [0, 1, 63, 64, 65, 200, 331, 500]       # keypoints per frame
SLOT_OF_FRAME = [-1, 9, 4, 0, 11, 2, 7, 5]       # frame f was planted into slot SLOT_OF_FRAME[f]
UNRELATED = [0, 0, 32, 32, 33, 150, 150, 200]    # -> slots of 1, 63, 64, 65, 250, 315, 450 rows
TWIN = 3                                         # a second slot of frame 6's rows at a LOWER index than 7: wins the tie
EMPTY = 6
SHIFT = [(0, 0), (3, -2), (16, -8), (-5, 7), (1, 1), (-24, 40), (9, 0), (-7, -13)]   # train pixel = query pixel + SHIFT[f]
FPC_E_INVALID = -1
BIG = 1e4                                        # a radius beyond the frame diagonal
MARGIN = 1e-3                                    # px at the four corners: the resolution of an fp32 H


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _maps(rng, dim):
    """-> prob [N,H,W] with COUNTS[f] isolated peaks (one per interior cell, distinct heights), desc map [N,dim,H/8,W/8]."""
    hc, wc = H // 8, W // 8
    prob = np.zeros((N, H, W), np.float32)
    cells = [(cy, cx) for cy in range(1, hc - 1) for cx in range(1, wc - 1)]
    for f, k in enumerate(COUNTS):
        pick = rng.permutation(len(cells))[:k]
        for r, c in enumerate(pick):
            cy, cx = cells[c]
            prob[f, cy * 8 + 4, cx * 8 + 4] = 0.9 - 0.001 * r
    dmap = rng.normal(size=(N, hc, wc, dim))
    dmap = (dmap / np.linalg.norm(dmap, axis=3, keepdims=True)).astype(np.float32)
    return prob, np.ascontiguousarray(dmap.transpose(0, 3, 1, 2))


def _build_slots(rng, res, dim):
    """planted()'s construction on the rows read back from the device -> {slot: (desc [k,dim] float32, xy [k,2] int32)}."""
    slots = {}
    for f, s in enumerate(SLOT_OF_FRAME):
        if s < 0:
            continue
        xy, _, d, _ = res[f]
        k = len(d)
        pick = np.arange(1) if k == 1 else rng.permutation(k)[:k // 2]
        rows = _unit(d[pick].astype(np.float64) + rng.normal(0, 0.02, (len(pick), dim)))
        pts = xy[pick] + np.array(SHIFT[f], np.int32)
        if UNRELATED[f]:
            rows = np.concatenate([rows, _unit(rng.normal(size=(UNRELATED[f], dim)))])
            pts = np.concatenate([pts, np.stack([rng.integers(0, W, UNRELATED[f]), rng.integers(0, H, UNRELATED[f])], 1)])
        slots[s] = (np.ascontiguousarray(rows, np.float32), np.ascontiguousarray(pts, np.int32))
    slots[TWIN] = (slots[SLOT_OF_FRAME[6]][0].copy(), slots[SLOT_OF_FRAME[6]][1].copy())
    return slots


def _store(e, slots):
    for s, (d, p) in slots.items():
        e.bank_store_rows(s, d, p)


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


class Restatement:
    """float64 on the rounded rows, computed once per (frame, slot) and shared by the tests; nothing below modifies it."""

    def __init__(self, res, slots, dim):
        self.dim = dim
        self.c = 8.0 * dim * 2.0 ** -24
        self.q = [bf16_round(r[2]).astype(np.float64) for r in res]
        self.t = {s: bf16_round(d[:ROWS]).astype(np.float64) for s, (d, _) in slots.items()}
        self.dd, self.tol = {}, {}
        for f in range(N):
            qn = (self.q[f] ** 2).sum(1)
            for s, t in self.t.items():
                tn = (t ** 2).sum(1)
                self.dd[f, s] = np.maximum(qn[:, None] + tn[None, :] - 2.0 * self.q[f] @ t.T, 0.0)
                self.tol[f, s] = self.c * np.maximum(1.0, qn)[:, None] * np.maximum(1.0, tn)[None, :]

    def pair(self, f, s, cross, md, ratio):
        """-> (match int32 [nq] by the rule, undecidable bool [nq]) of frame f against slot s."""
        nq = len(self.q[f])
        if s not in self.t or nq == 0:
            return np.full(nq, -1, np.int32), np.zeros(nq, bool)
        dd, tol = self.dd[f, s], float(self.tol[f, s].max())
        nt = dd.shape[1]
        rows = np.arange(nq)
        order = np.argsort(dd, axis=1, kind="stable")
        j1 = order[:, 0]
        d1 = dd[rows, j1]
        d2 = dd[rows, order[:, 1]] if nt >= 2 else np.full(nq, np.inf)
        ok = np.ones(nq, bool)
        und = d2 - d1 <= 2 * tol                                   # the winner itself
        if cross:
            col = dd[:, j1]                                        # [i', i]: column j1[i]
            ok &= np.argmin(col, axis=0) == rows
            if nq >= 2:
                other = np.where(np.eye(nq, dtype=bool), np.inf, col).min(axis=0)
                und |= np.abs(d1 - other) <= 2 * tol
        if md > 0:
            ok &= np.sqrt(d1) < md
            und |= np.abs(d1 - md * md) <= 2 * tol
        if ratio > 0:
            ok &= (nt >= 2) & (np.sqrt(d1) < ratio * np.sqrt(d2))
            if nt >= 2:
                und |= np.abs(d1 - ratio * ratio * d2) <= 2 * tol
        return np.where(ok, j1, -1).astype(np.int32), und


@pytest.fixture(scope="module", params=["resnet", "vgg"])
def banked(request):
    import torch
    from fpc_amd.engine import Engine
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    kw = dict(in_channels=1, arch="vgg") if request.param == "vgg" else {}
    e = Engine(H, W, max_batch=N, plan_flags=["guard_zones"], max_keypoints=CAP, **kw)
    dim = e.desc_dim
    assert dim == (256 if request.param == "vgg" else 128) and e.capacity == CAP
    rng = np.random.Generator(np.random.PCG64(7))
    prob, dmap = _maps(rng, dim)
    res = e.get_points(torch.from_numpy(prob), torch.from_numpy(dmap))
    assert [len(r[2]) for r in res] == COUNTS
    slots = _build_slots(rng, res, dim)
    assert sorted(len(d) for d, _ in slots.values()) == [1, 63, 64, 65, 250, 315, 315, 450] and EMPTY not in slots
    # the same rows in an fp32 bank first: its bytes and its answers
    f32 = {"bytes": e.bank_create(SLOTS, ROWS)}
    assert e.bank_info()["format"] == "f32"
    _store(e, slots)
    for opt in OPTIONS:
        _, best, _, _ = e.match_bank_async(N, cross_check=opt[0], max_dist=opt[1], ratio=opt[2], table=False)
        e.sync()
        f32[opt] = best.cpu().numpy()
    e.bank_destroy()
    nbytes = e.bank_create(SLOTS, ROWS, format="bf16")
    _store(e, slots)
    e.sync()
    ref = Restatement(res, slots, dim)
    yield e, res, slots, ref, f32, nbytes
    assert e.check_guards() == 0                        # the bank's zones, the query workspace's included
    e.bank_destroy()
    assert e.check_guards() == 0
    e.close()


def _slot_tables(e, s, cross, md, ratio):
    """Every frame against slot s: fpc_match_bank_guided under the identity and a radius beyond the frame -> host
    (match [N,cap], dist [N,cap])."""
    import torch
    slot = torch.full((N,), s, dtype=torch.int32, device=e.torch_device)
    eye = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    m, d = e.match_bank_guided_async(N, slot, eye, BIG, cross_check=cross, max_dist=md, ratio=ratio)
    e.sync()
    return _host(m, d)


def test_store_rounds_to_nearest_even(banked):
    e, res, slots, ref, f32, nbytes = banked
    lib = _lib.load()
    fmt, ptr, view = ctypes.c_int(-1), ctypes.c_void_p(), _lib.FpcBankView()
    assert lib.fpc_bank_format(e._ctx, ctypes.byref(fmt), ctypes.byref(ptr)) == 0
    assert lib.fpc_bank_get(e._ctx, ctypes.byref(view)) == 0
    assert fmt.value == BANK_BF16 and ptr.value and view.desc is None
    info = e.bank_info()
    assert info["format"] == "bf16" and info["bytes"] == nbytes == view.bytes and info["rows"] == ROWS
    print("bytes: bf16", nbytes, "fp32", f32["bytes"])
    assert nbytes < f32["bytes"]
    import torch
    bd, bx, bc = e.bank_view()
    assert bd.dtype == torch.bfloat16 and tuple(bd.shape) == (SLOTS, ROWS, ref.dim)
    bits = bd.view(torch.int16).cpu().numpy().view(np.uint16)
    bx, bc = _host(bx, bc)
    for s in range(SLOTS):
        if s not in slots:
            assert bc[s] == 0
            continue
        d, p = slots[s]
        k = min(len(d), ROWS)
        assert bc[s] == k
        np.testing.assert_array_equal(bits[s, :k], bf16_bits(d[:k]))
        np.testing.assert_array_equal(bits[s, :k], torch.from_numpy(d[:k]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
        np.testing.assert_array_equal(bx[s, :k], p[:k])
    assert bc[SLOT_OF_FRAME[7]] == ROWS < len(slots[SLOT_OF_FRAME[7]][0])      # truncated by `rows`


def test_values_are_within_the_derived_tolerance(banked):
    """No cross check, no thresholds: every row, ties or not."""
    e, res, slots, ref, f32, nbytes = banked
    worst = 0.0
    tables = {s: _slot_tables(e, s, False, 0.0, 0.0) for s in range(SLOTS)}
    _, best, m, d = e.match_bank_async(N, cross_check=False)
    e.sync()
    best, m, d = _host(best, m, d)
    for f in range(N):
        k = COUNTS[f]
        cases = [(s, tables[s][0][f], tables[s][1][f]) for s in range(SLOTS)] + [(int(best[f]), m[f], d[f])]
        for s, mm, dist in cases:
            assert (mm[k:] == -1).all() and np.isinf(dist[k:]).all()
            if s not in slots or k == 0:
                assert (mm == -1).all() and np.isinf(dist).all()
                continue
            dd, tol = ref.dd[f, s], ref.tol[f, s]
            rows = np.arange(k)
            assert (mm[:k] >= 0).all() and (mm[:k] < dd.shape[1]).all()
            jref = dd.argmin(axis=1)
            t = np.maximum(tol[rows, jref], tol[rows, mm[:k]])
            err = np.abs(dist[:k].astype(np.float64) ** 2 - dd[rows, jref])
            worst = max(worst, float((err / t).max()))
            assert (err <= t).all(), (f, s, float(err.max()))
            assert (dd[rows, mm[:k]] <= dd[rows, jref] + 2 * t).all(), (f, s)
    print("largest |dist^2 - d^2_ref| / tol:", worst)


def test_indices_scores_and_best_equal_the_restatement_on_decidable_rows(banked):
    e, res, slots, ref, f32, nbytes = banked
    triples = undecidable = 0
    for opt in OPTIONS:
        cross, md, ratio = opt
        score, best, m, d = e.match_bank_async(N, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        score, best, m, d = _host(score, best, m, d)
        for s in range(SLOTS):
            ms, _ = _slot_tables(e, s, cross, md, ratio)
            for f in range(N):
                k = COUNTS[f]
                want, und = ref.pair(f, s, cross, md, ratio)
                triples += k
                undecidable += int(und.sum())
                np.testing.assert_array_equal(ms[f, :k][~und], want[~und])
                certain = int((want[~und] >= 0).sum())
                assert certain <= score[f, s] <= certain + int(und.sum()), (opt, f, s, score[f, s], certain)
                assert score[f, s] == (ms[f] >= 0).sum()           # the score pass and the per-slot table agree exactly
                if best[f] == s:
                    np.testing.assert_array_equal(m[f], ms[f])
        assert (score[:, EMPTY] == 0).all() and (score[0] == 0).all() and best[0] == -1
        # one train row, or one query row against unrelated rows: the ratio test fails
        if ratio > 0:
            assert (score[:, SLOT_OF_FRAME[1]] == 0).all() and best[1] == -1
        else:
            assert best[1] == SLOT_OF_FRAME[1] and score[1, SLOT_OF_FRAME[1]] == 1
        planted = np.array(SLOT_OF_FRAME)
        planted[6] = TWIN                                          # two identical slots: the lower one
        np.testing.assert_array_equal(best[2:], planted[2:])
        assert (score[6, TWIN] == score[6, SLOT_OF_FRAME[6]]).all()
        np.testing.assert_array_equal(best, f32[opt])              # what the fp32 bank of the same rows answers
        print("options", opt, "best", best)
    print("undecidable", undecidable, "of", triples)
    assert undecidable <= 0.02 * triples


def test_self_consistency(banked):
    import torch
    e, res, slots, ref, f32, nbytes = banked
    for cross, md, ratio in OPTIONS + ((True, 0.0, 0.0),):
        score, best, m, d = e.match_bank_async(N, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        score, best, m, d = _host(score, best, m, d)
        np.testing.assert_array_equal(best, _expect_best(score))
        assert (score[:, EMPTY] == 0).all()
        for f in range(N):
            if best[f] >= 0:
                assert (m[f] >= 0).sum() == score[f, best[f]]
            else:
                assert (m[f] == -1).all() and np.isinf(d[f]).all()
    score, best, m, d = e.match_bank_async(N, max_dist=0.7)
    e.sync()
    top = int(score.max())
    s2, b2, m2, d2 = e.match_bank_async(N, max_dist=0.7, min_score=top + 1)
    s3, b3, _, _ = e.match_bank_async(N, max_dist=0.7, min_score=top)
    e.sync()
    np.testing.assert_array_equal(s2.cpu().numpy(), score.cpu().numpy())
    assert (b2.cpu().numpy() == -1).all() and (m2.cpu().numpy() == -1).all() and torch.isinf(d2).all()
    np.testing.assert_array_equal(b3.cpu().numpy(), _expect_best(score.cpu().numpy(), top))
    assert (b3.cpu().numpy() >= 0).any()


def _chain(e, sync):
    """fpc_match_bank -> fpc_homography_bank -> fpc_match_bank_guided -> fpc_homography_bank."""
    import torch
    step = e.sync if sync else (lambda: None)
    params = dict(iterations=256, seed=3)
    score, best, m1, d1 = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    step()
    h1, n1, k1 = e.homography_bank_async(N, best, m1, **params)
    step()
    m2, d2 = e.match_bank_guided_async(N, best, h1, 4.0, cross_check=True, max_dist=0.7)
    step()
    h2, n2, k2 = e.homography_bank_async(N, best, m2, **params)
    e.sync()
    return _host(score, best, m1, d1.view(torch.int32), h1.view(torch.int32), n1, k1, m2, d2.view(torch.int32),
                 h2.view(torch.int32), n2, k2)


def test_chain_repeats_and_asynchronous_flow(banked):
    e, res, slots, ref, f32, nbytes = banked
    a = _chain(e, sync=False)                                      # four calls, no host call in between
    b = _chain(e, sync=False)
    c = _chain(e, sync=True)
    for x, y, z in zip(a, b, c):
        np.testing.assert_array_equal(x, y)                        # repeated calls: bit-identical
        np.testing.assert_array_equal(x, z)                        # and equal to the synchronous flow
    best, h2, n1, n2 = a[1], a[9].view(np.float32), a[5], a[10]
    print("best", best, "inliers", n1, "->", n2)
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64)
    for f in range(2, N):                                          # (frames 0 / 1 have fewer than four pairs)
        assert n2[f] >= n1[f] >= 8
        p = corners @ h2[f].astype(np.float64).T
        p = p[:, :2] / p[:, 2:3]
        err = np.abs(p - (corners[:, :2] + np.array(SHIFT[f], np.float64))).max()
        print("frame", f, "inliers", n2[f], "corner error against the planted translation", err)
        assert err < MARGIN
    assert (a[9][:2] == 0).all() and (n2[:2] == 0).all()           # failed frames: nine zeros


def test_guided(banked):
    import torch
    e, res, slots, ref, f32, nbytes = banked
    eye = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    for cross, md, ratio in OPTIONS:
        score, best, m, d = e.match_bank_async(N, cross_check=cross, max_dist=md, ratio=ratio)
        gm, gd = e.match_bank_guided_async(N, best, eye, BIG, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        np.testing.assert_array_equal(gm.cpu().numpy(), m.cpu().numpy())
        np.testing.assert_array_equal(gd.view(torch.int32).cpu().numpy(), d.view(torch.int32).cpu().numpy())   # bit for bit
    # the planted translations, 4 px
    hs = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
    for f in range(N):
        hs[f, 0, 2], hs[f, 1, 2] = SHIFT[f]
    slot = torch.from_numpy(np.array([max(s, 0) for s in SLOT_OF_FRAME], np.int32)).to(e.torch_device)
    um, ud = e.match_bank_guided_async(N, slot, eye, BIG, cross_check=False)
    gm, gd = e.match_bank_guided_async(N, slot, hs, 4.0, cross_check=False)
    e.sync()
    um, ud, gm, gd = _host(um, ud.view(torch.int32), gm, gd.view(torch.int32))
    pairs = 0
    for f in range(1, N):
        xy, txy = res[f][0].astype(np.float64), slots[SLOT_OF_FRAME[f]][1].astype(np.float64)
        rows = np.flatnonzero(gm[f] >= 0)
        assert rows.max() < COUNTS[f] and gm[f, rows].max() < min(len(txy), ROWS)
        ex = xy[rows] + np.array(SHIFT[f], np.float64) - txy[gm[f, rows]]
        assert ((ex ** 2).sum(1) < 16.0).all()                     # the gate (w = 1)
        same = rows[gm[f, rows] == um[f, rows]]
        np.testing.assert_array_equal(gd[f, same], ud[f, same])    # the same pair: the same bits
        assert len(same) >= COUNTS[f] // 2 and len(rows) <= COUNTS[f]
        pairs += len(rows)
    assert pairs >= sum(c // 2 for c in COUNTS[2:]) + 1 and (gm[0] == -1).all()


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    from fpc_amd.engine import Engine
    e, res, slots, ref, f32, nbytes = banked
    lib = _lib.load()
    ctx, dev = e._ctx, e.torch_device
    sc = torch.full((N + 1, SLOTS), -7, dtype=torch.int32, device=dev)
    bs = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    hm = torch.eye(3, device=dev).repeat(N + 1, 1, 1).contiguous()
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = e.bank_view()[0].view(torch.int16).clone()
    assert lib.fpc_bank_create_ex(ctx, 4, 16, BANK_BF16) == FPC_E_INVALID        # a second bank
    assert lib.fpc_bank_create(ctx, 4, 16) == FPC_E_INVALID
    mb = lambda n, cross, md, ratio, ms, s=sc.data_ptr(), b=bs.data_ptr(): lib.fpc_match_bank(  # noqa: E731
        ctx, n, cross, md, ratio, ms, s, b, mt.data_ptr(), None)
    assert mb(N + 1, 1, 0.7, 0.0, 0) == FPC_E_INVALID
    assert mb(0, 1, 0.7, 0.0, 0) == FPC_E_INVALID
    assert mb(N, 1, -1.0, 0.0, 0) == FPC_E_INVALID
    assert mb(N, 1, 0.7, 1.5, 0) == FPC_E_INVALID
    assert mb(N, 1, 0.7, 0.0, -1) == FPC_E_INVALID
    assert mb(N, 1, 0.7, 0.0, 0, None, None) == FPC_E_INVALID
    assert lib.fpc_bank_store(ctx, N, 0) == FPC_E_INVALID
    assert lib.fpc_bank_store(ctx, 0, SLOTS) == FPC_E_INVALID
    assert lib.fpc_bank_clear(ctx, SLOTS) == FPC_E_INVALID
    kd, kc = e.keep_frame(5)
    kx = e.keep_frame_points(5)
    e.sync()
    sr = lambda s, d, x, c: lib.fpc_bank_store_rows(ctx, s, d, x, c)            # noqa: E731
    assert sr(SLOTS, kd.data_ptr(), kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID
    assert sr(0, None, kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID
    assert sr(0, kd.data_ptr() + 4, kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID
    bg = lambda n, sl, h, r, out: lib.fpc_match_bank_guided(ctx, n, sl, h, r, 1, 0.7, 0.0, out, None)   # noqa: E731
    assert bg(N + 1, slot.data_ptr(), hm.data_ptr(), 4.0, mt.data_ptr()) == FPC_E_INVALID
    assert bg(N, None, hm.data_ptr(), 4.0, mt.data_ptr()) == FPC_E_INVALID
    assert bg(N, slot.data_ptr(), None, 4.0, mt.data_ptr()) == FPC_E_INVALID
    assert bg(N, slot.data_ptr(), hm.data_ptr(), 0.0, mt.data_ptr()) == FPC_E_INVALID
    assert bg(N, slot.data_ptr(), hm.data_ptr(), 4.0, None) == FPC_E_INVALID
    assert lib.fpc_bank_format(ctx, None, None) == FPC_E_INVALID
    e.sync()
    for t in (sc, bs, mt):
        assert (t.cpu().numpy() == -7).all()
    assert torch.equal(e.bank_view()[0].view(torch.int16), before)
    # an unknown format: no bank comes into being
    d = Engine(H, W, max_batch=2, plan_flags=["guard_zones"])
    view, fmt = _lib.FpcBankView(), ctypes.c_int(-7)
    for bad in (2, -1, 16):
        assert lib.fpc_bank_create_ex(d._ctx, 4, 16, bad) == FPC_E_INVALID
    assert lib.fpc_bank_get(d._ctx, ctypes.byref(view)) == FPC_E_INVALID
    assert lib.fpc_bank_format(d._ctx, ctypes.byref(fmt), None) == FPC_E_INVALID and fmt.value == -7
    with pytest.raises(ValueError):
        d.bank_create(4, 16, format="fp16")
    assert lib.fpc_bank_create_ex(d._ctx, 0, 16, BANK_BF16) == FPC_E_INVALID
    assert lib.fpc_bank_create_ex(d._ctx, 4, d.capacity + 1, BANK_BF16) == FPC_E_INVALID
    d.bank_create(4, 16, format="bf16")                            # (and a context closed with a live bf16 bank frees it)
    assert d.check_guards() == 0
    d.close()
