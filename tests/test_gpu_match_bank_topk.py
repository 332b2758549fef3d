"""Verified relocalisation on the GPU (fpc_bank_topk_reserve / fpc_match_bank_topk / fpc_homography_bank_topk) held to the
existing calls, bit for bit: the scores are fpc_match_bank's, the candidates the numpy rule of tests/test_match_bank_topk.py
on those scores, every (frame, candidate) table fpc_match_bank_guided's with that slot, an identity H and a radius beyond
the frame, every (frame, candidate) homography fpc_homography_bank's with that column -- on a fp32 and a bf16 bank, on
ragged counts and in a D = 256 context -- and the decoy scene of the CPU test comes out as it does there: appearance takes
the decoy, the geometric check the true slot.  The planted frames are written into the library's device results as in
tests/test_gpu_match_guided.py; every context runs under the canary zones.  Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_match_guided import BIG, HOMS, N, engine, plant
from tests.test_homography_ransac import CORNER_BAR, FRAME_H, FRAME_W, corner_error
from tests.test_match_bank_topk import IDENTITY, decoy_slot, pick_rule, topk_rule
from tests.test_match_guided import PAIR_KEY, f10, planted_h, planted_scene

pytestmark = pytest.mark.gpu

FPC_E_INVALID = -1
SLOTS, KMAX = 6, 4
A, B, EMPTY, OTHER, TIE = 3, 1, 0, 2, (4, 5)     # the true key, its decoy, an empty slot, unrelated rows, two equal slots
OPTIONS = ((True, 0.7, 0.0), (False, 0.7, 0.0), (True, 0.0, 0.8))
PARAMS = dict(iterations=256, seed=3)


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


def _bank_bytes(e):
    v = _lib.FpcBankView()
    assert _lib.load().fpc_bank_get(e._ctx, ctypes.byref(v)) == 0
    return v.bytes, v.chunk


def fill_bank(e, scene, fmt):
    """6 slots: A the key, B its decoy, TIE two copies of the key's first 400 rows, OTHER unrelated rows, EMPTY nothing;
    then the reservation, which must leave the bank's own figures alone."""
    dim = scene["desc"].shape[2]
    rng = np.random.Generator(np.random.PCG64(5))
    other = rng.normal(size=(300, dim))
    other = (other / np.linalg.norm(other, axis=1, keepdims=True)).astype(np.float32)
    other_xy = np.stack([rng.integers(0, FRAME_W, 300), rng.integers(0, FRAME_H, 300)], 1).astype(np.int32)
    e.bank_create(SLOTS, format=fmt)
    slots = {A: (scene["key"], scene["key_xy"]), B: decoy_slot(scene), OTHER: (other, other_xy),
             TIE[0]: (scene["key"][:400], scene["key_xy"][:400]), TIE[1]: (scene["key"][:400], scene["key_xy"][:400])}
    assert len(slots[B][0]) <= e.capacity
    for sl, (d, p) in slots.items():
        e.bank_store_rows(sl, d, p)
    e.sync()
    before = _bank_bytes(e)
    assert e.bank_info()["bytes"] == before[0]
    nbytes = e.bank_topk_reserve(KMAX)
    pairs, cap = N * KMAX, e.capacity
    assert nbytes >= pairs * (cap * 16 + cap * 8 + cap * 16 + cap * 4)        # top-2, column minima, pair lists, rows
    assert _bank_bytes(e) == before                                          # bytes and chunk: unchanged
    return slots


@pytest.fixture(scope="module", params=["f32", "bf16"])
def rig(request):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    scene = planted_scene(11, [f10(name, i) for name, i in HOMS], nkey=500, cap=e.capacity)
    assert e.capacity == 1024 and scene["counts"].min() > 250
    plant(e, scene)
    slots = fill_bank(e, scene, request.param)
    yield e, scene, slots
    try:
        assert e.check_guards() == 0
        e.bank_destroy()
        assert _lib.load().fpc_bank_topk_reserve(e._ctx, 1, None) == FPC_E_INVALID     # the reservation went with the bank
    finally:
        e.close()


def _slot_tensor(e, col):
    import torch
    return torch.from_numpy(np.ascontiguousarray(col, dtype=np.int32)).to(e.torch_device)


def _assert_tables_equal_guided(e, n, cand, m, d, cross, md, ratio, label):
    """match / dist [n][k][cap] (host) against fpc_match_bank_guided per column: identity H, a radius beyond the frame."""
    hs = np.tile(IDENTITY, (n, 1))
    for j in range(cand.shape[1]):
        gm, gd = e.match_bank_guided_async(n, _slot_tensor(e, cand[:, j]), hs, BIG, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        gm, gd = _host(gm, gd)
        np.testing.assert_array_equal(m[:, j], gm, err_msg="%s column %d" % (label, j))
        np.testing.assert_array_equal(d[:, j].view(np.uint32), gd.view(np.uint32), err_msg="%s column %d" % (label, j))
        gone = cand[:, j] < 0
        assert (m[gone, j] == -1).all() and np.isinf(d[gone, j]).all()


def test_scores_and_candidates_equal_match_bank_and_the_rule(rig):
    e, s, _ = rig
    for cross, md, ratio in OPTIONS:
        ref_score, ref_best, _, _ = e.match_bank_async(N, cross, md, ratio, table=False)
        e.sync()
        ref_score, ref_best = _host(ref_score, ref_best)
        assert (ref_score[:, TIE[0]] == ref_score[:, TIE[1]]).all() and (ref_score[:, TIE[0]] > 0).all()   # the tie pair
        assert (ref_score[:, EMPTY] == 0).all()
        assert (ref_score[:, B] > ref_score[:, A]).all()
        planted_order = ratio == 0             # (under the ratio test the key's look-alike twins cost A and B rows: TIE leads)
        assert not planted_order or (ref_score[:, A] > ref_score[:, TIE[0]]).all()
        few = int(ref_score[:, TIE[0]].max()) + 1                  # only A and B can reach it: fewer than k candidates
        for k in (1, 3, 4):
            for min_score in (0, few, int(ref_score.max()) + 1):
                score, cs, csc, m, d = e.match_bank_topk(N, k, cross, md, ratio, min_score)
                np.testing.assert_array_equal(score, ref_score)
                want_slot, want_score = topk_rule(score, k, min_score)
                np.testing.assert_array_equal(cs, want_slot)
                np.testing.assert_array_equal(csc, want_score)
                np.testing.assert_array_equal((m >= 0).sum(2), csc)            # the tables count what the scores count
                if min_score == 0:
                    np.testing.assert_array_equal(cs[:, 0], ref_best)
                    assert (cs >= 0).all()
                    if planted_order:
                        np.testing.assert_array_equal(cs, np.tile(np.array([B, A, TIE[0], TIE[1]], np.int32)[:k], (N, 1)))
                    elif k > 1:
                        assert (cs[:, :2] == TIE).all()                            # equal scores: the lower slot first
                elif min_score == few and k > 2:
                    assert (cs[:, 2:] == -1).all() and (csc[:, 2:] == 0).all()
                    if planted_order:                  # B leads wherever it reaches the floor; A follows where it does
                        np.testing.assert_array_equal(cs[:, 0], np.where(score[:, B] >= few, B, -1))
                        if k > 1:
                            np.testing.assert_array_equal(cs[:, 1], np.where(score[:, A] >= few, A, -1))
                        assert (cs[:, 0] == B).sum() >= 4 and (cs == -1).any()
                elif min_score > few:
                    assert (cs == -1).all() and (m == -1).all() and np.isinf(d).all()
    # outputs that may be NULL: no score, no candidate scores, no tables
    import torch
    cs = torch.full((N, 3), -7, dtype=torch.int32, device=e.torch_device)
    torch.cuda.synchronize()
    assert _lib.load().fpc_match_bank_topk(e._ctx, N, 3, 1, 0.7, 0.0, 0, None, cs.data_ptr(), None, None, None) == 0
    e.sync()
    np.testing.assert_array_equal(cs.cpu().numpy(), np.tile(np.array([B, A, TIE[0]], np.int32), (N, 1)))


def test_tables_are_bit_identical_to_match_bank_guided(rig):
    e, s, _ = rig
    for cross, md, ratio in OPTIONS:
        few = 0
        for min_score in (0, None):
            if min_score is None:
                min_score = few
            score, cs, csc, m, d = e.match_bank_topk(N, KMAX, cross, md, ratio, min_score)
            few = int(score[:, TIE[0]].max()) + 1                    # second round: candidates of -1 in columns 2, 3
            _assert_tables_equal_guided(e, N, cs, m, d, cross, md, ratio, (cross, md, ratio, min_score))
            assert min_score > 0 or (m[:, :2] >= 0).sum() > 1000
        assert (cs[:, 2:] == -1).all()


def test_tables_on_ragged_counts(rig):
    e, s, _ = rig
    r = dict(s)
    r["counts"] = np.array([0, 1, 63, 64, 65, 130, 129, s["counts"][7]])
    assert (r["counts"] <= s["counts"]).all()
    plant(e, r)
    try:
        for cross, md, ratio in OPTIONS[:2]:
            for k in (2, KMAX):
                score, cs, csc, m, d = e.match_bank_topk(N, k, cross, md, ratio)
                want_slot, want_score = topk_rule(score, k)
                np.testing.assert_array_equal(cs, want_slot)
                np.testing.assert_array_equal(csc, want_score)
                assert (cs[0] == -1).all()                           # a frame without rows has no candidate
                _assert_tables_equal_guided(e, N, cs, m, d, cross, md, ratio, ("ragged", cross, md, ratio, k))
                for f, cnt in enumerate(r["counts"]):
                    assert (m[f, :, cnt:] == -1).all() and np.isinf(d[f, :, cnt:]).all()
                hm, ni, mask, pick, best = e.homography_bank_topk(N, _slot_tensor(e, cs), _slot_tensor(e, m), **PARAMS)
                _assert_homographies_equal_bank(e, N, cs, m, hm, ni, mask, pick, best)
                assert not hm[:2].any() and (pick[:2] == -1).all()   # 0 and 1 rows: fewer than 4 pairs
    finally:
        plant(e, s)


def _assert_homographies_equal_bank(e, n, cs, m, hm, ni, mask, pick, best):
    """Problem (f, j) against fpc_homography_bank called with column j; pick / best against the integer rule."""
    for j in range(cs.shape[1]):
        rh, rn, rmask = e.homography_bank(n, _slot_tensor(e, cs[:, j]), _slot_tensor(e, m[:, j]), **PARAMS)
        np.testing.assert_array_equal(hm[:, j].view(np.uint32), rh.view(np.uint32), err_msg="H column %d" % j)
        np.testing.assert_array_equal(ni[:, j], rn)
        np.testing.assert_array_equal(mask[:, j], rmask)
    want_pick, want_best = pick_rule(ni, cs)
    np.testing.assert_array_equal(pick, want_pick)
    np.testing.assert_array_equal(best, want_best)
    np.testing.assert_array_equal(mask.sum(2), ni)


def test_homographies_equal_homography_bank_and_the_decoy_loses(rig):
    e, s, _ = rig
    truth = planted_h(s, PAIR_KEY)
    for k, min_score in ((KMAX, 0), (3, None), (1, 0)):
        score, cs, csc, m, d = e.match_bank_topk(N, k, True, 0.7, 0.0, 0)
        if min_score is None:                             # candidates of -1: column 2, and column 1 where A scores below it
            few = int(score[:, TIE[0]].max()) + 1
            score, cs, csc, m, d = e.match_bank_topk(N, k, True, 0.7, 0.0, few)
            assert (cs[:, 2] == -1).all()
            np.testing.assert_array_equal(cs[:, 0], np.where(score[:, B] >= few, B, -1))
        hm, ni, mask, pick, best = e.homography_bank_topk(N, _slot_tensor(e, cs), _slot_tensor(e, m), **PARAMS)
        _assert_homographies_equal_bank(e, N, cs, m, hm, ni, mask, pick, best)
        print("k %d: candidates %s inliers %s pick %s" % (k, cs[0].tolist(), ni.tolist(), pick.tolist()))
        np.testing.assert_array_equal(ni[:, 0], 0)                             # the decoy supports no homography
        assert not hm[:, 0].any() and not mask[:, 0].any()
        if k == 1:
            assert (pick == -1).all() and (best == -1).all()                   # appearance alone loses every frame
            continue
        _, ref_best, _, _ = e.match_bank_async(N, True, 0.7, table=False)
        e.sync()
        np.testing.assert_array_equal(ref_best.cpu().numpy(), B)
        has_a = cs[:, 1] == A
        assert has_a.sum() >= 4 and (min_score is None or has_a.all())
        np.testing.assert_array_equal(pick, np.where(has_a, 1, -1))
        np.testing.assert_array_equal(best, np.where(has_a, A, -1))           # ... and the true slot is verified
        assert (ni[has_a, 1] >= 100).all()
        for f in np.flatnonzero(has_a):
            err = corner_error(hm[f, 1].astype(np.float64), truth[f].astype(np.float64).reshape(3, 3))
            assert err <= CORNER_BAR, (f, err)
        if min_score is None:
            assert not hm[:, 2].any() and (ni[:, 2] == 0).all()
    # pick_dev / best_dev / inlier_dev may be NULL
    import torch
    hd = torch.empty((N, k, 9), dtype=torch.float32, device=e.torch_device)
    nd = torch.empty((N, k), dtype=torch.int32, device=e.torch_device)
    p = e._ransac_params(PARAMS)
    csd, md = _slot_tensor(e, cs), _slot_tensor(e, m)
    torch.cuda.synchronize()
    assert _lib.load().fpc_homography_bank_topk(e._ctx, N, k, csd.data_ptr(), md.data_ptr(), ctypes.byref(p), hd.data_ptr(),
                                                nd.data_ptr(), None, None, None) == 0
    e.sync()
    np.testing.assert_array_equal(hd.cpu().numpy().view(np.uint32).reshape(N, k, 3, 3), hm.view(np.uint32))
    np.testing.assert_array_equal(nd.cpu().numpy(), ni)


def _chain(e):
    """The five calls, no host call in between, one synchronisation."""
    _, cs, csc, m, d = e.match_bank_topk_async(N, KMAX, True, 0.7)
    hm, ni, mask, pick, best = e.homography_bank_topk_async(N, cs, m, **PARAMS)
    h1 = hm[torch_arange(e), pick.clamp(min=0).long()]               # device-side gather of the picked H (torch, no sync)
    m2, d2 = e.match_bank_guided_async(N, best, h1, 8.0, cross_check=True, max_dist=0.7)
    h2, n2, mask2 = e.homography_bank_async(N, best, m2, **PARAMS)
    e.sync()
    return _host(cs, csc, m, d.view(cs.dtype), hm.view(cs.dtype), ni, mask, pick, best, m2, d2.view(cs.dtype),
                 h2.view(cs.dtype), n2, mask2)


def torch_arange(e):
    import torch
    return torch.arange(N, device=e.torch_device)


def test_chain_without_a_host_call_and_determinism(rig):
    e, s, _ = rig
    first, second = _chain(e), _chain(e)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)                                    # repeated calls: bit-identical
    cs, csc, m, d, hm, ni, mask, pick, best, m2, d2, h2, n2, mask2 = first
    print("chain: best", best.tolist(), "inliers", ni[np.arange(N), pick].tolist(), "->", n2.tolist())
    np.testing.assert_array_equal(best, A)
    assert (n2 >= 100).all()                                                   # the guided pass under the picked H
    truth = planted_h(s, PAIR_KEY)
    for f in range(N):
        assert corner_error(h2[f].view(np.float32).astype(np.float64), truth[f].astype(np.float64).reshape(3, 3)) <= CORNER_BAR
    # the convenience wrapper gives the same answer
    rb, rh, rn, rcs, rcsc = e.relocalise(N, KMAX, max_dist=0.7, **PARAMS)
    np.testing.assert_array_equal(rb, best)
    np.testing.assert_array_equal(rh.view(np.uint32), hm.view(np.uint32))
    np.testing.assert_array_equal(rn, ni)
    np.testing.assert_array_equal(rcs, cs)
    np.testing.assert_array_equal(rcsc, csc)
    assert e.check_guards() == 0


def test_bad_arguments_are_refused_and_write_nothing(rig):
    import torch
    e, s, _ = rig
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    cap = e.capacity
    sc = torch.full((N + 1, SLOTS), -7, dtype=torch.int32, device=dev)
    cs = torch.full((N + 1, KMAX + 1), -7, dtype=torch.int32, device=dev)
    csc = torch.full((N + 1, KMAX + 1), -7, dtype=torch.int32, device=dev)
    mt = torch.full((N + 1, KMAX + 1, cap), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, KMAX + 1, cap), -7.0, dtype=torch.float32, device=dev)
    hm = torch.full((N + 1, KMAX + 1, 9), -7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N + 1, KMAX + 1), -7, dtype=torch.int32, device=dev)
    mk = torch.full((N + 1, KMAX + 1, cap), 249, dtype=torch.uint8, device=dev)
    pk = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    bs = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    slot_in = torch.zeros((N + 1, KMAX + 1), dtype=torch.int32, device=dev)
    match_in = torch.zeros((N + 1, KMAX + 1, cap), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def mb(c=ctx, n=N, k=KMAX, md=0.7, ratio=0.0, min_score=0, slot=cs.data_ptr()):
        return lib.fpc_match_bank_topk(c, n, k, 1, md, ratio, min_score, sc.data_ptr(), slot, csc.data_ptr(), mt.data_ptr(),
                                       ds.data_ptr())

    def hb(c=ctx, n=N, k=KMAX, slot=slot_in.data_ptr(), match=match_in.data_ptr(), h=hm.data_ptr(), nn=ni.data_ptr(), **kw):
        p = e._ransac_params(dict(PARAMS, **kw))
        return lib.fpc_homography_bank_topk(c, n, k, slot, match, ctypes.byref(p), h, nn, mk.data_ptr(), pk.data_ptr(),
                                            bs.data_ptr())
    # the reservation: out of range, beyond the slots, twice
    for kmax in (0, -1, 17, SLOTS + 1, KMAX):
        assert lib.fpc_bank_topk_reserve(ctx, kmax, None) == FPC_E_INVALID
    # everything fpc_match_bank refuses, and the call's own
    assert mb(n=N + 1) == FPC_E_INVALID and mb(n=0) == FPC_E_INVALID
    assert mb(md=-1.0) == FPC_E_INVALID and mb(ratio=1.5) == FPC_E_INVALID and mb(ratio=-0.1) == FPC_E_INVALID
    assert mb(min_score=-1) == FPC_E_INVALID
    assert mb(k=0) == FPC_E_INVALID and mb(k=KMAX + 1) == FPC_E_INVALID and mb(k=-3) == FPC_E_INVALID
    assert mb(slot=None) == FPC_E_INVALID
    # everything fpc_homography_bank refuses, and the call's own
    assert hb(n=N + 1) == FPC_E_INVALID and hb(n=0) == FPC_E_INVALID
    assert hb(k=0) == FPC_E_INVALID and hb(k=KMAX + 1) == FPC_E_INVALID
    assert hb(slot=None) == FPC_E_INVALID and hb(match=None) == FPC_E_INVALID
    assert hb(h=None) == FPC_E_INVALID and hb(nn=None) == FPC_E_INVALID
    assert hb(iterations=0) == FPC_E_INVALID and hb(iterations=4097) == FPC_E_INVALID
    assert hb(reproj_threshold=0.0) == FPC_E_INVALID and hb(refits=5) == FPC_E_INVALID and hb(min_inliers=3) == FPC_E_INVALID
    lp = ctypes.POINTER(_lib.FpcRansacParams)()
    assert lib.fpc_homography_bank_topk(ctx, N, KMAX, slot_in.data_ptr(), match_in.data_ptr(), lp, hm.data_ptr(), ni.data_ptr(),
                                        None, None, None) == FPC_E_INVALID
    # a bank without a reservation; a context without a bank; results without descriptors
    d = engine(b=2)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        assert lib.fpc_bank_topk_reserve(d._ctx, 1, None) == FPC_E_INVALID     # no bank
        assert mb(c=d._ctx, n=2, k=1) == FPC_E_INVALID and hb(c=d._ctx, n=2, k=1) == FPC_E_INVALID
        d.bank_create(2)
        assert mb(c=d._ctx, n=2, k=1) == FPC_E_INVALID and hb(c=d._ctx, n=2, k=1) == FPC_E_INVALID   # no reservation
        assert lib.fpc_bank_topk_reserve(d._ctx, 3, None) == FPC_E_INVALID     # kmax above the slots
        assert d.bank_topk_reserve(2) > 0
        d.get_points(prob)                                                     # keypoints only
        assert mb(c=d._ctx, n=2, k=1) == FPC_E_INVALID
        z = torch.zeros((2, 2, cap), dtype=torch.int32, device=dev)
        assert not d.homography_bank_topk(2, z[:, :, 0].contiguous(), z, **PARAMS)[0].any()   # (needs no descriptors)
        assert d.check_guards() == 0
        d.bank_destroy()
    finally:
        d.close()
    e.sync()
    for t in (sc, cs, csc, mt, ni, pk, bs):
        assert (t.cpu().numpy() == -7).all()
    assert (ds.cpu().numpy() == -7.0).all() and (mk.cpu().numpy() == 249).all()
    assert (hm.cpu().numpy() == -7.0).all()
    assert mb() == 0 and hb() == 0                                             # (the valid forms of the calls above)
    e.sync()


def test_vgg_descriptors_both_formats():
    """FPC_ARCH_VGG: D = 256 -- the strips' other K extent."""
    e = engine(240, 320, in_channels=1, arch="vgg")
    try:
        assert e.desc_dim == 256
        s = planted_scene(4, [f10(name, i) for name, i in HOMS], nkey=300, dim=256, cap=e.capacity)
        plant(e, s)
        for fmt in ("f32", "bf16"):
            fill_bank(e, s, fmt)
            score, cs, csc, m, d = e.match_bank_topk(N, KMAX, True, 0.7)
            ref_score, _, _, _ = e.match_bank_async(N, True, 0.7, table=False)
            e.sync()
            np.testing.assert_array_equal(score, ref_score.cpu().numpy())
            np.testing.assert_array_equal(cs, np.tile(np.array([B, A, TIE[0], TIE[1]], np.int32), (N, 1)))
            np.testing.assert_array_equal((m >= 0).sum(2), csc)
            _assert_tables_equal_guided(e, N, cs, m, d, True, 0.7, 0.0, ("vgg", fmt))
            hm, ni, mask, pick, best = e.homography_bank_topk(N, _slot_tensor(e, cs), _slot_tensor(e, m), **PARAMS)
            _assert_homographies_equal_bank(e, N, cs, m, hm, ni, mask, pick, best)
            np.testing.assert_array_equal(best, A)
            assert e.check_guards() == 0
            e.bank_destroy()
    finally:
        e.close()
