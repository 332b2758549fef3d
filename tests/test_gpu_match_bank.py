"""The key-frame bank on the GPU (fpc_bank_* / fpc_match_bank / fpc_homography_bank): a detect batch matched against every
stored key frame in one asynchronous call.  Every comparison is integer or bit equality against calls that already exist
-- fpc_match_frames with the slot as its key, fpc_homography_frames with the slot's coordinates -- so no tolerance is
chosen here, except the identity case's 1e-3 px (the margin DESIGN.md section 7 derives for device homographies).
Synthetic weights at QVGA, 8 frames per batch, every context under the canary zones.  Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
SLOTS = 12
SLOT_OF_FRAME = [7, 2, 10, 0, 5, 11, 3, 8]            # frame f of batch 300 lives in slot SLOT_OF_FRAME[f]; 1, 4, 6, 9 stay empty
EMPTY = [1, 4, 6, 9]
FPC_E_INVALID = -1
# the option sets of test_gpu_match_frames.test_key_pairing_equals_pairwise_match, plus one with a ratio
OPTIONS = ((True, 0.0, 0.0), (False, 0.0, 0.0), (True, 0.7, 0.0), (False, 0.7, 0.0), (True, 0.0, 0.8))


def engine(h=H, w=W, b=N, **kw):
    from fpc_amd.engine import Engine
    kw.setdefault("plan_flags", ["guard_zones"])
    return Engine(h, w, max_batch=b, **kw)


def _store_batch(e):
    for f, s in enumerate(SLOT_OF_FRAME):
        e.bank_store(f, s)


@pytest.fixture(scope="module")
def banked():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(conf_thresh=0.001)
    e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(300, N, H, W))
    counts = np.array([len(r[2]) for r in res])
    assert counts.min() > 1000, counts
    rows = int(counts.max()) - 37                       # smaller than the largest count: that frame is truncated
    nbytes = e.bank_create(SLOTS, rows)
    info = e.bank_info()
    assert info["slots"] == SLOTS and info["rows"] == rows and info["desc_dim"] == 128 and info["bytes"] == nbytes
    assert 1 <= info["chunk"] <= SLOTS and nbytes >= SLOTS * rows * (128 * 4 + 8 + 4)
    _, _, bc = e.bank_view()
    e.sync()
    assert (bc.cpu().numpy() == 0).all()                # every slot starts empty
    _store_batch(e)
    e.sync()
    yield e, res, counts, rows
    assert e.check_guards() == 0                        # the bank's zones included
    e.bank_destroy()
    assert e.check_guards() == 0
    e.close()


def _slot_key(e, s):
    bd, bx, bc = e.bank_view()
    return (bd[s].clone(), bc[s:s + 1].clone()), (bx[s].clone(), bc[s:s + 1].clone())


def _frames_tables(e, n, s, cross, md, ratio):
    """fpc_match_frames of the last detect against bank slot s -> host (match [n,cap], dist bits [n,cap])."""
    key, _ = _slot_key(e, s)
    m, d = e.match_frames_async(n, key=key, pairing="key", cross_check=cross, max_dist=md, ratio=ratio)
    e.sync()
    return m.cpu().numpy(), d.cpu().numpy().view(np.uint32)


def _expect_best(score, min_score=0):
    best = np.argmax(score, axis=1)                     # argmax: the first (lowest) slot on ties
    top = score[np.arange(len(score)), best]
    return np.where(top >= max(min_score, 1), best, -1).astype(np.int32)


def test_bank_holds_the_stored_frames(banked):
    e, res, counts, rows = banked
    bd, bx, bc = (t.cpu().numpy() for t in e.bank_view())
    assert (bc[EMPTY] == 0).all()
    assert (counts > rows).any()                        # at least one frame was truncated
    for f, s in enumerate(SLOT_OF_FRAME):
        k = min(counts[f], rows)
        assert bc[s] == k
        np.testing.assert_array_equal(bd[s, :k], res[f][2][:k])          # the first (most confident) rows
        np.testing.assert_array_equal(bx[s, :k], res[f][0][:k])


def test_scores_best_and_table_equal_match_frames_per_slot(banked):
    e, res, counts, rows = banked
    for cross, md, ratio in OPTIONS:
        score, best, m, d = e.match_bank_async(N, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        score, best, m, d = score.cpu().numpy(), best.cpu().numpy(), m.cpu().numpy(), d.cpu().numpy().view(np.uint32)
        tables = {}
        for s in range(SLOTS):
            tables[s] = _frames_tables(e, N, s, cross, md, ratio)
            want = (tables[s][0] >= 0).sum(axis=1)
            print("options", (cross, md, ratio), "slot", s, "score", score[:, s], "match_frames", want)
            np.testing.assert_array_equal(score[:, s], want)
        assert (score[:, EMPTY] == 0).all()
        np.testing.assert_array_equal(best, _expect_best(score))
        for f in range(N):
            assert best[f] >= 0
            np.testing.assert_array_equal(m[f], tables[best[f]][0][f])
            np.testing.assert_array_equal(d[f], tables[best[f]][1][f])   # bit for bit
        if md > 0:
            # a frame detected again: its own slot reaches the largest score (every kept row is 0 away from its copy) ...
            own = score[np.arange(N), SLOT_OF_FRAME]
            np.testing.assert_array_equal(own, score.max(axis=1))
            if cross:
                np.testing.assert_array_equal(best, SLOT_OF_FRAME)       # ... and with the cross check it is the only one
            # (without the cross check every row of these synthetic-weight descriptors has SOME row of every other frame
            # closer than 0.7, so all stored slots tie at count[f] and the rule gives the lowest slot: asserted above)


def test_min_score_and_outputs_that_may_be_null(banked):
    import torch
    e, res, counts, rows = banked
    score, best, m, d = e.match_bank_async(N, max_dist=0.7)
    e.sync()
    top = int(score.cpu().numpy().max())
    s2, b2, m2, d2 = e.match_bank_async(N, max_dist=0.7, min_score=top + 1)
    e.sync()
    np.testing.assert_array_equal(s2.cpu().numpy(), score.cpu().numpy())
    assert (b2.cpu().numpy() == -1).all() and (m2.cpu().numpy() == -1).all() and torch.isinf(d2).all()
    s3, b3, m3, d3 = e.match_bank_async(N, max_dist=0.7, min_score=top)
    e.sync()
    want = _expect_best(score.cpu().numpy(), top)
    np.testing.assert_array_equal(b3.cpu().numpy(), want)
    assert (want >= 0).any() and ((m3.cpu().numpy() >= 0).any(axis=1) == (want >= 0)).all()
    # score only / best only / no table
    lib = _lib.load()
    sc = torch.full((N, SLOTS), -7, dtype=torch.int32, device=e.torch_device)
    bs = torch.full((N,), -7, dtype=torch.int32, device=e.torch_device)
    torch.cuda.synchronize()
    assert lib.fpc_match_bank(e._ctx, N, 1, 0.7, 0.0, 0, sc.data_ptr(), None, None, None) == 0
    assert lib.fpc_match_bank(e._ctx, N, 1, 0.7, 0.0, 0, None, bs.data_ptr(), None, None) == 0
    e.sync()
    np.testing.assert_array_equal(sc.cpu().numpy(), score.cpu().numpy())
    np.testing.assert_array_equal(bs.cpu().numpy(), best.cpu().numpy())


def test_clear_and_store_rows(banked):
    import torch
    e, res, counts, rows = banked
    e.bank_clear(SLOT_OF_FRAME[3])
    score, best, _, _ = e.match_bank_async(N, max_dist=0.7, table=False)
    e.sync()
    assert (score.cpu().numpy()[:, SLOT_OF_FRAME[3]] == 0).all() and best.cpu().numpy()[3] != SLOT_OF_FRAME[3]
    # a saved map: frame 3's host arrays back into its slot (truncated to `rows` by the device clamp)
    e.bank_store_rows(SLOT_OF_FRAME[3], res[3][2], res[3][0])
    # ... and a copy of frame 6 into an empty slot from device memory with a device count: ties go to the lower slot
    low = EMPTY[0]
    assert low < SLOT_OF_FRAME[6]
    e.bank_store_rows(low, e.keep_frame(6), e.keep_frame_points(6))
    score, best, _, _ = e.match_bank_async(N, max_dist=0.7, table=False)
    e.sync()
    score, best = score.cpu().numpy(), best.cpu().numpy()
    bd, bx, bc = (t.cpu().numpy() for t in e.bank_view())
    k = min(counts[3], rows)
    assert bc[SLOT_OF_FRAME[3]] == k and bc[low] == min(counts[6], rows)
    np.testing.assert_array_equal(bd[SLOT_OF_FRAME[3], :k], res[3][2][:k])
    np.testing.assert_array_equal(bx[SLOT_OF_FRAME[3], :k], res[3][0][:k])
    np.testing.assert_array_equal(score[:, low], score[:, SLOT_OF_FRAME[6]])     # two identical slots
    assert best[6] == low and best[3] == SLOT_OF_FRAME[3]
    e.bank_clear(low)
    # every slot empty: no slot, an all -1 table
    e.bank_clear()
    score, best, m, d = e.match_bank_async(N, max_dist=0.7)
    e.sync()
    assert (score.cpu().numpy() == 0).all() and (best.cpu().numpy() == -1).all()
    assert (m.cpu().numpy() == -1).all() and torch.isinf(d).all()
    _store_batch(e)                                      # (the module's later tests see the bank of the fixture again)
    e.sync()


def test_asynchronous_flow_equals_the_synchronous_calls(banked):
    import torch
    e, res, counts, rows = banked
    frames1 = torch.from_numpy(synth.make_batch(300, N, H, W)).to(e.torch_device).contiguous()
    frames2 = torch.from_numpy(synth.make_batch(400, N, H, W)).to(e.torch_device).contiguous()
    torch.cuda.synchronize()
    e.bank_clear()
    # one sequence, no host call between its parts
    e.detect_async(frames1, N)
    _store_batch(e)
    e.detect_async(frames2, N)
    score, best, m, d = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    hm, ni, mask = e.homography_bank_async(N, best, m)
    e.sync()
    got = [t.cpu().numpy() for t in (score, best, m, d.view(torch.int32), hm.view(torch.int32), ni, mask)]
    # the same with a synchronisation after every step
    e.bank_clear()
    e.sync()
    e.detect(frames1.cpu().numpy())
    _store_batch(e)
    e.sync()
    e.detect(frames2.cpu().numpy())
    score, best, m, d = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    e.sync()
    hm, ni, mask = e.homography_bank_async(N, best, m)
    e.sync()
    want = [t.cpu().numpy() for t in (score, best, m, d.view(torch.int32), hm.view(torch.int32), ni, mask)]
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    e.detect(synth.make_batch(300, N, H, W))             # (the module's later tests see batch 1 again)


def _assert_homography_equals_frames(e, n, slot, match, **params):
    """fpc_homography_bank against fpc_homography_frames with the bank xy of every slot that occurs, bit for bit."""
    import torch
    hm, ni, mask = e.homography_bank_async(n, slot, match, **params)
    e.sync()
    hm, ni, mask, sl = hm.cpu().numpy().view(np.uint32), ni.cpu().numpy(), mask.cpu().numpy(), slot.cpu().numpy()
    for s in sorted(set(sl.tolist())):
        rows_of = np.flatnonzero(sl == s)
        if s < 0 or s >= SLOTS:
            assert (hm[rows_of] == 0).all() and (ni[rows_of] == 0).all() and not mask[rows_of].any()
            continue
        _, key_xy = _slot_key(e, s)
        rh, rn, rm = e.homography_frames_async(n, match, key_xy=key_xy, pairing="key", **params)
        e.sync()
        np.testing.assert_array_equal(hm[rows_of], rh.cpu().numpy().view(np.uint32)[rows_of])
        np.testing.assert_array_equal(ni[rows_of], rn.cpu().numpy()[rows_of])
        np.testing.assert_array_equal(mask[rows_of], rm.cpu().numpy()[rows_of])
    return hm.view(np.float32), ni, mask


def test_homography_bank_equals_homography_frames_and_finds_the_identity(banked):
    import torch
    e, res, counts, rows = banked
    score, best, m, d = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    e.sync()
    np.testing.assert_array_equal(best.cpu().numpy(), SLOT_OF_FRAME)
    hm, ni, mask = _assert_homography_equals_frames(e, N, best, m)
    # a frame matched to its own stored copy: the identity, to 1e-3 px at the four image corners
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64)
    for f in range(N):
        assert ni[f] >= 8 and mask[f].sum() == ni[f]
        p = corners @ hm[f].astype(np.float64).T
        p = p[:, :2] / p[:, 2:3]
        err = np.abs(p - corners[:, :2]).max()
        print("frame", f, "inliers", ni[f], "corner error", err)
        assert err < 1e-3
    # slots given by the caller: out of range -> the frame fails; a wrong slot is still fpc_homography_frames' answer
    slot = best.clone()
    slot[1], slot[4], slot[6] = -1, SLOTS, SLOT_OF_FRAME[0]
    _assert_homography_equals_frames(e, N, slot, m, seed=5, iterations=256)
    hm2, ni2, mask2 = e.homography_bank(N, slot, m, seed=5, iterations=256)
    assert (hm2[[1, 4]] == 0).all() and (ni2[[1, 4]] == 0).all() and not mask2[[1, 4]].any()
    # a second batch against the bank of the first: whatever slots win, the two entry points agree
    e.detect(synth.make_batch(400, N, H, W))
    score, best, m, d = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    _assert_homography_equals_frames(e, N, best, m)
    e.detect(synth.make_batch(300, N, H, W))


def test_relocalise_batch(banked):
    from fpc_amd.inference import relocalise_batch
    e, res, counts, rows = banked
    out = relocalise_batch(e, N)
    assert [o[0] for o in out] == SLOT_OF_FRAME
    for f, (slot, score, hm, ninl) in enumerate(out):
        assert score >= ninl >= 8 and hm.shape == (3, 3) and abs(hm[2, 2] - 1) < 1e-6


def test_repeated_calls_are_bit_identical(banked):
    import torch
    e, res, counts, rows = banked
    outs = []
    for _ in range(2):
        score, best, m, d = e.match_bank_async(N, cross_check=True, max_dist=0.9, ratio=0.9)
        hm, ni, mask = e.homography_bank_async(N, best, m, seed=3)
        e.sync()
        outs.append([t.cpu().numpy() for t in (score, best, m, d.view(torch.int32), hm.view(torch.int32), ni, mask)])
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, res, counts, rows = banked
    lib = _lib.load()
    dev = e.torch_device
    sc = torch.full((N + 1, SLOTS), -7, dtype=torch.int32, device=dev)
    bs = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    hm = torch.full((N + 1, 9), -7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N + 1,), -7, dtype=torch.int32, device=dev)
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx = e._ctx
    mb = lambda n, cross, md, ratio, ms, s=sc.data_ptr(), b=bs.data_ptr(): lib.fpc_match_bank(  # noqa: E731
        ctx, n, cross, md, ratio, ms, s, b, mt.data_ptr(), None)
    assert mb(N + 1, 1, 0.7, 0.0, 0) == FPC_E_INVALID            # more frames than the last call
    assert mb(0, 1, 0.7, 0.0, 0) == FPC_E_INVALID
    assert mb(N, 1, -1.0, 0.0, 0) == FPC_E_INVALID               # max_dist < 0
    assert mb(N, 1, 0.7, 1.5, 0) == FPC_E_INVALID                # ratio outside [0, 1]
    assert mb(N, 1, 0.7, -0.1, 0) == FPC_E_INVALID
    assert mb(N, 1, 0.7, 0.0, -1) == FPC_E_INVALID               # min_score < 0
    assert mb(N, 1, 0.7, 0.0, 0, None, None) == FPC_E_INVALID    # neither score nor best
    assert lib.fpc_bank_create(ctx, 4, 16) == FPC_E_INVALID      # a bank already exists
    assert lib.fpc_bank_store(ctx, N, 0) == FPC_E_INVALID        # frame out of range
    assert lib.fpc_bank_store(ctx, -1, 0) == FPC_E_INVALID
    assert lib.fpc_bank_store(ctx, 0, SLOTS) == FPC_E_INVALID    # slot out of range
    assert lib.fpc_bank_store(ctx, 0, -1) == FPC_E_INVALID
    assert lib.fpc_bank_clear(ctx, SLOTS) == FPC_E_INVALID
    assert lib.fpc_bank_clear(ctx, -2) == FPC_E_INVALID
    kd, kc = e.keep_frame(0)
    kx = e.keep_frame_points(0)
    e.sync()
    sr = lambda s, d, x, c: lib.fpc_bank_store_rows(ctx, s, d, x, c)          # noqa: E731
    assert sr(SLOTS, kd.data_ptr(), kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID
    assert sr(0, None, kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID
    assert sr(0, kd.data_ptr(), None, kc.data_ptr()) == FPC_E_INVALID
    assert sr(0, kd.data_ptr(), kx.data_ptr(), None) == FPC_E_INVALID
    assert sr(0, kd.data_ptr() + 4, kx.data_ptr(), kc.data_ptr()) == FPC_E_INVALID      # not 16-byte aligned
    rp = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(rp))
    hb = lambda n, s, m, p, h=hm.data_ptr(), k=ni.data_ptr(): lib.fpc_homography_bank(ctx, n, s, m, p, h, k, None)  # noqa: E731
    assert hb(N + 1, slot.data_ptr(), mt.data_ptr(), ctypes.byref(rp)) == FPC_E_INVALID
    assert hb(0, slot.data_ptr(), mt.data_ptr(), ctypes.byref(rp)) == FPC_E_INVALID
    assert hb(N, None, mt.data_ptr(), ctypes.byref(rp)) == FPC_E_INVALID
    assert hb(N, slot.data_ptr(), None, ctypes.byref(rp)) == FPC_E_INVALID
    assert hb(N, slot.data_ptr(), mt.data_ptr(), None) == FPC_E_INVALID
    assert hb(N, slot.data_ptr(), mt.data_ptr(), ctypes.byref(rp), None) == FPC_E_INVALID
    bad = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(bad))
    bad.iterations = 0
    assert hb(N, slot.data_ptr(), mt.data_ptr(), ctypes.byref(bad)) == FPC_E_INVALID
    bad.iterations, bad.min_inliers = 16, 3
    assert hb(N, slot.data_ptr(), mt.data_ptr(), ctypes.byref(bad)) == FPC_E_INVALID
    e.sync()
    # nothing was written: outputs, and the bank itself
    for t in (sc, bs, mt, ni):
        assert (t.cpu().numpy() == -7).all()
    assert (hm.cpu().numpy() == -7.0).all()
    bc = e.bank_view()[2].cpu().numpy()
    for f, s in enumerate(SLOT_OF_FRAME):
        assert bc[s] == min(counts[f], rows)
    assert (bc[EMPTY] == 0).all()
    # results without descriptors: fpc_get_points without a descriptor map
    prob = torch.zeros((2, H, W), device=dev)
    e.get_points(prob)
    assert mb(2, 1, 0.7, 0.0, 0) == FPC_E_INVALID
    assert lib.fpc_bank_store(ctx, 0, 0) == FPC_E_INVALID
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))
    # contexts without a bank / without the descriptor head
    d = engine(b=2)
    d.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    d.detect(synth.make_batch(300, 2, H, W))
    view = _lib.FpcBankView()
    assert lib.fpc_match_bank(d._ctx, 2, 1, 0.7, 0.0, 0, sc.data_ptr(), bs.data_ptr(), None, None) == FPC_E_INVALID
    assert lib.fpc_bank_store(d._ctx, 0, 0) == FPC_E_INVALID
    assert lib.fpc_bank_clear(d._ctx, -1) == FPC_E_INVALID
    assert lib.fpc_bank_get(d._ctx, ctypes.byref(view)) == FPC_E_INVALID
    assert lib.fpc_bank_destroy(d._ctx) == FPC_E_INVALID
    assert lib.fpc_homography_bank(d._ctx, 2, slot.data_ptr(), mt.data_ptr(), ctypes.byref(rp), hm.data_ptr(), ni.data_ptr(), None) == FPC_E_INVALID
    assert lib.fpc_bank_create(d._ctx, 0, 16) == FPC_E_INVALID
    assert lib.fpc_bank_create(d._ctx, _lib.BANK_MAX_SLOTS + 1, 16) == FPC_E_INVALID
    assert lib.fpc_bank_create(d._ctx, 4, 0) == FPC_E_INVALID
    assert lib.fpc_bank_create(d._ctx, 4, d.capacity + 1) == FPC_E_INVALID
    assert d.check_guards() == 0
    d.close()                                            # (and a context closed with a live bank frees it: below)
    m = engine(descriptor_enabled=False, b=2)
    assert lib.fpc_bank_create(m._ctx, 4, 16) == FPC_E_INVALID
    m.close()
    e.sync()
    assert (sc.cpu().numpy() == -7).all()


@pytest.mark.parametrize("variant", ["one_slot_one_frame", "vgg", "bf16", "count_equals_rows"])
def test_edge_sizes(variant):
    """slots = 1 and n = 1; FPC_ARCH_VGG (D = 256); an FPC_BF16 context; count == rows (a small max_keypoints)."""
    import torch
    if variant == "vgg":
        e = engine(in_channels=1, arch="vgg")
        e.load_state_dict(synth.make_vgg_state_dict(4, 3.0))
        frames = synth.make_batch(300, N, H, W, gray=True)[:, :1]
    else:
        kw = {"max_keypoints": 200} if variant == "count_equals_rows" else {"dtype": "bf16"} if variant == "bf16" else {}
        e = engine(conf_thresh=0.001, **kw)
        e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
        frames = synth.make_batch(300, N, H, W)
    res = e.detect(np.ascontiguousarray(frames))
    counts = np.array([len(r[2]) for r in res])
    assert counts.sum() > 100
    slots = 1 if variant == "one_slot_one_frame" else 5
    n = 1 if variant == "one_slot_one_frame" else N
    e.bank_create(slots, 200 if variant == "count_equals_rows" else None)
    if variant == "count_equals_rows":
        assert e.capacity == 200 and (counts == 200).all()
    stored = {0: 0} if slots == 1 else {3: 1, 0: 2, 4: 6}      # slot -> frame; slot 1 / 2 stay empty
    for s, f in stored.items():
        e.bank_store(f, s)
    bd, bx, bc = e.bank_view()
    e.sync()
    assert bd.shape[2] == (256 if variant == "vgg" else 128)
    for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
        score, best, m, d = e.match_bank_async(n, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        score, best, m, d = score.cpu().numpy(), best.cpu().numpy(), m.cpu().numpy(), d.cpu().numpy().view(np.uint32)
        tables = {}
        for s in range(slots):
            mm, dd = e.match_frames_async(n, key=(bd[s].clone(), bc[s:s + 1].clone()), cross_check=cross, max_dist=md,
                                          ratio=ratio)
            e.sync()
            tables[s] = (mm.cpu().numpy(), dd.cpu().numpy().view(np.uint32))
            np.testing.assert_array_equal(score[:, s], (tables[s][0] >= 0).sum(axis=1))
        np.testing.assert_array_equal(best, _expect_best(score))
        for f in range(n):
            if best[f] >= 0:
                np.testing.assert_array_equal(m[f], tables[best[f]][0][f])
                np.testing.assert_array_equal(d[f], tables[best[f]][1][f])
            else:
                assert (m[f] == -1).all()
        if md > 0:
            for s, f in stored.items():
                if f < n and counts[f]:
                    assert best[f] == s
    score, best, m, _ = e.match_bank_async(n, max_dist=0.7)
    hm, ni, mask = e.homography_bank_async(n, best, m)
    e.sync()
    bh = best.cpu().numpy()
    for s in sorted(set(bh.tolist()) - {-1}):
        rh, rn, rm = e.homography_frames_async(n, m, key_xy=(bx[s].clone(), bc[s:s + 1].clone()))
        e.sync()
        rows_of = np.flatnonzero(bh == s)
        np.testing.assert_array_equal(hm.cpu().numpy().view(np.uint32)[rows_of], rh.cpu().numpy().view(np.uint32)[rows_of])
        np.testing.assert_array_equal(ni.cpu().numpy()[rows_of], rn.cpu().numpy()[rows_of])
        np.testing.assert_array_equal(mask.cpu().numpy()[rows_of], rm.cpu().numpy()[rows_of])
    assert e.check_guards() == 0
    e.close()                                            # fpc_destroy frees the bank that is still alive
