"""Map growth on the GPU (fpc_landmarks_pairs / fpc_landmarks_frames / fpc_landmarks_bank) against the float64 restatement and
the planted batches of tests/test_landmarks.py: the explicit call row by row, the frames call bit-identical to explicit pairs
and the bank call to the frames call (on either bank format, with and without landmark storage), a chain end to end -- key
frame B's landmarks, C localised and given landmarks, C stored, D localised against C -- without a host call in between,
determinism and the argument checks.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_homography_ransac import engine
from tests.test_landmarks import (CHAIN_PNP, CHAIN_ROT_BAR, CHAIN_TRANS_BAR, KQVGA, NEAR_CAP, STRIDE, WORLD_H, WORLD_N, WORLD_W,
                                  chain_scene, explicit_batch, frames_world, rule_of, world_lists)
from tests.test_pnp_ransac import FRAME_H, FRAME_W, KVEC, pose_errors

pytestmark = pytest.mark.gpu

H, W, N = WORLD_H, WORLD_W, WORLD_N
FPC_E_INVALID = -1
# Device against restatement: both evaluate the rule in fp64 in the same order (the device with contraction off) and round
# once to fp32 (resolution 6e-8), so the bar is test_gpu_pose_epipolar.py's XYZ_BAR, 1e-5 of a point's length.  Measured on
# the MI355X over the eight frames of explicit_batch(): worst difference 0.0 -- the same fp32 values -- and no row left out
# as near.  The chain's bars are the restated chain's (tests/test_landmarks.py), not the device's: the device reproduced its
# figures, 0.0178 deg / 3.070e-04 with every kind and 0.0224 deg / 1.051e-03 with kind 2 only.
XYZ_BAR = 1e-5
CAMS = dict(K_query=KQVGA, K_train=KQVGA)


@pytest.fixture(scope="module")
def qvga():
    """An 8-frame QVGA context whose last call left 8 frames of results; no PnP reservation: the calls need none."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    assert e.capacity >= STRIDE
    prob = torch.zeros((N, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((N, e.desc_dim, H // 8, W // 8)))
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(got, want, rows=slice(None)):
    for a, b in zip(got, want):
        _bits(a[rows], b[rows])


def _raw_pairs(e, q_xy, t_xy, t_xyz, t_valid, npairs, r, t, fill=0xFF, **params):
    """fpc_landmarks_pairs into outputs pre-filled with `fill` bytes -> host arrays (xyz, kind, counts)."""
    import torch
    dev = e.torch_device
    n, stride = q_xy.shape[0], q_xy.shape[1]
    p = e._landmark_params(None, None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (q_xy, t_xy, t_xyz, t_valid, npairs,
                                                                       r.astype(np.float32), t.astype(np.float32))]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev) for shape in ((n, stride * 12), (n, stride), (n, 8))]
    torch.cuda.synchronize()
    e._call("fpc_landmarks_pairs", n, ins[0], ins[1], ins[2], ins[3], ins[4], stride, ins[5], ins[6], ctypes.byref(p), *outs,
            inputs=ins)
    e.sync()
    xyz, kind, counts = (o.cpu().numpy() for o in outs)
    return xyz.view(np.float32).reshape(n, stride, 3), kind, counts.view(np.int32).reshape(n, 2)


def _pack(frames):
    n = len(frames)
    q_xy, t_xy = np.zeros((n, STRIDE, 2), np.float32), np.zeros((n, STRIDE, 2), np.float32)
    t_xyz, t_valid = np.zeros((n, STRIDE, 3), np.float32), np.zeros((n, STRIDE), np.uint8)
    for f, fr in enumerate(frames):
        q_xy[f], t_xy[f], t_xyz[f], t_valid[f] = fr.q_xy, fr.t_xy, fr.t_xyz, fr.t_valid
    return (q_xy, t_xy, t_xyz, t_valid, np.array([fr.npairs for fr in frames], np.int32),
            np.stack([fr.R for fr in frames]), np.stack([fr.t for fr in frames]))


def test_explicit_call_against_the_restatement(qvga):
    e = qvga
    frames = explicit_batch()
    assert [fr.npairs for fr in frames[:6]] == [0, 1, 255, 256, 257, STRIDE] and len(frames) == N
    args = _pack(frames)
    xyz, kind, counts = _raw_pairs(e, *args)
    assert set(np.unique(kind).tolist()) <= {0, 1, 2} and np.isfinite(xyz).all()     # no 0xFF left: every row was written
    worst, left_out = 0.0, 0
    for f, fr in enumerate(frames):
        m = fr.npairs
        want = rule_of(fr)
        assert not kind[f, m:].any() and not xyz[f, m:].any(), f                     # rows past the count: zeros
        assert tuple(counts[f]) == ((kind[f] == 1).sum(), (kind[f] == 2).sum()), f
        assert not xyz[f][kind[f] == 0].any(), f
        clear = ~want.near
        assert want.near.sum() <= NEAR_CAP * max(m, 1), f
        left_out += int(want.near.sum())
        np.testing.assert_array_equal(kind[f, :m][clear], want.kind[clear], err_msg=str(f))
        if clear.all():
            assert tuple(counts[f]) == want.counts, (f, counts[f], want.counts)
        both = (kind[f, :m] == want.kind) & (want.kind != 0)
        if both.any():
            ref = want.xyz[both]
            rel = np.linalg.norm(xyz[f, :m][both].astype(np.float64) - ref, axis=1) / np.linalg.norm(ref, axis=1)
            worst = max(worst, rel.max())
            assert rel.max() <= XYZ_BAR, (f, rel.max())
    for f in (6, 7):                                                                 # the all-zero pose and the NaN pose
        assert not kind[f].any() and not xyz[f].any() and not counts[f].any(), f
    assert counts[5, 0] > 200 and counts[5, 1] > 100 and counts[4, 1] > 50           # both branches ran
    print("explicit call: worst xyz difference %.3e of a point's length (bar %.0e), %d rows left out as near"
          % (worst, XYZ_BAR, left_out))
    # counts are clamped to [0, stride]; a frame is what it is alone; repeated calls give the same bits
    npairs = args[4].copy()
    npairs[5], npairs[0] = STRIDE + 9, -3
    again = _raw_pairs(e, *args[:4], npairs, *args[5:])
    _same(again, (xyz, kind, counts))
    alone = _raw_pairs(e, *(a[[5]] for a in args))
    _same(alone, (xyz[[5]], kind[[5]], counts[[5]]))
    # without landmarks every row is triangulated; without flags every finite landmark counts
    tri = e.landmarks_pairs(args[0], args[1], args[4], args[5], args[6])
    assert set(np.unique(tri[1]).tolist()) <= {0, 2} and not tri[2][:, 0].any() and tri[2][5, 1] > counts[5, 1]
    flagless = e.landmarks_pairs(args[0], args[1], args[4], args[5], args[6], t_xyz=args[2])
    want = rule_of(frames[5]._replace(t_valid=np.ones(STRIDE, np.uint8)))
    np.testing.assert_array_equal(flagless[1][5][~want.near], want.kind[~want.near])
    assert flagless[2][5, 0] > counts[5, 0]


def _plant_views(e, views):
    """The views' pixels and counts in place of the last call's results -> the match table (device, int32 [N,cap])."""
    import torch
    cap = e.capacity
    xy, count = e._points_view()
    hx, hm = np.zeros((N, cap, 2), np.int32), np.full((N, cap), -1, np.int32)
    for f, (pix, match, _, _) in enumerate(views):
        hx[f, :len(pix)], hm[f, :len(match)] = pix, match
        hm[f, len(match):len(match) + 8] = 3                                        # rows past the count are never pairs
    xy[:N].copy_(torch.from_numpy(hx))
    count[:N].copy_(torch.tensor([len(v[0]) for v in views], dtype=torch.int32))
    torch.cuda.synchronize()
    return torch.from_numpy(hm).to(e.torch_device)


def _scattered(ref, rows, npairs, cap):
    """The explicit call's outputs put back on the query rows their pairs came from."""
    xyz, kind = np.zeros((N, cap, 3), np.float32), np.zeros((N, cap), np.uint8)
    for f in range(N):
        xyz[f, rows[f]], kind[f, rows[f]] = ref[0][f, :npairs[f]], ref[1][f, :npairs[f]]
    return xyz, kind, ref[2]


def test_frames_and_bank_calls_are_bit_identical_to_explicit_pairs(qvga):
    import torch
    e = qvga
    cap, dev = e.capacity, e.torch_device
    world = frames_world()
    nkey = len(world.key_xy)
    match = _plant_views(e, world.views)
    rm = np.stack([v[2] for v in world.views]).astype(np.float32)
    tv = np.stack([v[3] for v in world.views]).astype(np.float32)
    rm[7], tv[7] = 0.0, 0.0                                                          # a failed frame among them

    def explicit(**how):
        q_xy, t_xy, t_xyz, t_valid, npairs, rows = world_lists(world, how.pop("nkey", nkey), cap, **how)
        lm = dict(t_xyz=t_xyz, t_valid=t_valid) if how.get("with_landmarks", True) else {}
        return _scattered(e.landmarks_pairs(q_xy, t_xy, npairs, rm, tv, **lm, **CAMS), rows, npairs, cap)
    got = e.landmarks_frames(N, match, rm, tv, world.key_xy, world.key_xyz, world.key_valid, **CAMS)
    _same(got, explicit())
    assert not got[1][7].any() and not got[0][7].any() and not got[2][7].any()
    assert (got[2][:7, 0] > 50).all() and (got[2][:7:2, 1] > 50).all()              # carried over; triangulated (wide views)
    assert got[2][1::2, 1].sum() < got[2][0:7:2, 1].sum()                            # the short baselines are cut
    for f, (pix, _, _, _) in enumerate(world.views):
        assert not got[1][f, len(pix):].any() and not got[0][f, len(pix):].any(), f  # rows past the count
    every = e.landmarks_frames(N, match, rm, tv, world.key_xy, world.key_xyz, None, **CAMS)      # no flags
    _same(every, explicit(key_valid=None))
    assert (every[2][:7, 0] > got[2][:7, 0]).all()
    kx = torch.from_numpy(world.key_xy).to(dev)
    kz = torch.from_numpy(world.key_xyz).to(dev)
    c300 = torch.tensor([300], dtype=torch.int32, device=dev)
    few = e.landmarks_frames(N, match, rm, tv, (kx, c300), (kz, c300), world.key_valid, **CAMS)  # a key count below the rows
    _same(few, explicit(nkey=300))
    bare = e.landmarks_frames(N, match, rm, tv, world.key_xy, **CAMS)               # a key without landmarks
    _same(bare, explicit(with_landmarks=False))
    assert not bare[2][:, 0].any() and set(np.unique(bare[1]).tolist()) == {0, 2}
    # the bank: slot s holds the key's rows (any descriptors) and its landmarks
    slots = 3
    desc = np.random.default_rng(1).normal(size=(nkey, e.desc_dim)).astype(np.float32)
    full_xyz, full_valid = np.zeros((cap, 3), np.float32), np.zeros(cap, bool)
    full_xyz[:nkey], full_valid[:nkey] = world.key_xyz, world.key_valid
    full_xyz[nkey:], full_valid[nkey:] = 1.0, True                                  # behind the count: invalid all the same
    slot = torch.tensor([0, 1, 2, -1, slots, 0, 1, 2], dtype=torch.int32, device=dev)
    banks = {}
    for fmt in ("f32", "bf16"):
        e.bank_create(slots, cap, format=fmt)
        try:
            for s, k in ((0, nkey), (1, nkey), (2, 300)):
                e.bank_store_rows(s, desc[:k], world.key_xy[:k])
            plain = e.landmarks_bank(N, slot, match, rm, tv, **CAMS)                # no landmark storage: triangulation only
            for v in plain:
                assert not v[[3, 4, 7]].any()                                        # no slot, or a failed pose: zeros
            _same(plain, bare, [0, 1, 5, 6])
            few_bare = e.landmarks_frames(N, match, rm, tv, (kx, c300), **CAMS)
            _same(plain, few_bare, [2])
            assert e.bank_landmarks_reserve() >= slots * cap * 16
            e.bank_store_landmarks(0, full_xyz, full_valid)
            e.bank_store_landmarks(1, full_xyz, None)
            e.bank_store_landmarks(2, full_xyz, full_valid)
            bank = banks[fmt] = e.landmarks_bank(N, slot, match, rm, tv, **CAMS)
            for v in bank:
                assert not v[[3, 4, 7]].any()
            for rows_of, ref in (([0, 5], got), ([1, 6], every), ([2], few)):
                _same(bank, ref, rows_of)
            _same(e.landmarks_bank(N, slot, match, rm, tv, **CAMS), bank)           # repeated calls: the same bits
            # ... and against fpc_landmarks_frames with the slot's own storage as the key
            lm = e.bank_landmarks()
            _, bxy, bc = e.bank_view()
            for s in range(slots):
                ref = e.landmarks_frames(N, match, rm, tv, (bxy[s].contiguous(), bc[s:s + 1].clone()),
                                         (lm[s, :, :3].contiguous(), bc[s:s + 1].clone()), lm[s, :, 3] != 0, **CAMS)
                _same(bank, ref, np.flatnonzero(slot.cpu().numpy() == s))
            assert e.check_guards() == 0
        finally:
            e.bank_destroy()
    _same(banks["bf16"], banks["f32"])                                              # it reads xy, counts and landmarks only


def test_chain_end_to_end_grows_the_map_at_one_scale():
    """Key frame B with landmarks, C localised against it and given landmarks of its own, C stored as a key frame, D
    localised against C -- on the device without a host call between the first store and the final read: fpc_bank_store_rows
    (B), fpc_bank_store_landmarks, fpc_pnp_bank (C against B), fpc_landmarks_bank, fpc_bank_store (C), fpc_bank_store_landmarks
    (its xyz and kind as they are, or kind == 2 only), fpc_pnp_bank (D against C).  D's pose against the planted composition
    meets twice the worst error of the restated chain (tests/test_landmarks.py)."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        assert e.pnp_reserve() > 0
        cap, dev = e.capacity, e.torch_device
        ch = chain_scene()
        assert cap >= len(ch.pb)
        prob = torch.zeros((2, FRAME_H, FRAME_W))
        prob[:, 40, 40] = 0.5
        e.get_points(prob, torch.ones((2, e.desc_dim, FRAME_H // 8, FRAME_W // 8)))
        xy, count = e._points_view()
        desc = np.random.default_rng(2).normal(size=(len(ch.pb), e.desc_dim)).astype(np.float32)

        def plant(pix):
            hx = np.zeros((2, cap, 2), np.int32)
            hx[0, :len(pix)] = pix
            xy[:2].copy_(torch.from_numpy(hx))
            count[:2].copy_(torch.tensor([len(pix), 0], dtype=torch.int32))

        def table(m):
            full = np.full((2, cap), -1, np.int32)
            full[0, :len(m)] = m
            return torch.from_numpy(full).to(dev)
        m_cb, m_dc = table(ch.m_cb), table(ch.m_dc)
        lm_b, has_b = np.zeros((cap, 3), np.float32), np.zeros(cap, bool)
        lm_b[:len(ch.lm_b)], has_b[:len(ch.has_b)] = ch.lm_b, ch.has_b
        lm_b_dev, has_b_dev = torch.from_numpy(lm_b).to(dev), torch.from_numpy(has_b).to(dev)
        pb = ch.pb.astype(np.int32)
        slot_b = torch.tensor([0, -1], dtype=torch.int32, device=dev)
        slot_c = torch.tensor([1, -1], dtype=torch.int32, device=dev)
        e.bank_create(2, cap)
        e.bank_landmarks_reserve()
        for kinds in ((1, 2), (2,)):
            torch.cuda.synchronize()
            # ---- from here on nothing returns to the host until the pose of D is read
            e.bank_store_rows(0, desc, pb)
            e.bank_store_landmarks(0, lm_b_dev, has_b_dev)
            plant(ch.pc)
            rc, tc, nic, _ = e.pnp_bank_async(2, slot_b, m_cb, K=KVEC, **CHAIN_PNP)
            xyz, kind, counts = e.landmarks_bank_async(2, slot_b, m_cb, rc, tc, K_query=KVEC, K_train=KVEC)
            e.bank_store(0, 1)                                                       # C becomes slot 1 ...
            e.bank_store_landmarks(1, xyz[0], kind[0] if kinds == (1, 2) else kind[0] == 2)      # ... with its landmarks
            plant(ch.pd)
            rd, td, nid, _ = e.pnp_bank_async(2, slot_c, m_dc, K=KVEC, **CHAIN_PNP)
            rc, tc, nic, counts, kind, rd, td, nid = e._host((rc, tc, nic, counts, kind, rd, td, nid))
            assert nic[0] > 200 and nic[1] == 0 and not counts[1].any() and not kind[1].any()
            assert counts[0, 0] > 200 and counts[0, 1] > 200, counts
            assert not kind[0, ch.wrong_c][ch.m_cb[ch.wrong_c] >= 0].sum() > 5       # a wrong match passes only by chance
            rot, tr = pose_errors(rd[0], td[0], (None, None, None, ch.r_dc, ch.t_dc))
            print("chain on the device, kinds %s: C %d carried over, %d triangulated; D %d inliers, rotation %.4f deg (bar "
                  "%.4f), translation %.3e relative (bar %.3e)" % (kinds, *counts[0], nid[0], rot, CHAIN_ROT_BAR, tr,
                                                                   CHAIN_TRANS_BAR))
            assert nid[0] > 150 and not rd[1].any()
            assert rot <= CHAIN_ROT_BAR and tr <= CHAIN_TRANS_BAR, (kinds, rot, tr)
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused(qvga):
    import torch
    e = qvga
    lib = _lib.load()
    cap, dev = e.capacity, e.torch_device
    xy = torch.zeros((N, cap, 2), dtype=torch.float32, device=dev)
    xyz_in = torch.zeros((N, cap, 3), dtype=torch.float32, device=dev)
    valid = torch.ones((N, cap), dtype=torch.uint8, device=dev)
    npairs = torch.full((N,), 10, dtype=torch.int32, device=dev)
    kxy = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    match = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    slot = torch.zeros((N,), dtype=torch.int32, device=dev)
    one = torch.ones((1,), dtype=torch.int32, device=dev)
    rm = torch.eye(3, dtype=torch.float32, device=dev).repeat(N, 1, 1).contiguous()
    tv = torch.ones((N, 3), dtype=torch.float32, device=dev)
    out_xyz = torch.full((N, cap, 3), 7.0, dtype=torch.float32, device=dev)
    out_kind = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    out_counts = torch.full((N, 2), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    xp, zp, vp, np_, kp, mp, lp, op, rp, tp = (t.data_ptr() for t in (xy, xyz_in, valid, npairs, kxy, match, slot, one, rm, tv))
    ox, ok_, oc = (t.data_ptr() for t in (out_xyz, out_kind, out_counts))
    kz, kv = xyz_in[0].data_ptr(), valid[0].data_ptr()

    def params(**kw):
        p = _lib.FpcLandmarkParams()
        lib.fpc_default_landmark_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    pairs = lambda n, a, b, c, d, m, stride, r, t, p, x, k: lib.fpc_landmarks_pairs(e._ctx, n, a, b, c, d, m, stride, r, t, p, x, k, oc)   # noqa: E731,E501
    frames = lambda n, a, c, z, v, m, r, t, p, x, k: lib.fpc_landmarks_frames(e._ctx, n, a, c, z, v, m, r, t, p, x, k, oc)   # noqa: E731,E501
    bank = lambda n, s, m, r, t, p, x, k: lib.fpc_landmarks_bank(e._ctx, n, s, m, r, t, p, x, k, oc)                # noqa: E731
    ok = params()
    assert bank(N, lp, mp, rp, tp, ok, ox, ok_) == FPC_E_INVALID                     # no bank
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(q_fx=0.0), params(q_fy=-1.0), params(q_fx=nan), params(q_cy=inf), params(t_fx=0.0), params(t_fy=-2.0),
               params(t_cx=nan), params(t_fy=inf), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
               params(reproj_threshold=nan), params(reproj_threshold=1e18), params(min_parallax_deg=-0.5),
               params(min_parallax_deg=90.0), params(min_parallax_deg=nan), None]
        for p in bad:
            assert pairs(N, xp, xp, zp, vp, np_, cap, rp, tp, p, ox, ok_) == FPC_E_INVALID
            assert frames(N, kp, op, kz, kv, mp, rp, tp, p, ox, ok_) == FPC_E_INVALID
            assert bank(N, lp, mp, rp, tp, p, ox, ok_) == FPC_E_INVALID
        for k in range(11):                                                          # t_xyz (2) and t_valid (3) may be NULL
            if k in (2, 3, 5):
                continue
            a = [xp, xp, zp, vp, np_, cap, rp, tp, ok, ox, ok_]
            a[k] = None
            assert pairs(N, *a) == FPC_E_INVALID, k
        assert pairs(0, xp, xp, zp, vp, np_, cap, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        assert pairs(N + 1, xp, xp, zp, vp, np_, cap, rp, tp, ok, ox, ok_) == FPC_E_INVALID      # above max_batch
        assert pairs(N, xp, xp, zp, vp, np_, cap + 1, rp, tp, ok, ox, ok_) == FPC_E_INVALID      # stride above capacity
        assert pairs(N, xp, xp, zp, vp, np_, 0, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        for k in range(10):                                                          # key_xyz (2) and key_valid (3) may be NULL
            if k in (2, 3):
                continue
            a = [kp, op, kz, kv, mp, rp, tp, ok, ox, ok_]
            a[k] = None
            assert frames(N, *a) == FPC_E_INVALID, k
        assert frames(0, kp, op, kz, kv, mp, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        assert frames(N + 1, kp, op, kz, kv, mp, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        for k in range(7):
            a = [lp, mp, rp, tp, ok, ox, ok_]
            a[k] = None
            assert bank(N, *a) == FPC_E_INVALID, k
        assert bank(0, lp, mp, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        assert bank(N + 1, lp, mp, rp, tp, ok, ox, ok_) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        assert (out_xyz.cpu() == 7.0).all() and (out_kind.cpu() == 7).all() and (out_counts.cpu() == 7).all()
        # the accepted forms: NULL landmarks, NULL flags, NULL counts
        assert lib.fpc_landmarks_pairs(e._ctx, N, xp, xp, None, None, np_, cap, rp, tp, ok, ox, ok_, None) == 0
        e.sync()
        assert (out_counts.cpu() == 7).all() and not out_kind.cpu().numpy().any()    # ten equal pixels under t = 1: nothing
        assert frames(N, kp, op, None, None, mp, rp, tp, ok, ox, ok_) == 0
        assert bank(N, lp, mp, rp, tp, params(min_parallax_deg=0.0), ox, ok_) == 0
        e.sync()
        # no match (frames, bank): every row 0
        for t in (out_xyz, out_kind, out_counts):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
        e.sync()
    with pytest.raises(TypeError):
        e.landmarks_pairs(xy, xy, npairs, rm, tv, min_front=5)
    with pytest.raises(ValueError):
        e.landmarks_pairs(xy, xy, npairs, rm, tv, K_query=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.landmarks_frames(N, match, rm, tv, None)
    with pytest.raises(ValueError):
        e.landmarks_bank(N, slot, match, rm, tv)                                     # no bank
