"""Pose-guided matching on the GPU (fpc_match_frames_guided_pose / fpc_match_bank_guided_pose) against the float64
restatement and the planted 3-D scenes of tests/test_match_pose.py: indices and distances for the key and the bank as train
sets and every option set, bit-equality with fpc_match_frames where every pair is a candidate, strips and tiles of 0, 1, 2,
63, 64 and 65 rows, invalid landmarks and landmarks behind the camera, failed and non-finite poses, bad and empty slots, a
bank without landmarks, the chain match -> PnP -> guided match -> PnP without a host call in between (bank and key),
device-read counts, determinism, the argument checks and a D = 256 context.  The planted frames are written straight into
the library's device results as tests/test_gpu_match_guided.py's plant does, so the kernel and the restatement read the same
fp32 rows and integer pixels.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_match_guided import _compare, _host, engine, plant
from tests.test_gpu_pnp_ransac import R_SAME_BAR, T_SAME_BAR, _assert_mask_is_the_reprojection_test
from tests.test_match_guided import FRAME_H, FRAME_W
from tests.test_match_pose import (GPU_SCENE, GPU_SLOT_OF, GPU_VGG_SCENE, KVEC, OPTIONS, RADIUS, all_pass_radius,
                                   gpu_bank_trains, key_train, landmark_ok, planted_pose, pose_frames_rule, pose_gate,
                                   scene_of)
from tests.test_pnp_ransac import ROT_BAR, TRANS_BAR, pnp_rule, pose_errors

pytestmark = pytest.mark.gpu

N = 8
FPC_E_INVALID = -1
PNP = dict(iterations=256, seed=3)             # the other fields: fpc_default_pnp_params (3 px, 4 refits, 12 inliers)
THR = 3.0


@pytest.fixture(scope="module")
def planted():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    scene = scene_of(GPU_SCENE)
    assert e.capacity == GPU_SCENE["cap"] and (scene["counts"] == 820).all() and scene["K"] == 780 and len(scene["key"]) == 792
    assert e.pnp_reserve() > 0
    plant(e, scene)
    yield e, scene
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _clean(s, rows=None):
    """The key without flags and without the rows behind the cameras: every landmark valid with c > 0."""
    k = s["K"] if rows is None else rows
    return s["key"][:k], s["clean_xyz"][:k], None


def _big(s, rs, ts, xy, counts, trains):
    big = all_pass_radius(rs, ts, KVEC, xy, counts, trains)
    assert big is not None                                                 # the premise of a bit identity, by the restatement
    for f, k in enumerate(counts):
        assert pose_gate(rs[f], ts[f], KVEC, xy[f, :k], trains[f][1], trains[f][2], big)[0].all()
    return big


def test_indices_and_distances_equal_the_restatement(planted):
    import torch
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    rs, ts = planted_pose(s)
    key, xyz, valid = key_train(s)
    trains = [key_train(s)] * N
    for cross, md, ratio in OPTIONS:
        m, d = e.match_frames_guided_pose_async(N, rs, ts, RADIUS, key, xyz, valid, K=KVEC, cross_check=cross, max_dist=md,
                                                ratio=ratio)
        e.sync()
        m, d = _host(m, d)
        _compare(m, d, pose_frames_rule(desc, xy, counts, trains, rs, ts, KVEC, RADIUS, cross, md, ratio), counts,
                 "key %s" % ((cross, md, ratio),))
        if ratio == 0:
            assert (m >= 0).sum() > 4000
        got = m[m >= 0]
        assert landmark_ok(s)[got].all() and (got < s["K"]).all()           # never an invalid landmark or one behind the camera
    # R as [n,3,3], K as a matrix and as the default, device tensors, and the per-frame form of the host wrapper
    kmat = np.array([[KVEC[0], 0, KVEC[2]], [0, KVEC[1], KVEC[3]], [0, 0, 1]])
    got = e.match_frames_guided_pose(N, torch.from_numpy(rs.reshape(N, 3, 3)).to(e.torch_device),
                                     torch.from_numpy(ts).to(e.torch_device), RADIUS, key, xyz, valid, K=kmat)
    assert [len(g[0]) for g in got] == list(counts)
    want = pose_frames_rule(desc, xy, counts, trains, rs, ts, KVEC, RADIUS)[0]
    truth_ok = landmark_ok(s)[np.maximum(s["ids"], 0)] & (s["ids"] >= 0)
    for f in range(N):
        assert (got[f][0] >= 0).sum() == truth_ok[f].sum() == (want[f] >= 0).sum()      # every planted pair, as on the CPU
    dflt = e.match_frames_guided_pose(N, rs, ts, RADIUS, key, xyz, valid)
    for a, b in zip(got, dflt):
        np.testing.assert_array_equal(a[0], b[0])
    # another camera is another gate
    off = e.match_frames_guided_pose(N, rs, ts, RADIUS, key, xyz, valid, K=(500.0, 500.0, 300.0, 240.0))
    assert 2 * sum(int((g[0] >= 0).sum()) for g in off) < sum(int((g[0] >= 0).sum()) for g in got)
    # the key's count and the landmarks as device pairs: rows past the count are no train rows
    kd = torch.from_numpy(key).to(e.torch_device)
    kx = torch.from_numpy(xyz).to(e.torch_device)
    c300 = torch.tensor([300], dtype=torch.int32, device=e.torch_device)
    m, d = e.match_frames_guided_pose_async(N, rs, ts, RADIUS, (kd, c300), (kx, c300), valid, cross_check=True, max_dist=0.7)
    e.sync()
    _compare(*_host(m, d), pose_frames_rule(desc, xy, counts, [key_train(s, 300)] * N, rs, ts, KVEC, RADIUS, True, 0.7),
             counts, "key count 300")


def test_all_pass_radius_is_bit_identical_to_match_frames(planted):
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    rs, ts = planted_pose(s)
    key, xyz, _ = _clean(s)
    big = _big(s, rs, ts, xy, counts, [_clean(s)] * N)
    for cross, md, ratio in OPTIONS:
        m, d = e.match_frames_guided_pose_async(N, rs, ts, big, key, xyz, cross_check=cross, max_dist=md, ratio=ratio)
        um, ud = e.match_frames_async(N, key=key, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        m, d, um, ud = _host(m, d, um, ud)
        np.testing.assert_array_equal(m, um)
        np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
    # under the gate: wherever the guided and the unguided winner coincide, dist is bit-equal
    m, d = e.match_frames_guided_pose_async(N, rs, ts, RADIUS, key, xyz, cross_check=False)
    um, ud = e.match_frames_async(N, key=key, cross_check=False)
    e.sync()
    m, d, um, ud = _host(m, d, um, ud)
    same = (m == um) & (m >= 0)
    assert same.sum() > 1000 and ((m != um) & (m >= 0)).sum() > 50           # ... and the gate did change winners
    np.testing.assert_array_equal(d.view(np.uint32)[same], ud.view(np.uint32)[same])


def test_strip_and_tile_edges(planted):
    """Device counts 0, 1, 2, 63, 64, 65 against a key of 1, 2 and 65 rows: the strip edge, the tile edge, and Lowe's test
    with fewer than two candidates.  Only the device counts change: rows are in random order, so the first k rows of a
    planted frame are a planted frame."""
    import torch
    e, s = planted
    n = 6
    small = np.array([0, 1, 2, 63, 64, 65])
    desc, xy = s["desc"][:n], s["xy"][:n]
    rs, ts = (v[:n] for v in planted_pose(s))
    _, count = e._results_view()
    count[:n].copy_(torch.from_numpy(small.astype(np.int32)))
    torch.cuda.synchronize()
    try:
        for nkey in (1, 2, 65):
            key, xyz, _ = _clean(s, nkey)
            trains = [_clean(s, nkey)] * n
            big = _big(s, rs, ts, xy, small, trains)
            for cross, md, ratio in OPTIONS:
                args = dict(cross_check=cross, max_dist=md, ratio=ratio)
                m, d = e.match_frames_guided_pose_async(n, rs, ts, RADIUS, key, xyz, **args)
                am, ad = e.match_frames_guided_pose_async(n, rs, ts, big, key, xyz, **args)
                um, ud = e.match_frames_async(n, key=key, **args)
                e.sync()
                m, d, am, ad, um, ud = _host(m, d, am, ad, um, ud)
                label = "nkey %d %s" % (nkey, (cross, md, ratio))
                _compare(m, d, pose_frames_rule(desc, xy, small, trains, rs, ts, KVEC, RADIUS, cross, md, ratio), small, label)
                _compare(am, ad, pose_frames_rule(desc, xy, small, trains, rs, ts, KVEC, big, cross, md, ratio), small, label)
                np.testing.assert_array_equal(am, um)
                np.testing.assert_array_equal(ad.view(np.uint32), ud.view(np.uint32))
                if ratio > 0 and nkey == 1:
                    assert (am == -1).all()                                 # one candidate: the ratio test fails
                if ratio == 0 and md == 0:
                    assert (am[5] >= 0).sum() >= (1 if cross else 65)       # (something was matched)
    finally:
        count[:n].copy_(torch.from_numpy(s["counts"][:n].astype(np.int32)))
        torch.cuda.synchronize()


def test_failed_and_non_finite_poses_and_repeated_calls(planted):
    import torch
    e, s = planted
    rs, ts = planted_pose(s)
    key, xyz, valid = key_train(s, s["K"])                                 # (without the rows behind the cameras, which
    br, bt = rs.copy(), ts.copy()                                          # (-R, -t) would bring to the front)
    br[1], bt[1] = -br[1], -bt[1]                                          # every landmark behind the camera: c < 0
    br[3], bt[3] = 0, 0                                                    # what a failed frame's pose is: c = 0
    br[5, 4] = np.nan
    bt[6, 2] = np.inf
    outs = []
    for _ in range(2):
        m, d = e.match_frames_guided_pose_async(N, torch.from_numpy(br).to(e.torch_device), bt, RADIUS, key, xyz, valid,
                                                cross_check=True, max_dist=0.9)
        e.sync()
        outs.append(_host(m, d.view(torch.int32)))
    m, d = outs[0]
    assert (m[[1, 3, 5, 6]] == -1).all() and (d[[1, 3, 5, 6]].view(np.float32) == np.inf).all()
    assert ((m[[0, 2, 4, 7]] >= 0).sum(axis=1) > 300).all()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])                 # repeated calls: bit-identical
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    gm, gd = e.match_frames_guided_pose_async(N, rs, ts, RADIUS, key, xyz, valid, cross_check=True, max_dist=0.9)
    e.sync()
    gm, gd = _host(gm, gd.view(torch.int32))
    ok = [0, 2, 4, 7]                                                     # the other frames are unaffected
    np.testing.assert_array_equal(m[ok], gm[ok])
    np.testing.assert_array_equal(d[ok], gd[ok])
    # R is used as given: (2 R, 2 t) is the same camera
    sm, sd = e.match_frames_guided_pose_async(N, 2 * rs, 2 * ts, RADIUS, key, xyz, valid, cross_check=True, max_dist=0.9)
    e.sync()
    np.testing.assert_array_equal(_host(sm)[0], gm)


def _pad(a, rows):
    out = np.zeros((rows,) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


@pytest.fixture(scope="module")
def banked(planted):
    e, s = planted
    slots, trains = gpu_bank_trains(s)
    e.bank_create(4)
    for sl, (d, p, _, _) in slots.items():                                # slot 1 stays empty
        e.bank_store_rows(sl, d, p)
    e.sync()
    yield e, s, slots, trains
    assert e.check_guards() == 0
    e.bank_destroy()


def _second_pose_is_the_restatements(tag, s, f, m2, train_xyz, train_ok, r2, t2, n2, mask2, same):
    """The device's second pose from its own pair list against pnp_rule on that list, within the margins of
    tests/test_gpu_pnp_ransac.py: the mask is the float64 test of the returned pose, the planted-truth bars hold, and where
    the device picked the restatement's inlier set the pose is the restatement's to R_SAME_BAR / T_SAME_BAR."""
    cnt = s["counts"][f]
    mask2 = mask2.astype(bool)
    rows = np.flatnonzero((m2[f, :cnt] >= 0) & train_ok[np.maximum(m2[f, :cnt], 0)])
    pxy, pxyz = s["xy"][f, rows].astype(np.float32), train_xyz[m2[f, rows]]
    want = pnp_rule(pxy, pxyz, PNP, f)
    assert not want.failed and r2[f].any(), (tag, f)
    _assert_mask_is_the_reprojection_test(r2[f], t2[f], mask2[f][rows], n2[f], pxy, pxyz)
    assert not np.delete(mask2[f], rows).any()
    cam = s["cams"][1 + f]
    rot, tr = pose_errors(r2[f], t2[f], (None, None, None, cam[0], cam[1]))
    print("  %s frame %d: %d pairs, %d inliers (restatement %d), rotation %.4f deg, translation %.3e"
          % (tag, f, len(rows), n2[f], want.ninliers, rot, tr))
    assert rot <= ROT_BAR and tr <= TRANS_BAR, (tag, f, rot, tr)
    if (mask2[f][rows] == want.mask).all():
        dr = np.abs(r2[f].astype(np.float64) - want.R).max()
        dt = np.linalg.norm(t2[f].astype(np.float64) - want.t) / np.linalg.norm(want.t)
        assert dr <= R_SAME_BAR and dt <= T_SAME_BAR, (tag, f, dr, dt)
        same.append(f)


def _first_inliers_are_matched(tag, s, m3, mask1, r1, t1, train_xyz, train_valid):
    """Radius = reproj_threshold, no cross check: every row the first PnP marked an inlier has a candidate -- its own pair --
    so it has a match; rows with a pair on the gate's borderline aside."""
    for f, cnt in enumerate(s["counts"]):
        _, edge = pose_gate(r1[f].reshape(9), t1[f], KVEC, s["xy"][f, :cnt], train_xyz, train_valid, THR)
        rows = np.flatnonzero(mask1[f, :cnt].astype(bool) & ~edge.any(1))
        assert len(rows) >= 12 and (m3[f, rows] >= 0).all(), (tag, f, len(rows))


def test_bank_variant_and_its_chain(banked):
    import torch
    e, s, slots, trains = banked
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    rs, ts = planted_pose(s)
    slot = torch.tensor(GPU_SLOT_OF, dtype=torch.int32, device=e.torch_device)
    # a bank without a landmark reservation: every row -1 / +inf
    m, d = e.match_bank_guided_pose_async(N, slot, rs, ts, RADIUS)
    e.sync()
    m, d = _host(m, d)
    assert (m == -1).all() and np.isinf(d).all()
    rows = e.bank_info()["rows"]
    assert e.bank_landmarks_reserve() >= 4 * rows * 16
    for sl, (_, _, xyz, valid) in slots.items():
        e.bank_store_landmarks(sl, _pad(xyz, rows), _pad(valid, rows))
    for cross, md, ratio in OPTIONS:
        m, d = e.match_bank_guided_pose_async(N, slot, rs, ts, RADIUS, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        m, d = _host(m, d)
        _compare(m, d, pose_frames_rule(desc, xy, counts, trains, rs, ts, KVEC, RADIUS, cross, md, ratio), counts,
                 "bank %s" % ((cross, md, ratio),))
        assert (m[[3, 6, 7]] == -1).all() and np.isinf(d[[3, 6, 7]]).all()      # a bad or an empty slot: -1 / +inf
    assert (e.match_bank_guided_pose(N, slot, rs, ts, RADIUS)[0][0] >= 0).sum() > 300      # the per-frame host form
    # every pair a candidate: fpc_match_frames with the slot as its key, bit for bit (slot 3 with every landmark valid)
    e.bank_store_rows(3, *slots[3][:2])
    e.bank_store_landmarks(3, _pad(s["clean_xyz"][:400], rows), None)
    clean3 = (s["key"][:400], s["clean_xyz"][:400], None)
    three = torch.full((N,), 3, dtype=torch.int32, device=e.torch_device)
    big = _big(s, rs, ts, xy, counts, [clean3] * N)
    bd, _, bc = e.bank_view()
    m, d = e.match_bank_guided_pose_async(N, three, rs, ts, big, cross_check=True, max_dist=0.7)
    um, ud = e.match_frames_async(N, key=(bd[3].clone(), bc[3:4].clone()), cross_check=True, max_dist=0.7)
    e.sync()
    m, d, um, ud = _host(m, d, um, ud)
    np.testing.assert_array_equal(m, um)
    np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
    assert (m >= 0).sum() > 1000
    # the chain through the bank, no host call in between
    score, best, m1, _ = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    r1, t1, n1, k1 = e.pnp_bank_async(N, best, m1, **PNP)
    m2, _ = e.match_bank_guided_pose_async(N, best, r1, t1, RADIUS, cross_check=True, max_dist=0.7)
    r2, t2, n2, k2 = e.pnp_bank_async(N, best, m2, **PNP)
    m3, _ = e.match_bank_guided_pose_async(N, best, r1, t1, THR, cross_check=False)
    e.sync()
    best, m2, m3, r1, t1, n1, k1, r2, t2, n2, k2 = _host(best, m2, m3, r1, t1, n1, k1, r2, t2, n2, k2)
    print("bank: best", best, "inliers", n1, "->", n2)
    assert (best == 2).all() and (n1 >= 12).all() and (n2 >= n1).all() and n2.sum() > n1.sum()
    same = []
    for f in range(N):
        _second_pose_is_the_restatements("bank", s, f, m2, s["key_xyz"], landmark_ok(s), r2, t2, n2, k2, same)
    assert len(same) >= N // 2, same
    _first_inliers_are_matched("bank", s, m3, k1, r1, t1, s["key_xyz"], s["key_valid"])


def test_full_chain_with_a_key(planted):
    e, s = planted
    key, xyz, valid = key_train(s)
    # four calls, no host call in between
    m1, _ = e.match_frames_async(N, key=key, cross_check=True, max_dist=0.7)
    r1, t1, n1, k1 = e.pnp_frames_async(N, m1, xyz, valid, **PNP)
    m2, _ = e.match_frames_guided_pose_async(N, r1, t1, RADIUS, key, xyz, valid, cross_check=True, max_dist=0.7)
    r2, t2, n2, k2 = e.pnp_frames_async(N, m2, xyz, valid, **PNP)
    m3, _ = e.match_frames_guided_pose_async(N, r1, t1, THR, key, xyz, valid, cross_check=False)
    e.sync()
    m2, m3, r1, t1, n1, k1, r2, t2, n2, k2 = _host(m2, m3, r1, t1, n1, k1, r2, t2, n2, k2)
    print("key: inliers", n1, "->", n2)
    assert (n1 >= 12).all() and (n2 >= n1).all() and n2.sum() > n1.sum()
    same = []
    for f in range(N):
        _second_pose_is_the_restatements("key", s, f, m2, xyz, landmark_ok(s), r2, t2, n2, k2, same)
    assert len(same) >= N // 2, same
    _first_inliers_are_matched("key", s, m3, k1, r1, t1, xyz, valid)


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, s, slots, _ = banked
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, e.capacity), -7.0, dtype=torch.float32, device=dev)
    rs, ts = planted_pose(s)
    rm = torch.from_numpy(np.tile(rs[0], (N + 1, 1))).to(dev)
    tv = torch.from_numpy(np.tile(ts[0], (N + 1, 1))).to(dev)
    key, kc = e._key(s["key"])
    kx = torch.from_numpy(s["key_xyz"]).to(dev)
    kv = torch.from_numpy(s["key_valid"].astype(np.uint8)).to(dev)
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    cam = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)

    def mg(n=N, k=key.data_ptr(), c=kc.data_ptr(), x=kx.data_ptr(), v=kv.data_ptr(), r=rm.data_ptr(), t=tv.data_ptr(),
           rad=3.0, md=0.0, ratio=0.0, out=mt.data_ptr(), **kw):
        q = dict(cam, **kw)
        return lib.fpc_match_frames_guided_pose(ctx, n, k, c, x, v, r, t, q["fx"], q["fy"], q["cx"], q["cy"], rad, 1, md, ratio,
                                                out, ds.data_ptr())

    def bg(n=N, sl=slot.data_ptr(), r=rm.data_ptr(), t=tv.data_ptr(), rad=3.0, md=0.0, ratio=0.0, out=mt.data_ptr(), **kw):
        q = dict(cam, **kw)
        return lib.fpc_match_bank_guided_pose(ctx, n, sl, r, t, q["fx"], q["fy"], q["cx"], q["cy"], rad, 1, md, ratio, out,
                                              ds.data_ptr())
    nan, inf = float("nan"), float("inf")
    for call in (mg, bg):
        # everything fpc_match_frames refuses
        assert call(n=N + 1) == FPC_E_INVALID and call(n=0) == FPC_E_INVALID
        assert call(md=-1.0) == FPC_E_INVALID and call(ratio=1.5) == FPC_E_INVALID and call(ratio=-0.1) == FPC_E_INVALID
        assert call(md=nan) == FPC_E_INVALID
        # ... and the calls' own
        assert call(r=None) == FPC_E_INVALID and call(t=None) == FPC_E_INVALID and call(out=None) == FPC_E_INVALID
        for rad in (0.0, -3.0, inf, nan):
            assert call(rad=rad) == FPC_E_INVALID
        for bad in (dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf)):
            assert call(**bad) == FPC_E_INVALID, bad
    assert mg(k=None) == FPC_E_INVALID and mg(c=None) == FPC_E_INVALID and mg(x=None) == FPC_E_INVALID
    assert mg(k=key.data_ptr() + 4) == FPC_E_INVALID                      # not 16-byte aligned
    assert bg(sl=None) == FPC_E_INVALID
    e.sync()
    assert (mt.cpu().numpy() == -7).all() and (ds.cpu().numpy() == -7.0).all()
    assert mg(v=None) == 0 and bg() == 0                                  # (valid forms of the calls above)
    e.sync()
    assert (mt.cpu().numpy()[:N] != -7).all()
    # a context without a bank; a bf16 bank; results without descriptors
    d = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        out = torch.full((2, d.capacity), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def bank_call():
            return lib.fpc_match_bank_guided_pose(d._ctx, 2, slot.data_ptr(), rm.data_ptr(), tv.data_ptr(), 500.0, 500.0,
                                                  320.0, 240.0, 3.0, 1, 0.0, 0.0, out.data_ptr(), None)

        def untouched():
            d.sync()
            return bool((out.cpu().numpy() == -7).all())
        assert bank_call() == FPC_E_INVALID and untouched()               # no bank: refused, nothing written
        d.bank_create(2, format="bf16")
        d.bank_store_rows(0, s["key"][:64], s["key_xy"][:64])
        d.sync()
        assert bank_call() == FPC_E_INVALID and untouched()               # FPC_BANK_BF16: that format's gate is a follow-up
        with pytest.raises(_lib.FpcError):
            d.match_bank_guided_pose_async(2, slot[:2], rm[:2], tv[:2], 3.0)
        assert untouched()
        d.bank_destroy()
        d.bank_create(2)
        assert bank_call() == 0 and not untouched()                       # (an f32 bank: accepted, and it writes)
        d.bank_destroy()
        out.fill_(-7)
        d.get_points(prob)
        torch.cuda.synchronize()
        assert lib.fpc_match_frames_guided_pose(d._ctx, 2, key.data_ptr(), kc.data_ptr(), kx.data_ptr(), None, rm.data_ptr(),
                                                tv.data_ptr(), 500.0, 500.0, 320.0, 240.0, 3.0, 1, 0.0, 0.0, out.data_ptr(),
                                                None) == FPC_E_INVALID
        assert untouched() and d.check_guards() == 0
    finally:
        d.close()


def test_vgg_descriptors():
    """FPC_ARCH_VGG: D = 256."""
    e = engine(240, 320, in_channels=1, arch="vgg")
    try:
        assert e.desc_dim == 256 and e.capacity == GPU_VGG_SCENE["cap"]
        s = scene_of(GPU_VGG_SCENE)
        plant(e, s)
        desc, xy, counts = s["desc"], s["xy"], s["counts"]
        rs, ts = planted_pose(s)
        key, xyz, valid = key_train(s)
        for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
            m, d = e.match_frames_guided_pose_async(N, rs, ts, RADIUS, key, xyz, valid, cross_check=cross, max_dist=md,
                                                    ratio=ratio)
            e.sync()
            _compare(*_host(m, d), pose_frames_rule(desc, xy, counts, [key_train(s)] * N, rs, ts, KVEC, RADIUS, cross, md, ratio),
                     counts, "vgg %s" % ((cross, md, ratio),))
        ckey, cxyz, _ = _clean(s)
        big = _big(s, rs, ts, xy, counts, [_clean(s)] * N)
        m, d = e.match_frames_guided_pose_async(N, rs, ts, big, ckey, cxyz)
        um, ud = e.match_frames_async(N, key=ckey)
        e.sync()
        m, d, um, ud = _host(m, d, um, ud)
        np.testing.assert_array_equal(m, um)
        np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
        assert (m >= 0).sum() > 500
        assert e.check_guards() == 0
    finally:
        e.close()
