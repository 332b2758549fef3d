"""RANSAC PnP on the GPU (fpc_ransac_pnp / fpc_pnp_frames / fpc_pnp_bank and the bank's landmark calls) against the float64
restatement and the planted scenes of tests/test_pnp_ransac.py: planted poses with outliers, the tails of the pair list, the
frames variant bit-identical to explicit pairs and the bank variant to the frames variant, the landmark storage and its
invalidation, a three-view chain end to end (two views give the landmarks at the scale |baseline| = 1, the third view's pose
comes back at that scale), determinism and the argument checks.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_gpu_homography_ransac import engine
from tests.test_pnp_ransac import (CASE_SETS, FRAME_H, FRAME_W, KVEC, PARAMS, ROT_BAR, TRANS_BAR, _rotation, camera_points,
                                   check_planted_pose, inliers_of, planted_scene, pnp_rule, pose_errors, reprojection_error,
                                   restated_batch)

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
THR = PARAMS["reproj_threshold"]
KQVGA = (250.0, 250.0, 160.0, 120.0)
# Device against restatement where both picked the same best sample (identical masks): both evaluate the polar step and the
# refits in fp64 and differ by the contraction of a * b + c into one rounding, so what is left is the fp32 rounding of the
# outputs.  Measured on the MI355X over the 22 frames of the three case sets (all 22 with the restatement's mask): worst
# difference 0.0 in every entry of R and of t -- the same fp32 values.  Ten times zero is no bar, so the bars are the
# resolution of the outputs' fp32 format, rounded up as test_gpu_pose_epipolar.py's R_BAR is: entries of R are <= 1
# (resolution 6e-8), and |dt| / |t| resolves 1.2e-7.
R_SAME_BAR, T_SAME_BAR = 1e-6, 1e-6                                  # per entry of R; |dt| / |t|


def _reserved(e):
    assert e.pnp_reserve() > 0
    return e


@pytest.fixture(scope="module")
def vga():
    """A 32-frame VGA context without the descriptor head (explicit pairs need no network); max_keypoints = 1280 so that a
    pair list can cross the 1 024-record LDS chunk."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = _reserved(engine(FRAME_H, FRAME_W, 32, descriptor_enabled=False, max_keypoints=1280))
    assert e.capacity >= 1100
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


@pytest.fixture(scope="module")
def qvga():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = _reserved(engine(conf_thresh=0.001))
    e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(300, N, H, W))
    assert min(len(r[0]) for r in res) > 1000
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _pack(lists, stride):
    """[(xy [m,2], xyz [m,3])] -> the call's inputs (xy float32 [n,stride,2], xyz float32 [n,stride,3], npairs int32 [n])."""
    xy, xyz = np.zeros((len(lists), stride, 2), np.float32), np.zeros((len(lists), stride, 3), np.float32)
    for f, (a, b) in enumerate(lists):
        xy[f, :len(a)], xyz[f, :len(b)] = a, b
    return xy, xyz, np.array([len(a) for a, _ in lists], np.int32)


def _assert_mask_is_the_reprojection_test(rm, tv, mask, ni, xy, xyz, kvec=KVEC, thr=THR):
    """mask / ninliers are the float64 test of the RETURNED pose (off the threshold's 1e-3 px neighbourhood), and nothing is
    set past the frame's pair count."""
    m = len(xy)
    assert ni == mask.sum() and not mask[m:].any()
    r64, t64 = rm.astype(np.float64), tv.astype(np.float64)
    clear = np.abs(reprojection_error(r64, t64, xy, xyz, kvec) - thr) > 1e-3
    np.testing.assert_array_equal(mask[:m][clear], inliers_of(r64, t64, xy, xyz, kvec, thr)[clear])


_DEVICE = {}


def _device_batch(e, rho, iterations):
    """The device's poses of one case set, computed once."""
    if (rho, iterations) not in _DEVICE:
        scenes, _ = restated_batch(rho, iterations)
        xy, xyz, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
        assert len(set(npairs.tolist())) > 1
        _DEVICE[rho, iterations] = e.ransac_pnp(xy, xyz, npairs, iterations=iterations, **PARAMS)
    return _DEVICE[rho, iterations]


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_device_against_the_restatement(vga, rho, iterations):
    scenes, results = restated_batch(rho, iterations)
    rm, tv, ni, mask = _device_batch(vga, rho, iterations)
    worst, same = np.zeros(2), 0
    for f, (scene, want) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not want.failed and rm[f].any(), (rho, f)
        check_planted_pose(rm[f], tv[f], mask[f, :m], scene, (rho, f, m))            # a different best sample may be picked
        _assert_mask_is_the_reprojection_test(rm[f], tv[f], mask[f], ni[f], scene[0], scene[1])
        # the count: the restatement's, give or take the pairs within 1e-3 px of the threshold
        assert abs(int(ni[f]) - want.ninliers) <= want.near.sum(), (rho, f, ni[f], want.ninliers, want.near.sum())
        if (mask[f, :m] == want.mask).all():                                         # the same sample: the same pose
            same += 1
            dr = np.abs(rm[f].astype(np.float64) - want.R).max()
            dt = np.linalg.norm(tv[f].astype(np.float64) - want.t) / np.linalg.norm(want.t)
            worst = np.maximum(worst, (dr, dt))
            assert dr <= R_SAME_BAR and dt <= T_SAME_BAR, (rho, f, dr, dt)
        print("rho %.1f frame %2d M %4d: %d inliers (restatement %d), rotation %.4f deg, translation %.3e"
              % (rho, f, m, ni[f], want.ninliers, *pose_errors(rm[f], tv[f], scene)))
    assert same >= len(scenes) // 2
    print("rho %.1f: %d of %d frames with the restatement's mask; worst difference there: R %.3e, t %.3e relative"
          % (rho, same, len(scenes), *worst))


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_device_meets_the_planted_truth_bars(vga, rho, iterations):
    scenes, _ = restated_batch(rho, iterations)
    rm, tv, ni, mask = _device_batch(vga, rho, iterations)
    for f, scene in enumerate(scenes):
        m = len(scene[0])
        rot, tr = check_planted_pose(rm[f], tv[f], mask[f, :m], scene, (rho, f, m))
        assert rot <= ROT_BAR and tr <= TRANS_BAR
        assert ni[f] >= PARAMS["min_inliers"] and not mask[f, m:].any()


def _raw_pnp(e, xy, xyz, npairs, mask=True, fill=0xFF, **params):
    """fpc_ransac_pnp into outputs pre-filled with `fill` bytes -> host arrays (R, t, ninliers, mask uint8)."""
    import torch
    dev = e.torch_device
    n, stride = xy.shape[0], xy.shape[1]
    p = e._pnp_params(None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (xy, xyz, npairs)]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev) for shape in ((n, 36), (n, 12), (n, 4), (n, stride))]
    torch.cuda.synchronize()
    e._call("fpc_ransac_pnp", n, ins[0], ins[1], ins[2], stride, ctypes.byref(p), outs[0], outs[1], outs[2],
            outs[3] if mask else None, inputs=ins)
    e.sync()
    rm, tv, ni, mk = (o.cpu().numpy() for o in outs)
    return rm.view(np.float32).reshape(n, 3, 3), tv.view(np.float32).reshape(n, 3), ni.view(np.int32).reshape(n), mk


def test_tails_of_the_pair_list(vga):
    e = vga
    cap = e.capacity
    xy, xyz, _, r, t = planted_scene(4, 0.0, cap)
    same = (np.repeat(xy[:1], 50, 0), np.repeat(xyz[:1], 50, 0))
    sizes = [1100, 0, 5, 6, 7, 256, 257, 1024, 1025, cap, 100]
    lists = [(xy[:m], xyz[:m]) for m in sizes] + [same]
    a, b, npairs = _pack(lists, cap)
    npairs[9] = cap + 9                                                              # above the stride: clamped
    params = dict(PARAMS, iterations=256)
    rm, tv, ni, mask = _raw_pnp(e, a, b, npairs, **params)
    assert set(np.unique(mask).tolist()) <= {0, 1}                                   # no 0xFF left: every row was written
    assert np.isfinite(rm).all() and np.isfinite(tv).all()
    for f in (1, 2, 11):                                                             # too few pairs / every sample degenerate
        assert not rm[f].any() and not tv[f].any() and ni[f] == 0 and not mask[f].any(), f
    for f, m in enumerate(sizes):
        want = pnp_rule(lists[f][0], lists[f][1], params, f)
        if want.failed:                                                              # (six or seven rounded pixels may fail)
            assert f in (1, 2, 3, 4), f
        if f in (1, 2) or (want.failed and not rm[f].any()):
            assert not rm[f].any() and not tv[f].any() and ni[f] == 0 and not mask[f].any(), f
            continue
        assert not mask[f, m:].any(), f                                              # rows past the count: 0
        _assert_mask_is_the_reprojection_test(rm[f], tv[f], mask[f].astype(bool), ni[f], lists[f][0], lists[f][1])
        if m >= 100:
            assert ni[f] >= 0.98 * m, (f, ni[f])
            rot, tr = pose_errors(rm[f], tv[f], (None, None, None, r, t))
            assert rot <= ROT_BAR and tr <= TRANS_BAR, (f, rot, tr)
            assert abs(int(ni[f]) - want.ninliers) <= want.near.sum(), f
    assert mask[0, 1024:1100].sum() >= 0.98 * 76                                     # the pairs behind the first chunk count
    assert mask[9, cap - 1] == 1 and ni[9] >= 0.98 * cap
    # a failed frame between two good ones: zeros, and its neighbours are what they are alone
    alone = _raw_pnp(e, a[[0]], b[[0]], npairs[[0]], **params)                       # n = 1
    np.testing.assert_array_equal(alone[0][0].view(np.uint32), rm[0].view(np.uint32))
    np.testing.assert_array_equal(alone[1][0].view(np.uint32), tv[0].view(np.uint32))
    np.testing.assert_array_equal(alone[3][0], mask[0])
    assert rm[0].any() and not rm[1].any() and not rm[2].any() and rm[5].any()
    # n = max_batch: every frame index draws its own samples, all recover the pose
    full = e.ransac_pnp(np.repeat(a[[10]], 32, 0), np.repeat(b[[10]], 32, 0), np.repeat(npairs[[10]], 32), **params)
    assert (full[2] >= 98).all() and len({full[0][f].tobytes() for f in range(32)}) > 1
    for f in range(32):
        rot, tr = pose_errors(full[0][f], full[1][f], (None, None, None, r, t))
        assert rot <= ROT_BAR and tr <= TRANS_BAR, (f, rot, tr)
    # min_inliers above what one frame can reach fails that frame only; T = 1 and T = 65 (a partial last workgroup)
    fm2 = _raw_pnp(e, a, b, npairs, **dict(params, min_inliers=101))
    assert not fm2[0][10].any() and not fm2[1][10].any() and fm2[2][10] == 0 and not fm2[3][10].any()
    np.testing.assert_array_equal(fm2[0][[0, 9]].view(np.uint32), rm[[0, 9]].view(np.uint32))
    one = _raw_pnp(e, a, b, npairs, **dict(params, iterations=1))
    assert one[2][10] == one[3][10].sum()
    more = _raw_pnp(e, a, b, npairs, **dict(params, iterations=65))
    assert more[2][10] >= 98 and more[2][0] >= 0.98 * 1100
    # refits = 0: the best sample's polar pose, a rotation all the same
    bare0 = _raw_pnp(e, a, b, npairs, **dict(params, refits=0))
    want0 = pnp_rule(lists[10][0], lists[10][1], dict(params, refits=0), 10)
    assert not want0.failed and np.abs(bare0[0][10].astype(np.float64) - want0.polar[0]).max() <= R_SAME_BAR
    assert np.linalg.norm(bare0[1][10].astype(np.float64) - want0.polar[1]) <= T_SAME_BAR * np.linalg.norm(want0.polar[1])
    assert abs(np.linalg.det(bare0[0][10].astype(np.float64)) - 1.0) < 1e-6 and bare0[2][10] == bare0[3][10].sum()
    # a NULL mask: R, t and the count are what they were
    bare = _raw_pnp(e, a, b, npairs, mask=False, **params)
    np.testing.assert_array_equal(bare[0].view(np.uint32), rm.view(np.uint32))
    np.testing.assert_array_equal(bare[2], ni)
    assert (bare[3] == 0xFF).all()
    # landmarks behind the camera are never inliers
    behind = ((-camera_points(r, t, xyz[:10]) - t) @ r).astype(np.float32)
    c, d, npq = _pack([(np.concatenate([xy[:100], xy[:10]]), np.concatenate([xyz[:100], behind]))], cap)
    got = e.ransac_pnp(c, d, npq, **params)
    assert got[2][0] >= 98 and not got[3][0, 100:].any()


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_determinism_and_seeds(vga):
    e = vga
    rho, iterations = CASE_SETS[1]
    scenes, _ = restated_batch(rho, iterations)
    first = _device_batch(e, rho, iterations)
    xy, xyz, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
    again = e.ransac_pnp(xy, xyz, npairs, iterations=iterations, **PARAMS)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # another seed picks other samples and still meets the planted bars on every frame (seed 3: like the case set's scene
    # seeds, one under which the restatement passes all six frames -- seeds 12345, 1 and 2 leave a 40-pair frame without a
    # best sample whose polar pose starts the refits, tests/test_pnp_ransac.py on CASE_M)
    other = e.ransac_pnp(xy, xyz, npairs, iterations=iterations, **dict(PARAMS, seed=3))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(other[0], first[0]))
    for f, scene in enumerate(scenes):
        m = len(scene[0])
        check_planted_pose(other[0][f], other[1][f], other[3][f, :m], scene, ("seed", f, m))


# ---- frames, bank, landmarks: a planted world seen by the frames of a QVGA context ----------------------------------------
def _world(nkey=700, seed=3):
    """A key frame's landmarks (in its camera frame) and N views of them -> (key_xyz float32 [nkey,3] with three rows that are
    not finite, key_valid bool [nkey], the finite key_xyz, [(xy int32 [k,2], match int32 [k], R, t)] per view).  A tenth of
    the landmarks is invalid; a fifth of a view's matches is wrong, some rows have no match, some a match outside the key's
    rows."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KQVGA
    px = np.stack([rng.uniform(20, W - 20, nkey), rng.uniform(20, H - 20, nkey)], 1)
    z = rng.uniform(4.0, 12.0, nkey)
    key_xyz = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    valid = rng.uniform(size=nkey) > 0.1
    views = []
    for f in range(N):
        r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(1.0, 6.0)))
        t = rng.normal(size=3) * 0.4
        xc = camera_points(r, t, key_xyz)
        pix = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)).astype(np.int32)
        seen = np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < W) & (pix[:, 1] >= 0) & (pix[:, 1] < H))
        rows = rng.permutation(seen)[:600 - 40 * f]                                 # the landmark each query row shows
        xy = pix[rows]
        match = rows.astype(np.int32)
        wrong = rng.choice(len(rows), len(rows) // 5, replace=False)                # a fifth of the matches are wrong
        match[wrong] = rng.integers(0, nkey, len(wrong))
        match[rng.choice(len(rows), 20, replace=False)] = -1                        # no match
        match[rng.choice(len(rows), 5, replace=False)] = nkey + 3                   # beyond the key's rows
        views.append((xy, match, r, t))
    bad = key_xyz.copy()
    bad[5, 1], bad[17, 0], bad[40, 2] = np.nan, np.inf, -np.inf                       # not finite: invalid whatever `valid` says
    valid[[5, 17]] = True
    return bad, valid, key_xyz, views


def _plant_views(e, views):
    """The views' pixels and counts in place of the last detect's results -> the match table (device, int32 [N,cap])."""
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


def _host_lists(views, key_xyz, valid, nkey, cap):
    """The frames variant's pair lists, gathered on the host: rows i < count with 0 <= match < nkey and a valid, finite
    landmark, ascending."""
    xy, xyz = np.zeros((N, cap, 2), np.float32), np.zeros((N, cap, 3), np.float32)
    npairs, rows = np.zeros(N, np.int32), []
    ok = valid & np.isfinite(key_xyz).all(1)
    for f, (pix, match, _, _) in enumerate(views):
        inside = (match >= 0) & (match < nkey)
        i = np.flatnonzero(inside & ok[np.where(inside, match, 0)])
        xy[f, :len(i)], xyz[f, :len(i)] = pix[i], key_xyz[match[i]]
        npairs[f] = len(i)
        rows.append(i)
    return xy, xyz, npairs, rows


def test_frames_and_bank_variants_are_bit_identical_to_explicit_pairs(qvga):
    import torch
    e = qvga
    cap, dev = e.capacity, e.torch_device
    key_xyz, valid, clean, views = _world()
    nkey = len(key_xyz)
    match = _plant_views(e, views)
    params = dict(K=KQVGA, iterations=256, seed=11, reproj_threshold=3.0, min_inliers=12)
    try:
        got = e.pnp_frames(N, match, key_xyz, valid, **params)
        xy, xyz, npairs, rows = _host_lists(views, key_xyz, valid, nkey, cap)
        assert npairs.min() > 150
        rm, tv, ni, mask = e.ransac_pnp(xy, xyz, npairs, **params)
        _bits(got[0], rm)
        _bits(got[1], tv)
        np.testing.assert_array_equal(got[2], ni)
        for f in range(N):
            back = np.zeros(cap, bool)
            back[rows[f]] = mask[f, :npairs[f]]
            np.testing.assert_array_equal(got[3][f], back)                           # invalid landmarks are not pairs
            rot, tr = pose_errors(got[0][f], got[1][f], (None, None, None, views[f][2], views[f][3]))
            assert ni[f] >= 0.7 * npairs[f] and rot <= 0.5, (f, ni[f], npairs[f], rot, tr)
        # valid = None: every finite row counts
        every = e.pnp_frames(N, match, key_xyz, None, **params)
        xy2, xyz2, npairs2, _ = _host_lists(views, key_xyz, np.ones(nkey, bool), nkey, cap)
        ref2 = e.ransac_pnp(xy2, xyz2, npairs2, **params)
        assert (npairs2 > npairs).all()
        _bits(every[0], ref2[0])
        _bits(every[1], ref2[1])
        # a key count below the rows: matches beyond it are no pairs
        kx = torch.from_numpy(key_xyz).to(dev)
        few = e.pnp_frames(N, match, (kx, torch.tensor([300], dtype=torch.int32, device=dev)), valid, **params)
        xy3, xyz3, npairs3, _ = _host_lists(views, key_xyz[:300], valid[:300], 300, cap)
        ref3 = e.ransac_pnp(xy3, xyz3, npairs3, **params)
        _bits(few[0], ref3[0])
        np.testing.assert_array_equal(few[2], ref3[2])
        # the bank: slot s holds the key's rows (any descriptors) and its landmarks
        slots = 3
        e.bank_create(slots, cap)
        try:
            assert e.bank_landmarks_reserve() >= slots * cap * 16
            desc = np.random.default_rng(1).normal(size=(nkey, e.desc_dim)).astype(np.float32)
            kxy = np.zeros((nkey, 2), np.int32)
            for s, k in ((0, nkey), (1, nkey), (2, 300)):
                e.bank_store_rows(s, desc[:k], kxy[:k])
            full_xyz, full_valid = np.zeros((cap, 3), np.float32), np.zeros(cap, bool)
            full_xyz[:nkey], full_valid[:nkey] = key_xyz, valid
            full_xyz[nkey:], full_valid[nkey:] = 1.0, True                          # behind the count: invalid all the same
            e.bank_store_landmarks(0, full_xyz, full_valid)
            e.bank_store_landmarks(1, full_xyz, None)
            e.bank_store_landmarks(2, full_xyz, full_valid)
            lm = e.bank_landmarks()
            e.sync()
            h = lm.cpu().numpy()
            fin = np.isfinite(key_xyz).all(1)
            np.testing.assert_array_equal(h[0, :nkey, 3], (valid & fin).astype(np.float32))
            np.testing.assert_array_equal(h[1, :nkey, 3], fin.astype(np.float32))         # without `valid`
            np.testing.assert_array_equal(h[2, :300, 3], (valid & fin)[:300].astype(np.float32))
            assert not h[0, nkey:].any() and not h[2, 300:].any()                    # rows behind the count: four zeros
            np.testing.assert_array_equal(h[0, :nkey, :3][fin].view(np.uint32), key_xyz[fin].view(np.uint32))
            slot = torch.tensor([0, 1, 2, -1, slots, 0, 1, 2], dtype=torch.int32, device=dev)
            bank = e.pnp_bank(N, slot, match, **params)
            for v in bank:
                assert not v[[3, 4]].any()                                           # no slot: the frame fails with zeros
            for rows_of, ref in (([0, 5], got), ([1, 6], every), ([2, 7], few)):
                for a, b in zip(bank, ref):
                    np.testing.assert_array_equal(a[rows_of].view(np.uint8), b[rows_of].view(np.uint8))
            # ... and against fpc_pnp_frames with the slot's own storage as the key
            _, _, bc = e.bank_view()
            for s in range(slots):
                ref = e.pnp_frames(N, match, (lm[s, :, :3].contiguous(), bc[s:s + 1].clone()), lm[s, :, 3] != 0, **params)
                rows_of = np.flatnonzero(slot.cpu().numpy() == s)
                for a, b in zip(bank, ref):
                    np.testing.assert_array_equal(a[rows_of].view(np.uint8), b[rows_of].view(np.uint8))
            # whatever rewrites or empties a slot invalidates its landmarks; the other slots keep theirs
            e.bank_store_rows(1, desc[:50], kxy[:50])
            e.sync()
            h = lm.cpu().numpy()
            assert not h[1].any() and h[0, :nkey, 3].sum() == (valid & fin).sum()
            e.bank_store(0, 2)                                                       # frame 0 of the last detect into slot 2
            e.sync()
            h = lm.cpu().numpy()
            assert not h[2].any() and h[0, :nkey, 3].any()
            gone = e.pnp_bank(N, slot, match, **params)
            assert not gone[0][[1, 2, 6, 7]].any() and not gone[2][[1, 2, 6, 7]].any()
            _bits(gone[0][[0, 5]], bank[0][[0, 5]])
            e.bank_clear(0)
            e.sync()
            assert not lm.cpu().numpy()[0].any()
            e.bank_store_rows(0, desc, kxy)
            e.bank_store_landmarks(0, full_xyz, full_valid)
            e.bank_clear()                                                           # every slot
            e.sync()
            assert not lm.cpu().numpy().any()
            assert e.check_guards() == 0
        finally:
            e.bank_destroy()
        # a bank without landmark storage leaves every frame without pairs
        e.bank_create(slots, cap)
        try:
            e.bank_store_rows(0, desc, kxy)
            none = e.pnp_bank(N, torch.zeros(N, dtype=torch.int32, device=dev), match, **params)
            for v in none:
                assert not v.any()
        finally:
            e.bank_destroy()
    finally:
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_bank_without_landmarks_is_what_it_was(qvga):
    """The same stores and clears with and without a landmark reservation leave the same bank (fpc_bank_get's contents)."""
    import torch
    e = qvga
    cap = e.capacity
    rng = np.random.default_rng(9)
    desc = rng.normal(size=(500, e.desc_dim)).astype(np.float32)
    kxy = rng.integers(0, 200, (500, 2)).astype(np.int32)

    def run(reserve):
        e.bank_create(3, cap)
        try:
            if reserve:
                e.bank_landmarks_reserve()
            e.bank_store(2, 0)
            e.bank_store_rows(1, desc, kxy)
            e.bank_store_rows(2, desc[:100], kxy[:100])
            e.bank_clear(2)
            e.bank_store(5, 2)
            info = e.bank_info()
            e.sync()
            return [t.cpu().numpy().copy() for t in e.bank_view()], info
        finally:
            e.bank_destroy()
    plain, info0 = run(False)
    with_lm, info1 = run(True)
    assert info0 == info1                                                            # fpc_bank_get().bytes included
    for a, b in zip(plain, with_lm):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert plain[2][1] == 500 and plain[2][2] > 1000
    torch.cuda.synchronize()


def test_three_views_end_to_end_recover_the_scale():
    """Two planted views of one 3-D scene give the landmarks, a third view's pose comes back at their scale -- on the device
    without a host call in between: fpc_bank_store_rows (view A), fpc_fundamental_bank and fpc_pose_bank (view B against A:
    R, the direction of t, and one point per row of B at the scale |baseline| = 1), fpc_bank_store + fpc_bank_store_landmarks
    (B becomes a key frame with landmarks), fpc_pnp_bank (view C against B).  C's translation in units of the A-B baseline,
    multiplied by the planted baseline, is the planted translation: the scale two views could not give.  (What is left of
    the error is the two-view pose's: its translation direction sets the scale of the landmarks.  The baseline is a third of
    the mean depth so that 480 rounded pairs pin it.)"""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = _reserved(engine(FRAME_H, FRAME_W, 2, max_keypoints=1024))
    try:
        cap, dev = e.capacity, e.torch_device
        rng = np.random.default_rng(21)
        fx, fy, cx, cy = KVEC
        npts = 900
        # the scene in B's camera frame (the query of the pose call), seen by A and C
        px = np.stack([rng.uniform(60, FRAME_W - 60, npts), rng.uniform(60, FRAME_H - 60, npts)], 1)
        z = rng.uniform(4.0, 12.0, npts)
        xb = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1)
        r_ab, t_ab = _rotation([0.2, 1.0, 0.1], np.deg2rad(8.0)), np.array([3.2, 0.5, 0.6])        # X_A = R X_B + t
        r_cb, t_cb = _rotation([1.0, -0.4, 0.3], np.deg2rad(6.0)), np.array([-0.9, 0.5, 0.7])      # X_C = R X_B + t
        baseline = np.linalg.norm(t_ab)

        def project(r, t):
            xc = camera_points(r, t, xb)
            pix = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)).astype(np.int32)
            return pix, (pix[:, 0] >= 0) & (pix[:, 0] < FRAME_W) & (pix[:, 1] >= 0) & (pix[:, 1] < FRAME_H)
        pa, in_a = project(r_ab, t_ab)
        pb, _ = project(np.eye(3), np.zeros(3))
        pc, in_c = project(r_cb, t_cb)
        # keypoints and descriptors of a detect-like call, then the planted rows in their place (as test_gpu_match_guided's)
        prob = torch.zeros((2, FRAME_H, FRAME_W))
        prob[:, 40, 40] = 0.5
        e.get_points(prob, torch.ones((2, e.desc_dim, FRAME_H // 8, FRAME_W // 8)))
        xy, count = e._points_view()
        desc = rng.normal(size=(npts, e.desc_dim)).astype(np.float32)

        def plant(pix, n):
            hx = np.zeros((2, cap, 2), np.int32)
            hx[0, :n] = pix[:n]
            xy[:2].copy_(torch.from_numpy(hx))
            count[:2].copy_(torch.tensor([n, 0], dtype=torch.int32))
        # A's rows are a permutation of the scene points it sees; B's and C's rows likewise
        rows_a = rng.permutation(np.flatnonzero(in_a))[:cap]
        rows_b = rng.permutation(npts)[:800]
        rows_c = rng.permutation(np.flatnonzero(in_c))[:700]
        where_a = np.full(npts, -1, np.int32)
        where_a[rows_a] = np.arange(len(rows_a))
        where_b = np.full(npts, -1, np.int32)
        where_b[rows_b] = np.arange(len(rows_b))
        m_ba = np.full((2, cap), -1, np.int32)
        m_ba[0, :len(rows_b)] = where_a[rows_b]                                       # B's row -> A's row (fpc_match's table)
        m_cb = np.full((2, cap), -1, np.int32)
        m_cb[0, :len(rows_c)] = where_b[rows_c]
        wrong = rng.choice(len(rows_c), 100, replace=False)                          # wrong matches among C's
        m_cb[0, wrong] = rng.integers(0, len(rows_b), 100)
        m_ba_dev, m_cb_dev = torch.from_numpy(m_ba).to(dev), torch.from_numpy(m_cb).to(dev)
        slot_a = torch.tensor([0, -1], dtype=torch.int32, device=dev)
        slot_b = torch.tensor([1, -1], dtype=torch.int32, device=dev)
        e.bank_create(2, cap)
        e.bank_landmarks_reserve()
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the pose of C is read
        e.bank_store_rows(0, desc[rows_a], pa[rows_a])
        plant(pb[rows_b], len(rows_b))
        fm, _, _ = e.fundamental_bank_async(2, slot_a, m_ba_dev, iterations=512, reproj_threshold=2.0, seed=5)
        r1, t1, nf, pts, front = e.pose_bank_async(2, slot_a, m_ba_dev, fm, K_query=KVEC, K_train=KVEC, reproj_threshold=2.0)
        e.bank_store(0, 1)                                                           # B becomes slot 1 ...
        e.bank_store_landmarks(1, pts[0], front[0])                                  # ... with its triangulated rows
        plant(pc[rows_c], len(rows_c))
        rm, tv, ni, mask = e.pnp_bank_async(2, slot_b, m_cb_dev, K=KVEC, iterations=1024, seed=3)
        out = e._host((r1, t1, nf, rm, tv, ni, mask))
        r1, t1, nf, rm, tv, ni, mask = out
        assert nf[0] >= 0.9 * (where_a[rows_b] >= 0).sum()
        assert abs(np.linalg.norm(t1[0]) - 1.0) < 1e-6
        right = np.ones(len(rows_c), bool)
        right[wrong] = False
        j = where_b[rows_c]
        right &= (j >= 0) & (where_a[rows_b][np.maximum(j, 0)] >= 0)                 # a right match to a row with a landmark
        assert ni[0] >= 0.75 * right.sum() and ni[1] == 0 and not rm[1].any(), (ni, right.sum())
        scene = (None, None, None, r_cb, t_cb)
        rot, tr = pose_errors(rm[0], tv[0].astype(np.float64) * baseline, scene)
        print("third view: rotation %.4f deg, translation %.3e relative (after the rescale by the planted baseline %.4f); "
              "|t| before the rescale %.4f, planted %.4f" % (rot, tr, baseline, np.linalg.norm(tv[0]), np.linalg.norm(t_cb)))
        assert rot <= ROT_BAR and tr <= TRANS_BAR, (rot, tr)
        assert not mask[0, wrong][m_cb[0, wrong] != where_b[rows_c][wrong]].sum() > 5
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused(qvga):
    import torch
    e = qvga
    lib = _lib.load()
    cap, dev = e.capacity, e.torch_device
    xy = torch.zeros((N, cap, 2), dtype=torch.float32, device=dev)
    xyz = torch.zeros((N, cap, 3), dtype=torch.float32, device=dev)
    npairs = torch.full((N,), 10, dtype=torch.int32, device=dev)
    match = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    slot = torch.zeros((N,), dtype=torch.int32, device=dev)
    one = torch.ones((1,), dtype=torch.int32, device=dev)
    valid = torch.ones((cap,), dtype=torch.uint8, device=dev)
    rm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    tv = torch.full((N, 3), 7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N,), 7, dtype=torch.int32, device=dev)
    mask = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    xp, zp, np_, mp, lp, op, vp = (t.data_ptr() for t in (xy, xyz, npairs, match, slot, one, valid))
    rp, tp, ip, bp = (t.data_ptr() for t in (rm, tv, ni, mask))
    kz = xyz[0].data_ptr()

    def params(**kw):
        p = _lib.FpcPnpParams()
        lib.fpc_default_pnp_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rp_ = lambda n, a, b, c, stride, p, r, t, i: lib.fpc_ransac_pnp(e._ctx, n, a, b, c, stride, p, r, t, i, bp)   # noqa: E731
    ff = lambda n, k, v, kc, m, p, r, t, i: lib.fpc_pnp_frames(e._ctx, n, k, v, kc, m, p, r, t, i, bp)           # noqa: E731
    fb = lambda n, s, m, p, r, t, i: lib.fpc_pnp_bank(e._ctx, n, s, m, p, r, t, i, bp)                           # noqa: E731
    ok = params()
    nbytes = ctypes.c_size_t(0)
    ptr = ctypes.c_void_p()
    assert lib.fpc_pnp_reserve(e._ctx, ctypes.byref(nbytes)) == FPC_E_INVALID        # a reservation exists
    assert lib.fpc_bank_landmarks_reserve(e._ctx, ctypes.byref(nbytes)) == FPC_E_INVALID     # no bank
    assert lib.fpc_bank_store_landmarks(e._ctx, 0, kz, vp) == FPC_E_INVALID
    assert lib.fpc_bank_landmarks_get(e._ctx, ctypes.byref(ptr)) == FPC_E_INVALID
    assert fb(N, lp, mp, ok, rp, tp, ip) == FPC_E_INVALID                            # no bank
    e.bank_create(2, cap)
    try:
        assert lib.fpc_bank_store_landmarks(e._ctx, 0, kz, vp) == FPC_E_INVALID      # no landmark reservation
        assert lib.fpc_bank_landmarks_get(e._ctx, ctypes.byref(ptr)) == FPC_E_INVALID
        assert lib.fpc_bank_landmarks_reserve(e._ctx, None) == 0
        assert lib.fpc_bank_landmarks_reserve(e._ctx, ctypes.byref(nbytes)) == FPC_E_INVALID     # a reservation exists
        assert lib.fpc_bank_store_landmarks(e._ctx, -1, kz, vp) == FPC_E_INVALID
        assert lib.fpc_bank_store_landmarks(e._ctx, 2, kz, vp) == FPC_E_INVALID
        assert lib.fpc_bank_store_landmarks(e._ctx, 0, None, vp) == FPC_E_INVALID
        assert lib.fpc_bank_landmarks_get(e._ctx, None) == FPC_E_INVALID
        assert lib.fpc_bank_store_landmarks(e._ctx, 0, kz, None) == 0
        assert lib.fpc_bank_landmarks_get(e._ctx, ctypes.byref(ptr)) == 0 and ptr.value
        nan, inf = float("nan"), float("inf")
        bad = [params(fx=0.0), params(fy=-1.0), params(fx=nan), params(fy=inf), params(cx=nan), params(cy=-inf),
               params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
               params(reproj_threshold=nan), params(refits=-1), params(refits=5), params(min_inliers=5), None]
        for p in bad:
            assert rp_(N, xp, zp, np_, cap, p, rp, tp, ip) == FPC_E_INVALID
            assert ff(N, kz, vp, op, mp, p, rp, tp, ip) == FPC_E_INVALID
            assert fb(N, lp, mp, p, rp, tp, ip) == FPC_E_INVALID
        for k in range(8):                                                           # a NULL in any pointer but the mask
            if k == 3:
                continue
            a = [xp, zp, np_, cap, ok, rp, tp, ip]
            a[k] = None
            assert rp_(N, *a) == FPC_E_INVALID, k
        assert rp_(0, xp, zp, np_, cap, ok, rp, tp, ip) == FPC_E_INVALID
        assert rp_(N + 1, xp, zp, np_, cap, ok, rp, tp, ip) == FPC_E_INVALID         # above max_batch
        assert rp_(N, xp, zp, np_, cap + 1, ok, rp, tp, ip) == FPC_E_INVALID         # stride above capacity
        assert rp_(N, xp, zp, np_, 0, ok, rp, tp, ip) == FPC_E_INVALID
        for k in range(8):                                                           # key_valid (1) may be NULL
            if k == 1:
                continue
            a = [kz, vp, op, mp, ok, rp, tp, ip]
            a[k] = None
            assert ff(N, *a) == FPC_E_INVALID, k
        assert ff(0, kz, vp, op, mp, ok, rp, tp, ip) == FPC_E_INVALID
        assert ff(N + 1, kz, vp, op, mp, ok, rp, tp, ip) == FPC_E_INVALID
        for k in range(6):
            a = [lp, mp, ok, rp, tp, ip]
            a[k] = None
            assert fb(N, *a) == FPC_E_INVALID, k
        assert fb(0, lp, mp, ok, rp, tp, ip) == FPC_E_INVALID
        assert fb(N + 1, lp, mp, ok, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert ff(3, kz, vp, op, mp, ok, rp, tp, ip) == FPC_E_INVALID
        assert fb(3, lp, mp, ok, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        for t in (rm, tv):
            assert (t.cpu() == 7.0).all()
        assert (ni.cpu() == 7).all() and (mask.cpu() == 7).all()
        assert ff(2, kz, None, op, mp, ok, rp, tp, ip) == 0
        assert fb(2, lp, mp, ok, rp, tp, ip) == 0
        assert rp_(N, xp, zp, np_, cap, ok, rp, tp, ip) == 0
        e.sync()
        # no match (frames, bank) or ten equal pairs (explicit): every frame fails with zeros
        for t in (rm, tv, ni, mask):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
        e.sync()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)
    # a context without a PnP reservation refuses the three calls
    bare = engine(conf_thresh=0.001)
    try:
        assert lib.fpc_ransac_pnp(bare._ctx, N, xp, zp, np_, cap, ok, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_pnp_frames(bare._ctx, 1, kz, vp, op, mp, ok, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_pnp_bank(bare._ctx, 1, lp, mp, ok, rp, tp, ip, bp) == FPC_E_INVALID
        h0, b0 = bare._l.fpc_plan_hash(bare._ctx), bare._l.fpc_packed_size(bare._ctx)
        assert bare.pnp_reserve() > 0                                                # ... and the reservation carves nothing
        assert (bare._l.fpc_plan_hash(bare._ctx), bare._l.fpc_packed_size(bare._ctx)) == (h0, b0)
        assert bare._l.fpc_plan_hash(bare._ctx) == e._l.fpc_plan_hash(e._ctx)
    finally:
        bare.close()
    with pytest.raises(TypeError):
        e.ransac_pnp(xy, xyz, npairs, min_front=5)
    with pytest.raises(ValueError):
        e.ransac_pnp(xy, xyz, npairs, K=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.pnp_bank(N, slot, match)                                                   # no bank
