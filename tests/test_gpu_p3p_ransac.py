"""Minimal-sample absolute pose on the GPU (fpc_ransac_p3p / fpc_p3p_frames / fpc_p3p_bank) against the float64 restatement
and the planted scenes of tests/test_p3p_ransac.py, box and planar: planted poses with outliers, the tails of the pair list,
determinism, the frames variant bit-identical to explicit pairs and the bank variant to the frames variant, the planar chain
end to end (two views of a plane give a key frame with coplanar landmarks through fpc_pose_homography_frames, a third view
is localised against it -- where fpc_pnp_bank fails -- and its pose feeds the guided match and the map growth) and the
argument checks.  The 6-point calls are covered by tests/test_gpu_pnp_ransac.py, whose helpers this file imports.  Every
context runs under the canary zones.
Need a real MI355X: pytest -m gpu

Device against restatement where both picked the same best sample (identical masks): both evaluate the solve and the refits
in fp64 and differ by the contraction of a * b + c into one rounding in the refits and by the last bits of cbrt, acos and cos,
so what is left is the fp32 rounding of the outputs: the bars are test_gpu_pnp_ransac.py's R_SAME_BAR / T_SAME_BAR.  Measured
on the MI355X over the 44 frames of the two families and three case sets: all 44 with the restatement's mask, worst
difference 0.0 in every entry of R and of t -- the same fp32 values."""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_homography_ransac import engine
from tests.test_gpu_match_guided import plant
from tests.test_gpu_pnp_ransac import (H, KQVGA, N, R_SAME_BAR, T_SAME_BAR, W, _assert_mask_is_the_reprojection_test, _bits,
                                       _host_lists, _pack, _reserved)
from tests.test_p3p_ransac import (CASE_SETS, FAMILIES, PARAMS, bars, check_planted_pose, p3p_rule, planar_scene,
                                   restated_batch)
from tests.test_pnp_ransac import FRAME_H, FRAME_W, _rotation, camera_points, planted_scene, pose_errors

pytestmark = pytest.mark.gpu

FPC_E_INVALID = -1
THR = PARAMS["reproj_threshold"]


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
    e = _reserved(engine(H, W, N, max_keypoints=1024))
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


_DEVICE = {}


def _device_batch(e, family, rho, iterations):
    """The device's poses of one family's case set, computed once."""
    key = family, rho, iterations
    if key not in _DEVICE:
        scenes, _ = restated_batch(family, rho, iterations)
        xy, xyz, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
        assert len(set(npairs.tolist())) > 1
        _DEVICE[key] = e.ransac_p3p(xy, xyz, npairs, iterations=iterations, **PARAMS)
    return _DEVICE[key]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_device_against_the_restatement(vga, family, rho, iterations):
    scenes, results = restated_batch(family, rho, iterations)
    rm, tv, ni, mask = _device_batch(vga, family, rho, iterations)
    worst, same = np.zeros(2), 0
    for f, (scene, want) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not want.failed and rm[f].any(), (family, rho, f)
        check_planted_pose(rm[f], tv[f], mask[f, :m], scene, (family, rho, f, m))    # a different best sample may be picked
        _assert_mask_is_the_reprojection_test(rm[f], tv[f], mask[f], ni[f], scene[0], scene[1])
        assert ni[f] >= PARAMS["min_inliers"] and not mask[f, m:].any()
        # the count: the restatement's, give or take the pairs within 1e-3 px of the threshold
        assert abs(int(ni[f]) - want.ninliers) <= want.near.sum(), (family, rho, f, ni[f], want.ninliers, want.near.sum())
        if (mask[f, :m] == want.mask).all():                                         # the same sample: the same pose
            same += 1
            dr = np.abs(rm[f].astype(np.float64) - want.R).max()
            dt = np.linalg.norm(tv[f].astype(np.float64) - want.t) / np.linalg.norm(want.t)
            worst = np.maximum(worst, (dr, dt))
            assert dr <= R_SAME_BAR and dt <= T_SAME_BAR, (family, rho, f, dr, dt)
        print("%s rho %.1f frame %2d M %4d: %d inliers (restatement %d), rotation %.4f deg, translation %.3e"
              % (family, rho, f, m, ni[f], want.ninliers, *pose_errors(rm[f], tv[f], scene)))
    assert same >= len(scenes) // 2
    print("%s rho %.1f: %d of %d frames with the restatement's mask; worst difference there: R %.3e, t %.3e relative"
          % (family, rho, same, len(scenes), *worst))


def _raw_p3p(e, xy, xyz, npairs, mask=True, fill=0xFF, **params):
    """fpc_ransac_p3p into outputs pre-filled with `fill` bytes -> host arrays (R, t, ninliers, mask uint8)."""
    import torch
    dev = e.torch_device
    n, stride = xy.shape[0], xy.shape[1]
    p = e._pnp_params(None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (xy, xyz, npairs)]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev) for shape in ((n, 36), (n, 12), (n, 4), (n, stride))]
    torch.cuda.synchronize()
    e._call("fpc_ransac_p3p", n, ins[0], ins[1], ins[2], stride, ctypes.byref(p), outs[0], outs[1], outs[2],
            outs[3] if mask else None, inputs=ins)
    e.sync()
    rm, tv, ni, mk = (o.cpu().numpy() for o in outs)
    return rm.view(np.float32).reshape(n, 3, 3), tv.view(np.float32).reshape(n, 3), ni.view(np.int32).reshape(n), mk


def test_tails_of_the_pair_list(vga):
    e = vga
    cap = e.capacity
    xy, xyz, _, r, t = planar_scene(4, 0.0, cap)
    same = (np.repeat(xy[:1], 50, 0), np.repeat(xyz[:1], 50, 0))
    sizes = [1100, 0, 3, 4, 5, 256, 257, 1024, 1025, cap, 100]
    lists = [(xy[:m], xyz[:m]) for m in sizes] + [same]
    a, b, npairs = _pack(lists, cap)
    npairs[9] = cap + 9                                                              # above the stride: clamped
    params = dict(PARAMS, iterations=64)
    rm, tv, ni, mask = _raw_p3p(e, a, b, npairs, **params)
    assert set(np.unique(mask).tolist()) <= {0, 1}                                   # no 0xFF left: every row was written
    assert np.isfinite(rm).all() and np.isfinite(tv).all()
    for f in (1, 2, 11):                                                             # too few pairs / every sample degenerate
        assert not rm[f].any() and not tv[f].any() and ni[f] == 0 and not mask[f].any(), f
    for f, m in enumerate(sizes):
        want = p3p_rule(lists[f][0], lists[f][1], params, f)
        assert want.failed == (f in (1, 2)), f
        if want.failed:
            continue
        assert rm[f].any() and not mask[f, m:].any(), f                              # rows past the count: 0
        _assert_mask_is_the_reprojection_test(rm[f], tv[f], mask[f].astype(bool), ni[f], lists[f][0], lists[f][1])
        assert abs(int(ni[f]) - want.ninliers) <= want.near.sum(), f
        rot, tr = pose_errors(rm[f], tv[f], (None, None, None, r, t))
        rot_bar, trans_bar = bars(m)
        assert rot <= rot_bar and tr <= trans_bar, (f, rot, tr)
        if m >= 100:
            assert ni[f] >= 0.98 * m, (f, ni[f])
    assert ni[3] == 4 and ni[4] == 5                                                 # the sample is (nearly) the whole list
    assert mask[0, 1024:1100].sum() >= 0.98 * 76                                     # the pairs behind the first chunk count
    assert mask[9, cap - 1] == 1 and ni[9] >= 0.98 * cap
    # a failed frame between two good ones: zeros, and its neighbours are what they are alone
    alone = _raw_p3p(e, a[[0]], b[[0]], npairs[[0]], **params)                       # n = 1
    _bits(alone[0][0], rm[0])
    _bits(alone[1][0], tv[0])
    np.testing.assert_array_equal(alone[3][0], mask[0])
    # min_inliers above what one frame can reach fails that frame only; T = 1 and T = 257 (a partial last workgroup)
    fm2 = _raw_p3p(e, a, b, npairs, **dict(params, min_inliers=101))
    assert not fm2[0][10].any() and not fm2[1][10].any() and fm2[2][10] == 0 and not fm2[3][10].any()
    _bits(fm2[0][[0, 9]], rm[[0, 9]])
    one = _raw_p3p(e, a, b, npairs, **dict(params, iterations=1))
    assert one[2][10] == one[3][10].sum()
    more = _raw_p3p(e, a, b, npairs, **dict(params, iterations=257))
    assert more[2][10] >= 98 and more[2][0] >= 0.98 * 1100
    # refits = 0: the best sample's rounded pose, a rotation without a polar step
    bare0 = _raw_p3p(e, a, b, npairs, **dict(params, refits=0))
    want0 = p3p_rule(lists[10][0], lists[10][1], dict(params, refits=0), 10)
    assert not want0.failed and np.abs(bare0[0][10].astype(np.float64) - want0.first[0]).max() <= R_SAME_BAR
    assert np.linalg.norm(bare0[1][10].astype(np.float64) - want0.first[1]) <= T_SAME_BAR * np.linalg.norm(want0.first[1])
    assert abs(np.linalg.det(bare0[0][10].astype(np.float64)) - 1.0) < 1e-6 and bare0[2][10] == bare0[3][10].sum()
    # a NULL mask: R, t and the count are what they were
    bare = _raw_p3p(e, a, b, npairs, mask=False, **params)
    _bits(bare[0], rm)
    np.testing.assert_array_equal(bare[2], ni)
    assert (bare[3] == 0xFF).all()
    # landmarks behind the camera are never inliers
    bxy, bxyz, _, br, bt = planted_scene(4, 0.0, 100)
    behind = ((-camera_points(br, bt, bxyz[:10]) - bt) @ br).astype(np.float32)
    c, d, npq = _pack([(np.concatenate([bxy, bxy[:10]]), np.concatenate([bxyz, behind]))], cap)
    got = e.ransac_p3p(c, d, npq, **params)
    assert got[2][0] >= 98 and not got[3][0, 100:].any()


def test_determinism_and_seeds(vga):
    e = vga
    rho, iterations = CASE_SETS[1]
    scenes, _ = restated_batch("planar", rho, iterations)
    first = _device_batch(e, "planar", rho, iterations)
    xy, xyz, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
    again = e.ransac_p3p(xy, xyz, npairs, iterations=iterations, **PARAMS)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # another seed picks other samples and still meets the planted bars on every frame
    other = e.ransac_p3p(xy, xyz, npairs, iterations=iterations, **dict(PARAMS, seed=3))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(other[0], first[0]))
    for f, scene in enumerate(scenes):
        m = len(scene[0])
        check_planted_pose(other[0][f], other[1][f], other[3][f, :m], scene, ("seed", f, m))


# ---- frames, bank: a planted planar world seen by the frames of a QVGA context ---------------------------------------------
def _flat_world(nkey=700, seed=3):
    """test_gpu_pnp_ransac._world with the key frame's landmarks on ONE plane (through depth 8, tilted 25 degrees): the same
    views, wrong matches, missing matches and invalid rows -> (key_xyz with three rows that are not finite, key_valid, the
    finite key_xyz, [(xy int32 [k,2], match int32 [k], R, t)] per view)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KQVGA
    px = np.stack([rng.uniform(20, W - 20, nkey), rng.uniform(20, H - 20, nkey)], 1)
    tilt, az = np.deg2rad(25.0), rng.uniform(0, 2 * np.pi)
    nrm = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
    ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(nkey)], 1)
    key_xyz = (ray * (8.0 * nrm[2] / (ray @ nrm))[:, None]).astype(np.float32)
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
    """The views' pixels and counts as the frames of the context (no descriptor is read by the pose calls) -> the match
    table (device, int32 [N,cap])."""
    import torch
    cap = e.capacity
    hx, hm = np.zeros((N, cap, 2), np.int32), np.full((N, cap), -1, np.int32)
    for f, (pix, match, _, _) in enumerate(views):
        hx[f, :len(pix)], hm[f, :len(match)] = pix, match
        hm[f, len(match):len(match) + 8] = 3                                        # rows past the count are never pairs
    plant(e, dict(desc=np.zeros((N, cap, e.desc_dim), np.float32), xy=hx, counts=np.array([len(v[0]) for v in views])))
    return torch.from_numpy(hm).to(e.torch_device)


def test_frames_and_bank_variants_are_bit_identical_to_explicit_pairs(qvga):
    import torch
    e = qvga
    cap, dev = e.capacity, e.torch_device
    key_xyz, valid, _, views = _flat_world()
    nkey = len(key_xyz)
    match = _plant_views(e, views)
    params = dict(K=KQVGA, iterations=256, seed=11, reproj_threshold=3.0, min_inliers=12)
    got = e.p3p_frames(N, match, key_xyz, valid, **params)
    xy, xyz, npairs, rows = _host_lists(views, key_xyz, valid, nkey, cap)
    assert npairs.min() > 150
    rm, tv, ni, mask = e.ransac_p3p(xy, xyz, npairs, **params)
    _bits(got[0], rm)
    _bits(got[1], tv)
    np.testing.assert_array_equal(got[2], ni)
    for f in range(N):
        back = np.zeros(cap, bool)
        back[rows[f]] = mask[f, :npairs[f]]
        np.testing.assert_array_equal(got[3][f], back)                               # invalid landmarks are not pairs
        rot, tr = pose_errors(got[0][f], got[1][f], (None, None, None, views[f][2], views[f][3]))
        assert ni[f] >= 0.7 * npairs[f] and rot <= 0.5, (f, ni[f], npairs[f], rot, tr)
    dlt = e.pnp_frames(N, match, key_xyz, valid, **params)                           # the 6-point model has nothing to say here
    assert not dlt[0].any() and not dlt[2].any()
    # the bank: slot s holds the key's rows (any descriptors) and its landmarks
    slots = 2
    e.bank_create(slots, cap)
    try:
        assert e.bank_landmarks_reserve() >= slots * cap * 16
        desc = np.random.default_rng(1).normal(size=(nkey, e.desc_dim)).astype(np.float32)
        kxy = np.zeros((nkey, 2), np.int32)
        for s, k in ((0, nkey), (1, 300)):
            e.bank_store_rows(s, desc[:k], kxy[:k])
        full_xyz, full_valid = np.zeros((cap, 3), np.float32), np.zeros(cap, bool)
        full_xyz[:nkey], full_valid[:nkey] = key_xyz, valid
        e.bank_store_landmarks(0, full_xyz, full_valid)
        e.bank_store_landmarks(1, full_xyz, full_valid)
        slot = torch.tensor([0, 1, -1, slots, 0, 1, 0, 1], dtype=torch.int32, device=dev)
        bank = e.p3p_bank(N, slot, match, **params)
        for v in bank:
            assert not v[[2, 3]].any()                                               # no slot: the frame fails with zeros
        for a, b in zip(bank, got):
            np.testing.assert_array_equal(a[[0, 4, 6]].view(np.uint8), b[[0, 4, 6]].view(np.uint8))
        kx = torch.from_numpy(key_xyz).to(dev)
        few = e.p3p_frames(N, match, (kx, torch.tensor([300], dtype=torch.int32, device=dev)), valid, **params)
        for a, b in zip(bank, few):
            np.testing.assert_array_equal(a[[1, 5, 7]].view(np.uint8), b[[1, 5, 7]].view(np.uint8))
        # ... and against fpc_p3p_frames with the slot's own storage as the key
        lm = e.bank_landmarks()
        _, _, bc = e.bank_view()
        for s in range(slots):
            ref = e.p3p_frames(N, match, (lm[s, :, :3].contiguous(), bc[s:s + 1].clone()), lm[s, :, 3] != 0, **params)
            rows_of = np.flatnonzero(slot.cpu().numpy() == s)
            for a, b in zip(bank, ref):
                np.testing.assert_array_equal(a[rows_of].view(np.uint8), b[rows_of].view(np.uint8))
        assert bank[2][[0, 1]].min() > 50
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()


# ---- the planar chain ---------------------------------------------------------------------------------------------------------
CHAIN_SEED, CHAIN_CAP = 21, 1024
# The planted-truth bars of the chain.  Its landmarks are not planted ones: they are the rays of B's ROUNDED pixels cut with the
# plane that fpc_pose_homography_* estimated from rounded pixels, so the third view's error is P3P's and the two-view
# call's together, and a planar landmark set leaves tilt and translation weakly separated.  As for ROT_BAR / TRANS_BAR the
# reference's own error sets the bar: the float64 restatements chained on the host (test_homography_ransac.ransac_rule ->
# test_pose_homography.pose_h_rule -> p3p_rule, restated_chain below) over the scenes of seeds 21 .. 28 show at worst a
# rotation error of 0.1208 degrees and a relative translation error of 1.385e-02 (seed 21, the test's: 0.0442 and 4.554e-03);
# the bars are twice the worst.
CHAIN_ROT_BAR, CHAIN_TRANS_BAR = 2 * 0.1208, 2 * 1.385e-02


def _rounded(r, t, xb):
    fx, fy, cx, cy = KQVGA
    xc = camera_points(r, t, xb)
    p = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)).astype(np.int32)
    return p, (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)


def chain_scene(seed=CHAIN_SEED, npts=900, cap=CHAIN_CAP):
    """One plane (through depth 8 of camera B, tilted 25 degrees) seen by three QVGA cameras A, B, C, every pixel rounded:
    the scene in B's frame, X_A = R_ab X_B + t_ab, X_C = R_cb X_B + t_cb; the A-B baseline is a third of the depth, as in
    test_gpu_pnp_ransac's three-view test.  Every view holds its scene points in an order of its own; a seventh of C's rows
    show another point's descriptor (desc_c: the scene point whose descriptor a row of C carries)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KQVGA
    px = np.stack([rng.uniform(30, W - 30, npts), rng.uniform(30, H - 30, npts)], 1)
    tilt, az = np.deg2rad(25.0), rng.uniform(0, 2 * np.pi)
    nrm = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), np.cos(tilt)])
    ray = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(npts)], 1)
    xb = ray * (8.0 * nrm[2] / (ray @ nrm))[:, None]
    r_ab, t_ab = _rotation([0.2, 1.0, 0.1], np.deg2rad(8.0)), np.array([2.6, 0.4, 0.5])
    r_cb, t_cb = _rotation([1.0, -0.4, 0.3], np.deg2rad(6.0)), np.array([-0.9, 0.5, 0.7])
    (pa, in_a), (pb, _), (pc, in_c) = _rounded(r_ab, t_ab, xb), _rounded(np.eye(3), np.zeros(3), xb), _rounded(r_cb, t_cb, xb)
    rows_a = rng.permutation(np.flatnonzero(in_a))[:cap]
    rows_b = rng.permutation(npts)[:800]
    rows_c = rng.permutation(np.flatnonzero(in_c))[:700]
    desc_c = rows_c.copy()
    wrong = rng.choice(len(rows_c), 100, replace=False)
    desc_c[wrong] = rng.permutation(rows_b)[:100]
    where_a, where_b = np.full(npts, -1, np.int64), np.full(npts, -1, np.int64)
    where_a[rows_a], where_b[rows_b] = np.arange(len(rows_a)), np.arange(len(rows_b))
    return dict(normal=nrm, r_ab=r_ab, t_ab=t_ab, r_cb=r_cb, t_cb=t_cb, pa=pa, pb=pb, pc=pc, rows_a=rows_a, rows_b=rows_b,
                rows_c=rows_c, desc_c=desc_c, where_a=where_a, where_b=where_b, npts=npts)


def restated_chain(seed):
    """The chain of the test below through the float64 restatements, on the host, with the matches an exact descriptor match
    gives -> (rotation error in degrees, relative translation error) of C's pose after the rescale by the planted baseline."""
    from tests.test_homography_ransac import ransac_rule
    from tests.test_pose_homography import pose_h_rule
    w = chain_scene(seed)
    m_ba = w["where_a"][w["rows_b"]]
    ok = m_ba >= 0
    src, dst = w["pb"][w["rows_b"]][ok].astype(np.float64), w["pa"][w["rows_a"]][m_ba[ok]].astype(np.float64)
    hm, _ = ransac_rule(src, dst, dict(iterations=256, seed=5), 0)
    hm = hm.astype(np.float32).astype(np.float64)
    both = pose_h_rule(src, dst, hm, k_query=KQVGA, k_train=KQVGA)
    which = int(np.argmax(np.where(both.nfront > 0, both.plane[:, :3] @ w["normal"], -2.0)))
    got = pose_h_rule(src, dst, hm, k_query=KQVGA, k_train=KQVGA, which=which)
    xyz_b, front_b = np.zeros((len(ok), 3), np.float32), np.zeros(len(ok), bool)
    xyz_b[ok], front_b[ok] = got.xyz, got.front
    m_cb = w["where_b"][w["desc_c"]]
    use = (m_cb >= 0) & front_b[np.maximum(m_cb, 0)]
    res = p3p_rule(w["pc"][w["rows_c"]][use].astype(np.float32), xyz_b[m_cb[use]], dict(iterations=256, seed=3), 0, kvec=KQVGA)
    assert not res.failed
    return pose_errors(res.R, res.t * np.linalg.norm(w["t_ab"]), (None, None, None, w["r_cb"], w["t_cb"]))


def test_planar_chain_end_to_end():
    """Two planted views of ONE PLANE give a key frame whose landmarks lie on one plane (up to their triangulation's
    noise), and a third view is localised against it: fpc_match_frames, fpc_homography_frames,
    fpc_pose_homography_frames (view B against the key A: both solutions; the caller keeps the one whose normal is the planted plane's), fpc_bank_store + fpc_bank_store_landmarks (xyz[0] and front[0]
    as they are: B becomes a key frame at the scale |baseline| = 1), fpc_match_bank (view C against B), fpc_p3p_bank.  C's
    translation in units of the A-B baseline, multiplied by the planted baseline, is the planted translation (the bars:
    CHAIN_ROT_BAR / CHAIN_TRANS_BAR above).  On the SAME inputs fpc_pnp_bank returns the failure outputs: the DLT has rank
    < 11 on a plane.  The pose then goes unchanged into fpc_match_bank_guided_pose and fpc_landmarks_bank, which return
    matches and landmarks: the chain runs on."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = _reserved(engine(H, W, 2, max_keypoints=CHAIN_CAP))
    try:
        cap = e.capacity
        assert cap == CHAIN_CAP
        w = chain_scene()
        rows_a, rows_b, rows_c, desc_c = w["rows_a"], w["rows_b"], w["rows_c"], w["desc_c"]
        assert len(rows_a) > 500 and len(rows_c) > 500
        rows = np.random.default_rng(1000 + CHAIN_SEED).normal(size=(w["npts"], e.desc_dim))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        baseline = np.linalg.norm(w["t_ab"])

        def frame0(points, which_desc):
            """Frame 0 of the context: the pixels `points` with the descriptors of the scene points `which_desc`."""
            desc, xy = np.zeros((2, cap, e.desc_dim), np.float32), np.zeros((2, cap, 2), np.int32)
            desc[0, :len(points)], xy[0, :len(points)] = rows[which_desc], points
            plant(e, dict(desc=desc, xy=xy, counts=np.array([len(points), 0])))
        # ---- B against the key A: H, its two poses, B's points on the plane
        frame0(w["pb"][rows_b], rows_b)
        key, key_xy = rows[rows_a], w["pa"][rows_a]
        m_ba, _ = e.match_frames_async(2, key=key, cross_check=True)
        hm, nih, _ = e.homography_frames_async(2, m_ba, key_xy=key_xy, iterations=256, seed=5)
        both = e.pose_homography_frames(2, m_ba, hm, key_xy=key_xy, K_query=KQVGA, K_train=KQVGA, points=False)
        planes, nfront = both[3][0], both[4][0]
        assert nfront.max() > 400, nfront
        which = int(np.argmax(np.where(nfront > 0, planes[:, :3] @ w["normal"], -2.0)))      # the caller's pick
        assert planes[which, :3] @ w["normal"] > np.cos(np.deg2rad(2.0))
        got = e.pose_homography_frames_async(2, m_ba, hm, key_xy=key_xy, K_query=KQVGA, K_train=KQVGA, which=which)
        e.bank_create(2, cap)
        e.bank_landmarks_reserve()
        e.bank_store(0, 1)                                                           # B becomes slot 1 ...
        e.bank_store_landmarks(1, got[6][0], got[7][0])                              # ... with its points, as they are
        xyz_b, front_b = e._host((got[6], got[7]))
        xyz_b, front_b = xyz_b[0], front_b[0].astype(bool)
        assert front_b[:len(rows_b)].sum() > 400 and not front_b[len(rows_b):].any()
        flat = xyz_b[front_b].astype(np.float64)
        # one plane up to the triangulation's noise: a rounded pixel pair (0.29 px rms each) at fx = 250 and a baseline of a
        # third of the depth moves a point by 0.29 sqrt(2) / (250 / 3) = 0.5 % of its depth (one sigma) along its ray; the
        # worst of some 500 points stays within 3 % of the largest depth
        off = np.abs(flat @ planes[which, :3].astype(np.float64) - planes[which, 3]).max()
        assert off < 0.03 * flat[:, 2].max(), (off, flat[:, 2].max())
        # ---- C against the bank
        frame0(w["pc"][rows_c], desc_c)
        _, best, m_cb, _ = e.match_bank_async(2, cross_check=True)
        p3p = e.p3p_bank_async(2, best, m_cb, K=KQVGA, iterations=256, seed=3)
        dlt = e.pnp_bank_async(2, best, m_cb, K=KQVGA, iterations=1024, seed=3)
        gm, gd = e.match_bank_guided_pose_async(2, best, p3p[0], p3p[1], 4.0, K=KQVGA)
        grown = e.landmarks_bank_async(2, best, gm, p3p[0], p3p[1], K_query=KQVGA, K_train=KQVGA)
        best, m_cb, gm = e._host((best, m_cb, gm))
        (rm, tv, ni, mask), dlt, grown = e._host(p3p), e._host(dlt), e._host(grown)
        assert best[0] == 1 and best[1] == -1
        nc = len(rows_c)
        j = w["where_b"][rows_c]
        right = (desc_c == rows_c) & (j >= 0) & front_b[np.maximum(j, 0)]            # a right match to a row with a landmark
        assert right.sum() > 300
        assert ni[0] >= 0.75 * right.sum() and ni[1] == 0 and not rm[1].any(), (ni, right.sum())
        rot, tr = pose_errors(rm[0], tv[0].astype(np.float64) * baseline, (None, None, None, w["r_cb"], w["t_cb"]))
        print("third view on a plane: rotation %.4f deg, translation %.3e relative (after the rescale by the planted baseline "
              "%.4f); %d inliers of %d right matches; |t| before the rescale %.4f"
              % (rot, tr, baseline, ni[0], right.sum(), np.linalg.norm(tv[0])))
        assert rot <= CHAIN_ROT_BAR and tr <= CHAIN_TRANS_BAR, (rot, tr)
        assert abs(np.linalg.det(rm[0].astype(np.float64)) - 1.0) < 1e-5
        assert not mask[0, :nc][~right & (m_cb[0, :nc] != j)].sum() > 5
        # the 6-point model on the same inputs: the failure outputs
        for v in dlt:
            assert not v.any()
        # the chain runs on: the pose gates the re-match and grows the map
        assert (gm[0, :nc] >= 0).sum() >= 0.9 * right.sum() and not (gm[0, nc:] >= 0).any()
        assert (gm[0, :nc][right] == j[right]).mean() > 0.95
        xyz_c, kind, counts = grown
        assert counts[0, 0] >= 0.9 * right.sum() and counts[0, 0] == (kind[0] == 1).sum() and not counts[1].any()
        carried = kind[0, :nc] == 1
        want = camera_points(rm[0].astype(np.float64), tv[0].astype(np.float64), xyz_b[gm[0, :nc][carried]])
        np.testing.assert_allclose(xyz_c[0, :nc][carried], want, rtol=1e-5, atol=1e-5)
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused(qvga):
    import torch
    e = qvga
    lib = _lib.load()
    cap, dev = e.capacity, e.torch_device
    plant(e, dict(desc=np.zeros((N, cap, e.desc_dim), np.float32), xy=np.zeros((N, cap, 2), np.int32),
                  counts=np.full(N, 10)))
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
    rp_ = lambda n, a, b, c, stride, p, r, t, i: lib.fpc_ransac_p3p(e._ctx, n, a, b, c, stride, p, r, t, i, bp)   # noqa: E731
    ff = lambda n, k, v, kc, m, p, r, t, i: lib.fpc_p3p_frames(e._ctx, n, k, v, kc, m, p, r, t, i, bp)           # noqa: E731
    fb = lambda n, s, m, p, r, t, i: lib.fpc_p3p_bank(e._ctx, n, s, m, p, r, t, i, bp)                           # noqa: E731
    ok = params()
    assert fb(N, lp, mp, ok, rp, tp, ip) == FPC_E_INVALID                            # no bank
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(fx=0.0), params(fy=-1.0), params(fx=nan), params(fy=inf), params(cx=nan), params(cy=-inf),
               params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
               params(reproj_threshold=nan), params(refits=-1), params(refits=5), params(min_inliers=3), None]
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
        # the one difference from the 6-point calls: min_inliers 4 and 5 are accepted here and refused there
        for k in (4, 5):
            assert lib.fpc_ransac_pnp(e._ctx, N, xp, zp, np_, cap, params(min_inliers=k), rp, tp, ip, bp) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        for t in (rm, tv):
            assert (t.cpu() == 7.0).all()
        assert (ni.cpu() == 7).all() and (mask.cpu() == 7).all()
        for k in (4, 5):
            assert rp_(N, xp, zp, np_, cap, params(min_inliers=k), rp, tp, ip) == 0
        assert ff(N, kz, None, op, mp, params(min_inliers=4), rp, tp, ip) == 0
        assert fb(N, lp, mp, params(min_inliers=4), rp, tp, ip) == 0
        e.sync()
        # no match (frames, bank) or ten equal pairs (explicit): every frame fails with zeros
        for t in (rm, tv, ni, mask):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
        e.sync()
    # a context without a PnP reservation refuses the three calls
    bare = engine(H, W, N, max_keypoints=1024)
    try:
        assert lib.fpc_ransac_p3p(bare._ctx, N, xp, zp, np_, cap, ok, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_p3p_frames(bare._ctx, 1, kz, vp, op, mp, ok, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_p3p_bank(bare._ctx, 1, lp, mp, ok, rp, tp, ip, bp) == FPC_E_INVALID
    finally:
        bare.close()
    with pytest.raises(TypeError):
        e.ransac_p3p(xy, xyz, npairs, min_front=5)
    with pytest.raises(ValueError):
        e.ransac_p3p(xy, xyz, npairs, K=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.p3p_bank(N, slot, match)                                                   # no bank
