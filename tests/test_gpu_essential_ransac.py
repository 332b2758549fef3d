"""Minimal-sample relative pose on the GPU (fpc_ransac_essential / fpc_essential_frames / fpc_essential_bank) against the
float64 restatement and the planted scenes of tests/test_essential_ransac.py: the device next to the restatement on every
planted frame (counts and masks equal, F and E bit for bit), the pose through fpc_pose_fundamental against the planted truth,
the gap the model closes (exactly planar pairs, a mostly planar scene), planar scenes against fpc_pose_homography's two
solutions, the tails of the pair list, determinism and the variants' bit-identities, the chain into the bank's landmarks
without a host call, and the argument checks.  Every context runs under the canary zones.
Measured on the MI355X: on all 36 planted frames the device's ninliers and mask equal the restatement's and its F and E are
the restatement's fp32 values bit for bit; worst pose error against the planted truth 2.55 degrees of rotation and 21.2 of
direction (the restatement's own worst frame); the planar frames lie within 1.28 / 16.4 degrees of a solution of
fpc_pose_homography; the refined pose of the chain within 0.009 / 0.050 (box) and 0.064 / 0.435 degrees (planar).
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_essential_ransac import (CASE_SETS, DIR_BAR, FAMILIES, GAP, KEEP, PARAMS, ROT_BAR, essential_rule,
                                         exact_planar_lists, gap_batch, planted_scene, pose_distance, pose_errors,
                                         restated_batch)
from tests.test_fundamental_ransac import FRAME_H, FRAME_W, sampson_distance
from tests.test_gpu_fundamental_ransac import _assert_form, _assert_mask_is_the_sampson_test, _pack
from tests.test_gpu_homography_ransac import _host_pairs, engine
from tests.test_gpu_match_guided import plant
from tests.test_pose_epipolar import KVEC

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
STRIDE = 256
FPC_E_INVALID = -1
THR = PARAMS["reproj_threshold"]


@pytest.fixture(scope="module")
def vga():
    """An 8-frame VGA context without the descriptor head: explicit pairs need no network."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, N, descriptor_enabled=False, max_keypoints=1024)
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


@pytest.fixture(scope="module")
def qvga():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(conf_thresh=0.001)
    e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(300, N, H, W))
    assert min(len(r[0]) for r in res) > 1000
    yield e, res
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_DEVICE = {}


def _device_batch(e, family, rho, iterations):
    """The device's answer to one planted case set, computed once and shared by the tests that need it."""
    key = (family, rho, iterations)
    if key not in _DEVICE:
        scenes, results = restated_batch(family, rho, iterations)
        src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], STRIDE)
        got = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, iterations=iterations, **PARAMS)
        pose = e.pose_fundamental(src, dst, npairs, got[0], K_query=KVEC, K_train=KVEC, reproj_threshold=THR)
        _DEVICE[key] = scenes, results, got, pose
    return _DEVICE[key]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_device_agrees_with_the_restatement(vga, family, rho, iterations):
    """Every planted frame: ninliers and the mask equal, F and E bit for bit."""
    scenes, results, (fm, em, ni, mask), _ = _device_batch(vga, family, rho, iterations)
    for f, (s, res) in enumerate(zip(scenes, results)):
        m = len(s[0])
        tag = (family, rho, f, m)
        same_f = np.array_equal(_bits(fm[f].reshape(-1)), _bits(res.F))
        same_e = np.array_equal(_bits(em[f].reshape(-1)), _bits(res.E))
        print("%s rho %.1f frame %d M %3d: device %d inliers, restatement %d; F bits equal %s, E bits equal %s, max |dF| %.3e"
              % (family, rho, f, m, ni[f], res.ninliers, same_f, same_e,
                 np.abs(fm[f].reshape(-1).astype(np.float64) - res.F).max()))
        assert ni[f] == res.ninliers, tag
        np.testing.assert_array_equal(mask[f, :m], res.mask, err_msg=str(tag))
        assert not mask[f, m:].any(), tag
        assert same_f and same_e, tag
        _assert_form(fm[f])
        _assert_form(em[f])
        _assert_mask_is_the_sampson_test(fm[f], mask[f], ni[f], s[0].astype(np.float64), s[1].astype(np.float64))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_pose_meets_the_planted_truth(vga, family, rho, iterations):
    """fpc_pose_fundamental on the returned F, with this call's threshold: the pairs it uses are the mask's, and R, t lie
    within twice the restatement's worst errors of the planted motion (planar: or of its plane twin)."""
    scenes, _, (fm, em, ni, mask), (rm, tv, nf, xyz, front) = _device_batch(vga, family, rho, iterations)
    for f, s in enumerate(scenes):
        m = len(s[0])
        assert fm[f].any() and nf[f] >= 8, (family, rho, f)
        assert not (front[f, :m] & ~mask[f, :m]).any(), (family, rho, f)                 # front is a subset of this mask
        rot, direction = pose_errors(rm[f], tv[f], s)
        print("%s rho %.1f frame %d M %3d: rotation %.4f deg, direction %.4f deg, %d in front of %d inliers"
              % (family, rho, f, m, rot, direction, nf[f], ni[f]))
        assert rot <= ROT_BAR and direction <= DIR_BAR, (family, rho, f, rot, direction)
        sv = np.linalg.svd(em[f].astype(np.float64), compute_uv=False)
        assert sv[2] <= 1e-6 * sv[0] and abs(sv[0] - sv[1]) <= 1e-5 * sv[0]             # E is an essential matrix


def test_exactly_planar_pairs_fail_the_eight_point_and_not_this_call(vga):
    e = vga
    lists = list(exact_planar_lists().values())
    src, dst, npairs = _pack(lists, STRIDE)
    f8, n8, m8 = e.ransac_fundamental(src, dst, npairs, iterations=1024, **PARAMS)
    assert not f8.any() and not n8.any() and not m8.any()
    fm, em, ni, mask = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, iterations=64, **PARAMS)
    for f, (s, d) in enumerate(lists):
        m = len(s)
        assert fm[f].any() and ni[f] == m and mask[f, :m].all() and not mask[f, m:].any(), f
        # (not bit for bit here: E = [t]x has a zero diagonal, and those entries of F hold what the refit's fp64 sums leave
        # of it, 1e-19, in whatever order they were added; half an fp32 ulp of the unit-norm F is the comparison)
        res = essential_rule(s, d, dict(PARAMS, iterations=64), f)
        assert np.abs(fm[f].reshape(-1).astype(np.float64) - res.F).max() <= 2.0 ** -25
        assert sampson_distance(fm[f].astype(np.float64), s, d).max() < THR


def test_mostly_planar_scene_with_outliers(vga):
    """A plane with 15 % of the points off it and 50 % outliers, at the budget tests/test_essential_ransac.py established:
    the 8-point call keeps fewer than KEEP of the planted pairs on at least one frame, this call on none."""
    e = vga
    scenes, ours, theirs = gap_batch()
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], STRIDE)
    params = dict(PARAMS, iterations=GAP["iterations"])
    fm, em, ni, mask = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, **params)
    f8, n8, m8 = e.ransac_fundamental(src, dst, npairs, **params)
    lost = 0
    for f, (s, res) in enumerate(zip(scenes, ours)):
        planted, m = s[2], len(s[0])
        assert ni[f] == res.ninliers and np.array_equal(mask[f, :m], res.mask), f
        assert mask[f, :m][planted].sum() >= KEEP * planted.sum(), f
        lost += (not f8[f].any()) or m8[f, :m][planted].sum() < KEEP * planted.sum()
        print("frame %d: essential %d of %d planted, 8-point %d" % (f, mask[f, :m][planted].sum(), planted.sum(),
                                                                   m8[f, :m][planted].sum()))
    assert lost >= 1


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_planar_scenes_against_the_homography_poses(vga, rho, iterations):
    """The pose of the returned E equals, up to the sign of t and the bars, one of the two solutions fpc_pose_homography
    gives for the same pairs."""
    e = vga
    scenes, _, (fm, em, ni, mask), (rm, tv, nf, xyz, front) = _device_batch(e, "planar", rho, iterations)
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], STRIDE)
    hm, hn, _ = e.ransac_homography(src, dst, npairs, iterations=iterations, reproj_threshold=3.0, seed=7)
    kind, hr, ht = e.pose_homography(src, dst, npairs, hm, K_query=KVEC, K_train=KVEC, points=False)[:3]
    for f in range(len(scenes)):
        assert kind[f] in (1, 2), (rho, f, kind[f])
        errs = [pose_distance(rm[f], tv[f], (hr[f, j].astype(np.float64), ht[f, j].astype(np.float64), True))
                for j in range(2) if hr[f, j].any()]
        rot, direction = min(errs, key=lambda v: v[0] / ROT_BAR + v[1] / DIR_BAR)
        print("planar rho %.1f frame %d: nearest homography solution at %.4f deg, %.4f deg (%d solutions)"
              % (rho, f, rot, direction, len(errs)))
        assert rot <= ROT_BAR and direction <= DIR_BAR, (rho, f, rot, direction)


def test_tails_of_the_pair_list(vga):
    e = vga
    s, d, _, _, _, _ = planted_scene("box", 3, 0.0, 200)
    nan = s[:40].copy()
    nan[3], nan[17, 1] = np.nan, np.inf
    rep = (np.concatenate([s[:30], s[:30]]), np.concatenate([d[:30], d[:30]]))
    same = (np.repeat(s[:1], 50, 0), np.repeat(d[:1], 50, 0))
    lists = [(s[:5], d[:5]), (s[:6], d[:6]), (s[:7], d[:7]), (s, d), rep, (nan, d[:40]), same, (s[:0], d[:0])]
    src, dst, npairs = _pack(lists, 200)
    npairs[3] = 200 + 9                                                              # above the stride: clamped
    params = dict(PARAMS, iterations=256, min_inliers=6)
    fm, em, ni, mask = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, **params)
    for f in (0, 6, 7):                                            # 5 pairs; all pairs identical; none: a zero F, no mask
        assert not fm[f].any() and not em[f].any() and ni[f] == 0 and not mask[f].any(), f
    for f, m in ((1, 6), (2, 7), (3, 200), (4, 60)):
        res = essential_rule(lists[f][0], lists[f][1], params, f)
        assert not res.failed and ni[f] == res.ninliers and np.array_equal(mask[f, :m], res.mask), (f, ni[f], res.ninliers)
        np.testing.assert_array_equal(_bits(fm[f].reshape(-1)), _bits(res.F))
        assert not mask[f, m:].any()
        _assert_form(fm[f])
    assert ni[1] == 6 and ni[2] >= 6 and ni[3] >= 196 and ni[4] >= 58
    # non-finite coordinates match nothing and poison nothing: the frame is solved from the others
    assert fm[5].any() and np.isfinite(fm[5]).all() and np.isfinite(em[5]).all() and ni[5] >= 36
    assert not mask[5, 3] and not mask[5, 17] and ni[5] == mask[5].sum()
    # E_dev = NULL: the other outputs are the same bits
    import torch
    dev = e.torch_device
    ts, td = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    tn = torch.from_numpy(npairs).to(dev)
    f2 = torch.empty((len(lists), 9), dtype=torch.float32, device=dev)
    n2 = torch.empty((len(lists),), dtype=torch.int32, device=dev)
    m2 = torch.empty((len(lists), 200), dtype=torch.uint8, device=dev)
    p = _lib.FpcEssentialParams()
    lib = _lib.load()
    lib.fpc_default_essential_params(ctypes.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    torch.cuda.synchronize()
    assert lib.fpc_ransac_essential(e._ctx, len(lists), ts.data_ptr(), td.data_ptr(), tn.data_ptr(), 200, ctypes.byref(p),
                                    f2.data_ptr(), None, n2.data_ptr(), m2.data_ptr()) == 0
    e.sync()
    np.testing.assert_array_equal(_bits(f2.cpu().numpy()), _bits(fm.reshape(-1, 9)))
    np.testing.assert_array_equal(n2.cpu().numpy(), ni)
    np.testing.assert_array_equal(m2.cpu().numpy().astype(bool), mask)
    # min_inliers above what a frame can reach fails that frame only; T = 1 and T = 65 (a partial last workgroup)
    fm3, em3, ni3, mask3 = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, **dict(params, min_inliers=61))
    assert not fm3[4].any() and not em3[4].any() and ni3[4] == 0 and not mask3[4].any()
    np.testing.assert_array_equal(_bits(fm3[3]), _bits(fm[3]))
    for t in (1, 65):
        one = e.ransac_essential(src, dst, npairs, K_query=KVEC, K_train=KVEC, **dict(params, iterations=t))
        res = essential_rule(s, d, dict(params, iterations=t), 3)
        assert one[2][3] == res.ninliers and np.array_equal(_bits(one[0][3].reshape(-1)), _bits(res.F)), t


def test_determinism_and_seeds(vga):
    e = vga
    scenes, _ = restated_batch("box", 0.3, 256)
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], STRIDE)
    a = e.ransac_essential(src, dst, npairs, iterations=256, seed=5)
    b = e.ransac_essential(src, dst, npairs, iterations=256, seed=5)
    c = e.ransac_essential(src, dst, npairs, iterations=256, seed=6)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint8) if x.dtype == bool else x.view(np.uint32), y.view(np.uint8) if y.dtype == bool else y.view(np.uint32))
    assert a[0].any(axis=(1, 2)).all()
    assert (_bits(a[0]) != _bits(c[0])).any()


def _assert_frames_equal_explicit(e, n, res, match_dev, key_pts, key_xy_host, pairing, **params):
    cap = e.capacity
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    got = e.essential_frames(n, match_dev, key_xy=key_pts, pairing=pairing, **params)
    empty = np.zeros((0, 2), np.int32)

    def train_of(f):
        if pairing == "previous" and f > 0:
            return xy[f - 1]
        return key_xy_host if key_xy_host is not None else empty
    src, dst, npairs, rows = _host_pairs(match_dev.cpu().numpy(), xy, counts, train_of, cap)
    fm, em, ni, mask = e.ransac_essential(src, dst, npairs, **params)
    np.testing.assert_array_equal(_bits(got[0]), _bits(fm))
    np.testing.assert_array_equal(_bits(got[1]), _bits(em))
    np.testing.assert_array_equal(got[2], ni)
    for f in range(n):
        back = np.zeros(cap, bool)
        back[rows[f]] = mask[f, :npairs[f]]
        np.testing.assert_array_equal(got[3][f], back)
    return got, npairs


def test_frames_and_bank_variants_are_bit_identical(qvga):
    e, res = qvga
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    params = dict(iterations=256, seed=11, K_query=(250.0, 250.0, 160.0, 120.0), K_train=(250.0, 250.0, 160.0, 120.0))
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "key", **params)
    assert npairs.min() > 50 and (got[2] >= 8).any()
    m, _ = e.match_frames_async(N, key=None, pairing="previous", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, None, None, "previous", **params)
    assert npairs[0] == 0 and not got[0][0].any() and got[2][0] == 0 and not got[3][0].any()   # frame 0 has no train set
    slots = 3
    e.bank_create(slots, e.capacity)
    try:
        for s in range(slots):
            e.bank_store(s + 1, s)
        e.detect(synth.make_batch(400, N, H, W))
        _, best, m, _ = e.match_bank_async(N, cross_check=True, max_dist=0.9)
        slot = best.clone()
        slot[1], slot[4] = -1, slots
        fm, em, ni, mask = e.essential_bank(N, slot, m, **params)
        sl = slot.cpu().numpy()
        for v in (fm, em, ni, mask):
            assert not v[[1, 4]].any()                                               # slot -1 / out of range: zeros
        assert set(sl.tolist()) - {-1, slots} and (ni >= 8).any()
        _, bx, bc = e.bank_view()
        for s in sorted(set(sl.tolist()) - {-1, slots}):
            rows_of = np.flatnonzero(sl == s)
            rf, re_, rn, rm = e.essential_frames(N, m, key_xy=(bx[s].clone(), bc[s:s + 1].clone()), pairing="key", **params)
            np.testing.assert_array_equal(_bits(fm)[rows_of], _bits(rf)[rows_of])
            np.testing.assert_array_equal(_bits(em)[rows_of], _bits(re_)[rows_of])
            np.testing.assert_array_equal(ni[rows_of], rn[rows_of])
            np.testing.assert_array_equal(mask[rows_of], rm[rows_of])
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.detect(synth.make_batch(300, N, H, W))


@pytest.mark.parametrize("family", FAMILIES)
def test_chain_end_to_end_into_the_banks_landmarks(family):
    """match_frames -> essential_frames -> pose_frames -> refine_pose_frames -> bank_store + bank_store_landmarks with no host
    call in between, the SAME calls on a scene with depth and on a planar one."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        cap = e.capacity
        scene = planted_scene(family, 4, 0.0, 200)
        s, d = scene[0], scene[1]
        m = len(s)
        rng = np.random.Generator(np.random.PCG64(9))
        rows = rng.normal(size=(m, e.desc_dim))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        order = rng.permutation(m)                                                   # the train frame holds the rows in another order
        desc, xy = np.zeros((2, cap, e.desc_dim), np.float32), np.zeros((2, cap, 2), np.int32)
        desc[0, :m], xy[0, :m] = rows[order], d[order]                               # frame 0: the train view
        desc[1, :m], xy[1, :m] = rows, s                                             # frame 1: the query view
        plant(e, dict(desc=desc, xy=xy, counts=np.array([m, m])))
        e.bank_create(2, cap)
        assert e.bank_landmarks_reserve() > 0
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the landmarks are read
        match, _ = e.match_frames_async(2, key=None, pairing="previous", cross_check=True)
        fm, em, ni, mask = e.essential_frames_async(2, match, pairing="previous", K_query=KVEC, K_train=KVEC,
                                                    iterations=256, seed=5, reproj_threshold=THR)
        lin = e.pose_frames_async(2, match, fm, pairing="previous", K_query=KVEC, K_train=KVEC, reproj_threshold=THR)
        got = e.refine_pose_frames_async(2, match, lin[0], lin[1], pairing="previous", K_query=KVEC, K_train=KVEC,
                                         reproj_threshold=THR)
        e.bank_store(1, 0)                                                           # the query frame becomes slot 0 ...
        e.bank_store_landmarks(0, got[3][1], got[4][1])                              # ... with its refined landmarks
        lm = e.bank_landmarks()
        match, ni, mask, lm = e._host((match, ni, mask, lm))
        lin, got = e._host(lin), e._host(got)
        assert (match[1, :m] == np.argsort(order)).all() and ni[1] >= 0.95 * m and ni[0] == 0
        front = got[4][1].astype(bool)
        # (the refinement's members are the inliers whose midpoint reprojects within the threshold in BOTH views: a floor of
        # half the pairs says that the chain produced a map, the identities below say that it is the refined one)
        assert got[2][1] >= 0.5 * m and not front[m:].any() and not (front[:m] & ~mask[1, :m]).any()
        np.testing.assert_array_equal(lm[0, :, :3][front].view(np.uint32), got[3][1][front].view(np.uint32))
        np.testing.assert_array_equal(lm[0, :, 3] != 0, front)
        for name, (r, t) in (("linear", (lin[0][1], lin[1][1])), ("refined", (got[0][1], got[1][1]))):
            rot, direction = pose_errors(r, t, scene)
            print("%s chain, %s: rotation %.4f deg, direction %.4f deg" % (family, name, rot, direction))
            assert rot <= ROT_BAR and direction <= DIR_BAR, (family, name, rot, direction)
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused(qvga):
    import torch
    e, res = qvga
    lib = _lib.load()
    cap, dev = e.capacity, e.torch_device
    src = torch.zeros((N, cap, 2), dtype=torch.float32, device=dev)
    npairs = torch.full((N,), 10, dtype=torch.int32, device=dev)
    match = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    slot = torch.zeros((N,), dtype=torch.int32, device=dev)
    key_pts = e.keep_frame_points(0)
    one = torch.ones((1,), dtype=torch.int32, device=dev)
    fm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    em = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N,), 7, dtype=torch.int32, device=dev)
    mask = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp, np_, mp, kp, op, lp = (t.data_ptr() for t in (src, npairs, match, key_pts, one, slot))
    hp, ep, ip, kp_mask = fm.data_ptr(), em.data_ptr(), ni.data_ptr(), mask.data_ptr()

    def params(**kw):
        p = _lib.FpcEssentialParams()
        lib.fpc_default_essential_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rf = lambda n, s, d, c, stride, p, h, i: lib.fpc_ransac_essential(e._ctx, n, s, d, c, stride, p, h, ep, i, kp_mask)   # noqa: E731
    ff = lambda n, pairing, k, kc, m, p, h, i: lib.fpc_essential_frames(e._ctx, n, pairing, k, kc, m, p, h, ep, i, kp_mask)   # noqa: E731
    fb = lambda n, s, m, p, h, i: lib.fpc_essential_bank(e._ctx, n, s, m, p, h, ep, i, kp_mask)   # noqa: E731
    ok = params()
    e.bank_create(2, cap)
    try:
        bad = [params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
               params(reproj_threshold=float("nan")), params(refits=-1), params(refits=5), params(min_inliers=5),
               params(q_fx=0.0), params(t_fy=-1.0), params(q_cx=float("nan")), params(t_cy=float("inf")), None]
        for p in bad:
            assert rf(N, sp, sp, np_, cap, p, hp, ip) == FPC_E_INVALID
            assert ff(N, 0, kp, op, mp, p, hp, ip) == FPC_E_INVALID
            assert fb(N, lp, mp, p, hp, ip) == FPC_E_INVALID
        assert rf(N, None, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID
        assert rf(N, sp, None, np_, cap, ok, hp, ip) == FPC_E_INVALID
        assert rf(N, sp, sp, None, cap, ok, hp, ip) == FPC_E_INVALID
        assert rf(N, sp, sp, np_, cap, ok, None, ip) == FPC_E_INVALID
        assert rf(N, sp, sp, np_, cap, ok, hp, None) == FPC_E_INVALID
        assert rf(0, sp, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID
        assert rf(N + 1, sp, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID             # above max_batch
        assert rf(N, sp, sp, np_, cap + 1, ok, hp, ip) == FPC_E_INVALID             # stride above capacity
        assert rf(N, sp, sp, np_, 0, ok, hp, ip) == FPC_E_INVALID
        assert ff(N, 2, kp, op, mp, ok, hp, ip) == FPC_E_INVALID                     # pairing
        assert ff(N, 0, None, None, mp, ok, hp, ip) == FPC_E_INVALID                 # FPC_PAIR_KEY without key points
        assert ff(N, 0, kp, None, mp, ok, hp, ip) == FPC_E_INVALID                   # key points without their count
        assert ff(N, 0, kp, op, None, ok, hp, ip) == FPC_E_INVALID
        assert ff(N, 0, kp, op, mp, ok, None, ip) == FPC_E_INVALID
        assert ff(N, 0, kp, op, mp, ok, hp, None) == FPC_E_INVALID
        assert ff(0, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
        assert ff(N + 1, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
        assert fb(N, None, mp, ok, hp, ip) == FPC_E_INVALID
        assert fb(N, lp, None, ok, hp, ip) == FPC_E_INVALID
        assert fb(N, lp, mp, ok, None, ip) == FPC_E_INVALID
        assert fb(N, lp, mp, ok, hp, None) == FPC_E_INVALID
        assert fb(0, lp, mp, ok, hp, ip) == FPC_E_INVALID
        e.sync()
        # nothing was written by a refused call
        assert (fm == 7.0).all() and (em == 7.0).all() and (ni == 7).all() and (mask == 7).all()
        # min_inliers = 6 is accepted, and without a bank the bank variant is refused
        assert rf(N, sp, sp, np_, cap, params(min_inliers=6), hp, ip) == 0
        e.sync()
    finally:
        e.bank_destroy()
    assert fb(N, lp, mp, ok, hp, ip) == FPC_E_INVALID
    with pytest.raises(TypeError):
        e.ransac_essential(src, src, npairs, min_front=3)
    assert e.check_guards() == 0
