"""RANSAC fundamental matrices on the GPU (fpc_ransac_fundamental / fpc_fundamental_frames / fpc_fundamental_bank) against
the float64 restatement and the planted scenes of tests/test_fundamental_ransac.py: planted epipolar geometries with
outliers, the edge cases, the frames variant bit-identical to explicit pairs and the bank variant to the frames variant, a
known camera translation end to end, determinism and the argument checks.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_fundamental_ransac import (CASE_SETS, FRAME_H, FRAME_W, KEEP, KINDS, PARAMS, check_conditions, epipolar_rms,
                                           inliers_of, planted_scene, ransac_rule, restated_batch, sampson_distance)
from tests.test_gpu_homography_ransac import _host_pairs, _planted_maps, engine

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
THR = PARAMS["reproj_threshold"]
# RMS symmetric epipolar distance allowed over the restatement's on the same case.  The issue allows 0.25 px (fp32 scoring
# and FMA contraction may pick a different, equally good best sample) and asks for 2 x the measured worst difference if that
# is 10 x loose: measured on the MI355X, the device's RMS distance equals the restatement's to the four digits printed in
# all 42 cases (worst difference 0.0 px), and twice zero is no bar -- so the bar is the resolution of an fp32 F in this
# distance, 9 coefficients x 2^-24 x 640 px ~ 3.4e-4 px, rounded up (the homography test's MARGIN is the precedent).
MARGIN = 1e-3


@pytest.fixture(scope="module")
def vga():
    """A 32-frame VGA context without the descriptor head (explicit pairs need no network); max_keypoints = 1280 so that a
    pair list can cross the 1 024-record LDS chunk."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 32, descriptor_enabled=False, max_keypoints=1280)
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
    e = engine(conf_thresh=0.001)
    e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(300, N, H, W))
    assert min(len(r[0]) for r in res) > 1000
    yield e, res
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _pack(lists, stride):
    """[(src [m,2], dst [m,2])] -> the call's inputs (src, dst float32 [n,stride,2], npairs int32 [n])."""
    src, dst = np.zeros((len(lists), stride, 2), np.float32), np.zeros((len(lists), stride, 2), np.float32)
    for f, (s, d) in enumerate(lists):
        src[f, :len(s)], dst[f, :len(d)] = s, d
    return src, dst, np.array([len(s) for s, _ in lists], np.int32)


def _assert_mask_is_the_sampson_test(fm, mask, ni, s, d, thr=THR):
    """mask / ninliers are the float64 Sampson test of the RETURNED F (off the threshold's 1e-3 px neighbourhood), and
    nothing is set past the frame's pair count."""
    m = len(s)
    assert ni == mask.sum() and not mask[m:].any()
    f64 = fm.astype(np.float64)
    dist = sampson_distance(f64, s, d)
    clear = np.abs(dist - thr) > 1e-3
    np.testing.assert_array_equal(mask[:m][clear], (dist < thr)[clear])
    np.testing.assert_array_equal(mask[:m][clear], inliers_of(f64, s, d, thr)[clear])


def _assert_form(fm):
    """Norm 1 and the sign rule, on the fp32 values."""
    f64 = fm.astype(np.float64).reshape(-1)
    assert abs(np.sqrt((f64 * f64).sum()) - 1.0) < 1e-6 and f64[np.argmax(np.abs(f64))] > 0


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_planted_geometries(vga, rho, iterations):
    e = vga
    scenes, results = restated_batch(rho, iterations)
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], 640)
    assert len(set(npairs.tolist())) > 1
    fm, ni, mask = e.ransac_fundamental(src, dst, npairs, iterations=iterations, **PARAMS)
    worst = -np.inf
    for f, (scene, (rf, _)) in enumerate(zip(scenes, results)):
        s, d, planted, a, b = scene
        rms = check_conditions(fm[f].astype(np.float64), mask[f, :len(s)], scene, (KINDS[f], f, rho))
        rrms = epipolar_rms(rf, a[planted], b[planted])
        worst = max(worst, rms - rrms)
        print("rho %.1f frame %2d %-8s: RMS %.4f px, restatement %.4f px, inliers %d of %d planted" %
              (rho, f, KINDS[f], rms, rrms, ni[f], planted.sum()))
        assert rms <= rrms + MARGIN, (f, rms, rrms)
        _assert_form(fm[f])
        _assert_mask_is_the_sampson_test(fm[f], mask[f], ni[f], s, d)
    print("rho %.1f: worst (device - restatement) RMS symmetric epipolar distance %.3e px" % (rho, worst))


def test_edges(vga):
    e = vga
    cap = e.capacity
    s, d, _, a, b = planted_scene("general", 2, 0.0, cap)
    same = np.repeat(s[:1], 50, 0)
    lists = [(s[:0], d[:0]), (s[:7], d[:7]), (a[:8], b[:8]), (same, same), (s[:1100], d[:1100]), (s, d), (s[:100], d[:100])]
    src, dst, npairs = _pack(lists, cap)
    npairs[5] = cap + 9                                                              # above the stride: clamped
    params = dict(PARAMS, iterations=256)
    fm, ni, mask = e.ransac_fundamental(src, dst, npairs, **params)
    for f in (0, 1, 3):                                                              # too few pairs / every sample degenerate
        assert not fm[f].any() and ni[f] == 0 and not mask[f].any(), f
    assert ni[2] == 8 and mask[2, :8].all() and not mask[2, 8:].any() and fm[2].any()   # exactly 8 consistent pairs
    for f, m in ((4, 1100), (5, cap), (6, 100)):                                     # 4: the second LDS chunk
        assert ni[f] >= KEEP * m and fm[f].any(), (f, ni[f])
        _assert_form(fm[f])
        _assert_mask_is_the_sampson_test(fm[f], mask[f], ni[f], src[f, :m].astype(np.float64), dst[f, :m].astype(np.float64))
    assert mask[4, 1024:1100].sum() >= KEEP * 76                                     # the pairs behind the first chunk count
    # T = 1 and T = 257 (a partial last workgroup)
    one = e.ransac_fundamental(src, dst, npairs, **dict(params, iterations=1))
    assert one[0][6].any() and one[1][6] >= 8 and one[1][6] == one[2][6].sum()
    more = e.ransac_fundamental(src, dst, npairs, **dict(params, iterations=257))
    assert more[1][6] >= KEEP * 100 and more[1][4] >= KEEP * 1100
    # min_inliers above what one frame can reach fails that frame only
    fm2, ni2, mask2 = e.ransac_fundamental(src, dst, npairs, **dict(params, min_inliers=101))
    assert not fm2[6].any() and ni2[6] == 0 and not mask2[6].any()
    np.testing.assert_array_equal(fm2[[4, 5]].view(np.uint32), fm[[4, 5]].view(np.uint32))
    assert not fm2[2].any() and ni2[2] == 0
    # refits = 0: the best sample's own F, rank 2 all the same
    fm0, ni0, mask0 = e.ransac_fundamental(src, dst, npairs, **dict(params, refits=0))
    sv = np.linalg.svd(fm0[4].astype(np.float64), compute_uv=False)
    assert sv[2] / sv[0] <= 1e-6 and ni0[4] == mask0[4].sum() >= 8
    _assert_form(fm0[4])


def _assert_frames_equal_explicit(e, n, res, match_dev, key_pts, key_xy_host, pairing, **params):
    cap = e.capacity
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    got = e.fundamental_frames(n, match_dev, key_xy=key_pts, pairing=pairing, **params)
    empty = np.zeros((0, 2), np.int32)

    def train_of(f):
        if pairing == "previous" and f > 0:
            return xy[f - 1]
        return key_xy_host if key_xy_host is not None else empty
    src, dst, npairs, rows = _host_pairs(match_dev.cpu().numpy(), xy, counts, train_of, cap)
    fm, ni, mask = e.ransac_fundamental(src, dst, npairs, **params)
    np.testing.assert_array_equal(got[0].view(np.uint32), fm.view(np.uint32))
    np.testing.assert_array_equal(got[1], ni)
    for f in range(n):
        back = np.zeros(cap, bool)
        back[rows[f]] = mask[f, :npairs[f]]
        np.testing.assert_array_equal(got[2][f], back)
    return got, npairs


def test_frames_variant_is_bit_identical_to_explicit_pairs(qvga):
    e, res = qvga
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    params = dict(iterations=256, seed=11)
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "key", **params)
    assert npairs.min() > 50 and (got[1] >= 8).any()
    m, _ = e.match_frames_async(N, key=key, pairing="previous", cross_check=True)
    got, _ = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "previous", **params)
    assert (got[1] >= 8).any()
    m, _ = e.match_frames_async(N, key=None, pairing="previous", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, None, None, "previous", **params)
    assert npairs[0] == 0 and not got[0][0].any() and got[1][0] == 0 and not got[2][0].any()   # frame 0 has no train set


def test_bank_variant_is_bit_identical_to_the_frames_variant(qvga):
    e, res = qvga
    slots = 3
    e.bank_create(slots, e.capacity)
    try:
        for s in range(slots):
            e.bank_store(s + 1, s)
        e.detect(synth.make_batch(400, N, H, W))                                     # another batch against the stored frames
        _, best, m, _ = e.match_bank_async(N, cross_check=True, max_dist=0.9)
        slot = best.clone()
        slot[1], slot[4] = -1, slots
        params = dict(iterations=256, seed=4)
        fm, ni, mask = e.fundamental_bank(N, slot, m, **params)
        sl = slot.cpu().numpy()
        assert not fm[[1, 4]].any() and not ni[[1, 4]].any() and not mask[[1, 4]].any()    # no slot: the frame fails
        assert set(sl.tolist()) - {-1, slots} and (ni >= 8).any()
        _, bx, bc = e.bank_view()
        for s in sorted(set(sl.tolist()) - {-1, slots}):
            rows_of = np.flatnonzero(sl == s)
            rf, rn, rm = e.fundamental_frames(N, m, key_xy=(bx[s].clone(), bc[s:s + 1].clone()), pairing="key", **params)
            np.testing.assert_array_equal(fm.view(np.uint32)[rows_of], rf.view(np.uint32)[rows_of])
            np.testing.assert_array_equal(ni[rows_of], rn[rows_of])
            np.testing.assert_array_equal(mask[rows_of], rm[rows_of])
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_known_camera_translation_end_to_end():
    """A known motion through keypoints -> descriptors -> match_frames(key = frame 0, cross check, ratio 0.8) ->
    fundamental_frames, all on the device.  As in test_gpu_homography_ransac's end-to-end test the views are cropped from
    one larger probability map and descriptor map (the network's outputs) and run through fpc_get_points.  An image shift
    alone is a homography: its pairs leave every 8-point system at rank 6, which the rule calls degenerate.  So the views
    are those of a camera translated SIDEWAYS in front of a scene of two depths: the upper half of the frame shifts by one
    multiple of 8 px, the lower half by another, both along x.  Two depths pin F = [(1, 0, 0)]x; the planted
    correspondence of a query pixel (x, y) is (x + d(y), y)."""
    import torch
    shifts = [(0, 0), (8, 24), (16, 40), (24, 8), (32, 16), (40, 56), (48, 24), (56, 32)]   # (upper, lower) per view
    prob, desc = _planted_maps()
    half = H // 2
    probs = np.stack([np.concatenate([prob[:half, a:a + W], prob[half:H, b:b + W]]) for a, b in shifts])
    descs = np.stack([np.concatenate([desc[:, :half // 8, a // 8:a // 8 + W // 8],
                                      desc[:, half // 8:H // 8, b // 8:b // 8 + W // 8]], 1) for a, b in shifts])
    e = engine()
    try:
        res = e.get_points(torch.from_numpy(probs), torch.from_numpy(np.ascontiguousarray(descs)))
        assert min(len(r[0]) for r in res) > 500
        key, key_pts = e.keep_frame(0), e.keep_frame_points(0)
        m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True, ratio=0.8)
        fm, ni, mask = e.fundamental_frames_async(N, m, key_xy=key_pts, pairing="key", iterations=256, seed=3)
        e.sync()
        fm, ni, mask, m = fm.cpu().numpy().astype(np.float64), ni.cpu().numpy(), mask.cpu().numpy(), m.cpu().numpy()
        for f, (a, b) in enumerate(shifts):
            if f == 0:
                continue                                                             # the key against itself: a homography
            xy = res[f][0].astype(np.float64)
            matched = int((m[f, :len(xy)] >= 0).sum())
            planted = xy + np.stack([np.where(xy[:, 1] < half, a, b), np.zeros(len(xy))], 1)
            dist = sampson_distance(fm[f], xy, planted)
            print("shifts (%d, %d): %d matched rows, %d inliers, worst planted Sampson distance %.3e px" %
                  (a, b, matched, ni[f], dist.max()))
            assert matched > 200 and ni[f] >= 0.9 * matched, (f, matched, ni[f])
            assert ni[f] == mask[f].sum()
            assert dist.max() < 3.0, (f, dist.max())
        assert e.check_guards() == 0
    finally:
        e.close()


def test_determinism_and_a_following_detect(qvga, vga):
    import torch
    e, res = qvga
    scenes, _ = restated_batch(*CASE_SETS[0])
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], 640)
    a = vga.ransac_fundamental(src, dst, npairs, iterations=256, seed=5)
    b = vga.ransac_fundamental(src, dst, npairs, iterations=256, seed=5)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    assert a[0].any(axis=(1, 2)).all()
    assert vga.check_guards() == 0
    # enqueued between a match and the next detect, the stage leaves that detect alone
    frames = torch.from_numpy(synth.make_batch(300, N, H, W)).to(e.torch_device).contiguous()
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    torch.cuda.synchronize()
    m, _ = e.match_frames_async(N, key=key)
    f1 = e.fundamental_frames_async(N, m, key_xy=key_pts, iterations=256, seed=1)
    e.detect_async(frames, N)
    m2, _ = e.match_frames_async(N, key=key)
    f2 = e.fundamental_frames_async(N, m2, key_xy=key_pts, iterations=256, seed=1)
    e.sync()
    again = e.fetch(N)
    for r0, r1 in zip(res, again):
        np.testing.assert_array_equal(r0[0], r1[0])
        np.testing.assert_array_equal(r0[1], r1[1])
        np.testing.assert_array_equal(r0[2], r1[2])
    for x, y in zip(f1, f2):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert e.check_guards() == 0


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
    ni = torch.full((N,), 7, dtype=torch.int32, device=dev)
    mask = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp, np_, mp, kp, op, lp = (t.data_ptr() for t in (src, npairs, match, key_pts, one, slot))
    hp, ip, kp_mask = fm.data_ptr(), ni.data_ptr(), mask.data_ptr()

    def params(**kw):
        p = _lib.FpcRansacParams()
        lib.fpc_default_ransac_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rf = lambda n, s, d, c, stride, p, h, i: lib.fpc_ransac_fundamental(e._ctx, n, s, d, c, stride, p, h, i, kp_mask)   # noqa: E731
    ff = lambda n, pairing, k, kc, m, p, h, i: lib.fpc_fundamental_frames(e._ctx, n, pairing, k, kc, m, p, h, i, kp_mask)   # noqa: E731
    fb = lambda n, s, m, p, h, i: lib.fpc_fundamental_bank(e._ctx, n, s, m, p, h, i, kp_mask)   # noqa: E731
    ok = params()
    e.bank_create(2, cap)
    try:
        bad = [params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
               params(reproj_threshold=float("nan")), params(refits=-1), params(refits=5), params(min_inliers=3),
               params(min_inliers=7), None]
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
        assert fb(N + 1, lp, mp, ok, hp, ip) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert ff(3, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
        assert fb(3, lp, mp, ok, hp, ip) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        assert (fm.cpu() == 7.0).all() and (ni.cpu() == 7).all() and (mask.cpu() == 7).all()
        assert ff(2, 0, kp, op, mp, ok, hp, ip) == 0
        assert ff(2, 1, None, None, mp, ok, hp, ip) == 0                             # PREVIOUS needs no key
        assert fb(2, lp, mp, ok, hp, ip) == 0
        assert rf(N, sp, sp, np_, cap, ok, hp, ip) == 0
        e.sync()
        assert not fm.cpu().numpy().any() and not ni.cpu().numpy().any() and not mask.cpu().numpy().any()   # no pairs: failed
    finally:
        e.bank_destroy()
    assert fb(2, lp, mp, ok, hp, ip) == FPC_E_INVALID                                # no bank
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))                                        # (the module's later tests see batch 1 again)
    with pytest.raises(ValueError):
        e.fundamental_frames(N, match, key_xy=key_pts, pairing="next")
    with pytest.raises(TypeError):
        e.ransac_fundamental(src, src, npairs, iteration=5)
    with pytest.raises(ValueError):
        e.fundamental_bank(N, slot, match)
