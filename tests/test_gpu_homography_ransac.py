"""RANSAC homographies on the GPU (fpc_ransac_homography / fpc_homography_frames) against the float64 restatement and the
planted truth of tests/test_homography_ransac.py: planted homographies with outliers, the frames variant bit-identical to
explicit pairs, a known translation end to end, the edge cases, determinism and the argument checks.  Every context runs
under the canary zones.  Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_homography_ransac import (CASE_NAMES, CASE_SETS, FRAME_H, FRAME_W, corner_error, inliers_of, planted_case,
                                          project, ransac_rule)

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
# 4-corner error allowed over the restatement's on the same case.  The issue allows 0.5 px (fp32 scoring may pick a
# different, equally good best sample) and asks for 2 x the measured worst difference if that is 10 x loose: measured on
# the MI355X, the device's H equals the restatement's after rounding to fp32 in all 96 cases (difference 0.0 px), and
# twice zero is no bar -- so the bar is the resolution of an fp32 H at the corners, 9 coefficients x 2^-24 x 640 px
# ~ 3.4e-4 px, rounded up.
MARGIN = 1e-3


def engine(h=H, w=W, b=N, **kw):
    from fpc_amd.engine import Engine
    kw.setdefault("plan_flags", ["guard_zones"])
    return Engine(h, w, max_batch=b, **kw)


@pytest.fixture(scope="module")
def vga():
    """A 32-frame VGA context without the descriptor head: explicit pairs need no network."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 32, descriptor_enabled=False, max_keypoints=1024)
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


def _batch(rho, stride):
    """The 32 planted cases of one outlier share as one call's inputs; frame f keeps 600 - 7 * (f % 5) pairs."""
    cases = [planted_case(name, i, rho, 600 - 7 * (f % 5)) for f, (name, i) in enumerate(CASE_NAMES)]
    src, dst = np.zeros((32, stride, 2), np.float32), np.zeros((32, stride, 2), np.float32)
    for f, (_, s, d, _) in enumerate(cases):
        src[f, :len(s)], dst[f, :len(d)] = s, d
    return cases, src, dst, np.array([len(c[1]) for c in cases], np.int32)


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_planted_homographies(vga, rho, iterations):
    e = vga
    cases, src, dst, npairs = _batch(rho, 640)
    assert len(set(npairs.tolist())) > 1
    params = dict(iterations=iterations, reproj_threshold=3.0, seed=7, refits=2)
    hm, ni, mask = e.ransac_homography(src, dst, npairs, **params)
    worst = -np.inf
    for f, (truth, s, d, planted) in enumerate(cases):
        rh, _ = ransac_rule(s, d, params, f)
        err, rerr = corner_error(hm[f].astype(np.float64), truth), corner_error(rh, truth)
        worst = max(worst, err - rerr)
        print("rho %.1f frame %2d: 4-corner error %.4f px, restatement %.4f px, inliers %d" % (rho, f, err, rerr, ni[f]))
        assert err <= rerr + MARGIN, (f, err, rerr)
        m = len(s)
        assert hm[f, 2, 2] == 1.0 and ni[f] == mask[f].sum() and not mask[f, m:].any()
        assert mask[f, :m][planted].all()
        # the mask is the plain reprojection test of the RETURNED H
        h64 = hm[f].astype(np.float64)
        dist = np.sqrt(((project(h64, s) - d) ** 2).sum(1))
        clear = np.abs(dist - 3.0) > 1e-3
        np.testing.assert_array_equal(mask[f, :m][clear], (dist < 3.0)[clear])
        np.testing.assert_array_equal(mask[f, :m][clear], inliers_of(h64, s, d, 3.0)[clear])
    print("rho %.1f: worst (device - restatement) 4-corner error %.3e px" % (rho, worst))


def _host_pairs(match, xy, counts, train_of, cap):
    """The frames variant's pair lists, gathered on the host: per frame rows i < count with a match, ascending."""
    n = len(counts)
    src, dst = np.zeros((n, cap, 2), np.float32), np.zeros((n, cap, 2), np.float32)
    npairs, rows = np.zeros(n, np.int32), []
    for f in range(n):
        t = train_of(f)
        m = match[f, :counts[f]]
        i = np.flatnonzero((m >= 0) & (m < len(t)))
        src[f, :len(i)], dst[f, :len(i)] = xy[f][i], t[m[i]] if len(i) else 0
        npairs[f] = len(i)
        rows.append(i)
    return src, dst, npairs, rows


def _assert_frames_equal_explicit(e, n, res, match_dev, key_pts, key_xy_host, pairing, **params):
    cap = e.capacity
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    got = e.homography_frames(n, match_dev, key_xy=key_pts, pairing=pairing, **params)
    empty = np.zeros((0, 2), np.int32)

    def train_of(f):
        if pairing == "previous" and f > 0:
            return xy[f - 1]
        return key_xy_host if key_xy_host is not None else empty
    src, dst, npairs, rows = _host_pairs(match_dev.cpu().numpy(), xy, counts, train_of, cap)
    hm, ni, mask = e.ransac_homography(src, dst, npairs, **params)
    np.testing.assert_array_equal(got[0].view(np.uint32), hm.view(np.uint32))
    np.testing.assert_array_equal(got[1], ni)
    for f in range(n):
        back = np.zeros(cap, bool)
        back[rows[f]] = mask[f, :npairs[f]]
        np.testing.assert_array_equal(got[2][f], back)
    return got, npairs


def test_frames_variant_is_bit_identical_to_explicit_pairs(qvga):
    e, res = qvga
    key = e.keep_frame(5)
    key_pts = e.keep_frame_points(5)
    assert tuple(key_pts.shape) == (e.capacity, 2)
    np.testing.assert_array_equal(key_pts[:len(res[5][0])].cpu().numpy(), res[5][0])
    params = dict(iterations=256, seed=11, min_inliers=4)
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "key", **params)
    assert npairs.min() > 50
    h5 = got[0][5]                                                                   # frame 5 against itself: the identity
    assert got[1][5] == npairs[5] and np.abs(h5 - np.eye(3)).max() < 1e-4
    m, _ = e.match_frames_async(N, key=key, pairing="previous", cross_check=True)
    _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "previous", **params)
    m, _ = e.match_frames_async(N, key=None, pairing="previous", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, None, None, "previous", **params)
    assert npairs[0] == 0 and not got[0][0].any() and got[1][0] == 0 and not got[2][0].any()   # frame 0 has no train set
    # the (xy, count) form of the key
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    a = e.homography_frames(N, m, key_xy=(key_pts, key[1]), **params)
    b = e.homography_frames(N, m, key_xy=key_pts, **params)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_frames_variant_on_the_vgg_network():
    e = engine(in_channels=1, arch="vgg")
    e.load_state_dict(synth.make_vgg_state_dict(4, 3.0))
    frames = synth.make_batch(300, N, H, W, gray=True)[:, :1]
    try:
        res = e.detect(np.ascontiguousarray(frames))
        assert e.desc_dim == 256 and sum(len(r[0]) for r in res) > 100
        key, key_pts = e.keep_frame(1), e.keep_frame_points(1)
        for pairing in ("key", "previous"):
            m, _ = e.match_frames_async(N, key=key, pairing=pairing, cross_check=True)
            _assert_frames_equal_explicit(e, N, res, m, key_pts, res[1][0], pairing, iterations=128, seed=2, min_inliers=4)
        assert e.check_guards() == 0
    finally:
        e.close()


def _planted_maps():
    """One larger probability map (1 500 isolated peaks) and descriptor map (unit normal) to crop 240 x 320 views from."""
    rng = np.random.Generator(np.random.PCG64(77))
    prob = np.zeros((H + 64, W + 64), np.float32)
    ys, xs = rng.integers(0, H + 64, 1500), rng.integers(0, W + 64, 1500)
    prob[ys, xs] = rng.uniform(0.1, 1.0, 1500).astype(np.float32)
    return prob, rng.normal(size=(128, (H + 64) // 8, (W + 64) // 8)).astype(np.float32)


def test_known_translation_end_to_end():
    """A known motion through keypoints -> descriptors -> match_frames(key = frame 0, cross check, ratio 0.8) ->
    homography_frames, all on the device: eight 240 x 320 views cropped at offsets that are multiples of 8 px (the
    network's stride) must give the translation with a 4-corner error <= 1 px and ninliers >= min_inliers.

    The premise was checked on the CPU first (the oracle's detect, the float64 matcher and restatement, T = 256, seed 3):
     - views cropped from one 304 x 384 synthetic IMAGE and run through the network do NOT satisfy it with the synthetic
       checkpoints this repository can make (random weights): at offset (8, 0) the restatement finds 700 inliers of the
       IDENTITY (4-corner error 8.03 px), at (32, 24) 19 inliers and 41.6 px, at (64, 64) 9 inliers and 90.5 px; with a
       noise texture blended into the image 105 inliers of the identity at (8, 0).  A random network's descriptors follow
       the position in the frame (its zero padding), not the content.  The device agrees with the restatement there
       (700 inliers, 8.05 px), so that variant would test the checkpoint, not this stage;
     - views cropped from one larger probability map and descriptor map (the network's OUTPUTS, which a trained network
       translates with the image) and run through fpc_get_points satisfy it: the restatement alone is within 1.3e-13 px
       at every offset below, with 280 .. 597 inliers.  That is what this test runs."""
    import torch
    offsets = [(0, 0), (8, 0), (16, 8), (32, 24), (56, 48), (64, 64), (24, 40), (48, 16)]
    prob, desc = _planted_maps()
    probs = np.stack([prob[oy:oy + H, ox:ox + W] for ox, oy in offsets])
    descs = np.stack([desc[:, oy // 8:oy // 8 + H // 8, ox // 8:ox // 8 + W // 8] for ox, oy in offsets])
    e = engine()
    try:
        res = e.get_points(torch.from_numpy(probs), torch.from_numpy(np.ascontiguousarray(descs)))
        assert min(len(r[0]) for r in res) > 500
        key, key_pts = e.keep_frame(0), e.keep_frame_points(0)
        m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True, ratio=0.8)
        hm, ni, mask = e.homography_frames_async(N, m, key_xy=key_pts, pairing="key", iterations=256, seed=3)
        e.sync()
        hm, ni = hm.cpu().numpy().astype(np.float64), ni.cpu().numpy()
        corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
        for f, (ox, oy) in enumerate(offsets):
            err = np.sqrt(((project(hm[f], corners) - (corners + [ox, oy])) ** 2).sum(1)).max()
            print("offset (%d, %d): %d inliers, 4-corner error %.3e px" % (ox, oy, ni[f], err))
            assert ni[f] >= 8, (f, ni[f])
            assert err <= 1.0, (f, err)
        assert ni[0] == len(res[0][0]) and ni.min() > 200
        assert e.check_guards() == 0
    finally:
        e.close()


def test_edges(vga):
    import torch
    e = vga
    cap = e.capacity
    truth, s, d, _ = planted_case("defaults", 3, 0.0, cap)
    src, dst = np.zeros((8, cap, 2), np.float32), np.zeros((8, cap, 2), np.float32)
    src[:], dst[:] = s, d
    src[4], dst[4] = s[0], s[0]                                                     # frame 4: all pairs identical
    npairs = np.array([0, 3, 4, cap, cap, 100, -5, cap + 9], np.int32)
    hm, ni, mask = e.ransac_homography(src, dst, npairs, iterations=256, seed=1, min_inliers=4)
    for f in (0, 1, 4, 6):                                                           # too few pairs / degenerate: failed
        assert not hm[f].any() and ni[f] == 0 and not mask[f].any(), f
    assert ni[2] == 4 and mask[2, :4].all() and not mask[2, 4:].any() and hm[2, 2, 2] == 1.0
    for f in (3, 7):                                                                 # npairs == stride == cap (7: clamped)
        assert ni[f] == cap and mask[f].all() and corner_error(hm[f].astype(np.float64), truth) < 1.0
    assert ni[5] == 100 and mask[5, :100].all() and not mask[5, 100:].any()
    # min_inliers above what the frame can reach
    hm2, ni2, mask2 = e.ransac_homography(src, dst, npairs, iterations=256, seed=1, min_inliers=101)
    assert not hm2[5].any() and ni2[5] == 0 and not mask2[5].any() and ni2[3] == cap
    # refits = 0: the best sample's own H
    hm0, ni0, mask0 = e.ransac_homography(src, dst, npairs, iterations=256, seed=1, min_inliers=4, refits=0)
    assert hm0[3, 2, 2] == 1.0 and ni0[3] == mask0[3].sum() >= 4 and corner_error(hm0[3].astype(np.float64), truth) < 20
    rh, rinl = ransac_rule(s, d, dict(iterations=256, seed=1, min_inliers=4, refits=0), 3)
    assert abs(int(ni0[3]) - int(rinl.sum())) <= cap // 20
    # inlier_dev = NULL
    lib = _lib.load()
    p = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(p))
    p.iterations, p.seed, p.min_inliers = 256, 1, 4
    sd_, dd_ = torch.from_numpy(src).to(e.torch_device), torch.from_numpy(dst).to(e.torch_device)
    nd = torch.from_numpy(npairs).to(e.torch_device)
    ho = torch.empty((8, 9), dtype=torch.float32, device=e.torch_device)
    no = torch.empty((8,), dtype=torch.int32, device=e.torch_device)
    torch.cuda.synchronize()
    assert lib.fpc_ransac_homography(e._ctx, 8, sd_.data_ptr(), dd_.data_ptr(), nd.data_ptr(), cap, ctypes.byref(p),
                                     ho.data_ptr(), no.data_ptr(), None) == 0
    e.sync()
    np.testing.assert_array_equal(ho.cpu().numpy().view(np.uint32).reshape(8, 3, 3), hm.view(np.uint32))
    np.testing.assert_array_equal(no.cpu().numpy(), ni)
    # the counts are read on the device: changed between two calls with no host synchronisation in between
    a = e.ransac_homography_async(sd_, dd_, nd, iterations=256, seed=1, min_inliers=4)
    with torch.cuda.stream(e.torch_stream()):
        nd.fill_(3)
    b = e.ransac_homography_async(sd_, dd_, nd, iterations=256, seed=1, min_inliers=4)
    with torch.cuda.stream(e.torch_stream()):
        nd.fill_(200)
    c = e.ransac_homography_async(sd_, dd_, nd, iterations=256, seed=1, min_inliers=4)
    e.sync()
    np.testing.assert_array_equal(a[1].cpu().numpy(), ni)
    assert not b[0].cpu().numpy().any() and not b[1].cpu().numpy().any() and not b[2].cpu().numpy().any()
    nc = c[1].cpu().numpy()
    assert nc[4] == 0 and (np.delete(nc, 4) == 200).all()


def test_frames_edges(qvga):
    import torch
    e, res = qvga
    cap = e.capacity
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    zero = torch.zeros((1,), dtype=torch.int32, device=e.torch_device)
    hm, ni, mask = e.homography_frames(N, m, key_xy=(key_pts, zero), iterations=64)   # nkey = 0: no row is a pair
    assert not hm.any() and not ni.any() and not mask.any()
    none = torch.full((N, cap), -1, dtype=torch.int32, device=e.torch_device)        # all matches -1
    hm, ni, mask = e.homography_frames(N, none, key_xy=key_pts, iterations=64)
    assert not hm.any() and not ni.any() and not mask.any()
    wild = torch.full((N, cap), 2 ** 30, dtype=torch.int32, device=e.torch_device)    # indices outside the train set
    hm, ni, mask = e.homography_frames(N, wild, key_xy=key_pts, iterations=64)
    assert not hm.any() and not ni.any() and not mask.any()


def test_determinism_and_a_following_detect(qvga, vga):
    import torch
    e, res = qvga
    cases, src, dst, npairs = _batch(0.0, 640)
    a = vga.ransac_homography(src, dst, npairs, iterations=256, seed=5)
    b = vga.ransac_homography(src, dst, npairs, iterations=256, seed=5)
    c = vga.ransac_homography(src, dst, npairs, iterations=256, seed=6)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[2], c[2])                       # another seed: the same inlier SETS on clean cases
    assert (a[1] == npairs).all()
    # enqueued between a match and the next detect, the stage leaves that detect alone
    frames = torch.from_numpy(synth.make_batch(300, N, H, W)).to(e.torch_device).contiguous()
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    torch.cuda.synchronize()
    m, _ = e.match_frames_async(N, key=key)
    h1 = e.homography_frames_async(N, m, key_xy=key_pts, iterations=256, seed=1)
    e.detect_async(frames, N)
    m2, _ = e.match_frames_async(N, key=key)
    h2 = e.homography_frames_async(N, m2, key_xy=key_pts, iterations=256, seed=1)
    e.sync()
    again = e.fetch(N)
    for r0, r1 in zip(res, again):
        np.testing.assert_array_equal(r0[0], r1[0])
        np.testing.assert_array_equal(r0[1], r1[1])
        np.testing.assert_array_equal(r0[2], r1[2])
    for x, y in zip(h1, h2):
        np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy())


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
    hm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N,), 7, dtype=torch.int32, device=dev)
    mask = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp, np_, mp, kp, op = src.data_ptr(), npairs.data_ptr(), match.data_ptr(), key_pts.data_ptr(), one.data_ptr()
    hp, ip, kp_mask, lp = hm.data_ptr(), ni.data_ptr(), mask.data_ptr(), slot.data_ptr()

    def params(**kw):
        p = _lib.FpcRansacParams()
        lib.fpc_default_ransac_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    rh = lambda n, s, d, c, stride, p, h, i: lib.fpc_ransac_homography(e._ctx, n, s, d, c, stride, p, h, i, kp_mask)   # noqa: E731
    hf = lambda n, pairing, k, kc, m, p, h, i: lib.fpc_homography_frames(e._ctx, n, pairing, k, kc, m, p, h, i, kp_mask)   # noqa: E731
    hb = lambda n, s, m, p, h, i: lib.fpc_homography_bank(e._ctx, n, s, m, p, h, i, kp_mask)   # noqa: E731
    ok = params()
    bad = [params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0), params(reproj_threshold=-1.0),
           params(reproj_threshold=float("nan")), params(refits=-1), params(refits=5), params(min_inliers=3), None]
    for p in bad:
        assert rh(N, sp, sp, np_, cap, p, hp, ip) == FPC_E_INVALID
        assert hf(N, 0, kp, op, mp, p, hp, ip) == FPC_E_INVALID
    assert rh(N, None, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID
    assert rh(N, sp, None, np_, cap, ok, hp, ip) == FPC_E_INVALID
    assert rh(N, sp, sp, None, cap, ok, hp, ip) == FPC_E_INVALID
    assert rh(N, sp, sp, np_, cap, ok, None, ip) == FPC_E_INVALID
    assert rh(N, sp, sp, np_, cap, ok, hp, None) == FPC_E_INVALID
    assert rh(0, sp, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID
    assert rh(N + 1, sp, sp, np_, cap, ok, hp, ip) == FPC_E_INVALID                 # above max_batch
    assert rh(N, sp, sp, np_, cap + 1, ok, hp, ip) == FPC_E_INVALID                 # stride above capacity
    assert rh(N, sp, sp, np_, 0, ok, hp, ip) == FPC_E_INVALID
    assert hf(N, 2, kp, op, mp, ok, hp, ip) == FPC_E_INVALID                         # pairing
    assert hf(N, 0, None, None, mp, ok, hp, ip) == FPC_E_INVALID                     # FPC_PAIR_KEY without key points
    assert hf(N, 0, kp, None, mp, ok, hp, ip) == FPC_E_INVALID                       # key points without their count
    assert hf(N, 0, kp, op, None, ok, hp, ip) == FPC_E_INVALID
    assert hf(N, 0, kp, op, mp, ok, None, ip) == FPC_E_INVALID
    assert hf(N, 0, kp, op, mp, ok, hp, None) == FPC_E_INVALID
    assert hf(0, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
    assert hf(N + 1, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
    assert hb(N, lp, mp, ok, hp, ip) == FPC_E_INVALID                               # no bank
    e.bank_create(2, cap)
    try:
        for p in bad:
            assert hb(N, lp, mp, p, hp, ip) == FPC_E_INVALID
        assert hb(N, None, mp, ok, hp, ip) == FPC_E_INVALID
        assert hb(N, lp, None, ok, hp, ip) == FPC_E_INVALID
        assert hb(N, lp, mp, ok, None, ip) == FPC_E_INVALID
        assert hb(N, lp, mp, ok, hp, None) == FPC_E_INVALID
        assert hb(0, lp, mp, ok, hp, ip) == FPC_E_INVALID
        assert hb(N + 1, lp, mp, ok, hp, ip) == FPC_E_INVALID
    finally:
        e.bank_destroy()
    e.sync()
    e.detect(synth.make_batch(300, 2, H, W))                                        # a detect of fewer frames bounds n
    assert hf(3, 0, kp, op, mp, ok, hp, ip) == FPC_E_INVALID
    e.sync()
    # nothing was written by any refused call
    assert (hm.cpu() == 7.0).all() and (ni.cpu() == 7).all() and (mask.cpu() == 7).all()
    assert hf(2, 0, kp, op, mp, ok, hp, ip) == 0
    assert hf(2, 1, None, None, mp, ok, hp, ip) == 0                                 # PREVIOUS needs no key
    assert rh(N, sp, sp, np_, cap, ok, hp, ip) == 0
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))                                        # (the module's later tests see batch 1 again)
    # a context that has not produced keypoints yet
    d = engine(descriptor_enabled=False, b=2)
    try:
        assert lib.fpc_homography_frames(d._ctx, 1, 1, None, None, mp, ok, hp, ip, None) == FPC_E_INVALID
        assert d.check_guards() == 0
    finally:
        d.close()
    with pytest.raises(ValueError):
        e.homography_frames(N, match, key_xy=key_pts, pairing="next")
    with pytest.raises(TypeError):
        e.ransac_homography(src, src, npairs, iteration=5)


def test_batch_helper_returns_inlier_correspondences(qvga):
    from fpc_amd.inference import estimate_homographies_batch
    e, res = qvga
    xy, conf, desc, _ = res[5]
    stop = np.hstack((xy.astype(np.float64), conf[:, None].astype(np.float64), desc))
    out = estimate_homographies_batch(e, N, stop, iterations=256, seed=11, min_inliers=4)
    assert len(out) == N
    hm, rows, idx = out[5]
    assert np.abs(hm - np.eye(3)).max() < 1e-4 and len(rows) == len(idx) > 50
    np.testing.assert_array_equal(rows[:, :2], stop[idx, :2])                       # frame 5 against itself
    for hm, rows, idx in out:
        assert hm.shape == (3, 3) and rows.shape[1] == 3 + e.desc_dim and len(rows) == len(idx)
        if len(idx):
            assert inliers_of(hm.astype(np.float64), rows[:, :2], stop[idx, :2], 3.0 + 1e-3).all()
