"""Sim(3) alignment on the GPU (fpc_ransac_sim3 / fpc_sim3_frames / fpc_sim3_bank) against the float64 restatement and the
planted scenes of tests/test_sim3_ransac.py: planted similarities with outliers, the tails of the pair list and of the
hypothesis grid, the frames variant bit-identical to explicit pairs and the bank variant to the frames variant (on banks of
both formats), the loop-closing chain end to end (a frame localised against one slot and given landmarks of its own is
aligned with a second slot that holds the same scene at 1 / 1.7 of the scale: s comes back as 1.7), determinism, the workspace
shared with the PnP calls and the argument checks.  Every context runs under the canary zones.  The match tables of the
frames and bank identity tests are planted (as in test_gpu_pnp_ransac.py); the end-to-end test plants keypoints and
descriptors in place of the last detect's and takes its tables from fpc_match_bank.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_gpu_homography_ransac import engine
from tests.test_pnp_ransac import planted_scene as pnp_scene
from tests.test_sim3_ransac import (CASE_SETS, FRAME_H, FRAME_W, KVEC, NEAR_CAP, PARAMS, ROT_BAR, SCALE_BAR, TRANS_BAR, _rotation,
                                    check_planted, inliers_of, near_threshold, planted_scene, restated_batch, sim3_errors,
                                    sim3_rule)

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
THR = PARAMS["reproj_threshold"]
THREADS = 256                                                        # hypotheses per workgroup of sim3_score_kernel
KQVGA = (250.0, 250.0, 160.0, 120.0)
SIGMA = 1.7                                                          # the end-to-end chain's scale ratio
# Device against restatement where both picked the same best sample (identical masks): both evaluate the triad and Horn's
# refit in fp64 and differ by the contraction of a * b + c into one rounding (the refit's sums and the quaternion; the triad
# is compiled without contraction), so what is left is the fp32 rounding of the outputs.  Measured on the MI355X over the 26
# frames of the three case sets (all 26 with the restatement's mask, none with another best sample): worst difference 0.0 in
# s, in every entry of R and in t -- the same fp32 values.  Ten times zero is no bar, so the bars are the resolution of the
# outputs' fp32 format, rounded up as test_gpu_pnp_ransac.py's are: entries of R are <= 1 (resolution 6e-8), s and
# |dt| / |t| resolve 1.2e-7.
S_SAME_BAR, R_SAME_BAR, T_SAME_BAR = 1e-6, 1e-6, 1e-6               # |ds| / s; per entry of R; |dt| / |t|
DIFFERENT_CAP = 0.25                                                 # share of frames that may pick another best sample


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
    """[(q [m,3], p [m,3])] -> the call's inputs (q float32 [n,stride,3], p float32 [n,stride,3], npairs int32 [n])."""
    q, p = np.zeros((len(lists), stride, 3), np.float32), np.zeros((len(lists), stride, 3), np.float32)
    for f, (a, b) in enumerate(lists):
        q[f, :len(a)], p[f, :len(b)] = a, b
    return q, p, np.array([len(a) for a, _ in lists], np.int32)


def _model(s, rm, tv):
    return float(s), rm.astype(np.float64), tv.astype(np.float64)


def _assert_mask_is_the_inlier_test(s, rm, tv, mask, ni, q, p, kq=KVEC, kt=KVEC, thr=THR):
    """mask / ninliers are the float64 test of the RETURNED model (off the threshold's 1e-3 px neighbourhood), nothing is set
    past the frame's pair count, and the neighbourhood holds at most NEAR_CAP of the pairs."""
    m = len(q)
    mask = mask.astype(bool)
    assert ni == mask.sum() and not mask[m:].any()
    q, p = q.astype(np.float64), p.astype(np.float64)
    near = near_threshold(_model(s, rm, tv), q, p, kq, kt, thr)
    assert near.sum() <= NEAR_CAP * m, (near.sum(), m)
    np.testing.assert_array_equal(mask[:m][~near], inliers_of(_model(s, rm, tv), q, p, kq, kt, thr)[~near])


_DEVICE = {}


def _device_batch(e, rho, iterations):
    """The device's models of one case set, computed once."""
    if (rho, iterations) not in _DEVICE:
        scenes, _ = restated_batch(rho, iterations)
        q, p, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
        assert len(set(npairs.tolist())) > 1
        _DEVICE[rho, iterations] = e.ransac_sim3(q, p, npairs, iterations=iterations, **PARAMS)
    return _DEVICE[rho, iterations]


@pytest.mark.parametrize("rho,iterations", CASE_SETS)
def test_device_against_the_restatement(vga, rho, iterations):
    scenes, results = restated_batch(rho, iterations)
    sv, rm, tv, ni, mask = _device_batch(vga, rho, iterations)
    worst, same = np.zeros(3), 0
    for f, (scene, want) in enumerate(zip(scenes, results)):
        m = len(scene[0])
        assert not want.failed and sv[f] > 0, (rho, f)
        check_planted(sv[f], rm[f], tv[f], mask[f, :m], scene, (rho, f, m))          # a different best sample may be picked
        _assert_mask_is_the_inlier_test(sv[f], rm[f], tv[f], mask[f], ni[f], scene[0], scene[1])
        assert want.near.sum() <= NEAR_CAP * m
        if (mask[f, :m] == want.mask).all():                                         # the same sample: the same model
            same += 1
            ds = abs(float(sv[f]) - want.s) / want.s
            dr = np.abs(rm[f].astype(np.float64) - want.R).max()
            dt = np.linalg.norm(tv[f].astype(np.float64) - want.t) / np.linalg.norm(want.t)
            worst = np.maximum(worst, (ds, dr, dt))
            assert ds <= S_SAME_BAR and dr <= R_SAME_BAR and dt <= T_SAME_BAR, (rho, f, ds, dr, dt)
            assert ni[f] == want.ninliers
        else:
            # the count: the restatement's, give or take the pairs within 1e-3 px of the threshold under either model
            near = want.near.sum() + near_threshold(_model(sv[f], rm[f], tv[f]), scene[0].astype(np.float64),
                                                    scene[1].astype(np.float64), KVEC, KVEC, THR).sum()
            print("rho %.1f frame %2d: another mask than the restatement's (%d differ, %d near the threshold)"
                  % (rho, f, (mask[f, :m] != want.mask).sum(), near))
            assert abs(int(ni[f]) - want.ninliers) <= near, (rho, f, ni[f], want.ninliers, near)
        print("rho %.1f frame %2d M %4d: %d inliers (restatement %d), rotation %.4f deg, scale %.3e, translation %.3e"
              % (rho, f, m, ni[f], want.ninliers, *sim3_errors(sv[f], rm[f], tv[f], scene)))
    assert len(scenes) - same <= DIFFERENT_CAP * len(scenes), (same, len(scenes))
    print("rho %.1f: %d of %d frames with the restatement's mask; worst difference there: s %.3e relative, R %.3e, t %.3e "
          "relative" % (rho, same, len(scenes), *worst))


def _raw_sim3(e, q, p, npairs, mask=True, fill=0xFF, **params):
    """fpc_ransac_sim3 into outputs pre-filled with `fill` bytes -> host arrays (s, R, t, ninliers, mask uint8)."""
    import torch
    dev = e.torch_device
    n, stride = q.shape[0], q.shape[1]
    prm = e._sim3_params(None, None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (q, p, npairs)]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev) for shape in ((n, 4), (n, 36), (n, 12), (n, 4), (n, stride))]
    torch.cuda.synchronize()
    e._call("fpc_ransac_sim3", n, ins[0], ins[1], ins[2], stride, ctypes.byref(prm), outs[0], outs[1], outs[2], outs[3],
            outs[4] if mask else None, inputs=ins)
    e.sync()
    sv, rm, tv, ni, mk = (o.cpu().numpy() for o in outs)
    return (sv.view(np.float32).reshape(n), rm.view(np.float32).reshape(n, 3, 3), tv.view(np.float32).reshape(n, 3),
            ni.view(np.int32).reshape(n), mk)


def _failed(out, f):
    return out[0][f] == 0 and not out[1][f].any() and not out[2][f].any() and out[3][f] == 0 and not out[4][f].any()


def test_tails_of_the_pair_list(vga):
    e = vga
    cap = e.capacity
    scene = planted_scene(4, 0.0, cap)
    q, p = scene[0], scene[1]
    same = (np.repeat(q[:1], 50, 0), np.repeat(p[:1], 50, 0))
    rng = np.random.default_rng(8)
    noise = (rng.uniform(-4, 4, (200, 3)).astype(np.float32) + np.float32([0, 0, 8]),
             rng.uniform(-4, 4, (200, 3)).astype(np.float32) + np.float32([0, 0, 8]))
    sizes = [1100, 2, 3, 4, 255, 256, 257, 1024, 1025, cap, 100]
    lists = [(q[:m], p[:m]) for m in sizes] + [same, noise]
    a, b, npairs = _pack(lists, cap)
    npairs[9] = cap + 9                                                              # above the stride: clamped
    params = dict(PARAMS, iterations=256, min_inliers=3)
    out = _raw_sim3(e, a, b, npairs, **params)
    sv, rm, tv, ni, mask = out
    assert set(np.unique(mask).tolist()) <= {0, 1}                                   # no 0xFF left: every row was written
    assert np.isfinite(sv).all() and np.isfinite(rm).all() and np.isfinite(tv).all()
    assert _failed(out, 1) and _failed(out, 11)                                      # two pairs / every sample degenerate
    for f, m in enumerate(sizes):
        if f == 1:
            continue
        want = sim3_rule(lists[f][0], lists[f][1], params, f)
        assert not want.failed and sv[f] > 0, f
        assert not mask[f, m:].any(), f                                              # rows past the count: 0
        _assert_mask_is_the_inlier_test(sv[f], rm[f], tv[f], mask[f], ni[f], lists[f][0], lists[f][1])
        rot, sc, tr = sim3_errors(sv[f], rm[f], tv[f], scene)
        assert rot <= ROT_BAR and sc <= SCALE_BAR and tr <= TRANS_BAR, (f, rot, sc, tr)
        if (mask[f, :m].astype(bool) == want.mask).all():
            assert ni[f] == want.ninliers and abs(float(sv[f]) - want.s) <= S_SAME_BAR * want.s, f
    assert mask[0, 1024:1100].sum() >= 0.5 * 76                                      # the pairs behind the first chunk count
    assert ni[9] >= 0.5 * cap and mask[9, 1024:].any()
    # outliers only, under the default min_inliers: the frame fails with zeros, its neighbours are what they were
    strict = _raw_sim3(e, a, b, npairs, **dict(params, min_inliers=12))
    assert _failed(strict, 12) and _failed(strict, 2) and _failed(strict, 3)
    np.testing.assert_array_equal(strict[1][[0, 9]].view(np.uint32), rm[[0, 9]].view(np.uint32))
    # a frame alone (n = 1) is what it is in the batch
    alone = _raw_sim3(e, a[[0]], b[[0]], npairs[[0]], **params)
    for x, y in zip(alone, out):
        np.testing.assert_array_equal(x[:1].view(np.uint8), y[:1].view(np.uint8))
    # n = max_batch: every frame index draws its own samples, all recover the similarity
    full = e.ransac_sim3(np.repeat(a[[10]], 32, 0), np.repeat(b[[10]], 32, 0), np.repeat(npairs[[10]], 32), **params)
    assert len({full[1][f].tobytes() for f in range(32)}) > 1
    for f in range(32):
        rot, sc, tr = sim3_errors(full[0][f], full[1][f], full[2][f], scene)
        assert rot <= ROT_BAR and sc <= SCALE_BAR and tr <= TRANS_BAR, (f, rot, sc, tr)
    # a min_inliers that rejects the best model fails that frame only
    fm2 = _raw_sim3(e, a, b, npairs, **dict(params, min_inliers=101))
    assert _failed(fm2, 10)
    np.testing.assert_array_equal(fm2[1][[0, 9]].view(np.uint32), rm[[0, 9]].view(np.uint32))
    # the tails of the hypothesis grid: T = 1, and a last workgroup of 255, 256 and 1 hypotheses
    for t in (1, THREADS - 1, THREADS, THREADS + 1):
        got = _raw_sim3(e, a, b, npairs, **dict(params, iterations=t))
        want = sim3_rule(lists[10][0], lists[10][1], dict(params, iterations=t), 10)
        assert got[3][10] == got[4][10].sum()
        assert (got[0][10] == 0) == want.failed, t
        if not want.failed and (got[4][10, :100].astype(bool) == want.mask).all():
            assert abs(float(got[0][10]) - want.s) <= S_SAME_BAR * want.s, t
    # refits 0 / 1 / 4: refits = 0 returns the best sample's own model, and more refits never lower the count
    counts = []
    for refits in (0, 1, 4):
        got = _raw_sim3(e, a, b, npairs, **dict(params, refits=refits))
        want = sim3_rule(lists[10][0], lists[10][1], dict(params, refits=refits), 10)
        counts.append(int(got[3][10]))
        _assert_mask_is_the_inlier_test(got[0][10], got[1][10], got[2][10], got[4][10], got[3][10], lists[10][0], lists[10][1])
        if refits == 0:
            assert abs(float(got[0][10]) - want.first[0]) <= S_SAME_BAR * want.first[0]
            assert np.abs(got[1][10].astype(np.float64) - want.first[1]).max() <= R_SAME_BAR
            assert np.linalg.norm(got[2][10].astype(np.float64) - want.first[2]) <= T_SAME_BAR * np.linalg.norm(want.first[2])
            assert abs(np.linalg.det(got[1][10].astype(np.float64)) - 1.0) < 1e-6
    assert counts == sorted(counts), counts                                          # the monotone guard
    # a NULL mask: s, R, t and the count are what they were
    bare = _raw_sim3(e, a, b, npairs, mask=False, **params)
    np.testing.assert_array_equal(bare[1].view(np.uint32), rm.view(np.uint32))
    np.testing.assert_array_equal(bare[0].view(np.uint32), sv.view(np.uint32))
    np.testing.assert_array_equal(bare[3], ni)
    assert (bare[4] == 0xFF).all()
    # non-finite coordinates in explicit pairs: still pairs, never inliers
    bad_q, bad_p = q[:100].copy(), p[:100].copy()
    bad_q[3, 1], bad_q[9, 2], bad_p[20, 0], bad_p[31, 2] = np.nan, np.inf, -np.inf, np.nan
    c, d, npq = _pack([(bad_q, bad_p)], cap)
    got = e.ransac_sim3(c, d, npq, **params)
    want = sim3_rule(bad_q, bad_p, params, 0)
    assert got[0][0] > 0 and not got[4][0, [3, 9, 20, 31]].any() and not want.mask[[3, 9, 20, 31]].any()
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()
    _assert_mask_is_the_inlier_test(got[0][0], got[1][0], got[2][0], got[4][0], got[3][0], bad_q, bad_p)
    if (got[4][0, :100] == want.mask).all():
        assert got[3][0] == want.ninliers
    # fix_scale = 1 on two sets at one scale: s is exactly 1, R and t are the planted ones
    rigid = (q[:300].astype(np.float64) / scene[3]).astype(np.float32)
    c, d, npq = _pack([(rigid, p[:300])], cap)
    got = e.ransac_sim3(c, d, npq, **dict(params, fix_scale=1))
    assert got[0][0] == 1.0
    rot, _, tr = sim3_errors(1.0, got[1][0], got[2][0] * scene[3], scene)
    assert rot <= ROT_BAR and tr <= TRANS_BAR


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_determinism_and_the_shared_workspace(vga):
    e = vga
    rho, iterations = CASE_SETS[1]
    scenes, _ = restated_batch(rho, iterations)
    first = _device_batch(e, rho, iterations)
    q, p, npairs = _pack([(s[0], s[1]) for s in scenes], 1152)
    # a PnP call, the Sim(3) call, the PnP call again: each packs its own list into the shared records
    sc = [pnp_scene(i, 0.0, 300) for i in range(4)]
    xy, xyz = np.stack([s[0] for s in sc]), np.stack([s[1] for s in sc])
    np3 = np.full(4, 300, np.int32)
    pnp_before = e.ransac_pnp(xy, xyz, np3, iterations=256, seed=7)
    again = e.ransac_sim3(q, p, npairs, iterations=iterations, **PARAMS)
    pnp_after = e.ransac_pnp(xy, xyz, np3, iterations=256, seed=7)
    for a, b in zip(first, again):
        _bits(a, b)
    for a, b in zip(pnp_before, pnp_after):
        _bits(a, b)
    assert (pnp_before[2] >= 290).all()
    last = e.ransac_sim3(q, p, npairs, iterations=iterations, **PARAMS)             # ... and the other way round
    for a, b in zip(first, last):
        _bits(a, b)
    # another seed picks other samples and still meets the planted bars
    other = e.ransac_sim3(q, p, npairs, iterations=iterations, **dict(PARAMS, seed=3))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(other[1], first[1]))
    for f, scene in enumerate(scenes):
        m = len(scene[0])
        if m >= 40:
            check_planted(other[0][f], other[1][f], other[2][f], other[4][f, :m], scene, ("seed", f, m))


# ---- frames, bank: a planted world seen by the frames of a QVGA context ---------------------------------------------------
def _world(nkey=700, seed=3):
    """A key frame's landmarks and N frames' own landmarks of the same points -> (key_xyz float32 [nkey,3] with three rows
    that are not finite, key_valid bool [nkey], [(q_xyz float32 [k,3], q_valid bool [k], match int32 [k], s, R, t)] per
    view).  A tenth of the landmarks on either side is invalid, two query rows per view are not finite; a fifth of a view's
    matches is wrong, some rows have no match, some a match outside the key's rows."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KQVGA
    px = np.stack([rng.uniform(20, W - 20, nkey), rng.uniform(20, H - 20, nkey)], 1)
    z = rng.uniform(4.0, 12.0, nkey)
    key_xyz = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    valid = rng.uniform(size=nkey) > 0.1
    views = []
    for f in range(N):
        r = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(1.0, 6.0)))
        s = float(rng.uniform(0.6, 1.8))
        t = rng.normal(size=3) * 0.4 * s
        rows = rng.permutation(nkey)[:600 - 40 * f]                                  # the landmark each query row shows
        xq = s * (key_xyz[rows].astype(np.float64) @ r.T) + t
        xq *= 1.0 + 0.001 * rng.normal(size=(len(rows), 1))                          # a relative depth error along the ray
        qv = rng.uniform(size=len(rows)) > 0.1
        xq = xq.astype(np.float32)
        xq[7, 0], xq[11, 2] = np.nan, np.inf
        qv[[7]] = True
        match = rows.astype(np.int32)
        wrong = rng.choice(len(rows), len(rows) // 5, replace=False)                # a fifth of the matches are wrong
        match[wrong] = rng.integers(0, nkey, len(wrong))
        match[rng.choice(len(rows), 20, replace=False)] = -1                        # no match
        match[rng.choice(len(rows), 5, replace=False)] = nkey + 3                   # beyond the key's rows
        views.append((xq, qv, match, s, r, t))
    key_xyz[5, 1], key_xyz[17, 0], key_xyz[40, 2] = np.nan, np.inf, -np.inf          # not finite: invalid whatever `valid` says
    valid[[5, 17]] = True
    return key_xyz, valid, views


def _plant_views(e, views):
    """The views' counts in place of the last detect's, their landmarks and flags as landmarks_*_async leaves them -> device
    tensors (q_xyz float32 [N,cap,3], q_valid uint8 [N,cap], match int32 [N,cap])."""
    import torch
    cap = e.capacity
    _, count = e._points_view()
    hq, hv, hm = np.zeros((N, cap, 3), np.float32), np.zeros((N, cap), np.uint8), np.full((N, cap), -1, np.int32)
    for f, (xq, qv, match, _, _, _) in enumerate(views):
        hq[f, :len(xq)], hv[f, :len(qv)], hm[f, :len(match)] = xq, 2 * qv, match       # (a kind: 2 is as valid as 1)
        hm[f, len(match):len(match) + 8] = 3                                        # rows past the count are never pairs
        hq[f, len(match):len(match) + 8], hv[f, len(match):len(match) + 8] = 1.0, 1
    count[:N].copy_(torch.tensor([len(v[0]) for v in views], dtype=torch.int32))
    torch.cuda.synchronize()
    return tuple(torch.from_numpy(x).to(e.torch_device) for x in (hq, hv, hm))


def _host_lists(views, key_xyz, valid, nkey, cap, use_qvalid=True):
    """The frames variant's pair lists, gathered on the host: rows i < count with 0 <= match < nkey and a valid, finite
    landmark on both sides, ascending."""
    q, p = np.zeros((N, cap, 3), np.float32), np.zeros((N, cap, 3), np.float32)
    npairs, rows = np.zeros(N, np.int32), []
    ok = valid & np.isfinite(key_xyz).all(1)
    for f, (xq, qv, match, _, _, _) in enumerate(views):
        inside = (match >= 0) & (match < nkey)
        qok = (qv if use_qvalid else np.ones(len(qv), bool)) & np.isfinite(xq).all(1)
        i = np.flatnonzero(inside & qok & ok[np.where(inside, match, 0)])
        q[f, :len(i)], p[f, :len(i)] = xq[i], key_xyz[match[i]]
        npairs[f] = len(i)
        rows.append(i)
    return q, p, npairs, rows


def test_frames_and_bank_variants_are_bit_identical_to_explicit_pairs(qvga):
    import torch
    e = qvga
    cap, dev = e.capacity, e.torch_device
    key_xyz, valid, views = _world()
    nkey = len(key_xyz)
    q_dev, v_dev, match = _plant_views(e, views)
    params = dict(K_query=KQVGA, K_train=KQVGA, iterations=256, seed=11, reproj_threshold=3.0, min_inliers=12)
    try:
        got = e.sim3_frames(N, match, q_dev, v_dev, key_xyz, valid, **params)
        q, p, npairs, rows = _host_lists(views, key_xyz, valid, nkey, cap)
        assert npairs.min() > 150
        ref = e.ransac_sim3(q, p, npairs, **params)
        for a, b in zip(got[:4], ref[:4]):
            _bits(a, b)
        for f in range(N):
            back = np.zeros(cap, bool)
            back[rows[f]] = ref[4][f, :npairs[f]]
            np.testing.assert_array_equal(got[4][f], back)                           # invalid landmarks are not pairs
            rot, sc, tr = sim3_errors(got[0][f], got[1][f], got[2][f], (None, None, None, *views[f][3:]))
            assert ref[3][f] >= 0.6 * npairs[f] and rot <= 0.5 and sc <= SCALE_BAR, (f, ref[3][f], npairs[f], rot, sc, tr)
        # q_valid = None and key_valid = None: every finite row counts
        every = e.sim3_frames(N, match, q_dev, None, key_xyz, None, **params)
        q2, p2, npairs2, _ = _host_lists(views, key_xyz, np.ones(nkey, bool), nkey, cap, use_qvalid=False)
        ref2 = e.ransac_sim3(q2, p2, npairs2, **params)
        assert (npairs2 > npairs).all()
        for a, b in zip(every[:4], ref2[:4]):
            _bits(a, b)
        # a key count below the rows: matches beyond it are no pairs
        kx = torch.from_numpy(key_xyz).to(dev)
        few = e.sim3_frames(N, match, q_dev, v_dev, (kx, torch.tensor([300], dtype=torch.int32, device=dev)), valid, **params)
        q3, p3, npairs3, _ = _host_lists(views, key_xyz[:300], valid[:300], 300, cap)
        ref3 = e.ransac_sim3(q3, p3, npairs3, **params)
        for a, b in zip(few[:4], ref3[:4]):
            _bits(a, b)
        # the bank, in both formats: slot s holds the key's rows (any descriptors) and its landmarks
        slots = 3
        desc = np.random.default_rng(1).normal(size=(nkey, e.desc_dim)).astype(np.float32)
        kxy = np.zeros((nkey, 2), np.int32)
        full_xyz, full_valid = np.zeros((cap, 3), np.float32), np.zeros(cap, bool)
        full_xyz[:nkey], full_valid[:nkey] = key_xyz, valid
        slot = torch.tensor([0, 1, 2, -1, slots, 0, 1, 2], dtype=torch.int32, device=dev)
        banks = {}
        for fmt in ("f32", "bf16"):
            e.bank_create(slots, cap, format=fmt)
            try:
                # without landmark storage every frame is left without pairs
                none = e.sim3_bank(N, torch.zeros(N, dtype=torch.int32, device=dev), match, q_dev, v_dev, **params)
                for v in none:
                    assert not v.any()
                e.bank_landmarks_reserve()
                for s, k in ((0, nkey), (1, nkey), (2, 300)):
                    e.bank_store_rows(s, desc[:k], kxy[:k])
                e.bank_store_landmarks(0, full_xyz, full_valid)
                e.bank_store_landmarks(1, full_xyz, None)
                e.bank_store_landmarks(2, full_xyz, full_valid)
                bank = e.sim3_bank(N, slot, match, q_dev, v_dev, **params)
                for v in bank:
                    assert not v[[3, 4]].any()                                       # no slot: the frame fails with zeros
                for rows_of in ([0, 5], [2, 7]):
                    want = got if rows_of[0] == 0 else few
                    for a, b in zip(bank, want):
                        _bits(a[rows_of], b[rows_of])
                loose = e.sim3_bank(N, slot, match, q_dev, None, **params)           # slot 1: every finite row on both sides
                for a, b in zip(loose, every):
                    _bits(a[[1, 6]], b[[1, 6]])
                # ... and against fpc_sim3_frames with the slot's own storage as the key, at the same frame index
                lm = e.bank_landmarks()
                _, _, bc = e.bank_view()
                for s in range(slots):
                    own = e.sim3_frames(N, match, q_dev, v_dev, (lm[s, :, :3].contiguous(), bc[s:s + 1].clone()),
                                        lm[s, :, 3] != 0, **params)
                    rows_of = np.flatnonzero(slot.cpu().numpy() == s)
                    for a, b in zip(bank, own):
                        _bits(a[rows_of], b[rows_of])
                banks[fmt] = bank
                assert e.check_guards() == 0
            finally:
                e.bank_destroy()
        for a, b in zip(banks["f32"], banks["bf16"]):                                # it reads counts and landmarks only
            _bits(a, b)
    finally:
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_loop_closing_chain_end_to_end_recovers_the_scale(qvga):
    """A key frame with landmarks in slot 0; a frame whose keypoints and descriptors are planted in place of the last
    detect's is matched against the bank (fpc_match_bank: slot 0), localised (fpc_pnp_bank) and given landmarks of its own at
    that slot's scale (fpc_landmarks_bank: carried over where the key row has a landmark, triangulated where it has none).
    Then the loop candidate appears: slot 1 gets the same key frame with its landmarks divided by SIGMA and slot 0 is
    cleared; the frame is matched against the bank again (slot 1) and aligned with it (fpc_sim3_bank with the xyz and kind
    of the landmarks call as they are) -- nothing returns to the host in between.  s comes back as SIGMA, R as fpc_pnp_bank's
    against slot 1, t as SIGMA times that call's."""
    import torch
    e = qvga
    cap, dev = e.capacity, e.torch_device
    rng = np.random.default_rng(31)
    fx, fy, cx, cy = KQVGA
    npts = 800
    px = np.stack([rng.uniform(30, W - 30, npts), rng.uniform(30, H - 30, npts)], 1)
    z = rng.uniform(4.0, 12.0, npts)
    pa = np.round(px).astype(np.int32)
    xa = np.stack([(pa[:, 0] - cx) / fx * z, (pa[:, 1] - cy) / fy * z, z], 1).astype(np.float32)      # on the pixels' rays
    r0, t0 = _rotation([0.3, 1.0, -0.2], np.deg2rad(7.0)), np.array([1.6, -0.4, 0.5])                  # X_C = R X_A + t
    xc = xa.astype(np.float64) @ r0.T + t0
    pc = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)).astype(np.int32)
    seen = np.flatnonzero((pc[:, 0] >= 0) & (pc[:, 0] < W) & (pc[:, 1] >= 0) & (pc[:, 1] < H))
    rows_c = rng.permutation(seen)[:600]
    looks = rows_c.copy()                                                            # the key row each query row LOOKS like
    wrong = rng.choice(len(rows_c), 80, replace=False)
    looks[wrong] = rng.integers(0, npts, len(wrong))
    has_a = rng.uniform(size=npts) > 0.3                                             # slot 0: three rows in ten without a landmark
    desc = rng.normal(size=(npts, e.desc_dim)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    lm0, v0, lm1 = np.zeros((cap, 3), np.float32), np.zeros(cap, bool), np.zeros((cap, 3), np.float32)
    lm0[:npts], v0[:npts], lm1[:npts] = xa, has_a, (xa.astype(np.float64) / SIGMA).astype(np.float32)
    xy, count = e._points_view()
    dview, _ = e._results_view()
    hx, hd = np.zeros((N, cap, 2), np.int32), np.zeros((N, cap, e.desc_dim), np.float32)
    hx[0, :len(rows_c)], hd[0, :len(rows_c)] = pc[rows_c], desc[looks]
    pnp = dict(K=KQVGA, iterations=512, seed=5)
    bank = dict(cross_check=True, max_dist=0.7)
    e.bank_create(2, cap)
    try:
        e.bank_landmarks_reserve()
        xy[:N].copy_(torch.from_numpy(hx))
        dview[:N].copy_(torch.from_numpy(hd))
        count[:N].copy_(torch.tensor([len(rows_c)] + [0] * (N - 1), dtype=torch.int32))
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the similarity is read
        e.bank_store_rows(0, desc, pa)
        e.bank_store_landmarks(0, lm0, v0)
        _, best, match, _ = e.match_bank_async(N, **bank)
        rc, tc, nic, _ = e.pnp_bank_async(N, best, match, **pnp)
        xyz, kind, counts = e.landmarks_bank_async(N, best, match, rc, tc, K_query=KQVGA, K_train=KQVGA)
        e.bank_store_rows(1, desc, pa)                                               # the loop candidate appears ...
        e.bank_store_landmarks(1, lm1, None)
        e.bank_clear(0)                                                              # ... and the first slot is retired
        _, loop, match2, _ = e.match_bank_async(N, **bank)
        sim = e.sim3_bank_async(N, loop, match2, xyz, kind, K_query=KQVGA, K_train=KQVGA, iterations=512, seed=5)
        r1, t1, ni1, _ = e.pnp_bank_async(N, loop, match2, **pnp)
        best, loop, match, match2, counts, r1, t1, ni1, sv, rm, tv, ni, mask = e._host(
            (best, loop, match, match2, counts, r1, t1, ni1, *sim))
        assert best[0] == 0 and loop[0] == 1 and (best[1:] == -1).all() and (loop[1:] == -1).all(), (best, loop)
        np.testing.assert_array_equal(match, match2)                                 # the same key rows in either slot
        m0 = match2[0, :len(rows_c)]
        assert (m0 == looks).mean() > 0.8 and (m0[m0 >= 0] == looks[m0 >= 0]).all()   # (the cross check drops a few rows)
        assert counts[0, 0] > 250 and counts[0, 1] > 80, counts                       # carried over, triangulated
        assert ni1[0] > 400 and ni[0] > 0.8 * counts[0].sum(), (ni1, ni, counts)
        for v in (sv, rm, tv, ni, mask):
            assert not v[1:].any()                                                   # no slot: zeros
        truth = (None, None, None, SIGMA, r1[0].astype(np.float64), SIGMA * t1[0].astype(np.float64))
        rot, sc, tr = sim3_errors(sv[0], rm[0], tv[0], truth)
        print("loop closing: s %.5f (planted %.2f), rotation against fpc_pnp_bank's %.4f deg, translation %.3e relative; "
              "%d inliers of %d landmarks (%d carried over, %d triangulated)" % (sv[0], SIGMA, rot, tr, ni[0], counts[0].sum(),
                                                                                *counts[0]))
        assert rot <= ROT_BAR and sc <= SCALE_BAR and tr <= TRANS_BAR, (rot, sc, tr)
        rot, sc, tr = sim3_errors(sv[0], rm[0], tv[0], (None, None, None, SIGMA, r0, t0))
        assert rot <= ROT_BAR and sc <= SCALE_BAR and tr <= TRANS_BAR, (rot, sc, tr)
        off = np.flatnonzero((m0 >= 0) & (m0 != rows_c))                             # a wrong match passes only by chance
        assert len(off) > 20 and not mask[0, off].sum() > 5
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.sync()
        e.detect(synth.make_batch(300, N, H, W))


def test_bad_arguments_are_refused(qvga):
    import torch
    e = qvga
    lib = _lib.load()
    cap, dev = e.capacity, e.torch_device
    xyz = torch.zeros((N, cap, 3), dtype=torch.float32, device=dev)
    npairs = torch.full((N,), 10, dtype=torch.int32, device=dev)
    match = torch.full((N, cap), -1, dtype=torch.int32, device=dev)
    slot = torch.zeros((N,), dtype=torch.int32, device=dev)
    one = torch.ones((1,), dtype=torch.int32, device=dev)
    valid = torch.ones((N, cap), dtype=torch.uint8, device=dev)
    sv = torch.full((N,), 7.0, dtype=torch.float32, device=dev)
    rm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    tv = torch.full((N, 3), 7.0, dtype=torch.float32, device=dev)
    ni = torch.full((N,), 7, dtype=torch.int32, device=dev)
    mask = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    zp, np_, mp, lp, op, vp = (t.data_ptr() for t in (xyz, npairs, match, slot, one, valid))
    sp, rp, tp, ip, bp = (t.data_ptr() for t in (sv, rm, tv, ni, mask))
    kz = xyz[0].data_ptr()

    def params(**kw):
        p = _lib.FpcSim3Params()
        lib.fpc_default_sim3_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    ex = lambda n, a, b, c, stride, p, s, r, t, i: lib.fpc_ransac_sim3(e._ctx, n, a, b, c, stride, p, s, r, t, i, bp)   # noqa: E731
    ff = lambda n, q, qv, k, v, kc, m, p, s, r, t, i: lib.fpc_sim3_frames(e._ctx, n, q, qv, k, v, kc, m, p, s, r, t, i, bp)  # noqa: E731
    fb = lambda n, q, qv, sl, m, p, s, r, t, i: lib.fpc_sim3_bank(e._ctx, n, q, qv, sl, m, p, s, r, t, i, bp)          # noqa: E731
    ok = params()
    assert fb(N, zp, vp, lp, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID                # no bank
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(q_fx=0.0), params(q_fy=-1.0), params(t_fx=nan), params(t_fy=inf), params(q_cx=nan), params(t_cy=-inf),
               params(t_fx=0.0), params(iterations=0), params(iterations=4097), params(reproj_threshold=0.0),
               params(reproj_threshold=-1.0), params(reproj_threshold=nan), params(reproj_threshold=2e18), params(refits=-1),
               params(refits=5), params(min_inliers=2), params(fix_scale=2), params(fix_scale=-1), None]
        for p in bad:
            assert ex(N, zp, zp, np_, cap, p, sp, rp, tp, ip) == FPC_E_INVALID
            assert ff(N, zp, vp, kz, vp, op, mp, p, sp, rp, tp, ip) == FPC_E_INVALID
            assert fb(N, zp, vp, lp, mp, p, sp, rp, tp, ip) == FPC_E_INVALID
        for k in range(9):                                                           # a NULL in any pointer but the mask
            if k == 3:
                continue
            a = [zp, zp, np_, cap, ok, sp, rp, tp, ip]
            a[k] = None
            assert ex(N, *a) == FPC_E_INVALID, k
        assert ex(0, zp, zp, np_, cap, ok, sp, rp, tp, ip) == FPC_E_INVALID
        assert ex(N + 1, zp, zp, np_, cap, ok, sp, rp, tp, ip) == FPC_E_INVALID      # above max_batch
        assert ex(N, zp, zp, np_, cap + 1, ok, sp, rp, tp, ip) == FPC_E_INVALID      # stride above capacity
        assert ex(N, zp, zp, np_, 0, ok, sp, rp, tp, ip) == FPC_E_INVALID
        for k in range(11):                                                          # q_valid (1) and key_valid (3) may be NULL
            if k in (1, 3):
                continue
            a = [zp, vp, kz, vp, op, mp, ok, sp, rp, tp, ip]
            a[k] = None
            assert ff(N, *a) == FPC_E_INVALID, k
        assert ff(0, zp, vp, kz, vp, op, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        assert ff(N + 1, zp, vp, kz, vp, op, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        for k in range(9):                                                           # q_valid (1) may be NULL
            if k == 1:
                continue
            a = [zp, vp, lp, mp, ok, sp, rp, tp, ip]
            a[k] = None
            assert fb(N, *a) == FPC_E_INVALID, k
        assert fb(0, zp, vp, lp, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        assert fb(N + 1, zp, vp, lp, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert ff(3, zp, vp, kz, vp, op, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        assert fb(3, zp, vp, lp, mp, ok, sp, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        for t in (sv, rm, tv):
            assert (t.cpu() == 7.0).all()
        assert (ni.cpu() == 7).all() and (mask.cpu() == 7).all()
        assert ff(2, zp, None, kz, None, op, mp, ok, sp, rp, tp, ip) == 0
        assert fb(2, zp, None, lp, mp, ok, sp, rp, tp, ip) == 0
        assert ex(N, zp, zp, np_, cap, ok, sp, rp, tp, ip) == 0
        e.sync()
        # no match (frames, bank) or ten equal pairs (explicit): every frame fails with zeros
        for t in (sv, rm, tv, ni, mask):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
        e.sync()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)
    # a context without a PnP reservation refuses the three calls
    bare = engine(conf_thresh=0.001)
    try:
        assert lib.fpc_ransac_sim3(bare._ctx, N, zp, zp, np_, cap, ok, sp, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_sim3_frames(bare._ctx, 1, zp, vp, kz, vp, op, mp, ok, sp, rp, tp, ip, bp) == FPC_E_INVALID
        assert lib.fpc_sim3_bank(bare._ctx, 1, zp, vp, lp, mp, ok, sp, rp, tp, ip, bp) == FPC_E_INVALID
    finally:
        bare.close()
    with pytest.raises(TypeError):
        e.ransac_sim3(xyz, xyz, npairs, min_front=5)
    with pytest.raises(ValueError):
        e.ransac_sim3(xyz, xyz, npairs, K_query=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.sim3_bank(N, slot, match, xyz)                                             # no bank
