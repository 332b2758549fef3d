"""Epipolar guided matching on the GPU (fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar) against the
float64 restatement and the planted 3-D scenes of tests/test_match_epipolar.py: indices and distances for the three train-set
choices and every option set, bit-equality with fpc_match_frames where every pair is a candidate, strips and tiles of 0, 1,
2, 63, 64 and 65 rows, the chain match -> fundamental -> guided match -> fundamental without a host call in between (frames
and bank), failed frames and bad slots, device-read counts, determinism, the argument checks and a D = 256 context.  The
planted frames are written straight into the library's device results as tests/test_gpu_match_guided.py's plant does, so the
kernel and the restatement read the same fp32 rows and integer pixels.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_fundamental_ransac import epipolar_rms, ransac_rule
from tests.test_gpu_fundamental_ransac import MARGIN
from tests.test_gpu_match_guided import _compare, _host, _pairs, engine, plant
from tests.test_match_epipolar import (ALL_PASS, GPU_SCENE, GPU_VGG_SCENE, OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS,
                                       epipolar_frames_rule, epipolar_gate, planted_f, planted_truth, scene_of, trains_of)
from tests.test_match_guided import FRAME_H, FRAME_W

pytestmark = pytest.mark.gpu

N = 8
FPC_E_INVALID = -1
PAIRINGS = (("key", PAIR_KEY, True), ("previous", PAIR_PREVIOUS, True), ("previous", PAIR_PREVIOUS, False))


@pytest.fixture(scope="module")
def planted():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    scene = scene_of(GPU_SCENE)
    assert e.capacity == GPU_SCENE["cap"] and (scene["counts"] == 820).all() and len(scene["key"]) == 780
    plant(e, scene)
    yield e, scene
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _all_pass(fs, xy, counts, trains):
    """The premise of a bit identity: under ALL_PASS every pair of every frame is a candidate, by the restatement."""
    return all(epipolar_gate(fs[f], xy[f, :k], trains[f][1], ALL_PASS)[0].all() for f, k in enumerate(counts))


def test_indices_and_distances_equal_the_restatement(planted):
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        fs = planted_f(s, pcode)
        trains = trains_of(desc, xy, counts, key, key_xy, pcode)
        for cross, md, ratio in OPTIONS:
            m, d = e.match_frames_guided_epipolar_async(N, fs, RADIUS, key=key, key_xy=key_xy, pairing=pairing,
                                                        cross_check=cross, max_dist=md, ratio=ratio)
            e.sync()
            m, d = _host(m, d)
            rule = epipolar_frames_rule(desc, xy, counts, trains, fs, RADIUS, cross, md, ratio)
            _compare(m, d, rule, counts, "%s key=%s %s" % (pairing, with_key, (cross, md, ratio)))
            if ratio == 0:
                assert (m[1:] >= 0).sum() > 3000
        if not with_key:
            assert (m[0] == -1).all() and np.isinf(d[0]).all()             # frame 0 has no train set
    # F as [n,3,3], and the per-frame form of the host wrapper
    got = e.match_frames_guided_epipolar(N, planted_f(s, PAIR_KEY).reshape(N, 3, 3), RADIUS, key=s["key"], key_xy=s["key_xy"])
    assert [len(g[0]) for g in got] == list(counts)
    assert sum(int((g[0] >= 0).sum()) for g in got) == N * len(s["key"])      # every planted pair, as on the CPU


def test_all_pass_radius_is_bit_identical_to_match_frames(planted):
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        fs = planted_f(s, pcode)
        assert _all_pass(fs, xy, counts, trains_of(desc, xy, counts, key, key_xy, pcode))
        for cross, md, ratio in OPTIONS:
            m, d = e.match_frames_guided_epipolar_async(N, fs, ALL_PASS, key=key, key_xy=key_xy, pairing=pairing,
                                                        cross_check=cross, max_dist=md, ratio=ratio)
            um, ud = e.match_frames_async(N, key=key, pairing=pairing, cross_check=cross, max_dist=md, ratio=ratio)
            e.sync()
            m, d, um, ud = _host(m, d, um, ud)
            np.testing.assert_array_equal(m, um)
            np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
        # under the gate: wherever the guided and the unguided winner coincide, dist is bit-equal
        m, d = e.match_frames_guided_epipolar_async(N, fs, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=False)
        um, ud = e.match_frames_async(N, key=key, pairing=pairing, cross_check=False)
        e.sync()
        m, d, um, ud = _host(m, d, um, ud)
        same = (m == um) & (m >= 0)
        assert same.sum() > 1000 and ((m != um) & (m >= 0)).sum() > 50       # ... and the gate did change winners
        np.testing.assert_array_equal(d.view(np.uint32)[same], ud.view(np.uint32)[same])


def test_strip_and_tile_edges(planted):
    """Device counts 0, 1, 2, 63, 64, 65 against a key of 1, 2 and 65 rows, and against the frame before: the strip edge, the
    tile edge, and Lowe's test with fewer than two candidates.  Only the device counts change: rows are in random order, so
    the first k rows of a planted frame are a planted frame."""
    import torch
    e, s = planted
    n = 6
    small = np.array([0, 1, 2, 63, 64, 65])
    desc, xy = s["desc"][:n], s["xy"][:n]
    _, count = e._results_view()
    count[:n].copy_(torch.from_numpy(small.astype(np.int32)))
    torch.cuda.synchronize()
    try:
        for nkey in (1, 2, 65):
            key, key_xy = s["key"][:nkey], s["key_xy"][:nkey]
            for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
                fs = planted_f(s, pcode)[:n]
                trains = trains_of(desc, xy, small, key, key_xy, pcode)
                assert _all_pass(fs, xy, small, trains)
                for cross, md, ratio in OPTIONS:
                    args = dict(key=key, key_xy=key_xy, pairing=pairing, cross_check=cross, max_dist=md, ratio=ratio)
                    m, d = e.match_frames_guided_epipolar_async(n, fs, RADIUS, **args)
                    am, ad = e.match_frames_guided_epipolar_async(n, fs, ALL_PASS, **args)
                    args.pop("key_xy")
                    um, ud = e.match_frames_async(n, **args)
                    e.sync()
                    m, d, am, ad, um, ud = _host(m, d, am, ad, um, ud)
                    label = "nkey %d %s %s" % (nkey, pairing, (cross, md, ratio))
                    _compare(m, d, epipolar_frames_rule(desc, xy, small, trains, fs, RADIUS, cross, md, ratio), small, label)
                    _compare(am, ad, epipolar_frames_rule(desc, xy, small, trains, fs, ALL_PASS, cross, md, ratio), small, label)
                    np.testing.assert_array_equal(am, um)
                    np.testing.assert_array_equal(ad.view(np.uint32), ud.view(np.uint32))
                    if ratio > 0 and nkey == 1 and pcode == PAIR_KEY:
                        assert (am == -1).all()                             # one candidate: the ratio test fails
                    if ratio == 0 and md == 0:
                        assert (am[5] >= 0).sum() >= (1 if cross else 65)   # (something was matched)
    finally:
        count[:n].copy_(torch.from_numpy(s["counts"][:n].astype(np.int32)))
        torch.cuda.synchronize()


def _planted_pairs(s, pcode, f, txy):
    truth = planted_truth(s, pcode)
    rows = np.flatnonzero(truth[f, :s["counts"][f]] >= 0)
    return s["xy"][f, rows].astype(np.float64), txy[truth[f, rows]].astype(np.float64)


def _assert_f_is_the_restatements(tag, f, fdev, m2, s, pcode, txy, params):
    """The device's F from its own pair list against the float64 ransac_rule on that list: the measure and the MARGIN of
    tests/test_gpu_fundamental_ransac.py, the RMS symmetric epipolar distance of the frame's planted pairs."""
    src, dst = _pairs(m2, s["xy"], s["counts"], f, txy)
    rf, _ = ransac_rule(src, dst, params, f)
    assert np.any(rf), (tag, f)
    a, b = _planted_pairs(s, pcode, f, txy)
    rms, rrms = epipolar_rms(fdev.astype(np.float64), a, b), epipolar_rms(rf, a, b)
    print("  %s frame %d: %d pairs, RMS %.4f px, restatement %.4f px" % (tag, f, len(src), rms, rrms))
    assert rms <= rrms + MARGIN, (tag, f, rms, rrms)


def test_full_chain_on_the_device(planted):
    e, s = planted
    xy, counts = s["xy"], s["counts"]
    params = dict(iterations=256, seed=3)
    for pairing, pcode, _ in PAIRINGS[:2]:
        key, key_xy = s["key"], s["key_xy"]
        # four calls, no host call in between
        m1, _ = e.match_frames_async(N, key=key, pairing=pairing, cross_check=True)
        f1, n1, _ = e.fundamental_frames_async(N, m1, key_xy=key_xy, pairing=pairing, **params)
        m2, _ = e.match_frames_guided_epipolar_async(N, f1, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=True)
        f2, n2, _ = e.fundamental_frames_async(N, m2, key_xy=key_xy, pairing=pairing, **params)
        e.sync()
        m2, n1, f2, n2 = _host(m2, n1, f2, n2)
        trains = trains_of(s["desc"], xy, counts, key, key_xy, pcode)
        print(pairing, "inliers", n1, "->", n2)
        assert (n1 >= 8).all() and (n2 >= 8).all() and n2.sum() > n1.sum()
        for f in range(N):
            _assert_f_is_the_restatements(pairing, f, f2[f], m2, s, pcode, trains[f][1], params)


@pytest.fixture(scope="module")
def banked(planted):
    e, s = planted
    rng = np.random.Generator(np.random.PCG64(5))
    other = rng.normal(size=(500, 128))
    other = (other / np.linalg.norm(other, axis=1, keepdims=True)).astype(np.float32)
    other_xy = np.stack([rng.integers(0, FRAME_W, 500), rng.integers(0, FRAME_H, 500)], 1).astype(np.int32)
    e.bank_create(4)
    slots = {2: (s["key"], s["key_xy"]), 0: (other, other_xy), 3: (s["key"][:400], s["key_xy"][:400])}   # slot 1 stays empty
    for sl, (d, p) in slots.items():
        e.bank_store_rows(sl, d, p)
    e.sync()
    yield e, s, slots
    assert e.check_guards() == 0
    e.bank_destroy()


def test_bank_variant(banked):
    import torch
    e, s, slots = banked
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    fs = planted_f(s, PAIR_KEY)
    slot_host = np.array([2, 3, 2, -1, 0, 2, 4, 1], np.int32)            # -1, 4: outside the bank; 1: an empty slot
    slot = torch.from_numpy(slot_host).to(e.torch_device)
    empty = (desc[0, :0], xy[0, :0])
    trains = [slots.get(int(v), empty) for v in slot_host]
    for cross, md, ratio in OPTIONS:
        m, d = e.match_bank_guided_epipolar_async(N, slot, fs, RADIUS, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        m, d = _host(m, d)
        _compare(m, d, epipolar_frames_rule(desc, xy, counts, trains, fs, RADIUS, cross, md, ratio), counts,
                 "bank %s" % ((cross, md, ratio),))
        assert (m[[3, 6, 7]] == -1).all() and np.isinf(d[[3, 6, 7]]).all()      # a bad or an empty slot: -1 / +inf
    assert (e.match_bank_guided_epipolar(N, slot, fs, RADIUS)[0][0] >= 0).sum() > 300      # the per-frame host form
    # every pair a candidate: fpc_match_frames with the slot as its key, bit for bit
    assert _all_pass(fs, xy, counts, trains)
    bd, bx, bc = e.bank_view()
    m, d = e.match_bank_guided_epipolar_async(N, slot, fs, ALL_PASS, cross_check=True, max_dist=0.7)
    e.sync()
    m, d = _host(m, d)
    for sl in (0, 2, 3):
        um, ud = e.match_frames_async(N, key=(bd[sl].clone(), bc[sl:sl + 1].clone()), cross_check=True, max_dist=0.7)
        e.sync()
        um, ud = _host(um, ud)
        rows = np.flatnonzero(slot_host == sl)
        np.testing.assert_array_equal(m[rows], um[rows])
        np.testing.assert_array_equal(d.view(np.uint32)[rows], ud.view(np.uint32)[rows])
    # the chain through the bank, no host call in between
    params = dict(iterations=256, seed=3)
    score, best, m1, _ = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    f1, n1, _ = e.fundamental_bank_async(N, best, m1, **params)
    m2, _ = e.match_bank_guided_epipolar_async(N, best, f1, RADIUS, cross_check=True, max_dist=0.7)
    f2, n2, _ = e.fundamental_bank_async(N, best, m2, **params)
    e.sync()
    best, m2, n1, f2, n2 = _host(best, m2, n1, f2, n2)
    print("bank: best", best, "inliers", n1, "->", n2)
    assert (best == 2).all() and (n1 >= 8).all() and (n2 >= 8).all() and n2.sum() > n1.sum()
    for f in range(N):
        _assert_f_is_the_restatements("bank", f, f2[f], m2, s, PAIR_KEY, s["key_xy"], params)


def test_failed_frames_and_repeated_calls(planted):
    import torch
    e, s = planted
    fs = planted_f(s, PAIR_KEY)
    bad = fs.copy()
    bad[1] = -bad[1]                                                       # the gate is even in F: no sign rule
    bad[3] = 0                                                             # what a failed frame's F is
    bad[5, 4] = np.nan
    bad[6, 8] = np.inf
    outs = []
    for _ in range(2):
        m, d = e.match_frames_guided_epipolar_async(N, torch.from_numpy(bad).to(e.torch_device), RADIUS, key=s["key"],
                                                    key_xy=s["key_xy"], cross_check=True, max_dist=0.9)
        e.sync()
        outs.append(_host(m, d.view(torch.int32)))
    m, d = outs[0]
    assert (m[[3, 5, 6]] == -1).all() and (d[[3, 5, 6]].view(np.float32) == np.inf).all()
    assert ((m[[0, 1, 2, 4, 7]] >= 0).sum(axis=1) > 300).all()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])                 # repeated calls: bit-identical
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    gm, gd = e.match_frames_guided_epipolar_async(N, fs, RADIUS, key=s["key"], key_xy=s["key_xy"], cross_check=True, max_dist=0.9)
    e.sync()
    gm, gd = _host(gm, gd.view(torch.int32))
    ok = [0, 1, 2, 4, 7]                                                  # the other frames are unaffected, -F is F
    np.testing.assert_array_equal(m[ok], gm[ok])
    np.testing.assert_array_equal(d[ok], gd[ok])


def test_counts_are_read_on_the_device_right_behind_get_points():
    """fpc_get_points, keep_frame, keep_frame_points and the guided call enqueued back to back: eight views cropped from one
    larger probability / descriptor map at x offsets that are multiples of 8 px; F is that of a pure x-shift,
    [0 0 0; 0 0 -1; 0 1 0] / sqrt(2), so a row's candidates share its y (|y - v| sqrt(1/2) < radius).  A band, unlike the
    homography gate's disc, holds other points too.  The sampler's grid does not shift by whole cells with the view, so a
    point's descriptor in view f is near, not equal to, its descriptor in the key view (measured: within 0.1 for 597 of 614
    rows at 8 px, for 37 of 613 at 32 px) against ~1 between different points: most rows, not all, take their own point."""
    import torch
    from tests.test_gpu_homography_ransac import H, W, _planted_maps
    offsets = [0, 8, 16, 32, 56, 64, 24, 48]
    prob, dmap = _planted_maps()
    probs = torch.from_numpy(np.stack([prob[:H, ox:ox + W] for ox in offsets]))
    descs = torch.from_numpy(np.stack([dmap[:, :H // 8, ox // 8:ox // 8 + W // 8] for ox in offsets]))
    fs = np.tile((np.array([0, 0, 0, 0, 0, -1, 0, 1, 0]) / np.sqrt(2.0)).astype(np.float32), (N, 1))
    e = engine(H, W, max_keypoints=0)
    try:
        probs, descs = probs.to(e.torch_device).contiguous(), descs.to(e.torch_device).contiguous()
        fdev = torch.from_numpy(fs).to(e.torch_device)
        torch.cuda.synchronize()
        _lib.check(e._l.fpc_get_points(e._ctx, probs.data_ptr(), descs.data_ptr(), N), "fpc_get_points")
        kept, kept_xy = e.keep_frame(0), e.keep_frame_points(0)
        m, d = e.match_frames_guided_epipolar_async(N, fdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True)
        e.sync()
        res = e.fetch(N)
        counts = np.array([len(r[0]) for r in res])
        assert counts.min() > 500 and len(set(counts.tolist())) > 1
        cap = e.capacity
        desc, xy = np.zeros((N, cap, 128), np.float32), np.zeros((N, cap, 2), np.int32)
        for f, r in enumerate(res):
            xy[f, :counts[f]], desc[f, :counts[f]] = r[0], r[2]
        trains = trains_of(desc, xy, counts, res[0][2], res[0][0], PAIR_KEY)
        m, d = _host(m, d)
        _compare(m, d, epipolar_frames_rule(desc, xy, counts, trains, fs, 2.0, True), counts, "x-shift")
        for f, ox in enumerate(offsets):
            rows = np.flatnonzero(m[f, :counts[f]] >= 0)
            assert len(rows) > 200
            assert (np.abs(xy[f, rows, 1] - res[0][0][m[f, rows], 1]) <= 2).all()            # inside the band
            own = (xy[f, rows] + [ox, 0] == res[0][0][m[f, rows]]).all(1)                      # the same scene point
            print("x-shift %d px: %d rows matched, %d of them to their own point" % (ox, len(rows), own.sum()))
            assert own.sum() > 0.5 * len(rows)
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, s, slots = banked
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, e.capacity), -7.0, dtype=torch.float32, device=dev)
    fm = torch.from_numpy(np.tile(planted_f(s, PAIR_KEY)[0], (N + 1, 1))).to(dev)
    key, kc = e._key(s["key"])
    kx, _ = e._key_xy(s["key_xy"])
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    K, P = PAIR_KEY, PAIR_PREVIOUS

    def mg(n=N, pairing=K, k=key.data_ptr(), c=kc.data_ptr(), x=kx.data_ptr(), h=fm.data_ptr(), r=4.0, md=0.0, ratio=0.0,
           out=mt.data_ptr()):
        return lib.fpc_match_frames_guided_epipolar(ctx, n, pairing, k, c, x, h, r, 1, md, ratio, out, ds.data_ptr())

    def bg(n=N, sl=slot.data_ptr(), h=fm.data_ptr(), r=4.0, md=0.0, ratio=0.0, out=mt.data_ptr()):
        return lib.fpc_match_bank_guided_epipolar(ctx, n, sl, h, r, 1, md, ratio, out, ds.data_ptr())
    # everything fpc_match_frames refuses
    assert mg(n=N + 1) == FPC_E_INVALID and mg(n=0) == FPC_E_INVALID
    assert mg(pairing=2) == FPC_E_INVALID
    assert mg(md=-1.0) == FPC_E_INVALID and mg(ratio=1.5) == FPC_E_INVALID and mg(ratio=-0.1) == FPC_E_INVALID
    assert mg(out=None) == FPC_E_INVALID
    assert mg(k=None, c=None, x=None) == FPC_E_INVALID                    # FPC_PAIR_KEY without a key
    assert mg(c=None) == FPC_E_INVALID                                    # a key without its count
    assert mg(k=key.data_ptr() + 4) == FPC_E_INVALID                      # not 16-byte aligned
    # and the guided calls' own, with F_dev for H_dev
    assert mg(h=None) == FPC_E_INVALID
    for r in (0.0, -4.0, float("inf"), float("nan")):
        assert mg(r=r) == FPC_E_INVALID and bg(r=r) == FPC_E_INVALID
    assert mg(x=None) == FPC_E_INVALID                                    # FPC_PAIR_KEY without key_xy
    assert mg(pairing=P, x=None) == FPC_E_INVALID                         # a key without key_xy
    assert bg(n=N + 1) == FPC_E_INVALID and bg(n=0) == FPC_E_INVALID
    assert bg(sl=None) == FPC_E_INVALID and bg(h=None) == FPC_E_INVALID and bg(out=None) == FPC_E_INVALID
    assert bg(md=-1.0) == FPC_E_INVALID and bg(ratio=1.5) == FPC_E_INVALID
    e.sync()
    assert (mt.cpu().numpy() == -7).all() and (ds.cpu().numpy() == -7.0).all()
    assert mg(pairing=P, k=None, c=None, x=None) == 0 and bg() == 0       # (the valid forms of the calls above)
    e.sync()
    # a context without a bank; a bf16 bank; results without descriptors
    d = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        out = torch.full((2, d.capacity), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def bank_call():
            return lib.fpc_match_bank_guided_epipolar(d._ctx, 2, slot.data_ptr(), fm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                      out.data_ptr(), None)
        def untouched():
            d.sync()
            return bool((out.cpu().numpy() == -7).all())
        assert bank_call() == FPC_E_INVALID and untouched()               # no bank: refused, nothing written
        d.bank_create(2, format="bf16")
        d.bank_store_rows(0, s["key"][:64], s["key_xy"][:64])
        d.sync()
        assert lib.fpc_match_bank_guided(d._ctx, 2, slot.data_ptr(), fm.data_ptr(), 4.0, 1, 0.0, 0.0, out.data_ptr(), None) == 0
        d.sync()
        out.fill_(-7)
        torch.cuda.synchronize()
        assert bank_call() == FPC_E_INVALID and untouched()               # FPC_BANK_BF16: that format's gate is the follow-up
        with pytest.raises(_lib.FpcError):
            d.match_bank_guided_epipolar_async(2, slot[:2], fm[:2], 4.0)
        assert untouched()
        d.bank_destroy()
        d.bank_create(2)
        assert bank_call() == 0 and not untouched()                       # (an f32 bank: accepted, and it writes)
        d.bank_destroy()
        out.fill_(-7)
        d.get_points(prob)
        torch.cuda.synchronize()
        assert lib.fpc_match_frames_guided_epipolar(d._ctx, 2, P, None, None, None, fm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                    out.data_ptr(), None) == FPC_E_INVALID
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
        for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
            fs = planted_f(s, pcode)
            trains = trains_of(desc, xy, counts, s["key"], s["key_xy"], pcode)
            for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
                m, d = e.match_frames_guided_epipolar_async(N, fs, RADIUS, key=s["key"], key_xy=s["key_xy"], pairing=pairing,
                                                            cross_check=cross, max_dist=md, ratio=ratio)
                e.sync()
                _compare(*_host(m, d), epipolar_frames_rule(desc, xy, counts, trains, fs, RADIUS, cross, md, ratio), counts,
                         "vgg %s %s" % (pairing, (cross, md, ratio)))
            assert _all_pass(fs, xy, counts, trains)
            m, d = e.match_frames_guided_epipolar_async(N, fs, ALL_PASS, key=s["key"], key_xy=s["key_xy"], pairing=pairing)
            um, ud = e.match_frames_async(N, key=s["key"], pairing=pairing)
            e.sync()
            m, d, um, ud = _host(m, d, um, ud)
            np.testing.assert_array_equal(m, um)
            np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
            assert (m >= 0).sum() > 500
        assert e.check_guards() == 0
    finally:
        e.close()
