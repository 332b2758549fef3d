"""Guided matching on the GPU (fpc_match_frames_guided / fpc_match_bank_guided) against the float64 restatement and the
planted scenes of tests/test_match_guided.py: indices and distances for the three train-set choices and every option set,
bit-equality with fpc_match_frames, the chain match -> homography -> guided match -> homography without a host call in
between, failed frames and bad slots, device-read counts, determinism, the argument checks and a D = 256 context.  The
planted frames are written straight into the library's device results (desc, xy, count of fpc_results) behind a
fpc_get_points call with a descriptor map, so the kernel and the restatement read the same fp32 rows and integer pixels.
Every context runs under the canary zones.  Need a real MI355X: pytest -m gpu"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_homography_ransac import FRAME_H, FRAME_W, corner_error, ransac_rule
from tests.test_match_guided import (OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS, f10, guided_frames_rule, left_out,
                                     planted_h, planted_scene, trains_of)

pytestmark = pytest.mark.gpu

N = 8
FPC_E_INVALID = -1
HOMS = [("defaults", 1), ("preprocess", 3), ("defaults", 8), ("preprocess", 10), ("defaults", 12), ("preprocess", 5),
        ("defaults", 4), ("preprocess", 13)]
MARGIN = 1e-3                 # px at the four corners: the resolution of an fp32 H
BIG = 1e4                     # a radius beyond the frame diagonal (800 px)
PAIRINGS = (("key", PAIR_KEY, True), ("previous", PAIR_PREVIOUS, True), ("previous", PAIR_PREVIOUS, False))


def engine(h=FRAME_H, w=FRAME_W, b=N, **kw):
    from fpc_amd.engine import Engine
    kw.setdefault("plan_flags", ["guard_zones"])
    kw.setdefault("max_keypoints", 1024)
    return Engine(h, w, max_batch=b, **kw)


def plant(e, scene):
    """A fpc_get_points call with a descriptor map (so that the context holds N frames of keypoints with descriptors), then
    the scene's rows, pixels and counts in place of its results."""
    import torch
    n = len(scene["counts"])
    prob = torch.zeros((n, e.h, e.w))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((n, e.desc_dim, e.h // 8, e.w // 8)))
    desc, count = e._results_view()
    xy, _ = e._points_view()
    assert scene["desc"].shape[1] == e.capacity
    desc[:n].copy_(torch.from_numpy(scene["desc"]))
    xy[:n].copy_(torch.from_numpy(scene["xy"]))
    count[:n].copy_(torch.from_numpy(scene["counts"].astype(np.int32)))
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def planted():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    scene = planted_scene(11, [f10(name, i) for name, i in HOMS], nkey=600, cap=e.capacity)
    assert scene["counts"].min() > 300 and len(scene["key"]) == 780
    plant(e, scene)
    yield e, scene
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _compare(m, d, rule, counts, label):
    """Device table against the restatement's (match, d1, d2, borderline): indices but for the left-out rows (<= 1 % of a
    frame's rows), dist^2 within 2e-6, rows past the count -1 / +inf."""
    rm, rd1, rd2, border = rule
    out = left_out(rd1, rd2, border)
    for f, k in enumerate(counts):
        ok = ~out[f, :k]
        print("%s frame %d: %d rows, %d left out, %d matched" % (label, f, k, k - ok.sum(), (rm[f, :k] >= 0).sum()))
        assert k - ok.sum() <= 0.01 * k
        np.testing.assert_array_equal(m[f, :k][ok], rm[f, :k][ok])
        fin = np.isfinite(rd1[f, :k])
        np.testing.assert_array_equal(np.isfinite(d[f, :k]), fin)
        np.testing.assert_allclose(d[f, :k][fin].astype(np.float64) ** 2, rd1[f, :k][fin] ** 2, rtol=0, atol=2e-6)
        assert (m[f, k:] == -1).all() and np.isinf(d[f, k:]).all()


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


def test_indices_and_distances_equal_the_restatement(planted):
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        hs = planted_h(s, pcode)
        trains = trains_of(desc, xy, counts, key, key_xy, pcode)
        for cross, md, ratio in OPTIONS:
            m, d = e.match_frames_guided_async(N, hs, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=cross,
                                               max_dist=md, ratio=ratio)
            e.sync()
            m, d = _host(m, d)
            rule = guided_frames_rule(desc, xy, counts, trains, hs, RADIUS, cross, md, ratio)
            _compare(m, d, rule, counts, "%s key=%s %s" % (pairing, with_key, (cross, md, ratio)))
            if ratio == 0:
                assert (m[1:] >= 0).sum() > 1000
        if not with_key:
            assert (m[0] == -1).all() and np.isinf(d[0]).all()             # frame 0 has no train set
    # the per-frame form of the host wrapper
    got = e.match_frames_guided(N, planted_h(s, PAIR_KEY), RADIUS, key=s["key"], key_xy=s["key_xy"])
    assert [len(g[0]) for g in got] == list(counts)


def test_large_radius_is_bit_identical_to_match_frames(planted):
    e, s = planted
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        hs = planted_h(s, pcode)
        for cross, md, ratio in OPTIONS:
            m, d = e.match_frames_guided_async(N, hs, BIG, key=key, key_xy=key_xy, pairing=pairing, cross_check=cross,
                                               max_dist=md, ratio=ratio)
            um, ud = e.match_frames_async(N, key=key, pairing=pairing, cross_check=cross, max_dist=md, ratio=ratio)
            e.sync()
            m, d, um, ud = _host(m, d, um, ud)
            np.testing.assert_array_equal(m, um)
            np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
        # under the gate: wherever the guided and the unguided winner coincide, dist is bit-equal
        m, d = e.match_frames_guided_async(N, hs, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=False)
        um, ud = e.match_frames_async(N, key=key, pairing=pairing, cross_check=False)
        e.sync()
        m, d, um, ud = _host(m, d, um, ud)
        same = (m == um) & (m >= 0)
        assert same.sum() > 1000 and ((m != um) & (m >= 0)).sum() > 50       # ... and the gate did change winners
        np.testing.assert_array_equal(d.view(np.uint32)[same], ud.view(np.uint32)[same])


def _corners_close(h_dev, h_rule):
    return corner_error(h_dev.astype(np.float64), h_rule)


def _pairs(m, xy, counts, f, txy):
    rows = np.flatnonzero((m[f, :counts[f]] >= 0) & (m[f, :counts[f]] < len(txy)))
    return xy[f, rows].astype(np.float64), txy[m[f, rows]].astype(np.float64)


def test_full_chain_on_the_device(planted):
    e, s = planted
    xy, counts = s["xy"], s["counts"]
    params = dict(iterations=256, seed=3)
    for pairing, pcode, with_key in PAIRINGS[:2]:
        key, key_xy = s["key"], s["key_xy"]
        # four calls, no host call in between
        m1, _ = e.match_frames_async(N, key=key, pairing=pairing, cross_check=True)
        h1, n1, _ = e.homography_frames_async(N, m1, key_xy=key_xy, pairing=pairing, **params)
        m2, _ = e.match_frames_guided_async(N, h1, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=True)
        h2, n2, _ = e.homography_frames_async(N, m2, key_xy=key_xy, pairing=pairing, **params)
        e.sync()
        m2, h1, n1, h2, n2 = _host(m2, h1, n1, h2, n2)
        trains = trains_of(s["desc"], xy, counts, key, key_xy, pcode)
        print(pairing, "inliers", n1, "->", n2)
        assert (n1 >= 8).all() and (n2 >= n1).all() and n2.sum() > n1.sum()
        for f in range(N):
            src, dst = _pairs(m2, xy, counts, f, trains[f][1])
            rh, _ = ransac_rule(src, dst, params, f)
            err = _corners_close(h2[f], rh)
            print("  frame %d: %d pairs, device H against the restatement's: %.3e px" % (f, len(src), err))
            assert err < MARGIN, (pairing, f, err)


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
    hs = planted_h(s, PAIR_KEY)
    slot_host = np.array([2, 3, 2, -1, 0, 2, 4, 1], np.int32)            # -1, 4: outside the bank; 1: an empty slot
    slot = torch.from_numpy(slot_host).to(e.torch_device)
    empty = (desc[0, :0], xy[0, :0])
    trains = [slots.get(int(v), empty) for v in slot_host]
    for cross, md, ratio in OPTIONS:
        m, d = e.match_bank_guided_async(N, slot, hs, RADIUS, cross_check=cross, max_dist=md, ratio=ratio)
        e.sync()
        m, d = _host(m, d)
        _compare(m, d, guided_frames_rule(desc, xy, counts, trains, hs, RADIUS, cross, md, ratio), counts,
                 "bank %s" % ((cross, md, ratio),))
        assert (m[[3, 6, 7]] == -1).all() and np.isinf(d[[3, 6, 7]]).all()      # a bad or an empty slot: -1 / +inf
    assert (e.match_bank_guided(N, slot, hs, RADIUS)[0][0] >= 0).sum() > 300          # the per-frame host form
    # a radius beyond the frame: fpc_match_frames with the slot as its key, bit for bit
    bd, bx, bc = e.bank_view()
    m, d = e.match_bank_guided_async(N, slot, hs, BIG, cross_check=True, max_dist=0.7)
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
    h1, n1, _ = e.homography_bank_async(N, best, m1, **params)
    m2, _ = e.match_bank_guided_async(N, best, h1, RADIUS, cross_check=True, max_dist=0.7)
    h2, n2, _ = e.homography_bank_async(N, best, m2, **params)
    e.sync()
    best, m2, n1, h2, n2 = _host(best, m2, n1, h2, n2)
    print("bank: best", best, "inliers", n1, "->", n2)
    assert (best == 2).all() and (n1 >= 8).all() and (n2 >= n1).all() and n2.sum() > n1.sum()
    for f in range(N):
        src, dst = _pairs(m2, xy, counts, f, s["key_xy"])
        rh, _ = ransac_rule(src, dst, params, f)
        err = _corners_close(h2[f], rh)
        print("  frame %d: %d pairs, device H against the restatement's: %.3e px" % (f, len(src), err))
        assert err < MARGIN, (f, err)


def test_failed_frames_and_repeated_calls(planted):
    import torch
    e, s = planted
    hs = planted_h(s, PAIR_KEY)
    bad = hs.copy()
    bad[3] = 0                                                             # what a failed frame's homography is
    bad[5, 4] = np.nan
    bad[6, 8] = np.inf
    outs = []
    for _ in range(2):
        m, d = e.match_frames_guided_async(N, torch.from_numpy(bad).to(e.torch_device), RADIUS, key=s["key"],
                                           key_xy=s["key_xy"], cross_check=True, max_dist=0.9)
        e.sync()
        outs.append(_host(m, d.view(torch.int32)))
    m, d = outs[0]
    assert (m[[3, 5, 6]] == -1).all() and (d[[3, 5, 6]].view(np.float32) == np.inf).all()
    assert ((m[[0, 1, 2, 4, 7]] >= 0).sum(axis=1) > 100).all()
    np.testing.assert_array_equal(outs[0][0], outs[1][0])                 # repeated calls: bit-identical
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_counts_are_read_on_the_device_right_behind_get_points():
    """fpc_get_points, keep_frame, keep_frame_points and the guided call enqueued back to back: eight views cropped from one
    larger probability / descriptor map at offsets that are multiples of 8 px, the known translations as H."""
    import torch
    from tests.test_gpu_homography_ransac import H, W, _planted_maps
    offsets = [(0, 0), (8, 0), (16, 8), (32, 24), (56, 48), (64, 64), (24, 40), (48, 16)]
    prob, dmap = _planted_maps()
    probs = torch.from_numpy(np.stack([prob[oy:oy + H, ox:ox + W] for ox, oy in offsets]))
    descs = torch.from_numpy(np.stack([dmap[:, oy // 8:oy // 8 + H // 8, ox // 8:ox // 8 + W // 8] for ox, oy in offsets]))
    hs = np.stack([np.array([1, 0, ox, 0, 1, oy, 0, 0, 1], np.float32) for ox, oy in offsets])
    e = engine(H, W, max_keypoints=0)
    try:
        probs, descs = probs.to(e.torch_device).contiguous(), descs.to(e.torch_device).contiguous()
        hdev = torch.from_numpy(hs).to(e.torch_device)
        torch.cuda.synchronize()
        _lib.check(e._l.fpc_get_points(e._ctx, probs.data_ptr(), descs.data_ptr(), N), "fpc_get_points")
        kept, kept_xy = e.keep_frame(0), e.keep_frame_points(0)
        m, d = e.match_frames_guided_async(N, hdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True)
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
        _compare(m, d, guided_frames_rule(desc, xy, counts, trains, hs, 2.0, True), counts, "translation")
        for f, (ox, oy) in enumerate(offsets):
            rows = np.flatnonzero(m[f, :counts[f]] >= 0)
            assert len(rows) > 200
            np.testing.assert_array_equal(xy[f, rows] + [ox, oy], res[0][0][m[f, rows]])     # the same scene point
        assert e.check_guards() == 0
    finally:
        e.close()


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, s, slots = banked
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, e.capacity), -7.0, dtype=torch.float32, device=dev)
    hm = torch.from_numpy(np.tile(np.eye(3, dtype=np.float32).reshape(9), (N + 1, 1))).to(dev)
    key, kc = e._key(s["key"])
    kx, _ = e._key_xy(s["key_xy"])
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    K, P = PAIR_KEY, PAIR_PREVIOUS

    def mg(n=N, pairing=K, k=key.data_ptr(), c=kc.data_ptr(), x=kx.data_ptr(), h=hm.data_ptr(), r=4.0, md=0.0, ratio=0.0,
           out=mt.data_ptr()):
        return lib.fpc_match_frames_guided(ctx, n, pairing, k, c, x, h, r, 1, md, ratio, out, ds.data_ptr())

    def bg(n=N, sl=slot.data_ptr(), h=hm.data_ptr(), r=4.0, md=0.0, ratio=0.0, out=mt.data_ptr()):
        return lib.fpc_match_bank_guided(ctx, n, sl, h, r, 1, md, ratio, out, ds.data_ptr())
    # everything fpc_match_frames refuses
    assert mg(n=N + 1) == FPC_E_INVALID and mg(n=0) == FPC_E_INVALID
    assert mg(pairing=2) == FPC_E_INVALID
    assert mg(md=-1.0) == FPC_E_INVALID and mg(ratio=1.5) == FPC_E_INVALID and mg(ratio=-0.1) == FPC_E_INVALID
    assert mg(out=None) == FPC_E_INVALID
    assert mg(k=None, c=None, x=None) == FPC_E_INVALID                    # FPC_PAIR_KEY without a key
    assert mg(c=None) == FPC_E_INVALID                                    # a key without its count
    assert mg(k=key.data_ptr() + 4) == FPC_E_INVALID                      # not 16-byte aligned
    # and the guided call's own
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
    # a context without a bank; results without descriptors
    d = engine(b=2)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        out = torch.full((2, d.capacity), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert lib.fpc_match_bank_guided(d._ctx, 2, slot.data_ptr(), hm.data_ptr(), 4.0, 1, 0.0, 0.0, out.data_ptr(),
                                         None) == FPC_E_INVALID
        d.get_points(prob)
        assert lib.fpc_match_frames_guided(d._ctx, 2, P, None, None, None, hm.data_ptr(), 4.0, 1, 0.0, 0.0, out.data_ptr(),
                                           None) == FPC_E_INVALID
        d.sync()
        assert (out.cpu().numpy() == -7).all() and d.check_guards() == 0
    finally:
        d.close()


def test_vgg_descriptors():
    """FPC_ARCH_VGG: D = 256."""
    e = engine(240, 320, in_channels=1, arch="vgg")
    try:
        assert e.desc_dim == 256
        s = planted_scene(4, [f10(name, i) for name, i in HOMS], nkey=300, dim=256, cap=e.capacity)
        plant(e, s)
        desc, xy, counts = s["desc"], s["xy"], s["counts"]
        for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
            hs = planted_h(s, pcode)
            trains = trains_of(desc, xy, counts, s["key"], s["key_xy"], pcode)
            for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
                m, d = e.match_frames_guided_async(N, hs, RADIUS, key=s["key"], key_xy=s["key_xy"], pairing=pairing,
                                                   cross_check=cross, max_dist=md, ratio=ratio)
                e.sync()
                _compare(*_host(m, d), guided_frames_rule(desc, xy, counts, trains, hs, RADIUS, cross, md, ratio), counts,
                         "vgg %s %s" % (pairing, (cross, md, ratio)))
            m, d = e.match_frames_guided_async(N, hs, BIG, key=s["key"], key_xy=s["key_xy"], pairing=pairing)
            um, ud = e.match_frames_async(N, key=s["key"], pairing=pairing)
            e.sync()
            m, d, um, ud = _host(m, d, um, ud)
            np.testing.assert_array_equal(m, um)
            np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
            assert (m >= 0).sum() > 500
        assert e.check_guards() == 0
    finally:
        e.close()
