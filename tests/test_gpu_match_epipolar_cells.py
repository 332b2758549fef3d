"""Cell-ordered epipolar guided matching on the GPU (fpc_match_frames_guided_epipolar_cells /
fpc_match_bank_guided_epipolar_cells): the output bit for bit against the existing device calls
(fpc_match_frames_guided_epipolar / fpc_match_bank_guided_epipolar, same context, same planted results) for the three
train-set choices, every option set and radii of 2, 4, 16 and 10^6 px (there against fpc_match_frames as well), ragged counts
across the strip, tile and list edges, failed and non-finite F, the bank variant, the argument checks, a D = 256 context,
device-read counts, the chain match -> fundamental -> guided match (cells) -> fundamental without a host call in between, and
the tile counters against the float64 restatement of tests/test_match_epipolar_cells.py.  Every context runs under the canary
zones.  Need a real MI355X: pytest -m gpu"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_match_epipolar import PAIRINGS, _all_pass, _assert_f_is_the_restatements
from tests.test_gpu_match_guided import _host, engine, plant
from tests.test_match_epipolar import (ALL_PASS, GPU_SCENE, GPU_VGG_SCENE, OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS, planted_f,
                                       scene_of, trains_of)
from tests.test_match_epipolar_cells import UNIFORM_RADII, uniform_bounds, uniform_scene
from tests.test_match_guided import FRAME_H, FRAME_W

pytestmark = pytest.mark.gpu

N = 8
FPC_E_INVALID = -1
RADII = (2.0, 4.0, 16.0, ALL_PASS)


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


def _same(e, n, fs, radius, key, key_xy, pairing, cross, md, ratio, label):
    """Both device calls on the same inputs -> the new call's (match, dist, stats) after asserting bit-identity."""
    m, d, st = e.match_frames_guided_epipolar_cells_async(n, fs, radius, key=key, key_xy=key_xy, pairing=pairing,
                                                          cross_check=cross, max_dist=md, ratio=ratio, stats=True)
    rm, rd = e.match_frames_guided_epipolar_async(n, fs, radius, key=key, key_xy=key_xy, pairing=pairing, cross_check=cross,
                                                  max_dist=md, ratio=ratio)
    e.sync()
    m, d, st, rm, rd = _host(m, d, st, rm, rd)
    np.testing.assert_array_equal(m, rm, err_msg=str(label))
    np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32), err_msg=str(label))
    assert (0 <= st[:, 0]).all() and (st[:, 0] <= st[:, 1]).all(), (label, st)
    return m, d, st


def _equals_match_frames(e, n, m, d, key, pairing, cross, md, ratio):
    um, ud = e.match_frames_async(n, key=key, pairing=pairing, cross_check=cross, max_dist=md, ratio=ratio)
    e.sync()
    um, ud = _host(um, ud)
    np.testing.assert_array_equal(m, um)
    np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))


def test_bit_identical_on_the_planted_scene(planted):
    e, s = planted
    desc, xy, counts = s["desc"], s["xy"], s["counts"]
    matched = 0
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        fs = planted_f(s, pcode)
        # the premise of the identity with fpc_match_frames, on the restatement
        assert _all_pass(fs, xy, counts, trains_of(desc, xy, counts, key, key_xy, pcode))
        for radius in RADII:
            for cross, md, ratio in OPTIONS:
                m, d, st = _same(e, N, fs, radius, key, key_xy, pairing, cross, md, ratio, (pairing, with_key, radius, cross, md, ratio))
                matched += (m >= 0).sum()
                if radius == ALL_PASS:
                    _equals_match_frames(e, N, m, d, key, pairing, cross, md, ratio)
                    assert (st[:, 0] == st[:, 1]).all()                      # every pair a candidate: every tile
                if not with_key:
                    assert (m[0] == -1).all() and np.isinf(d[0]).all() and (st[0] == 0).all()      # frame 0: no train set
    assert matched > 50000
    got = e.match_frames_guided_epipolar_cells(N, planted_f(s, PAIR_KEY).reshape(N, 3, 3), RADIUS, key=s["key"],
                                               key_xy=s["key_xy"])                                  # F as [n,3,3]; the host form
    assert [len(g[0]) for g in got] == list(counts)
    assert sum(int((g[0] >= 0).sum()) for g in got) == N * len(s["key"])      # every planted pair, as the epipolar call
    assert e.check_guards() == 0


def test_bit_identical_on_ragged_counts(planted):
    """Counts 0, 1, 63, 64, 65, 129, 130 and one frame at cap (its rows past the scene's 820 are unrelated ones), against the
    key, against the frame before, and against a key of 0, 1 and 65 rows: the strip, tile and list edges."""
    import torch
    e, s = planted
    cap = e.capacity
    rng = np.random.Generator(np.random.PCG64(12))
    r = dict(s)
    r["desc"], r["xy"] = s["desc"].copy(), s["xy"].copy()
    more = rng.normal(size=(cap - 820, s["desc"].shape[2]))
    r["desc"][7, 820:] = (more / np.linalg.norm(more, axis=1, keepdims=True)).astype(np.float32)
    r["xy"][7, 820:] = np.stack([rng.integers(0, FRAME_W, cap - 820), rng.integers(0, FRAME_H, cap - 820)], 1)
    r["counts"] = np.array([0, 1, 63, 64, 65, 129, 130, cap])
    plant(e, r)
    try:
        matched = 0
        for pairing, pcode, with_key in PAIRINGS:
            key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
            fs = planted_f(s, pcode)
            assert _all_pass(fs, r["xy"], r["counts"], trains_of(r["desc"], r["xy"], r["counts"], key, key_xy, pcode))
            for radius in (4.0, ALL_PASS):
                for cross, md, ratio in OPTIONS:
                    m, d, st = _same(e, N, fs, radius, key, key_xy, pairing, cross, md, ratio, (pairing, with_key, radius, cross, md, ratio))
                    matched += (m[7] >= 0).sum()
                    if radius == ALL_PASS:
                        _equals_match_frames(e, N, m, d, key, pairing, cross, md, ratio)
            if pcode == PAIR_KEY:
                np.testing.assert_array_equal(st[:, 1], [-(-k // 64) * -(-len(s["key"]) // 64) for k in r["counts"]])
        assert matched > 1000
        # a key of 65 rows, of 1 row, and an empty key: the count is what the device holds
        kd, kx = torch.from_numpy(s["key"]).to(e.torch_device), torch.from_numpy(s["key_xy"]).to(e.torch_device)
        for nk in (65, 1, 0):
            cnt = torch.tensor([nk], dtype=torch.int32, device=e.torch_device)
            for radius in (4.0, ALL_PASS):
                for cross, md, ratio in ((True, 0.0, 0.0), (False, 0.7, 0.8)):
                    m, _, st = _same(e, N, planted_f(s, PAIR_KEY), radius, (kd, cnt), (kx, cnt), "key", cross, md, ratio,
                                     ("key rows", nk, radius))
                    np.testing.assert_array_equal(st[:, 1], [-(-nk // 64) * -(-k // 64) for k in r["counts"]])
                    if nk == 0:
                        assert (m == -1).all()
        assert e.check_guards() == 0
    finally:
        plant(e, s)


def test_failed_and_non_finite_f_repeated_calls_and_null_stats(planted):
    import torch
    e, s = planted
    fs = planted_f(s, PAIR_KEY)
    bad = fs.copy()
    bad[1] = -bad[1]                                                       # the gate is even in F: no sign rule
    bad[3] = 0                                                             # what a failed frame's F is
    bad[5, 4] = np.nan
    bad[6, 8] = np.inf
    bad[2, 0] = -np.inf
    dead, live = [2, 3, 5, 6], [0, 1, 4, 7]
    for radius in (RADIUS, ALL_PASS):
        outs = []
        for _ in range(3):
            outs.append(_same(e, N, torch.from_numpy(bad).to(e.torch_device), radius, s["key"], s["key_xy"], "key", True, 0.9,
                              0.0, ("bad F", radius)))
        m, d, st = outs[0]
        assert (m[dead] == -1).all() and np.isinf(d[dead]).all()
        assert (st[dead, 0] == 0).all() and (st[:, 1] > 0).all() and (st[live, 0] > 0).all()
        assert ((m[live] >= 0).sum(axis=1) > 300).all()
        for o in outs[1:]:                                                 # repeated calls: bit-identical, counters included
            np.testing.assert_array_equal(o[0], m)
            np.testing.assert_array_equal(o[1].view(np.uint32), d.view(np.uint32))
            np.testing.assert_array_equal(o[2], st)
        gm, gd, gst = _same(e, N, fs, radius, s["key"], s["key_xy"], "key", True, 0.9, 0.0, ("good F", radius))
        np.testing.assert_array_equal(m[live], gm[live])                   # the other frames are unaffected, -F is F
        np.testing.assert_array_equal(d.view(np.uint32)[live], gd.view(np.uint32)[live])
        np.testing.assert_array_equal(st[live], gst[live])
        # stats_dev = NULL: the same tables
        m2, d2 = e.match_frames_guided_epipolar_cells_async(N, bad, radius, key=s["key"], key_xy=s["key_xy"], cross_check=True,
                                                            max_dist=0.9)
        e.sync()
        m2, d2 = _host(m2, d2)
        np.testing.assert_array_equal(m2, m)
        np.testing.assert_array_equal(d2.view(np.uint32), d.view(np.uint32))
    assert e.check_guards() == 0


@pytest.fixture(scope="module")
def banked(planted):
    e, s = planted
    rng = np.random.Generator(np.random.PCG64(5))
    other = rng.normal(size=(500, 128))
    other = (other / np.linalg.norm(other, axis=1, keepdims=True)).astype(np.float32)
    other_xy = np.stack([rng.integers(0, FRAME_W, 500), rng.integers(0, FRAME_H, 500)], 1).astype(np.int32)
    e.bank_create(4)
    for sl, (d, p) in {2: (s["key"], s["key_xy"]), 0: (other, other_xy), 3: (s["key"][:400], s["key_xy"][:400])}.items():
        e.bank_store_rows(sl, d, p)                                          # slot 1 stays empty
    e.sync()
    yield e, s
    assert e.check_guards() == 0
    e.bank_destroy()


def test_bank_variant(banked):
    import torch
    e, s = banked
    fs = planted_f(s, PAIR_KEY)
    slot_host = np.array([2, 3, 2, -1, 0, 2, 4, 1], np.int32)            # -1, 4: outside the bank; 1: an empty slot
    slot = torch.from_numpy(slot_host).to(e.torch_device)
    size = e.bank_info()["bytes"]
    for radius in RADII:
        for cross, md, ratio in OPTIONS:
            m, d, st = e.match_bank_guided_epipolar_cells_async(N, slot, fs, radius, cross_check=cross, max_dist=md, ratio=ratio,
                                                                stats=True)
            rm, rd = e.match_bank_guided_epipolar_async(N, slot, fs, radius, cross_check=cross, max_dist=md, ratio=ratio)
            e.sync()
            m, d, st, rm, rd = _host(m, d, st, rm, rd)
            np.testing.assert_array_equal(m, rm)
            np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32))
            assert (m[[3, 6, 7]] == -1).all() and (st[[3, 6, 7]] == 0).all() and (st[[0, 1, 2, 4, 5], 1] > 0).all()
            assert (st[:, 0] <= st[:, 1]).all()
    assert (m[[0, 2, 5]] >= 0).sum() > 300
    assert (e.match_bank_guided_epipolar_cells(N, slot, fs, RADIUS)[0][0] >= 0).sum() > 300       # the per-frame host form
    m2, _ = e.match_bank_guided_epipolar_cells_async(N, slot, fs, ALL_PASS, cross_check=False, ratio=0.8)     # stats_dev = NULL
    e.sync()
    np.testing.assert_array_equal(_host(m2)[0], m)
    assert e.bank_info()["bytes"] == size and e.check_guards() == 0
    # the chain through the bank, no host call in between
    params = dict(iterations=256, seed=3)
    score, best, m1, _ = e.match_bank_async(N, cross_check=True, max_dist=0.7)
    f1, n1, _ = e.fundamental_bank_async(N, best, m1, **params)
    m2, _ = e.match_bank_guided_epipolar_cells_async(N, best, f1, RADIUS, cross_check=True, max_dist=0.7)
    f2, n2, _ = e.fundamental_bank_async(N, best, m2, **params)
    e.sync()
    best, m2, n1, f2, n2 = _host(best, m2, n1, f2, n2)
    print("bank: best", best, "inliers", n1, "->", n2)
    assert (best == 2).all() and (n1 >= 8).all() and (n2 >= 8).all() and n2.sum() > n1.sum()
    for f in range(N):
        _assert_f_is_the_restatements("bank", f, f2[f], m2, s, PAIR_KEY, s["key_xy"], params)


def test_bf16_bank_is_refused_and_nothing_is_written():
    import torch
    e = engine()
    try:
        s = scene_of(GPU_SCENE)
        plant(e, s)
        e.bank_create(2, format="bf16")
        e.bank_store_rows(0, s["key"], s["key_xy"])
        dev = e.torch_device
        mt = torch.full((N, e.capacity), -7, dtype=torch.int32, device=dev)
        ds = torch.full((N, e.capacity), -7.0, dtype=torch.float32, device=dev)
        st = torch.full((N, 2), -7, dtype=torch.int32, device=dev)
        slot = torch.zeros((N,), dtype=torch.int32, device=dev)
        fm = torch.from_numpy(planted_f(s, PAIR_KEY)).to(dev)
        torch.cuda.synchronize()
        assert _lib.load().fpc_match_bank_guided_epipolar_cells(e._ctx, N, slot.data_ptr(), fm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                                mt.data_ptr(), ds.data_ptr(), st.data_ptr()) == FPC_E_INVALID
        with pytest.raises(_lib.FpcError):
            e.match_bank_guided_epipolar_cells_async(N, slot, fm, 4.0)
        e.sync()
        assert (mt.cpu().numpy() == -7).all() and (ds.cpu().numpy() == -7.0).all() and (st.cpu().numpy() == -7).all()
        assert e.check_guards() == 0
        e.bank_destroy()
    finally:
        e.close()


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, s = banked
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, e.capacity), -7.0, dtype=torch.float32, device=dev)
    st = torch.full((N + 1, 2), -7, dtype=torch.int32, device=dev)
    fm = torch.from_numpy(np.tile(planted_f(s, PAIR_KEY)[0], (N + 1, 1))).to(dev)
    key, kc = e._key(s["key"])
    kx, _ = e._key_xy(s["key_xy"])
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    K, P = PAIR_KEY, PAIR_PREVIOUS

    def mg(n=N, pairing=K, k=key.data_ptr(), c=kc.data_ptr(), x=kx.data_ptr(), h=fm.data_ptr(), r=4.0, md=0.0, ratio=0.0,
           out=mt.data_ptr()):
        return lib.fpc_match_frames_guided_epipolar_cells(ctx, n, pairing, k, c, x, h, r, 1, md, ratio, out, ds.data_ptr(),
                                                          st.data_ptr())

    def bg(n=N, sl=slot.data_ptr(), h=fm.data_ptr(), r=4.0, md=0.0, ratio=0.0, out=mt.data_ptr()):
        return lib.fpc_match_bank_guided_epipolar_cells(ctx, n, sl, h, r, 1, md, ratio, out, ds.data_ptr(), st.data_ptr())
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
    assert (mt.cpu().numpy() == -7).all() and (ds.cpu().numpy() == -7.0).all() and (st.cpu().numpy() == -7).all()
    assert mg(pairing=P, k=None, c=None, x=None) == 0 and bg() == 0       # (the valid forms of the calls above)
    e.sync()
    assert (st.cpu().numpy()[:N] >= 0).all() and (st.cpu().numpy()[N] == -7).all()
    assert e.check_guards() == 0
    # a context without a bank; results without descriptors
    d = engine(b=2)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        out = torch.full((2, d.capacity), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert lib.fpc_match_bank_guided_epipolar_cells(d._ctx, 2, slot.data_ptr(), fm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                        out.data_ptr(), None, st.data_ptr()) == FPC_E_INVALID
        d.get_points(prob)
        assert lib.fpc_match_frames_guided_epipolar_cells(d._ctx, 2, P, None, None, None, fm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                          out.data_ptr(), None, st.data_ptr()) == FPC_E_INVALID
        d.sync()
        assert (out.cpu().numpy() == -7).all() and (st.cpu().numpy()[N] == -7).all() and d.check_guards() == 0
    finally:
        d.close()


def test_vgg_descriptors():
    """FPC_ARCH_VGG: D = 256, a 240 x 320 frame (10 x 8 cells; the scene's pixels reach beyond it: clamped cells)."""
    e = engine(240, 320, in_channels=1, arch="vgg")
    try:
        assert e.desc_dim == 256 and e.capacity == GPU_VGG_SCENE["cap"]
        s = scene_of(GPU_VGG_SCENE)
        plant(e, s)
        for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
            fs = planted_f(s, pcode)
            assert _all_pass(fs, s["xy"], s["counts"], trains_of(s["desc"], s["xy"], s["counts"], s["key"], s["key_xy"], pcode))
            for radius in RADII:
                for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
                    m, d, st = _same(e, N, fs, radius, s["key"], s["key_xy"], pairing, cross, md, ratio, ("vgg", pairing, radius))
                    if radius == ALL_PASS:
                        _equals_match_frames(e, N, m, d, s["key"], pairing, cross, md, ratio)
            assert (m >= 0).sum() > 500
        assert e.check_guards() == 0
    finally:
        e.close()


def test_counts_are_read_on_the_device_right_behind_get_points():
    """fpc_get_points, keep_frame, keep_frame_points and both epipolar calls enqueued back to back
    (tests/test_gpu_match_epipolar.py's x-shift scene): the counts the new call orders and matches by are the ones the device
    holds."""
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
        m, d, st = e.match_frames_guided_epipolar_cells_async(N, fdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True,
                                                              stats=True)
        rm, rd = e.match_frames_guided_epipolar_async(N, fdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True)
        e.sync()
        res = e.fetch(N)
        counts = np.array([len(r[0]) for r in res])
        assert counts.min() > 500 and len(set(counts.tolist())) > 1
        m, d, st, rm, rd = _host(m, d, st, rm, rd)
        np.testing.assert_array_equal(m, rm)
        np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32))
        np.testing.assert_array_equal(st[:, 1], [-(-k // 64) * -(-counts[0] // 64) for k in counts])
        print("x-shift: visited", st[:, 0].tolist(), "of", st[:, 1].tolist())
        assert (0 < st[:, 0]).all()
        for f in range(N):
            rows = np.flatnonzero(m[f, :counts[f]] >= 0)
            assert len(rows) > 200 and (m[f, counts[f]:] == -1).all()
            assert (np.abs(res[f][0][rows, 1] - res[0][0][m[f, rows], 1]) <= 2).all()            # inside the band
        assert e.check_guards() == 0
    finally:
        e.close()


def test_full_chain_on_the_device(planted):
    e, s = planted
    xy, counts = s["xy"], s["counts"]
    params = dict(iterations=256, seed=3)
    for pairing, pcode, _ in PAIRINGS[:2]:
        key, key_xy = s["key"], s["key_xy"]
        # four calls, no host call in between
        m1, _ = e.match_frames_async(N, key=key, pairing=pairing, cross_check=True)
        f1, n1, _ = e.fundamental_frames_async(N, m1, key_xy=key_xy, pairing=pairing, **params)
        m2, _ = e.match_frames_guided_epipolar_cells_async(N, f1, RADIUS, key=key, key_xy=key_xy, pairing=pairing,
                                                           cross_check=True)
        f2, n2, _ = e.fundamental_frames_async(N, m2, key_xy=key_xy, pairing=pairing, **params)
        e.sync()
        m2, n1, f2, n2 = _host(m2, n1, f2, n2)
        trains = trains_of(s["desc"], xy, counts, key, key_xy, pcode)
        print(pairing, "inliers", n1, "->", n2)
        assert (n1 >= 8).all() and (n2 >= 8).all() and n2.sum() > n1.sum()
        for f in range(N):
            _assert_f_is_the_restatements(pairing, f, f2[f], m2, s, pcode, trains[f][1], params)
    assert e.check_guards() == 0


def test_culling_visits_what_the_boxes_allow_and_no_less_than_needed():
    """8 frames of about 2 000 uniform rows against a 2 000-row key under planted sideways cameras with a mild rotation: per
    frame, the kernel's visited count lies between the tiles that hold a candidate at a radius scaled by 1 - 1e-9 and the
    tiles the float64 box rule admits at a radius scaled by 1 + 1e-9 (the kernel widens its bounds by 2^-49 of the line's
    terms, far inside that).  As a condition on the input, the box rule itself admits at most half of the grid."""
    e = engine(max_keypoints=0)
    try:
        s = uniform_scene(e.capacity)
        counts = s["counts"]
        assert 1900 <= counts.min() and len(set(counts.tolist())) > 1
        bounds = {}
        for radius in UNIFORM_RADII:
            need, upper, grid = uniform_bounds(e.capacity, radius)
            print("radius %g: needed %.3f, upper %.3f of the grid" % (radius, need.sum() / grid.sum(), upper.sum() / grid.sum()))
            assert (need <= upper).all() and 2 * upper.sum() <= grid.sum()        # a condition on the input
            bounds[radius] = need, upper, grid
        plant(e, s)
        for radius in UNIFORM_RADII:
            need, upper, grid = bounds[radius]
            for cross, md, ratio in ((True, 0.0, 0.0), (False, 0.7, 0.8)):
                m, d, st = _same(e, N, s["fs"], radius, s["key"], s["key_xy"], "key", cross, md, ratio, ("uniform", radius))
                print("radius %g: visited %s = %.3f of the grid" % (radius, st[:, 0].tolist(), st[:, 0].sum() / grid.sum()))
                np.testing.assert_array_equal(st[:, 1], grid)
                assert (need <= st[:, 0]).all() and (st[:, 0] <= upper).all(), (need, st[:, 0], upper)
                assert ratio > 0 or (m >= 0).sum() > 8000          # (Lowe's test needs a second candidate: fewer rows pass it)
        assert e.check_guards() == 0
    finally:
        e.close()
