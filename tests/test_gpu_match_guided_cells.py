"""Cell-ordered guided matching on the GPU (fpc_cell_order / fpc_match_frames_guided_cells / fpc_match_bank_guided_cells):
the order against np.lexsort, the output bit for bit against the existing device calls (fpc_match_frames_guided /
fpc_match_bank_guided, same context, same planted results) for the three train-set choices, every option set and radii of
4, 16 and 10^4 px, the tile counters against the float64 restatement of tests/test_match_guided_cells.py, the chain match ->
homography -> guided_cells -> homography without a host call in between, device-read counts, determinism, the argument
checks and a D = 256 context.  Every context runs under the canary zones.  Need a real MI355X: pytest -m gpu"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_homography_ransac import FRAME_H, FRAME_W, corner_error, ransac_rule
from tests.test_match_guided import OPTIONS, PAIR_KEY, PAIR_PREVIOUS, RADIUS, f10, planted_h, planted_scene, trains_of
from tests.test_match_guided_cells import cell_order, crafted_scene, needed_tiles, visited_tiles
from tests.test_gpu_match_guided import BIG, HOMS, MARGIN, N, PAIRINGS, _host, _pairs, engine, plant

pytestmark = pytest.mark.gpu

FPC_E_INVALID = -1
RADII = (4.0, 16.0, BIG)


def _scene():
    return planted_scene(11, [f10(name, i) for name, i in HOMS], nkey=600, cap=1024)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    assert e.capacity == 1024
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


@pytest.fixture(scope="module")
def planted(ctx):
    s = _scene()
    plant(ctx, s)
    return ctx, s


def _same(e, n, hs, radius, key, key_xy, pairing, cross, md, ratio, label):
    """Both device calls on the same inputs -> the new call's (match, dist, stats) after asserting bit-identity."""
    m, d, st = e.match_frames_guided_cells_async(n, hs, radius, key=key, key_xy=key_xy, pairing=pairing, cross_check=cross,
                                                 max_dist=md, ratio=ratio, stats=True)
    rm, rd = e.match_frames_guided_async(n, hs, radius, key=key, key_xy=key_xy, pairing=pairing, cross_check=cross,
                                         max_dist=md, ratio=ratio)
    e.sync()
    m, d, st, rm, rd = _host(m, d, st, rm, rd)
    np.testing.assert_array_equal(m, rm, err_msg=str(label))
    np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32), err_msg=str(label))
    return m, d, st


def _sweep(e, s, hs_of, n, big_is_unguided=True):
    matched = 0
    for pairing, pcode, with_key in PAIRINGS:
        key, key_xy = (s["key"], s["key_xy"]) if with_key else (None, None)
        hs = hs_of(pcode)
        for radius in RADII:
            for cross, md, ratio in OPTIONS:
                m, d, _ = _same(e, n, hs, radius, key, key_xy, pairing, cross, md, ratio, (pairing, with_key, radius, cross, md, ratio))
                matched += (m >= 0).sum()
                if radius == BIG and big_is_unguided:
                    um, ud = e.match_frames_async(n, key=key, pairing=pairing, cross_check=cross, max_dist=md, ratio=ratio)
                    e.sync()
                    um, ud = _host(um, ud)
                    np.testing.assert_array_equal(m, um)
                    np.testing.assert_array_equal(d.view(np.uint32), ud.view(np.uint32))
    return matched


def test_cell_order_equals_lexsort(ctx):
    import torch
    e = ctx
    stride = 1024
    rng = np.random.Generator(np.random.PCG64(9))
    counts = np.array([0, 1, 63, 64, 65, 1000, stride, 700, 500], np.int32)
    xy = np.stack([rng.integers(0, FRAME_W, (len(counts), stride)), rng.integers(0, FRAME_H, (len(counts), stride))], 2)
    xy[7] = np.stack([rng.integers(96, 128, stride), rng.integers(160, 192, stride)], 1)                    # one cell
    xy[8] = np.stack([rng.integers(-300, FRAME_W + 300, stride), rng.integers(-300, FRAME_H + 300, stride)], 1)
    xy = xy.astype(np.int32)
    assert (xy[8] < 0).any() and (xy[8, :, 0] >= FRAME_W).any() and (xy[8, :, 1] >= FRAME_H).any()
    got = []
    for _ in range(2):
        perm = e.cell_order_async(xy, counts)
        e.sync()
        got.append(perm.cpu().numpy())
    for s, cnt in enumerate(counts):
        np.testing.assert_array_equal(got[0][s, :cnt], cell_order(xy[s, :cnt]), err_msg="set %d" % s)
        np.testing.assert_array_equal(got[0][s, :cnt], got[1][s, :cnt])
    # a count beyond the stride is clamped; a negative one is an empty set
    perm = e.cell_order_async(xy[:2], np.array([stride + 50, -3], np.int32))
    e.sync()
    np.testing.assert_array_equal(perm.cpu().numpy()[0], cell_order(xy[0]))
    lib, dev = _lib.load(), e.torch_device
    out = torch.full((2, stride), -7, dtype=torch.int32, device=dev)
    x, c = torch.from_numpy(xy[:2]).to(dev), torch.from_numpy(counts[:2]).to(dev)
    torch.cuda.synchronize()
    for args in ((None, c.data_ptr(), 2, stride, out.data_ptr()), (x.data_ptr(), None, 2, stride, out.data_ptr()),
                 (x.data_ptr(), c.data_ptr(), 0, stride, out.data_ptr()), (x.data_ptr(), c.data_ptr(), 2, 0, out.data_ptr()),
                 (x.data_ptr(), c.data_ptr(), 2, stride, None)):
        assert lib.fpc_cell_order(e._ctx, *args) == FPC_E_INVALID
    e.sync()
    assert (out.cpu().numpy() == -7).all()


def test_bit_identical_on_the_planted_scene(planted):
    e, s = planted
    assert _sweep(e, s, lambda pcode: planted_h(s, pcode), N) > 10000
    got = e.match_frames_guided_cells(N, planted_h(s, PAIR_KEY), RADIUS, key=s["key"], key_xy=s["key_xy"])   # the host form
    assert [len(g[0]) for g in got] == list(s["counts"])


def test_bit_identical_with_failed_homographies(planted):
    e, s = planted
    for pairing, pcode, with_key in PAIRINGS[:2]:
        hs = planted_h(s, pcode).copy()
        hs[1] = 0
        hs[2, 4] = np.nan
        hs[3, 8] = np.inf
        hs[4, 0] = -np.inf
        hs[5] = np.array([1, 0, 0, 0, 1, 0, -1.0 / 320, 0, 1], np.float32)          # w <= 0 right of x = 320
        hs[6] = -hs[6]                                                               # w < 0 everywhere
        for radius in RADII:
            m, d, st = _same(e, N, hs, radius, s["key"], s["key_xy"], pairing, True, 0.0, 0.0, (pairing, radius))
            assert (m[[1, 2, 3, 4, 6]] == -1).all() and np.isinf(d[[1, 2, 3, 4, 6]]).all()
            assert (st[[1, 2, 3, 4, 6], 0] == 0).all() and (st[:, 1] > 0).all()
            right = s["xy"][5, :s["counts"][5], 0] >= 320
            assert right.sum() > 50 and (m[5, :s["counts"][5]][right] == -1).all()
            if radius == BIG:
                assert (m[5, :s["counts"][5]][~right] >= 0).sum() > 50


def test_bit_identical_on_ragged_counts(ctx, planted):
    e, s = planted
    r = dict(s)
    r["counts"] = np.array([0, 1, 63, 64, 65, 130, 129, s["counts"][7]])
    assert (r["counts"] <= s["counts"]).all()
    plant(e, r)
    try:
        _sweep(e, r, lambda pcode: planted_h(s, pcode), N)
        # a key of 1 row, and an empty key: the count is what the device holds
        import torch
        kd, kx = torch.from_numpy(s["key"]).to(e.torch_device), torch.from_numpy(s["key_xy"]).to(e.torch_device)
        for nk in (1, 0):
            cnt = torch.tensor([nk], dtype=torch.int32, device=e.torch_device)
            for radius in (4.0, BIG):
                m, _, st = _same(e, N, planted_h(s, PAIR_KEY), radius, (kd, cnt), (kx, cnt), "key", True, 0.0, 0.0, ("key rows", nk, radius))
                assert (st[:, 1] == [nk * -(-k // 64) for k in r["counts"]]).all()
    finally:
        plant(e, s)


def test_bit_identical_on_the_crafted_scene(ctx, planted):
    e, s = planted
    c = crafted_scene(cap=e.capacity)
    plant(e, c)
    try:
        assert _sweep(e, c, lambda pcode: c["hs"], 4) > 1000
        # frame 3 holds the key's own rows: every row finds itself or its exact copy
        m, d, _ = _same(e, 4, c["hs"], 4.0, c["key"], c["key_xy"], "key", False, 0.0, 0.0, "ties")
        k3 = c["counts"][3]
        assert (m[3, :k3] >= 0).all() and (c["key"][m[3, :k3]] == c["desc"][3, :k3]).all()
    finally:
        plant(e, s)


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
    hs = planted_h(s, PAIR_KEY)
    slot_host = np.array([2, 3, 2, -1, 0, 2, 4, 1], np.int32)            # -1, 4: outside the bank; 1: an empty slot
    slot = torch.from_numpy(slot_host).to(e.torch_device)
    size = e.bank_info()["bytes"]
    for radius in RADII:
        for cross, md, ratio in OPTIONS:
            m, d, st = e.match_bank_guided_cells_async(N, slot, hs, radius, cross_check=cross, max_dist=md, ratio=ratio, stats=True)
            rm, rd = e.match_bank_guided_async(N, slot, hs, radius, cross_check=cross, max_dist=md, ratio=ratio)
            e.sync()
            m, d, st, rm, rd = _host(m, d, st, rm, rd)
            np.testing.assert_array_equal(m, rm)
            np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32))
            assert (m[[3, 6, 7]] == -1).all() and (st[[3, 6, 7]] == 0).all() and (st[[0, 1, 2, 4, 5], 1] > 0).all()
    assert (m[[0, 2, 5]] >= 0).sum() > 300
    assert (e.match_bank_guided_cells(N, slot, hs, RADIUS)[0][0] >= 0).sum() > 300          # the per-frame host form
    assert e.bank_info()["bytes"] == size


def test_bf16_bank_is_refused_and_nothing_is_written():
    import torch
    e = engine()
    try:
        s = _scene()
        plant(e, s)
        e.bank_create(2, format="bf16")
        e.bank_store_rows(0, s["key"], s["key_xy"])
        dev = e.torch_device
        mt = torch.full((N, e.capacity), -7, dtype=torch.int32, device=dev)
        ds = torch.full((N, e.capacity), -7.0, dtype=torch.float32, device=dev)
        st = torch.full((N, 2), -7, dtype=torch.int32, device=dev)
        slot = torch.zeros((N,), dtype=torch.int32, device=dev)
        hm = torch.from_numpy(planted_h(s, PAIR_KEY)).to(dev)
        torch.cuda.synchronize()
        assert _lib.load().fpc_match_bank_guided_cells(e._ctx, N, slot.data_ptr(), hm.data_ptr(), 4.0, 1, 0.0, 0.0, mt.data_ptr(),
                                                       ds.data_ptr(), st.data_ptr()) == FPC_E_INVALID
        e.sync()
        assert (mt.cpu().numpy() == -7).all() and (ds.cpu().numpy() == -7.0).all() and (st.cpu().numpy() == -7).all()
        m, _ = e.match_bank_guided_async(N, slot, hm, 4.0)                       # (the existing call works on it)
        e.sync()
        assert (m.cpu().numpy() >= 0).sum() > 300 and e.check_guards() == 0
        e.bank_destroy()
    finally:
        e.close()


def _uniform_scene(cap, nkey=2000, dim=128):
    """8 frames of about 2 000 uniform points against a 2 000-row key under a mild perspective H, +-1 px noise."""
    rng = np.random.Generator(np.random.PCG64(31))
    unit = lambda v: (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    key = unit(rng.normal(size=(nkey, dim)))
    key_xy = np.stack([rng.integers(0, FRAME_W, nkey), rng.integers(0, FRAME_H, nkey)], 1).astype(np.int32)
    desc, xy = np.zeros((N, cap, dim), np.float32), np.zeros((N, cap, 2), np.int32)
    counts, hs = np.zeros(N, np.int64), np.zeros((N, 9), np.float32)
    for f in range(N):
        g = np.array([[1 + 0.02 * f, 0.01 * f, 3.0 * f - 8], [-0.01 * f, 1 - 0.01 * f, 5.0 - 2 * f], [2e-5 * f, -1e-5 * f, 1.0]])
        p = np.concatenate([key_xy.astype(np.float64), np.ones((nkey, 1))], 1) @ g.T          # key pixel -> frame pixel
        p = p[:, :2] / p[:, 2:3] + rng.integers(-1, 2, (nkey, 2))
        ok = np.flatnonzero((p[:, 0] >= 0) & (p[:, 0] < FRAME_W) & (p[:, 1] >= 0) & (p[:, 1] < FRAME_H))
        extra = max(0, nkey - len(ok) - 7 * f)
        d = np.concatenate([unit(key[ok] + rng.normal(0, 0.02, (len(ok), dim))), unit(rng.normal(size=(extra, dim)))])
        q = np.concatenate([np.rint(p[ok]), np.stack([rng.integers(0, FRAME_W, extra), rng.integers(0, FRAME_H, extra)], 1)])
        o = rng.permutation(len(d))
        counts[f] = len(d)
        desc[f, :len(d)], xy[f, :len(d)] = d[o], q[o].astype(np.int32)
        h = np.linalg.inv(g)
        hs[f] = (h / h[2, 2]).astype(np.float32).reshape(9)
    return dict(key=key, key_xy=key_xy, desc=desc, xy=xy, counts=counts, hs=hs)


def test_culling_visits_what_the_boxes_allow_and_no_less_than_needed():
    e = engine(max_keypoints=0)
    try:
        s = _uniform_scene(e.capacity)
        counts = s["counts"]
        assert 1900 <= counts.min() and len(set(counts.tolist())) > 1
        bounds = {}
        for radius in (4.0, 16.0):
            need = np.array([needed_tiles(s["hs"][f], s["xy"][f, :counts[f]], s["key_xy"], radius, scale=1 - 1e-9).sum()
                             for f in range(N)])
            upper = np.array([visited_tiles(s["hs"][f], s["xy"][f, :counts[f]], s["key_xy"], radius, scale=1 + 1e-9)[2].sum()
                              for f in range(N)])
            grid = np.array([-(-counts[f] // 64) * -(-len(s["key"]) // 64) for f in range(N)])
            print("radius %g: needed %.3f, upper %.3f of the grid" % (radius, need.sum() / grid.sum(), upper.sum() / grid.sum()))
            assert (need <= upper).all() and 2 * upper.sum() <= grid.sum()        # a condition on the input
            bounds[radius] = need, upper, grid
        plant(e, s)
        for radius in (4.0, 16.0):
            need, upper, grid = bounds[radius]
            for cross, md, ratio in ((True, 0.0, 0.0), (False, 0.7, 0.8)):
                m, d, st = _same(e, N, s["hs"], radius, s["key"], s["key_xy"], "key", cross, md, ratio, ("uniform", radius))
                print("radius %g: visited %s" % (radius, st[:, 0].tolist()))
                np.testing.assert_array_equal(st[:, 1], grid)
                assert (need <= st[:, 0]).all() and (st[:, 0] <= upper).all(), (need, st[:, 0], upper)
                assert ratio > 0 or (m >= 0).sum() > 8000          # (Lowe's test needs a second candidate: few rows pass it)
            m2, d2 = e.match_frames_guided_cells_async(N, s["hs"], radius, key=s["key"], key_xy=s["key_xy"], cross_check=False,
                                                       max_dist=0.7, ratio=0.8)         # stats_dev = NULL
            e.sync()
            np.testing.assert_array_equal(_host(m2)[0], m)
        assert e.check_guards() == 0
    finally:
        e.close()


def test_full_chain_on_the_device(planted):
    e, s = planted
    xy, counts = s["xy"], s["counts"]
    params = dict(iterations=256, seed=3)
    for pairing, pcode, with_key in PAIRINGS[:2]:
        key, key_xy = s["key"], s["key_xy"]
        # four calls, no host call in between
        m1, _ = e.match_frames_async(N, key=key, pairing=pairing, cross_check=True)
        h1, n1, _ = e.homography_frames_async(N, m1, key_xy=key_xy, pairing=pairing, **params)
        m2, _ = e.match_frames_guided_cells_async(N, h1, RADIUS, key=key, key_xy=key_xy, pairing=pairing, cross_check=True)
        h2, n2, _ = e.homography_frames_async(N, m2, key_xy=key_xy, pairing=pairing, **params)
        e.sync()
        m2, h1, n1, h2, n2 = _host(m2, h1, n1, h2, n2)
        trains = trains_of(s["desc"], xy, counts, key, key_xy, pcode)
        print(pairing, "inliers", n1, "->", n2)
        assert (n1 >= 8).all() and (n2 >= n1).all() and n2.sum() > n1.sum()
        for f in range(N):
            src, dst = _pairs(m2, xy, counts, f, trains[f][1])
            rh, _ = ransac_rule(src, dst, params, f)
            err = corner_error(h2[f].astype(np.float64), rh)
            print("  frame %d: %d pairs, device H against the restatement's: %.3e px" % (f, len(src), err))
            assert err < MARGIN, (pairing, f, err)


def test_counts_are_read_on_the_device_right_behind_get_points():
    """fpc_get_points, keep_frame, keep_frame_points and both guided calls enqueued back to back (tests/test_gpu_match_guided.py's
    translation scene): the counts the new call orders and matches by are the ones the device holds."""
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
        m, d, st = e.match_frames_guided_cells_async(N, hdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True, stats=True)
        rm, rd = e.match_frames_guided_async(N, hdev, 2.0, key=kept, key_xy=(kept_xy, kept[1]), cross_check=True)
        e.sync()
        res = e.fetch(N)
        counts = np.array([len(r[0]) for r in res])
        assert counts.min() > 500 and len(set(counts.tolist())) > 1
        m, d, st, rm, rd = _host(m, d, st, rm, rd)
        np.testing.assert_array_equal(m, rm)
        np.testing.assert_array_equal(d.view(np.uint32), rd.view(np.uint32))
        np.testing.assert_array_equal(st[:, 1], [-(-k // 64) * -(-counts[0] // 64) for k in counts])
        for f, (ox, oy) in enumerate(offsets):
            rows = np.flatnonzero(m[f, :counts[f]] >= 0)
            assert len(rows) > 200 and (m[f, counts[f]:] == -1).all()
            np.testing.assert_array_equal(res[f][0][rows] + [ox, oy], res[0][0][m[f, rows]])     # the same scene point
        assert e.check_guards() == 0
    finally:
        e.close()


def test_repeated_calls_are_bit_identical(planted):
    e, s = planted
    hs = planted_h(s, PAIR_PREVIOUS)
    outs = []
    for _ in range(3):
        m, d, st = e.match_frames_guided_cells_async(N, hs, RADIUS, key=s["key"], key_xy=s["key_xy"], pairing="previous",
                                                     cross_check=True, max_dist=0.9, stats=True)
        e.sync()
        outs.append(_host(m, d, st))
    assert (outs[0][0] >= 0).sum() > 1000 and (outs[0][2][:, 0] > 0).all()
    for o in outs[1:]:
        np.testing.assert_array_equal(o[0], outs[0][0])
        np.testing.assert_array_equal(o[1].view(np.uint32), outs[0][1].view(np.uint32))
        np.testing.assert_array_equal(o[2], outs[0][2])


def test_bad_arguments_are_refused_and_write_nothing(banked):
    import torch
    e, s = banked
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    mt = torch.full((N + 1, e.capacity), -7, dtype=torch.int32, device=dev)
    ds = torch.full((N + 1, e.capacity), -7.0, dtype=torch.float32, device=dev)
    st = torch.full((N + 1, 2), -7, dtype=torch.int32, device=dev)
    hm = torch.from_numpy(np.tile(np.eye(3, dtype=np.float32).reshape(9), (N + 1, 1))).to(dev)
    key, kc = e._key(s["key"])
    kx, _ = e._key_xy(s["key_xy"])
    slot = torch.zeros((N + 1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    K, P = PAIR_KEY, PAIR_PREVIOUS

    def mg(n=N, pairing=K, k=key.data_ptr(), c=kc.data_ptr(), x=kx.data_ptr(), h=hm.data_ptr(), r=4.0, md=0.0, ratio=0.0,
           out=mt.data_ptr()):
        return lib.fpc_match_frames_guided_cells(ctx, n, pairing, k, c, x, h, r, 1, md, ratio, out, ds.data_ptr(), st.data_ptr())

    def bg(n=N, sl=slot.data_ptr(), h=hm.data_ptr(), r=4.0, md=0.0, ratio=0.0, out=mt.data_ptr()):
        return lib.fpc_match_bank_guided_cells(ctx, n, sl, h, r, 1, md, ratio, out, ds.data_ptr(), st.data_ptr())
    # everything fpc_match_frames refuses
    assert mg(n=N + 1) == FPC_E_INVALID and mg(n=0) == FPC_E_INVALID
    assert mg(pairing=2) == FPC_E_INVALID
    assert mg(md=-1.0) == FPC_E_INVALID and mg(ratio=1.5) == FPC_E_INVALID and mg(ratio=-0.1) == FPC_E_INVALID
    assert mg(out=None) == FPC_E_INVALID
    assert mg(k=None, c=None, x=None) == FPC_E_INVALID                    # FPC_PAIR_KEY without a key
    assert mg(c=None) == FPC_E_INVALID                                    # a key without its count
    assert mg(k=key.data_ptr() + 4) == FPC_E_INVALID                      # not 16-byte aligned
    # and the guided calls' own
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
    # a context without a bank; results without descriptors
    d = engine(b=2)
    try:
        prob = torch.zeros((2, d.h, d.w))
        prob[:, 40, 40] = 0.5
        d.get_points(prob, torch.ones((2, d.desc_dim, d.h // 8, d.w // 8)))
        out = torch.full((2, d.capacity), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        assert lib.fpc_match_bank_guided_cells(d._ctx, 2, slot.data_ptr(), hm.data_ptr(), 4.0, 1, 0.0, 0.0, out.data_ptr(),
                                               None, st.data_ptr()) == FPC_E_INVALID
        d.get_points(prob)
        assert lib.fpc_match_frames_guided_cells(d._ctx, 2, P, None, None, None, hm.data_ptr(), 4.0, 1, 0.0, 0.0,
                                                 out.data_ptr(), None, st.data_ptr()) == FPC_E_INVALID
        d.sync()
        assert (out.cpu().numpy() == -7).all() and (st.cpu().numpy()[N] == -7).all() and d.check_guards() == 0
    finally:
        d.close()


def test_vgg_descriptors():
    """FPC_ARCH_VGG: D = 256, a 240 x 320 frame (10 x 8 cells)."""
    e = engine(240, 320, in_channels=1, arch="vgg")
    try:
        assert e.desc_dim == 256
        s = planted_scene(4, [f10(name, i) for name, i in HOMS], nkey=300, dim=256, cap=e.capacity)
        plant(e, s)
        for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
            hs = planted_h(s, pcode)
            for radius in RADII:
                for cross, md, ratio in ((True, 0.7, 0.0), (False, 0.0, 0.8)):
                    m, _, st = _same(e, N, hs, radius, s["key"], s["key_xy"], pairing, cross, md, ratio, ("vgg", pairing, radius))
            assert (m >= 0).sum() > 500
        assert e.check_guards() == 0
    finally:
        e.close()
