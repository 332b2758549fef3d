"""Local bundle adjustment on the GPU (fpc_refine_window / fpc_refine_window_frames / fpc_refine_window_bank) against the
float64 restatement and the planted box scenes of tests/test_refine_window.py: the explicit call next to the restatement
under the same fp32 inputs, the smallest shapes at which the kernels take another path (a staging pass of 8 landmarks, a
chunk of 64, a workgroup of 256 key rows; 1 and 16 frames), the tails of every output, the chain identities (frames =
explicit, bank = frames on either bank format, repeats, aliasing), the reservation, and the chain detect -> match_bank ->
pnp_bank -> refine_window_bank -> bank_store_landmarks -> pnp_bank without a host call.  The context runs under the canary
zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_homography_ransac import engine
from tests.test_refine_window import KVEC, NONE, ORDER_MARGIN, box_scene, refined_set, scene_errors, window_rule

pytestmark = pytest.mark.gpu

FPC_E_INVALID = -1
FRAME_H, FRAME_W, FRAMES = 480, 640, 16
# Device against restatement under the SAME fp32 inputs: test_gpu_refine_pose.py's bars, for its reasons -- both sides evaluate
# the rule in fp64 and round the state to fp32 behind every attempt, and differ by the order of the sums, which a rounding of
# the state can turn into one fp32 ulp of a state entry: 1e-5 for R and t, 1e-4 of a point's length for xyz, with the same
# attempt and accept counts.  A scene off the restatement's path is reported and held to the fallback bound, four times the
# restatement's ascending-against-descending difference (tests/test_refine_window.py: zero).
R_BAR, XYZ_BAR = 1e-5, 1e-4
CAMS = dict(K_query=KVEC, K_train=KVEC)


@pytest.fixture(scope="module")
def win():
    """A 16-frame VGA context whose last call left 16 frames of results (with descriptors); a call before the reservation
    is refused (the fixture records it), then the reservation is made."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, FRAMES, max_keypoints=320)
    prob = torch.zeros((FRAMES, FRAME_H, FRAME_W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((FRAMES, e.desc_dim, FRAME_H // 8, FRAME_W // 8)))
    sc = box_scene(1, 2)
    with pytest.raises(_lib.FpcError) as refused:
        e.refine_window(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, **CAMS)
    e.refused_before_reservation = (refused.value.code, str(refused.value))
    plan = e._l.fpc_plan_hash(e._ctx)
    assert e.window_reserve() >= 16 * e.capacity * 12
    assert e._l.fpc_plan_hash(e._ctx) == plan                                        # nothing is carved
    with pytest.raises(_lib.FpcError):
        e.window_reserve()                                                           # a second reserve is refused
    e.pnp_reserve()
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _same(got, want):
    for a, b in zip(got, want):
        _bits(a, b)


def _padded(sc, cap):
    """The scene's key arrays padded to the capacity (rows behind the key's count hold valid-looking garbage)."""
    n = len(sc.x0)
    key_xy, key_xyz = np.full((cap, 2), 100.0, np.float32), np.full((cap, 3), 4.0, np.float32)
    key_xy[:n], key_xyz[:n] = sc.key_xy, sc.x0
    return key_xy, key_xyz


def _raw(e, sc, nkey=None, key_valid=None, fill=0xFF, pad=64, **params):
    """fpc_refine_window into outputs pre-filled with `fill` bytes and `pad` bytes longer than the call may write -> host
    arrays (R, t, nobs, xyz, kind, obs, stats) and the pad bytes of every output."""
    import torch
    dev, cap = e.torch_device, e.capacity
    n, stride = sc.idx.shape
    p = e._window_params(KVEC, KVEC, params)
    key_xy, key_xyz = _padded(sc, cap)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (
        sc.xy.astype(np.float32), sc.idx.astype(np.int32), sc.nobs.astype(np.int32), key_xy, key_xyz,
        np.ones(cap, np.uint8) if key_valid is None else key_valid, np.array([len(sc.x0) if nkey is None else nkey], np.int32),
        sc.r0.astype(np.float32), sc.t0.astype(np.float32))]
    sizes = (n * 36, n * 12, n * 4, cap * 12, cap, n * stride, 16)
    outs = [torch.full((s + pad,), fill, dtype=torch.uint8, device=dev) for s in sizes]
    torch.cuda.synchronize()
    e._call("fpc_refine_window", n, ins[0], ins[1], ins[2], stride, ins[3], ins[4], ins[5], ins[6], ins[7], ins[8],
            ctypes.byref(p), *outs, inputs=ins)
    e.sync()
    host = [o.cpu().numpy() for o in outs]
    tails = [h[s:] for h, s in zip(host, sizes)]
    r, t, nobs, xyz, kind, obs, stats = (h[:s] for h, s in zip(host, sizes))
    return (r.view(np.float32).reshape(n, 3, 3), t.view(np.float32).reshape(n, 3), nobs.view(np.int32), xyz.view(np.float32).reshape(cap, 3),
            kind, obs.reshape(n, stride), stats.view(np.float32)), tails


def _rule(sc, cap, **kw):
    key_xy, key_xyz = _padded(sc, cap)
    kw.setdefault("nkey", len(sc.x0))
    return window_rule(sc.xy, sc.idx, sc.nobs, key_xy, key_xyz, sc.r0, sc.t0, **kw)


def _compare(got, want, tag):
    """The device outputs against the restatement's Window -> (worst differences R, t, relative xyz; the same path?)."""
    rm, tv, nobs, xyz, kind, obs, stats = got
    obs = obs.astype(bool)
    rows = len(want.kind)                                                           # (a restatement without the padding)
    assert not kind[rows:].any() and not xyz[rows:].any(), tag
    xyz, kind = xyz[:rows], kind[:rows]
    assert not want.near, tag
    assert set(np.unique(kind).tolist()) <= {0, 1, 2} and not xyz[kind == 0].any(), tag
    if want.failed:
        assert not rm.any() and not tv.any() and not nobs.any() and not obs.any() and not stats.any(), tag
        np.testing.assert_array_equal(kind, want.kind)
        np.testing.assert_array_equal(xyz, want.xyz.astype(np.float32))
        return 0.0, 0.0, 0.0, True
    np.testing.assert_array_equal(rm.reshape(len(rm), -1).any(1), want.kept, err_msg=str(tag))
    assert not tv[~want.kept].any() and not nobs[~want.kept].any() and not obs[~want.kept].any(), tag
    assert abs(stats[0] - want.stats[0]) <= 1e-6 * want.stats[0], (tag, stats, want.stats)
    same = stats[2] == want.stats[2] and stats[3] == want.stats[3]
    clear = ~want.edge
    np.testing.assert_array_equal(kind[clear], want.kind[clear], err_msg=str(tag))
    np.testing.assert_array_equal(kind == 2, want.kind == 2, err_msg=str(tag))
    _bits(xyz[want.kind == 2], want.xyz[want.kind == 2].astype(np.float32))           # untouched landmarks: copied
    assert nobs.tolist() == obs.sum(1).tolist(), tag
    if not want.edge.any():
        np.testing.assert_array_equal(obs, want.obs, err_msg=str(tag))
    dr, dt = np.abs(rm.astype(np.float64) - want.R).max(), np.abs(tv.astype(np.float64) - want.t).max()
    both = (kind == 1) & (want.kind == 1)
    ref = want.xyz[both]
    rel = (np.linalg.norm(xyz[both].astype(np.float64) - ref, axis=1) / np.linalg.norm(ref, axis=1)).max() if both.any() else 0.0
    assert stats[1] <= stats[0], (tag, stats)
    if same:
        assert dr <= R_BAR and dt <= R_BAR and rel <= XYZ_BAR, (tag, dr, dt, rel)
    else:
        print("OFF THE RESTATEMENT'S PATH:", tag, stats, want.stats, dr, dt, rel)
        assert dr <= 4 * ORDER_MARGIN[0] and dt <= 4 * ORDER_MARGIN[1] and rel <= 4 * ORDER_MARGIN[2], (tag, dr, dt, rel)
    return dr, dt, rel, same


def _tails_intact(tails, tag):
    for i, tl in enumerate(tails):
        assert (tl == 0xFF).all(), (tag, i)


def test_a_call_before_the_reservation_is_refused(win):
    code, text = win.refused_before_reservation
    assert code == FPC_E_INVALID and text.startswith("fpc_refine_window:"), win.refused_before_reservation


@pytest.mark.parametrize("share", (0.0, 0.3))
def test_explicit_call_agrees_with_the_restatement(win, share):
    scenes, refined = refined_set(share)
    worst, off = np.zeros(3), []
    before, after = [], []
    for i, (sc, want) in enumerate(zip(scenes, refined)):
        got, tails = _raw(win, sc)
        _tails_intact(tails, (share, i))
        dr, dt, dx, same = _compare(got, want, (share, i, sc.frames))
        if same:
            worst = np.maximum(worst, (dr, dt, dx))
        else:
            off.append(i)
        n = len(sc.x0)
        before.append(scene_errors(sc, sc.r0, sc.t0, sc.x0, np.where(want.active[:n], 1, 0)))
        after.append(scene_errors(sc, got[0], got[1], got[3][:n], got[4][:n]))
        assert 1 <= got[6][3] <= got[6][2] <= 8 and got[6][1] < got[6][0], (i, got[6])
    before, after = np.array(before), np.array(after)
    print("share %.1f: %d of %d scenes on the restatement's path (off: %s); worst |dR| %.3e, |dt| %.3e, relative |dX| %.3e"
          % (share, len(scenes) - len(off), len(scenes), off, *worst))
    print("share %.1f on the device: mean rotation error %.4f -> %.4f deg, mean median point error %.4f -> %.4f"
          % (share, before[:, 0].mean(), after[:, 0].mean(), before[:, 1].mean(), after[:, 1].mean()))
    assert after[:, 0].mean() < before[:, 0].mean() and after[:, 1].mean() < before[:, 1].mean()


def _edge_scene(seed, frames, landmarks):
    """A scene for the shape cases: duplicate rows, a landmark no frame sees, and (from 3 frames on) a frame without
    observations in the middle of the window."""
    sc = box_scene(seed, frames, landmarks=landmarks, stride=landmarks + 8)
    for f in range(frames):
        m = int(sc.nobs[f])
        rows = np.flatnonzero(sc.idx[f, :m] == 2)
        sc.idx[f, rows] = -1                                                         # landmark 2: seen by no frame
        k = min(6, m)                                                                # (m > 6 in every case below)
        sc.idx[f, m:m + k], sc.xy[f, m:m + k] = sc.idx[f, :k], sc.xy[f, :k] + 1.0     # duplicates, a pixel off: the lower row wins
        sc.nobs[f] = m + k
    if frames >= 3:
        sc.nobs[frames // 2] = 0
    return sc


@pytest.mark.parametrize("frames,landmarks", [(1, 100), (4, 7), (4, 8), (4, 9), (16, 63), (16, 64), (16, 65), (3, 255), (3, 256),
                                              (3, 257)])
def test_smallest_shapes_that_can_go_wrong(win, frames, landmarks):
    sc = _edge_scene(31 * frames + landmarks, frames, landmarks)
    cap = win.capacity
    assert landmarks < cap                                                          # nkey below the capacity
    want = _rule(sc, cap, min_obs=3)
    got, tails = _raw(win, sc, min_obs=3)
    _tails_intact(tails, (frames, landmarks))
    _compare(got, want, (frames, landmarks))
    assert want.kind[2] == 2 and got[4][2] == 2 and not got[4][landmarks:].any() and not got[3][landmarks:].any()
    if frames >= 3:
        assert not want.kept[frames // 2] and not got[0][frames // 2].any() and want.kept.sum() == frames - 1
    if frames == 16:
        assert ((want.tab != NONE).sum(0) == 15).any()                              # a landmark every kept frame sees
    k = min(6, int(sc.nobs[0]) // 2)
    m = int(sc.nobs[0]) - k
    assert not (got[5][0, m:m + k] & got[5][0, :k]).any() and got[5][0, :k].any()   # a duplicate loses to a lower member row
    again, _ = _raw(win, sc, min_obs=3)
    _same(again, got)                                                               # repeated calls: the same bits


def _plant(e, sc):
    """The scene's integer pixels and counts in place of the last call's results -> the match table (device, int32
    [n,cap]); stride == capacity, so that pair k of the explicit call is query row k."""
    import torch
    n, cap = sc.idx.shape
    assert cap == e.capacity
    xy, count = e._points_view()
    xy[:n].copy_(torch.from_numpy(sc.xy.astype(np.int32)))
    count[:n].copy_(torch.from_numpy(sc.nobs.astype(np.int32)))
    torch.cuda.synchronize()
    return torch.from_numpy(sc.idx.astype(np.int32)).to(e.torch_device)


def test_frames_and_bank_calls_are_bit_identical_to_the_explicit_call(win):
    import torch
    e = win
    cap, dev = e.capacity, e.torch_device
    sc = box_scene(77, 6, share=0.3, landmarks=200, stride=cap)
    sc.r0[4] = 0.0                                                                   # a dead frame among them
    match = _plant(e, sc)
    key_xy, key_xyz = _padded(sc, cap)
    valid = np.ones(cap, np.uint8)
    valid[11] = 0
    nkey = torch.tensor([200], dtype=torch.int32, device=dev)
    kx = (torch.from_numpy(key_xy.astype(np.int32)).to(dev), nkey)
    kz = (torch.from_numpy(key_xyz).to(dev), nkey)
    ref, _ = _raw(e, sc, key_valid=valid)
    assert ref[0][0].any() and not ref[0][4].any() and ref[4][11] == 0 and (ref[4][:200] == 1).sum() > 150
    got = e.refine_window_frames(6, match, sc.r0, sc.t0, kx, kz, valid, **CAMS)
    _same(got, ref)
    _same(e.refine_window_frames(6, match, sc.r0, sc.t0, kx, kz, valid, **CAMS), got)            # repeated
    _same(e.refine_window_frames(6, match, sc.r0, sc.t0, kx, kz, valid, alias=True, **CAMS), got)  # outputs over the inputs
    wrapped = e.refine_window(sc.xy, sc.idx, sc.nobs, key_xy, kz, sc.r0, sc.t0, valid, alias=True, **CAMS)
    _same(wrapped, ref)
    # the bank: slot 1 holds the key's rows (any descriptors) and its landmarks; frame 2's best is another slot
    desc = np.random.default_rng(1).normal(size=(200, e.desc_dim)).astype(np.float32)
    slot = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.int32, device=dev)
    one = torch.tensor([1], dtype=torch.int32, device=dev)
    r2 = sc.r0.copy()
    r2[2] = 0.0
    want2 = e.refine_window_frames(6, match, r2, sc.t0, kx, kz, valid, **CAMS)
    assert not want2[0][2].any() and want2[0][1].any()
    banks = {}
    for fmt in ("f32", "bf16"):
        e.bank_create(2, cap, format=fmt)
        try:
            e.bank_store_rows(1, desc, key_xy[:200].astype(np.int32))
            e.bank_store_rows(0, desc[:50], key_xy[:50].astype(np.int32))
            none = e.refine_window_bank(6, one, match, sc.r0, sc.t0, **CAMS)       # no landmark storage: the call fails
            assert not none[0].any() and not none[2].any() and not none[4].any() and not none[6].any()
            e.bank_landmarks_reserve()
            e.bank_store_landmarks(1, key_xyz, valid)
            _same(e.refine_window_bank(6, one, match, sc.r0, sc.t0, **CAMS), got)
            banks[fmt] = e.refine_window_bank(6, 1, match, sc.r0, sc.t0, slot=slot, **CAMS)
            _same(banks[fmt], want2)
            _same(e.refine_window_bank(6, 1, match, sc.r0, sc.t0, slot=slot, **CAMS), banks[fmt])
            out = e.refine_window_bank(6, 5, match, sc.r0, sc.t0, **CAMS)          # a key slot outside the bank: fails
            assert not out[0].any() and not out[4].any() and not out[3].any()
            assert e.check_guards() == 0
        finally:
            e.bank_destroy()
    _same(banks["bf16"], banks["f32"])


def test_bad_arguments_are_refused(win):
    e = win
    sc = box_scene(5, 2)
    for bad in (dict(min_obs=2), dict(iterations=0), dict(iterations=17), dict(lambda0=0.0), dict(lambda0=float("inf")),
                dict(reproj_threshold=0.0), dict(K_query=(0.0, 500.0, 320.0, 240.0)), dict(K_train=(500.0, float("nan"), 320.0, 240.0))):
        kw = dict(CAMS)
        kw.update(bad)
        with pytest.raises(Exception):
            e.refine_window(sc.xy, sc.idx, sc.nobs, sc.key_xy, sc.x0, sc.r0, sc.t0, **kw)
    lib, p = e._l, e._window_params(KVEC, KVEC, {})
    import torch
    buf = torch.zeros(4096, dtype=torch.float32, device=e.torch_device)
    d = buf.data_ptr()
    args = [d, d, d, 8, d, d, None, d, d, d, ctypes.byref(p), d, d, d, d, d, None, None]
    assert lib.fpc_refine_window(e._ctx, 17, *args) == FPC_E_INVALID                # n > 16
    assert lib.fpc_refine_window(e._ctx, 0, *args) == FPC_E_INVALID
    for hole in (0, 1, 2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15):                    # every required pointer
        holed = list(args)
        holed[hole] = None
        assert lib.fpc_refine_window(e._ctx, 2, *holed) == FPC_E_INVALID, hole
    assert lib.fpc_refine_window_frames(e._ctx, 2, d, d, d, None, None, d, d, ctypes.byref(p), d, d, d, d, d, None, None) == FPC_E_INVALID
    assert lib.fpc_refine_window_bank(e._ctx, 2, d, None, d, d, d, ctypes.byref(p), d, d, d, d, d, None, None) == FPC_E_INVALID   # no bank
    assert e.check_guards() == 0


def test_chain_end_to_end_improves_its_own_map(win):
    """Planted frames (their descriptors, pixels and counts in place of a detect's results, as the chain tests of the other
    families plant theirs) -> fpc_match_bank -> fpc_pnp_bank -> fpc_refine_window_bank -> fpc_bank_store_landmarks ->
    fpc_pnp_bank again, with no host call in between: the second PnP finds no fewer inliers in any frame."""
    import torch
    e = win
    cap, dev, n = e.capacity, e.torch_device, 6
    sc = box_scene(91, n, landmarks=240, stride=cap, depth_noise=0.04)
    rng = np.random.default_rng(4)
    d = rng.normal(size=(240, e.desc_dim)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    frames_desc = np.zeros((n, cap, e.desc_dim), np.float32)
    for f in range(n):
        m = int(sc.nobs[f])
        frames_desc[f, :m] = d[sc.idx[f, :m]]
    _plant(e, sc)
    desc, _ = e._results_view()
    desc[:n].copy_(torch.from_numpy(frames_desc))
    key_xy, key_xyz = _padded(sc, cap)
    e.bank_create(2, cap)
    try:
        e.bank_landmarks_reserve()
        e.bank_store_rows(0, d, key_xy[:240].astype(np.int32))
        e.bank_store_landmarks(0, key_xyz, np.arange(cap) < 240)
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the counts are read
        score, best, match, _ = e.match_bank_async(n, cross_check=True, max_dist=0.5)
        pnp = dict(K=KVEC, iterations=256, reproj_threshold=3.0, seed=5)
        r1, t1, n1, _ = e.pnp_bank_async(n, best, match, **pnp)
        rw = e.refine_window_bank_async(n, best[:1], match, r1, t1, slot=best, **CAMS)
        e.bank_store_landmarks(0, rw[3], rw[4])
        r2, t2, n2, _ = e.pnp_bank_async(n, best, match, **pnp)
        best, n1, n2, kind, stats, nobs = e._host((best, n1, n2, rw[4], rw[6], rw[2]))
        print("chain: inliers %s -> %s, window rms %.3f -> %.3f px, %d attempts, %d accepted, %d refined, observations %s"
              % (n1.tolist(), n2.tolist(), stats[0], stats[1], stats[2], stats[3], (kind == 1).sum(), nobs.tolist()))
        assert (best == 0).all() and (n1 > 100).sum() >= 4                          # (a frame the first PnP loses may come back)
        assert (kind[:240] == 1).sum() > 200 and stats[3] >= 1 and stats[1] < stats[0]
        assert (n2 >= n1).all(), (n1, n2)
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
