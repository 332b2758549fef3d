"""Relative pose on the GPU (fpc_pose_fundamental / fpc_pose_frames / fpc_pose_bank) against the float64 restatement and the
planted scenes of tests/test_pose_epipolar.py: the device's pose under its own RANSAC F next to the restatement's under the
same F, the planted-truth bars, the tails of the pair list and of the outputs, the frames variant bit-identical to explicit
pairs and the bank variant to the frames variant, determinism and the argument checks.  Every context runs under the canary
zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_fundamental_ransac import FRAME_H, FRAME_W, KINDS, PARAMS
from tests.test_gpu_homography_ransac import _host_pairs, engine
from tests.test_pose_epipolar import (KVEC, ROUNDED_SETS, THR, check_planted_pose, exact_f, pose_batch, pose_rule, pose_scene)

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
KQVGA = (250.0, 250.0, 160.0, 120.0)
# Device against restatement under the SAME fp32 F: both evaluate the rule in fp64 and differ by the contraction of
# a * b + c into one rounding, so the bars are those of the outputs' fp32 format: 1e-6 per entry of R and t (magnitude <= 1,
# resolution 6e-8), 1e-5 of a point's length for xyz.  Measured on the MI355X over the 28 frames of the two case sets: worst
# difference 2.94e-08 in R, 2.96e-08 in t, 5.83e-08 of a point's length in xyz -- half a unit of fp32 rounding of the device's
# outputs, the restatement's not being rounded: below a tenth of either bar.
R_BAR, XYZ_BAR = 1e-6, 1e-5


@pytest.fixture(scope="module")
def vga():
    """A 32-frame VGA context without the descriptor head (explicit pairs need no network); max_keypoints = 1280 so that a
    pair list can cross 4 x 256 pairs and the 1 024-record chunk of the RANSAC kernels."""
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


def _compare(got, f, m, want, tag):
    """Frame f of the device outputs (R, t, nfront, xyz, front) against the restatement's Pose over its m pairs -> the
    worst differences (R, t, relative xyz)."""
    rm, tv, nf, xyz, front = (v[f] for v in got)
    assert not front[m:].any() and not xyz[m:].any(), tag                          # nothing behind the pair count
    assert nf == front.sum(), tag
    dr, dt = np.abs(rm.astype(np.float64) - want.R).max(), np.abs(tv.astype(np.float64) - want.t).max()
    assert dr <= R_BAR and dt <= R_BAR, (tag, dr, dt)
    clear = ~want.near
    np.testing.assert_array_equal(front[:m][clear], want.front[clear], err_msg=str(tag))
    if clear.all():
        assert nf == want.nfront, tag
    both = front[:m] & want.front
    ref = want.xyz[both]
    rel = np.linalg.norm(xyz[:m][both].astype(np.float64) - ref, axis=1) / np.linalg.norm(ref, axis=1) if both.any() else np.zeros(1)
    assert rel.max() <= XYZ_BAR, (tag, rel.max())
    assert not xyz[:m][~front[:m]].any(), tag
    return dr, dt, rel.max()


_DEVICE = {}


def _device_poses(e, rho, iterations):
    """The device's F (its own fpc_ransac_fundamental) and pose of one rounded case set, computed once."""
    if (rho, iterations) not in _DEVICE:
        scenes = pose_batch(rho)
        src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], 640)
        assert len(scenes) == 14 and npairs.max() <= 600 and len(set(npairs.tolist())) > 1
        fm, ni, _ = e.ransac_fundamental_async(src, dst, npairs, iterations=iterations, **PARAMS)
        got = e.pose_fundamental(src, dst, npairs, fm, reproj_threshold=THR)         # F passed on as the device wrote it
        _DEVICE[rho, iterations] = scenes, fm.cpu().numpy(), ni.cpu().numpy(), got
    return _DEVICE[rho, iterations]


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_explicit_call_agrees_with_the_restatement(vga, rho, iterations):
    scenes, fm, ni, got = _device_poses(vga, rho, iterations)
    worst = np.zeros(3)
    for f, scene in enumerate(scenes):
        s, d = scene[0], scene[1]
        assert fm[f].any() and 0 < got[2][f] <= ni[f]          # the threshold F was estimated with: the pairs of its mask
        want = pose_rule(s, d, fm[f].astype(np.float64), KVEC, KVEC, THR)
        assert not want.failed, f
        worst = np.maximum(worst, _compare(got, f, len(s), want, (rho, f)))
        rm = got[0][f].astype(np.float64)
        assert abs(np.linalg.det(rm) - 1.0) < 1e-6 and abs(np.linalg.norm(got[1][f].astype(np.float64)) - 1.0) < 1e-6
    print("rho %.1f: worst device - restatement difference: R %.3e, t %.3e, xyz %.3e relative" % (rho, *worst))


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_device_meets_the_planted_truth_bars(vga, rho, iterations):
    scenes, fm, ni, got = _device_poses(vga, rho, iterations)
    for f, scene in enumerate(scenes):
        m = len(scene[0])
        errs = check_planted_pose(got[0][f], got[1][f], got[2][f], got[3][f, :m], got[4][f, :m], scene, (KINDS[f], f, rho))
        print("rho %.1f frame %2d %-8s: rotation %.4f deg, direction %.4f deg, depth %.5f, %d in front of %d planted"
              % (rho, f, KINDS[f], *errs, got[2][f], scene[2].sum()))


def _raw_pose(e, src, dst, npairs, fm, xyz=True, front=True, fill=0xFF, **params):
    """fpc_pose_fundamental into outputs pre-filled with `fill` bytes -> host arrays (R, t, nfront, xyz, front uint8)."""
    import torch
    dev = e.torch_device
    n, stride = src.shape[0], src.shape[1]
    p = e._pose_params(None, None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (src, dst, npairs, fm.reshape(n, 9).astype(np.float32))]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev)
            for shape in ((n, 36), (n, 12), (n, 4), (n, stride, 12), (n, stride))]
    torch.cuda.synchronize()
    e._call("fpc_pose_fundamental", n, ins[0], ins[1], ins[2], stride, ins[3], ctypes.byref(p), outs[0], outs[1], outs[2],
            outs[3] if xyz else None, outs[4] if front else None, inputs=ins)
    e.sync()
    rm, tv, nf, pts, fr = (o.cpu().numpy() for o in outs)
    return (rm.view(np.float32).reshape(n, 3, 3), tv.view(np.float32).reshape(n, 3), nf.view(np.int32).reshape(n),
            pts.view(np.float32).reshape(n, stride, 3), fr)


def test_tails_of_the_pair_list_and_of_the_outputs(vga):
    e = vga
    cap = e.capacity
    s, d, _, _, _, r, t, _ = pose_scene("general", 2, 0.0, cap)
    f0 = exact_f(r, t)
    f0 = (f0 / np.sqrt((f0 * f0).sum())).astype(np.float32)
    # 1 100 pairs cross 4 x 256 and the 1 024-record chunk; 0, 7 and 8 pairs; a count above the stride is clamped
    lists = [(s[:1100], d[:1100]), (s[:0], d[:0]), (s[:7], d[:7]), (s[:8], d[:8]), (s[:100], d[:100]), (s, d), (s[:300], d[:300])]
    src, dst, npairs = _pack(lists, cap)
    npairs[5] = cap + 9
    fm = np.repeat(f0[None], len(lists), 0)
    fm[6] = 0.0                                                                      # a failed frame of the fundamental call
    got = _raw_pose(e, src, dst, npairs, fm, reproj_threshold=3.0, min_front=8)
    rm, tv, nf, xyz, front = got
    assert set(np.unique(front).tolist()) <= {0, 1}                                  # no 0xFF left: every row was written
    assert np.isfinite(xyz).all() and np.isfinite(rm).all() and np.isfinite(tv).all()
    for f in (1, 2, 6):                                                              # no pairs / below min_front / zero F
        assert not rm[f].any() and not tv[f].any() and nf[f] == 0 and not front[f].any() and not xyz[f].any(), f
    for f, (a, b) in enumerate(lists):
        want = pose_rule(a, b, fm[f].astype(np.float64), KVEC, KVEC, 3.0, 8)
        if f in (1, 2, 6):
            assert want.failed
            continue
        _compare((rm, tv, nf, xyz, front.astype(bool)), f, len(a), want, f)
    assert nf[3] == 8 and front[3, :8].all()
    assert nf[0] >= 0.98 * 1100 and front[0, 1024:1100].sum() >= 0.98 * 76          # the pairs behind the chunk count
    assert nf[5] >= 0.98 * cap and front[5, cap - 1] == 1
    for f, m in ((0, 1100), (3, 8), (4, 100)):                                       # rows past the count: zero bytes
        assert not front[f, m:].any() and not xyz[f, m:].view(np.uint32).any()
    # a stride of its own, not the capacity: the rows of frame f start at f x stride
    src2, dst2, npairs2 = _pack(lists[2:5], 130)
    got2 = _raw_pose(e, src2, dst2, npairs2, fm[2:5], reproj_threshold=3.0, min_front=8)
    for k in range(3):
        np.testing.assert_array_equal(got2[0][k].view(np.uint32), rm[2 + k].view(np.uint32))
        np.testing.assert_array_equal(got2[3][k].view(np.uint32), xyz[2 + k, :130].view(np.uint32))
        np.testing.assert_array_equal(got2[4][k], front[2 + k, :130])
        assert got2[2][k] == nf[2 + k]
    # min_front above what one frame reaches fails that frame only
    got3 = _raw_pose(e, src, dst, npairs, fm, reproj_threshold=3.0, min_front=101)
    assert not got3[0][4].any() and got3[2][4] == 0 and not got3[4][4].any() and not got3[3][4].any()
    np.testing.assert_array_equal(got3[0][[0, 5]].view(np.uint32), rm[[0, 5]].view(np.uint32))
    # a non-finite F fails its frame
    bad = fm.copy()
    bad[0, 1, 1], bad[4, 2, 0] = np.nan, np.inf
    got4 = _raw_pose(e, src, dst, npairs, bad, reproj_threshold=3.0, min_front=8)
    for f in (0, 4):
        assert not got4[0][f].any() and not got4[1][f].any() and got4[2][f] == 0 and not got4[4][f].any() and not got4[3][f].any()
    np.testing.assert_array_equal(got4[3][5].view(np.uint32), xyz[5].view(np.uint32))


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _assert_frames_equal_explicit(e, n, res, match_dev, key_pts, key_xy_host, pairing, **params):
    cap = e.capacity
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    fm, _, _ = e.fundamental_frames_async(n, match_dev, key_xy=key_pts, pairing=pairing, iterations=256, seed=11)
    got = e.pose_frames(n, match_dev, fm, key_xy=key_pts, pairing=pairing, **params)
    empty = np.zeros((0, 2), np.int32)

    def train_of(f):
        if pairing == "previous" and f > 0:
            return xy[f - 1]
        return key_xy_host if key_xy_host is not None else empty
    src, dst, npairs, rows = _host_pairs(match_dev.cpu().numpy(), xy, counts, train_of, cap)
    rm, tv, nf, xyz, front = e.pose_fundamental(src, dst, npairs, fm, **params)
    _bits(got[0], rm)
    _bits(got[1], tv)
    np.testing.assert_array_equal(got[2], nf)
    for f in range(n):
        back_f, back_x = np.zeros(cap, bool), np.zeros((cap, 3), np.float32)
        back_f[rows[f]], back_x[rows[f]] = front[f, :npairs[f]], xyz[f, :npairs[f]]
        np.testing.assert_array_equal(got[4][f], back_f)
        _bits(got[3][f], back_x)
    return got, npairs


def test_frames_variant_is_bit_identical_to_explicit_pairs(qvga):
    e, res = qvga
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    params = dict(K_query=KQVGA, K_train=np.array([[250.0, 0, 160.0], [0, 250.0, 120.0], [0, 0, 1.0]]), min_front=1)
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "key", **params)
    assert npairs.min() > 50 and (got[2] > 0).any()
    m, _ = e.match_frames_async(N, key=key, pairing="previous", cross_check=True)
    got, _ = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "previous", **params)
    assert (got[2] > 0).any()
    m, _ = e.match_frames_async(N, key=None, pairing="previous", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, None, None, "previous", **params)
    assert npairs[0] == 0 and not got[0][0].any() and not got[1][0].any() and got[2][0] == 0    # frame 0 has no train set
    assert not got[3][0].any() and not got[4][0].any()


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
        params = dict(K_query=KQVGA, K_train=KQVGA, min_front=1)
        fm, _, _ = e.fundamental_bank_async(N, slot, m, iterations=256, seed=4)
        # a valid F for the frames without a slot, so that it is the slot that fails them
        fm[1], fm[4] = fm[0], fm[0]
        got = e.pose_bank(N, slot, m, fm, **params)
        sl = slot.cpu().numpy()
        for v in got:
            assert not v[[1, 4]].any()                                               # no slot: the frame fails with zeros
        assert set(sl.tolist()) - {-1, slots} and (got[2] > 0).any()
        _, bx, bc = e.bank_view()
        for s in sorted(set(sl.tolist()) - {-1, slots}):
            rows_of = np.flatnonzero(sl == s)
            ref = e.pose_frames(N, m, fm, key_xy=(bx[s].clone(), bc[s:s + 1].clone()), pairing="key", **params)
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a[rows_of].view(np.uint8), b[rows_of].view(np.uint8))
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_determinism_and_null_point_outputs(vga):
    e = vga
    scenes, fm, _, got = _device_poses(e, *ROUNDED_SETS[0])
    src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], 640)
    again = e.pose_fundamental(src, dst, npairs, fm, reproj_threshold=THR)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (got[2] > 0).all()
    bare = e.pose_fundamental(src, dst, npairs, fm, points=False, reproj_threshold=THR)
    assert bare[3] is None and bare[4] is None
    for a, b in zip(got[:3], bare[:3]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    # one of the two NULL, through the raw call: the other one and R, t, nfront are what they were
    for kw in (dict(xyz=False), dict(front=False)):
        raw = _raw_pose(e, src, dst, npairs, fm, reproj_threshold=THR, **kw)
        _bits(raw[0], got[0])
        _bits(raw[1], got[1])
        np.testing.assert_array_equal(raw[2], got[2])
        if "xyz" in kw:
            assert (raw[3].view(np.uint32) == 0xFFFFFFFF).all()
            np.testing.assert_array_equal(raw[4].astype(bool), got[4])
        else:
            assert (raw[4] == 0xFF).all()
            _bits(raw[3], got[3])
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
    fin = torch.zeros((N, 9), dtype=torch.float32, device=dev)
    fin[:, 8] = 1.0                                                 # e = 1 against zero gradients: no pair passes the Sampson test
    rm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    tv = torch.full((N, 3), 7.0, dtype=torch.float32, device=dev)
    nf = torch.full((N,), 7, dtype=torch.int32, device=dev)
    xyz = torch.full((N, cap, 3), 7.0, dtype=torch.float32, device=dev)
    front = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sp, np_, mp, kp, op, lp, fp = (t.data_ptr() for t in (src, npairs, match, key_pts, one, slot, fin))
    rp, tp, ip, xp, bp = (t.data_ptr() for t in (rm, tv, nf, xyz, front))

    def params(**kw):
        p = _lib.FpcPoseParams()
        lib.fpc_default_pose_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    pf = lambda n, s, d, c, stride, f, p, r, t, i: lib.fpc_pose_fundamental(e._ctx, n, s, d, c, stride, f, p, r, t, i, xp, bp)   # noqa: E731
    ff = lambda n, pairing, k, kc, m, f, p, r, t, i: lib.fpc_pose_frames(e._ctx, n, pairing, k, kc, m, f, p, r, t, i, xp, bp)   # noqa: E731
    fb = lambda n, s, m, f, p, r, t, i: lib.fpc_pose_bank(e._ctx, n, s, m, f, p, r, t, i, xp, bp)   # noqa: E731
    ok = params()
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(q_fx=0.0), params(q_fy=-1.0), params(t_fx=0.0), params(t_fy=-500.0), params(q_fx=nan), params(t_fy=inf),
               params(q_cx=nan), params(q_cy=inf), params(t_cx=-inf), params(t_cy=nan), params(reproj_threshold=0.0),
               params(reproj_threshold=-1.0), params(reproj_threshold=nan), params(min_front=0), params(min_front=-3), None]
        for p in bad:
            assert pf(N, sp, sp, np_, cap, fp, p, rp, tp, ip) == FPC_E_INVALID
            assert ff(N, 0, kp, op, mp, fp, p, rp, tp, ip) == FPC_E_INVALID
            assert fb(N, lp, mp, fp, p, rp, tp, ip) == FPC_E_INVALID
        for k in range(9):                                                           # a NULL in any pointer but xyz / front
            if k == 3:
                continue
            a = [sp, sp, np_, cap, fp, ok, rp, tp, ip]
            a[k] = None
            assert pf(N, *a) == FPC_E_INVALID, k
        assert pf(0, sp, sp, np_, cap, fp, ok, rp, tp, ip) == FPC_E_INVALID
        assert pf(N + 1, sp, sp, np_, cap, fp, ok, rp, tp, ip) == FPC_E_INVALID     # above max_batch
        assert pf(N, sp, sp, np_, cap + 1, fp, ok, rp, tp, ip) == FPC_E_INVALID     # stride above capacity
        assert pf(N, sp, sp, np_, 0, fp, ok, rp, tp, ip) == FPC_E_INVALID
        assert ff(N, 2, kp, op, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID             # pairing
        assert ff(N, 0, None, None, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID         # FPC_PAIR_KEY without key points
        assert ff(N, 0, kp, None, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID           # key points without their count
        for k in (4, 5, 6, 7, 8, 9):
            a = [0, kp, op, mp, fp, ok, rp, tp, ip]
            a[k - 1] = None
            assert ff(N, *a) == FPC_E_INVALID, k
        assert ff(0, 0, kp, op, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        assert ff(N + 1, 0, kp, op, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        for k in range(8):
            a = [lp, mp, fp, ok, rp, tp, ip]
            if k < 7:
                a[k] = None
                assert fb(N, *a) == FPC_E_INVALID, k
        assert fb(0, lp, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        assert fb(N + 1, lp, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert ff(3, 0, kp, op, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        assert fb(3, lp, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        for t in (rm, tv, xyz):
            assert (t.cpu() == 7.0).all()
        assert (nf.cpu() == 7).all() and (front.cpu() == 7).all()
        assert ff(2, 0, kp, op, mp, fp, ok, rp, tp, ip) == 0
        assert ff(2, 1, None, None, mp, fp, ok, rp, tp, ip) == 0                     # PREVIOUS needs no key
        assert fb(2, lp, mp, fp, ok, rp, tp, ip) == 0
        assert pf(N, sp, sp, np_, cap, fp, ok, rp, tp, ip) == 0
        e.sync()
        # no match (frames, bank) or no pair within the threshold of this F (explicit): every frame fails with zeros
        for t in (rm, tv, nf, xyz, front):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
    assert fb(2, lp, mp, fp, ok, rp, tp, ip) == FPC_E_INVALID                        # no bank
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))                                        # (the module's later tests see batch 1 again)
    with pytest.raises(ValueError):
        e.pose_frames(N, match, fin, key_xy=key_pts, pairing="next")
    with pytest.raises(TypeError):
        e.pose_fundamental(src, src, npairs, fin, min_inliers=5)
    with pytest.raises(ValueError):
        e.pose_fundamental(src, src, npairs, fin, K_query=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.pose_bank(N, slot, match, fin)
