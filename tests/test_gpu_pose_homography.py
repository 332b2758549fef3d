"""Relative pose from a homography on the GPU (fpc_pose_homography / fpc_pose_homography_frames / fpc_pose_homography_bank)
against the float64 restatement and the planted scenes of tests/test_pose_homography.py: the device's outputs under its own
RANSAC H next to the restatement's under the same H, the planted-truth bars, the tails of the pair list and of the outputs,
the frames variant bit-identical to explicit pairs and the bank variant to the frames variant, determinism, the shared
workspace, the chain into the bank's landmarks and the argument checks.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes
import types

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_gpu_homography_ransac import _host_pairs, engine
from tests.test_gpu_match_guided import plant
from tests.test_homography_ransac import FRAME_H, FRAME_W
from tests.test_pose_homography import (FAILED, KVEC, ROTATION, SEEDS, SIZES, SMALL, THR, TWOFOLD, UNIQUE, check_planted,
                                        exact_h, plane_scene, pose_h_rule, scene_of, solution_errors, within_bars)

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1
KQVGA = (250.0, 250.0, 160.0, 120.0)
# Device against restatement under the SAME fp32 H: both evaluate the rule in fp64 and differ by the contraction of
# a * b + c into one rounding, so the bars are those of the outputs' fp32 format: 1e-6 per entry of R, t and N (magnitude
# <= 1, resolution 6e-8), 1e-5 relative for d, 1e-5 of a point's length for xyz.  Measured on the MI355X over the 40 frames
# of the two shares: worst difference 2.98e-08 in R, 2.97e-08 in t, 2.98e-08 in N, 5.25e-08 relative in d, 5.86e-08 of a
# point's length in xyz -- half a unit of fp32 rounding of the device's outputs, the restatement's not being rounded: below
# a tenth of every bar.  kind, the counts and front are equal on every frame, and no pair of these scenes lies within 1e-9
# relative of a threshold (the square roots next to the lambda conditions moved nothing: lambda1 - 1 and 1 - lambda3 are
# above 0.01 on every scene).
R_BAR, D_BAR, XYZ_BAR = 1e-6, 1e-5, 1e-5
H_PARAMS = dict(iterations=256, seed=3, min_inliers=4)


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


def _frame(got, f):
    """Frame f of the device outputs as an object with the restatement's field names."""
    kind, rm, tv, pl, nf, npl, xyz, front = (None if v is None else v[f] for v in got)
    return types.SimpleNamespace(kind=int(kind), R=rm, t=tv, plane=pl, nfront=nf, nplane=npl, xyz=xyz, front=front)


def _compare(got, f, m, want, tag):
    """Frame f of the device outputs against the restatement's PoseH over its m pairs -> the worst differences (R, t, N,
    relative d, relative xyz)."""
    g = _frame(got, f)
    assert not g.front[m:].any() and not g.xyz[m:].any(), tag                      # nothing behind the pair count
    assert want.near.sum() <= 0.02 * max(m, 1), (tag, want.near.sum())
    clear = ~want.near
    front = g.front[:m].astype(bool)
    np.testing.assert_array_equal(front[clear], want.front[clear], err_msg=str(tag))
    slack = int(want.near.sum())
    assert np.abs(g.nfront - want.nfront).max() <= slack and np.abs(g.nplane - want.nplane).max() <= slack, \
        (tag, g.nfront, want.nfront, g.nplane, want.nplane)
    if slack == 0:
        assert g.kind == want.kind, (tag, g.kind, want.kind)
    if g.kind == want.kind == ROTATION or (g.kind == want.kind and slack == 0):
        diffs = [np.abs(g.R.astype(np.float64) - want.R).max(), np.abs(g.t.astype(np.float64) - want.t).max(),
                 np.abs(g.plane[:, :3].astype(np.float64) - want.plane[:, :3]).max()]
        dd = np.abs(g.plane[:, 3].astype(np.float64) - want.plane[:, 3]) / np.maximum(want.plane[:, 3], 1e-300)
        diffs.append(float(dd[want.plane[:, 3] > 0].max(initial=0.0)))
        assert not g.plane[:, 3][want.plane[:, 3] == 0].any(), tag
        assert max(diffs[:3]) <= R_BAR and diffs[3] <= D_BAR, (tag, diffs)
    else:
        diffs = [0.0] * 4
    both = front & want.front
    ref = want.xyz[both]
    rel = np.linalg.norm(g.xyz[:m][both].astype(np.float64) - ref, axis=1) / np.linalg.norm(ref, axis=1) if both.any() else np.zeros(1)
    assert rel.max() <= XYZ_BAR, (tag, rel.max())
    assert not g.xyz[:m][~front].any(), tag
    return (*diffs, rel.max())


_DEVICE = {}


def _device_poses(e, share):
    """The 20 integer-pixel scenes of one off-plane share, the device's H of them (its own fpc_ransac_homography) and its
    pose under that H, computed once.  min_front is per call, so the frames of 8 pairs come from a call of their own."""
    if share not in _DEVICE:
        scenes = [(m, seed, scene_of(m, seed, share)) for m in SIZES for seed in SEEDS]
        src, dst, npairs = _pack([(s["src"], s["dst"]) for _, _, s in scenes], 1104)
        hm, ni, _ = e.ransac_homography_async(src, dst, npairs, **H_PARAMS)
        calls = {mf: e.pose_homography(src, dst, npairs, hm, min_front=mf) for mf in sorted({SMALL.get(m, 8) for m in SIZES})}
        got = [v.copy() for v in calls[8]]
        for f, (m, _, _) in enumerate(scenes):
            for a, b in zip(got, calls[SMALL.get(m, 8)]):
                a[f] = b[f]
        _DEVICE[share] = scenes, hm.cpu().numpy(), ni.cpu().numpy(), got
    return _DEVICE[share]


@pytest.mark.parametrize("share", [0.0, 0.15])
def test_explicit_call_agrees_with_the_restatement(vga, share):
    scenes, hm, ni, got = _device_poses(vga, share)
    worst = np.zeros(5)
    for f, (m, seed, s) in enumerate(scenes):
        assert hm[f].any() and ni[f] >= 4, (f, ni[f])
        want = pose_h_rule(s["src"], s["dst"], hm[f].astype(np.float64), KVEC, KVEC, THR, SMALL.get(m, 8))   # H as written
        assert want.kind in (UNIQUE, TWOFOLD), (f, want.kind)
        worst = np.maximum(worst, _compare(got, f, m, want, (share, m, seed)))
        for j in range(2 if got[0][f] == TWOFOLD else 1):
            assert abs(np.linalg.det(got[1][f, j].astype(np.float64)) - 1.0) < 1e-6
            assert abs(np.linalg.norm(got[2][f, j].astype(np.float64)) - 1.0) < 1e-6
    print("share %.2f: worst device - restatement difference: R %.3e, t %.3e, N %.3e, d %.3e relative, xyz %.3e relative"
          % (share, *worst))


@pytest.mark.parametrize("share", [0.0, 0.15])
def test_device_meets_the_planted_truth_bars(vga, share):
    scenes, hm, ni, got = _device_poses(vga, share)
    for f, (m, seed, s) in enumerate(scenes):
        g = _frame(got, f)
        errs = check_planted(g, g.xyz[:m], g.front[:m].astype(bool), s, share, (m, seed, share), SMALL.get(m, 8))
        print("share %.2f M %4d seed %d: kind %d, rotation %.4f deg, direction %.4f deg, normal %.4f deg, d %.5f, depth %.5f, "
              "support %s, plane pairs %s" % (share, m, seed, g.kind, *errs, g.nfront.tolist(), g.nplane.tolist()))


def test_pure_rotation_on_the_device(vga):
    e = vga
    scenes = [plane_scene(seed, 0.15, 200, pure_rotation=True) for seed in range(6)]
    src, dst, npairs = _pack([(s["src"], s["dst"]) for s in scenes], 256)
    hm, ni, _ = e.ransac_homography_async(src, dst, npairs, **H_PARAMS)
    got = e.pose_homography(src, dst, npairs, hm)
    hm = hm.cpu().numpy()
    from tests.test_pose_epipolar import angle_deg
    from tests.test_pose_homography import PURE_ROT_BAR
    for f, s in enumerate(scenes):
        want = pose_h_rule(s["src"], s["dst"], hm[f].astype(np.float64))
        assert want.kind == ROTATION and got[0][f] == ROTATION, (f, want.kind, got[0][f], want.b)
        _compare(got, f, 200, want, ("rotation", f))
        err = angle_deg((np.trace(got[1][f, 0].astype(np.float64) @ s["R"].T) - 1.0) / 2.0)
        assert err <= PURE_ROT_BAR, (f, err)
        for v in (got[1][f, 1], got[2][f], got[3][f], got[4][f], got[5][f], got[6][f], got[7][f]):
            assert not v.any(), f                                                    # everything else of the frame is zero


OUT_BYTES = (4, 72, 24, 32, 8, 8)           # kind, R, t, plane, nfront, nplane of one frame


def _raw(e, src, dst, npairs, hm, skip=(), fill=0xFF, **params):
    """fpc_pose_homography into outputs pre-filled with `fill` bytes, each one frame longer than the call's n -> host arrays
    (kind, R, t, plane, nfront, nplane, xyz, front uint8) of the n frames, and the untouched-tail check is done here.
    skip: names of the optional outputs to pass as NULL."""
    import torch
    dev = e.torch_device
    n, stride = src.shape[0], src.shape[1]
    p = e._pose_h_params(None, None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (src, dst, npairs, hm.reshape(n, 9).astype(np.float32))]
    outs = [torch.full((n + 1, b), fill, dtype=torch.uint8, device=dev) for b in OUT_BYTES + (stride * 12, stride)]
    names = ("kind", "R", "t", "plane", "nfront", "nplane", "xyz", "front")
    torch.cuda.synchronize()
    e._call("fpc_pose_homography", n, ins[0], ins[1], ins[2], stride, ins[3], ctypes.byref(p),
            *[None if k in skip else o for k, o in zip(names, outs)], inputs=ins)
    e.sync()
    host = [o.cpu().numpy() for o in outs]
    for k, o in zip(names, host):
        assert (o[n] == fill).all(), k                                               # nothing behind the last frame's rows
        if k in skip:
            assert (o == fill).all(), k
    kind, rm, tv, pl, nf, npl, pts, fr = (o[:n] for o in host)
    return (kind.view(np.int32).reshape(n), rm.view(np.float32).reshape(n, 2, 3, 3), tv.view(np.float32).reshape(n, 2, 3),
            pl.view(np.float32).reshape(n, 2, 4), nf.view(np.int32).reshape(n, 2), npl.view(np.int32).reshape(n, 2),
            pts.view(np.float32).reshape(n, stride, 3), fr)


def _h32(s):
    hm = exact_h(s)
    return (hm / hm[2, 2]).astype(np.float32)


def test_tails_of_the_pair_list_and_of_the_outputs(vga):
    e = vga
    cap = e.capacity
    s = plane_scene(1, 0.15, cap)
    a, b = s["src"], s["dst"]
    h0 = _h32(s)
    sizes = [1, 4, 255, 256, 300, 257, 1024, 1025, cap, cap]
    lists = [(a[:k], b[:k]) for k in sizes]
    src, dst, npairs = _pack(lists, cap)
    npairs[9] = cap + 9                                                              # a count above the stride is clamped
    hm = np.repeat(h0[None], len(lists), 0)
    hm[4] = 0.0                                                                      # a failed frame of the homography call
    got = _raw(e, src, dst, npairs, hm, min_front=1)
    kind, rm, tv, pl, nf, npl, xyz, front = got
    assert set(np.unique(front).tolist()) <= {0, 1}                                  # no 0xFF left: every row was written
    assert all(np.isfinite(v).all() for v in (rm, tv, pl, xyz))
    for v in got:
        assert not v[4].any()                                                        # the zero H: FAILED, zeros
    for f, (x, y) in enumerate(lists):
        want = pose_h_rule(x, y, hm[f].astype(np.float64), min_front=1)
        assert (want.kind == FAILED and want.zeros) if f == 4 else want.kind in (UNIQUE, TWOFOLD), (f, want.kind)
        _compare(got, f, len(x), want, f)
        assert not front[f, len(x):].any() and not xyz[f, len(x):].view(np.uint32).any()        # rows past the count: zero bytes
    assert nf[6, 0] >= 0.95 * 1024 and nf[7, 0] >= 0.95 * 1025 and front[7, 1024] + front[7, 1023] >= 1
    assert nf[8, 0] >= 0.95 * cap and front[8, cap - 20:].sum() >= 15              # the pairs behind the chunk count
    for v in got:
        np.testing.assert_array_equal(v[9:10].view(np.uint8), v[8:9].view(np.uint8))   # the clamped count: the full list
    # a stride of its own, not the capacity: the rows of frame f start at f x stride
    src2, dst2, npairs2 = _pack(lists[2:6], 330)
    got2 = _raw(e, src2, dst2, npairs2, hm[2:6], min_front=1)
    for k in range(4):
        for v2, v in zip(got2[:6], got[:6]):
            np.testing.assert_array_equal(v2[k:k + 1].view(np.uint8), v[2 + k:3 + k].view(np.uint8))
        np.testing.assert_array_equal(got2[6][k].view(np.uint32), xyz[2 + k, :330].view(np.uint32))
        np.testing.assert_array_equal(got2[7][k], front[2 + k, :330])
    # the optional outputs as NULL, one at a time and together: the others are what they were
    names = ("kind", "R", "t", "plane", "nfront", "nplane", "xyz", "front")
    for skip in (("plane",), ("nplane",), ("xyz",), ("front",), ("plane", "nplane", "xyz", "front")):
        raw = _raw(e, src, dst, npairs, hm, skip=skip, min_front=1)
        for k, v2, v in zip(names, raw, got):
            if k not in skip:
                np.testing.assert_array_equal(v2.view(np.uint8), v.view(np.uint8), err_msg=k)
    # which = 1 writes solution 1's points; R, t, the plane and the counts do not move
    other = _raw(e, src, dst, npairs, hm, min_front=1, which=1)
    for v2, v in zip(other[:6], got[:6]):
        np.testing.assert_array_equal(v2.view(np.uint8), v.view(np.uint8))
    for f in (2, 6, 8):
        want = pose_h_rule(*lists[f], hm[f].astype(np.float64), min_front=1, which=1)
        _compare(other, f, len(lists[f][0]), want, ("which", f))
        assert other[7][f].sum() == nf[f, 1] and (kind[f] == TWOFOLD) == bool(other[7][f].any())
    # min_front above what a candidate keeps drops it; above every candidate's the frame fails, and that frame only
    top = _raw(e, src, dst, npairs, hm, min_front=int(npl[5].max()) + 1)
    for v in top:
        assert not v[[0, 1, 2, 3, 4, 5]].any()
    for v2, v in zip(top, got):
        np.testing.assert_array_equal(v2[[6, 7, 8]].view(np.uint8), v[[6, 7, 8]].view(np.uint8))
    # a non-finite H and a rank-2 H fail their frames
    bad = hm.copy()
    bad[0, 1, 1], bad[6, 2, 0] = np.nan, np.inf
    x0 = np.array([100.0, 90.0, 1.0])
    bad[8] = (h0.astype(np.float64) - np.outer(h0.astype(np.float64) @ x0, x0) / (x0 @ x0)).astype(np.float32)
    got4 = _raw(e, src, dst, npairs, bad, reproj_threshold=1e6, min_front=1)
    for f in (0, 6):
        for v in got4:
            assert not v[f].any(), f
    want = pose_h_rule(*lists[8], bad[8].astype(np.float64), thr=1e6, min_front=1)
    _compare(got4, 8, cap, want, "rank 2")                                           # (fp32 rounding leaves lambda3 ~ 1e-15 lambda1)
    print("rank-2 H: kind %d on the device, %d by the restatement" % (got4[0][8], want.kind))
    assert e.check_guards() == 0


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _assert_frames_equal_explicit(e, n, res, match_dev, key_pts, key_xy_host, pairing, **params):
    cap = e.capacity
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    hm, _, _ = e.homography_frames_async(n, match_dev, key_xy=key_pts, pairing=pairing, iterations=256, seed=11, min_inliers=4)
    got = e.pose_homography_frames(n, match_dev, hm, key_xy=key_pts, pairing=pairing, **params)
    empty = np.zeros((0, 2), np.int32)

    def train_of(f):
        if pairing == "previous" and f > 0:
            return xy[f - 1]
        return key_xy_host if key_xy_host is not None else empty
    src, dst, npairs, rows = _host_pairs(match_dev.cpu().numpy(), xy, counts, train_of, cap)
    ref = e.pose_homography(src, dst, npairs, hm, **params)
    for a, b in zip(got[:6], ref[:6]):
        _bits(a, b)
    for f in range(n):
        back_f, back_x = np.zeros(cap, bool), np.zeros((cap, 3), np.float32)
        back_f[rows[f]], back_x[rows[f]] = ref[7][f, :npairs[f]], ref[6][f, :npairs[f]]
        np.testing.assert_array_equal(got[7][f], back_f)
        _bits(got[6][f], back_x)
    return got, npairs


def test_frames_variant_is_bit_identical_to_explicit_pairs(qvga):
    e, res = qvga
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    params = dict(K_query=KQVGA, K_train=np.array([[250.0, 0, 160.0], [0, 250.0, 120.0], [0, 0, 1.0]]), min_front=1)
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    fm, _, _ = e.fundamental_frames_async(N, m, key_xy=key_pts, iterations=256, seed=11)
    before = e.pose_frames(N, m, fm, key_xy=key_pts, K_query=KQVGA, K_train=KQVGA, min_front=1)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "key", **params)
    assert npairs.min() > 50 and got[0][5] == ROTATION                             # frame 5 against itself: H = I, no baseline
    assert np.abs(got[1][5, 0] - np.eye(3)).max() < 1e-4 and not got[4][5].any() and not got[7][5].any()
    print("kinds of the QVGA frames against frame 5:", got[0].tolist())
    # the shared pair-list workspace: an fpc_pose_frames call returns the same bits after a homography-pose call as before
    after = e.pose_frames(N, m, fm, key_xy=key_pts, K_query=KQVGA, K_train=KQVGA, min_front=1)
    for a, b in zip(before, after):
        _bits(a, b)
    again = e.pose_homography_frames(N, m, e.homography_frames_async(N, m, key_xy=key_pts, iterations=256, seed=11,
                                                                     min_inliers=4)[0], key_xy=key_pts, **params)
    for a, b in zip(got, again):
        _bits(a, b)                                                                  # repeated calls: the same bits
    m, _ = e.match_frames_async(N, key=key, pairing="previous", cross_check=True)
    _assert_frames_equal_explicit(e, N, res, m, key_pts, res[5][0], "previous", **params)
    m, _ = e.match_frames_async(N, key=None, pairing="previous", cross_check=True)
    got, npairs = _assert_frames_equal_explicit(e, N, res, m, None, None, "previous", **params)
    assert npairs[0] == 0
    for v in got:
        assert not v[0].any()                                                        # frame 0 has no train set: FAILED, zeros


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
        hm, _, _ = e.homography_bank_async(N, slot, m, iterations=256, seed=4, min_inliers=4)
        # a valid H for the frames without a slot, so that it is the slot that fails them
        hm[1], hm[4] = hm[0], hm[0]
        assert hm[0].any()
        got = e.pose_homography_bank(N, slot, m, hm, **params)
        sl = slot.cpu().numpy()
        for v in got:
            assert not v[[1, 4]].any()                                               # no slot: the frame fails with zeros
        assert set(sl.tolist()) - {-1, slots} and (got[0] > 0).any()
        print("kinds of the bank frames:", got[0].tolist())
        again = e.pose_homography_bank(N, slot, m, hm, **params)
        for a, b in zip(got, again):
            _bits(a, b)
        _, bx, bc = e.bank_view()
        for s in sorted(set(sl.tolist()) - {-1, slots}):
            rows_of = np.flatnonzero(sl == s)
            ref = e.pose_homography_frames(N, m, hm, key_xy=(bx[s].clone(), bc[s:s + 1].clone()), pairing="key", **params)
            for a, b in zip(got, ref):
                _bits(a[rows_of], b[rows_of])
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_chain_end_to_end_into_the_banks_landmarks():
    """Keypoints and descriptors planted on a plane with 15 % of them off it: fpc_bank_store_rows (the key frame),
    fpc_match_bank, fpc_homography_bank, fpc_pose_homography_bank, fpc_bank_store + fpc_bank_store_landmarks (xyz[0] and
    front[0] as they are), with no host call in between; then the bank's landmarks are what was written and the pose meets
    the planted-truth bars.  fpc_fundamental_bank -> fpc_pose_bank runs beside it on the same batch and is reported, not
    asserted: the case of the fundamental section's caveat."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        cap, dev = e.capacity, e.torch_device
        m = 600
        s = plane_scene(3, 0.15, m)
        rng = np.random.Generator(np.random.PCG64(9))
        rows = rng.normal(size=(m, e.desc_dim))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        order = rng.permutation(m)                                                   # the key frame holds the rows in another order
        desc, xy = np.zeros((2, cap, e.desc_dim), np.float32), np.zeros((2, cap, 2), np.int32)
        desc[0, :m], xy[0, :m] = rows, s["src"]
        plant(e, dict(desc=desc, xy=xy, counts=np.array([m, 0])))
        e.bank_create(2, cap)
        assert e.bank_landmarks_reserve() > 0
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the landmarks are read
        e.bank_store_rows(0, rows[order], s["dst"][order].astype(np.int32))
        _, best, match, _ = e.match_bank_async(2, cross_check=True)
        hm, ni, _ = e.homography_bank_async(2, best, match, iterations=256, seed=5)
        got = e.pose_homography_bank_async(2, best, match, hm, K_query=KVEC, K_train=KVEC)
        e.bank_store(0, 1)                                                           # the query frame becomes slot 1 ...
        e.bank_store_landmarks(1, got[6][0], got[7][0])                              # ... with its landmarks
        fm, nfi, _ = e.fundamental_bank_async(2, best, match, iterations=256, seed=5)
        beside = e.pose_bank_async(2, best, match, fm, K_query=KVEC, K_train=KVEC)
        lm = e.bank_landmarks()
        best, match, ni, lm, nfi = e._host((best, match, ni, lm, nfi))
        got, beside = e._host(got), e._host(beside)
        assert best[0] == 0 and best[1] == -1 and (match[0, :m] == np.argsort(order)).all() and ni[0] >= 0.84 * m
        g = _frame(got, 0)
        front = g.front.astype(bool)
        errs = check_planted(g, g.xyz[:m], front[:m], s, 0.15, "chain")
        print("chain: kind %d, support %s, plane pairs %s, rotation %.4f deg, direction %.4f deg, normal %.4f deg, d %.5f, "
              "depth %.5f" % (g.kind, g.nfront.tolist(), g.nplane.tolist(), *errs))
        for v in got:
            assert not v[1].any()                                                    # the frame without a slot
        # the landmarks of slot 1 are the call's points: xyz where front, w = 1 there and 0 elsewhere
        assert g.nfront[0] >= 0.95 * m and not front[m:].any()
        np.testing.assert_array_equal(lm[1, :, :3][front].view(np.uint32), g.xyz[front].view(np.uint32))
        np.testing.assert_array_equal(lm[1, :, 3] != 0, front)
        assert not lm[1, :, :3][~front].any()
        # beside it, through F
        rot = "failed" if not beside[0][0].any() else "%.3f deg rotation error, %.3f deg direction error" % solution_errors(
            types.SimpleNamespace(R=beside[0][None, 0], t=beside[1][None, 0], plane=np.array([[0, 0, 1.0, 1.0]])), 0, s)[:2]
        print("chain through F on the same batch: %d inliers of F, %d in front; %s" % (nfi[0], beside[2][0], rot))
        assert within_bars(errs[:4])
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
    hin = torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 9).repeat(N, 1).contiguous()
    outs = [torch.full(shape, 7, dtype=dt, device=dev)
            for shape, dt in (((N,), torch.int32), ((N, 18), torch.float32), ((N, 6), torch.float32), ((N, 8), torch.float32),
                              ((N, 2), torch.int32), ((N, 2), torch.int32), ((N, cap, 3), torch.float32), ((N, cap), torch.uint8))]
    torch.cuda.synchronize()
    sp, np_, mp, kp, op, lp, hp = (t.data_ptr() for t in (src, npairs, match, key_pts, one, slot, hin))
    o = [t.data_ptr() for t in outs]

    def params(**kw):
        p = _lib.FpcPoseHomographyParams()
        lib.fpc_default_pose_homography_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    ph = lambda n, s, d, c, stride, h, p, out=o: lib.fpc_pose_homography(e._ctx, n, s, d, c, stride, h, p, *out)   # noqa: E731
    pf = lambda n, pairing, k, kc, m, h, p, out=o: lib.fpc_pose_homography_frames(e._ctx, n, pairing, k, kc, m, h, p, *out)   # noqa: E731
    pb = lambda n, s, m, h, p, out=o: lib.fpc_pose_homography_bank(e._ctx, n, s, m, h, p, *out)   # noqa: E731
    ok = params()
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(q_fx=0.0), params(q_fy=-1.0), params(t_fx=0.0), params(t_fy=-500.0), params(q_fx=nan), params(t_fy=inf),
               params(q_cx=nan), params(q_cy=inf), params(t_cx=-inf), params(t_cy=nan), params(reproj_threshold=0.0),
               params(reproj_threshold=-1.0), params(reproj_threshold=nan), params(min_front=0), params(min_front=-3),
               params(min_baseline=-1e-3), params(min_baseline=nan), params(min_baseline=inf), params(which=2),
               params(which=-1), None]
        for p in bad:
            assert ph(N, sp, sp, np_, cap, hp, p) == FPC_E_INVALID
            assert pf(N, 0, kp, op, mp, hp, p) == FPC_E_INVALID
            assert pb(N, lp, mp, hp, p) == FPC_E_INVALID
        for k in (0, 1, 2, 4):                                                       # a NULL input, a NULL required output
            a = [sp, sp, np_, cap, hp, ok]
            a[k] = None
            assert ph(N, *a) == FPC_E_INVALID, k
        for k in (0, 1, 2, 4):                                                       # kind, R, t, nfront
            out = list(o)
            out[k] = None
            assert ph(N, sp, sp, np_, cap, hp, ok, out) == FPC_E_INVALID, k
            assert pf(N, 0, kp, op, mp, hp, ok, out) == FPC_E_INVALID, k
            assert pb(N, lp, mp, hp, ok, out) == FPC_E_INVALID, k
        assert ph(0, sp, sp, np_, cap, hp, ok) == FPC_E_INVALID
        assert ph(N + 1, sp, sp, np_, cap, hp, ok) == FPC_E_INVALID                  # above max_batch
        assert ph(N, sp, sp, np_, cap + 1, hp, ok) == FPC_E_INVALID                  # stride above capacity
        assert ph(N, sp, sp, np_, 0, hp, ok) == FPC_E_INVALID
        assert pf(N, 2, kp, op, mp, hp, ok) == FPC_E_INVALID                          # pairing
        assert pf(N, 0, None, None, mp, hp, ok) == FPC_E_INVALID                      # FPC_PAIR_KEY without key points
        assert pf(N, 0, kp, None, mp, hp, ok) == FPC_E_INVALID                        # key points without their count
        assert pf(N, 0, kp, op, None, hp, ok) == FPC_E_INVALID
        assert pf(N, 0, kp, op, mp, None, ok) == FPC_E_INVALID
        assert pf(0, 0, kp, op, mp, hp, ok) == FPC_E_INVALID
        assert pf(N + 1, 0, kp, op, mp, hp, ok) == FPC_E_INVALID
        assert pb(N, None, mp, hp, ok) == FPC_E_INVALID
        assert pb(N, lp, None, hp, ok) == FPC_E_INVALID
        assert pb(N, lp, mp, None, ok) == FPC_E_INVALID
        assert pb(0, lp, mp, hp, ok) == FPC_E_INVALID
        assert pb(N + 1, lp, mp, hp, ok) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert pf(3, 0, kp, op, mp, hp, ok) == FPC_E_INVALID
        assert pb(3, lp, mp, hp, ok) == FPC_E_INVALID
        e.sync()
        for t in outs:                                                               # nothing was written by any refused call
            assert (t.cpu() == 7).all()
        assert pf(2, 0, kp, op, mp, hp, ok) == 0
        assert pf(2, 1, None, None, mp, hp, ok) == 0                                 # PREVIOUS needs no key
        assert pb(2, lp, mp, hp, ok) == 0
        e.sync()
        for t in outs:                                                               # no match: no pairs, FAILED, zeros
            assert not t[:2].cpu().numpy().any() and (t[2:].cpu() == 7).all()
        assert ph(N, sp, sp, np_, cap, hp, ok) == 0
        e.sync()
        # ten pairs (0, 0) -> (0, 0) under H = I: a rotation by nothing, and nothing else
        host = [t.cpu().numpy() for t in outs]
        assert (host[0] == ROTATION).all() and np.abs(host[1][:, :9] - np.eye(3).ravel()).max() < 1e-6
        for v in (host[1][:, 9:], *host[2:]):
            assert not v.any()
    finally:
        e.bank_destroy()
    assert pb(2, lp, mp, hp, ok) == FPC_E_INVALID                                    # no bank
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))                                        # (the module's later tests see batch 1 again)
    with pytest.raises(ValueError):
        e.pose_homography_frames(N, match, hin, key_xy=key_pts, pairing="next")
    with pytest.raises(TypeError):
        e.pose_homography(src, src, npairs, hin, min_inliers=5)
    with pytest.raises(ValueError):
        e.pose_homography(src, src, npairs, hin, K_query=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.pose_homography_bank(N, slot, match, hin)
