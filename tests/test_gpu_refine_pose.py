"""Two-view bundle adjustment on the GPU (fpc_refine_pose / fpc_refine_pose_frames / fpc_refine_pose_bank) against the
float64 restatement and the planted scenes of tests/test_refine_pose.py: the device next to the restatement under the same
fp32 inputs, the planted-truth conditions on the device's own outputs, the tails of the pair list and of the outputs, the
chain identities (frames = explicit, bank = frames, repeats, aliasing, a bf16 bank, plan hash), the chain into the bank's
landmarks without a host call, and the argument checks.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_fundamental_ransac import FRAME_H, FRAME_W, KINDS
from tests.test_gpu_homography_ransac import _host_pairs, engine
from tests.test_gpu_match_guided import plant
from tests.test_gpu_pose_epipolar import H, KQVGA, N, W, _bits, _pack, qvga, vga  # noqa: F401  (qvga, vga: fixtures)
from tests.test_pose_epipolar import EXACT, KVEC, ROUNDED_SETS, THR, pose_errors, pose_scene
from tests.test_refine_pose import (MEAN_DIRECTION_SHARE, check_exact, check_refined_pose, exact_case, f32, refine_rule,
                                    refined_poses)

pytestmark = pytest.mark.gpu

FPC_E_INVALID = -1
# Device against restatement under the SAME fp32 inputs.  Both evaluate the rule in fp64 and round the state to fp32 behind
# every attempt; they differ by the contraction of a * b + c into one rounding and by the order of the sums, which a rounding
# of the state can turn into one fp32 ulp of a state entry.  The bars are about ten times what the restatement measures
# against itself when disturbed by one fp32 ulp in every entry of the input R (2.7e-7 in R, 1.1e-6 in t, 5.8e-6 of a point's
# length in xyz): 1e-5 for R and t, 1e-4 of a point's length for xyz, with the same attempt and accept counts; where the
# counts differ (a flipped accept decision) the final cost agrees to 1e-3 relative.
# Measured on the MI355X over the 28 frames of the two case sets: every frame on the restatement's accept path (the same
# attempt and accept counts), worst difference 6.9e-17 in R, 8.9e-16 in t, 3.0e-17 of a point's length in xyz: both sides
# are fp32 values, so the comparison is exact and these are single fp32 ulps of entries near zero.
R_BAR, XYZ_BAR, COST_BAR = 1e-5, 1e-4, 1e-3


def _compare(got, f, m, want, tag):
    """Frame f of the device outputs (R, t, nfront, xyz, front, stats) against the restatement's Refined over its m pairs
    -> (worst differences R, t, relative xyz; the same path?)."""
    rm, tv, nf, xyz, front, stats = (v[f] for v in got)
    front = front.astype(bool)
    assert not front[m:].any() and not xyz[m:].any(), tag                          # nothing behind the pair count
    assert nf == front.sum(), tag
    assert not xyz[:m][~front[:m]].any(), tag                                       # rows of non-members are zero
    if want.failed:
        assert not rm.any() and not tv.any() and nf == 0 and not front.any() and not stats.any(), tag
        return 0.0, 0.0, 0.0, True
    clear = ~(want.near | want.edge)
    np.testing.assert_array_equal(front[:m][clear], want.front[clear], err_msg=str(tag))
    assert abs(stats[0] - want.stats[0]) <= 1e-5 * want.stats[0] + 1e-9, (tag, stats, want.stats)
    same = stats[2] == want.stats[2] and stats[3] == want.stats[3]
    dr, dt = np.abs(rm.astype(np.float64) - want.R).max(), np.abs(tv.astype(np.float64) - want.t).max()
    both = front[:m] & want.front
    ref = want.xyz[both]
    rel = np.linalg.norm(xyz[:m][both].astype(np.float64) - ref, axis=1) / np.linalg.norm(ref, axis=1) if both.any() else np.zeros(1)
    if same:
        assert dr <= R_BAR and dt <= R_BAR, (tag, dr, dt)
        assert rel.max() <= XYZ_BAR, (tag, rel.max())
    c_dev, c_ref = float(stats[1]) ** 2, float(want.stats[1]) ** 2                 # C / (2 m) over the same members
    assert abs(c_dev - c_ref) <= COST_BAR * c_ref + 1e-12, (tag, stats, want.stats)
    return dr, dt, rel.max(), same


_DEVICE = {}


def _device_refined(e, rho, iterations):
    """The device's refinement of one rounded case set from the restated linear poses, computed once."""
    if (rho, iterations) not in _DEVICE:
        scenes, poses, refined = refined_poses(rho, iterations)
        src, dst, npairs = _pack([(s[0], s[1]) for s in scenes], 640)
        assert len(scenes) == 14 and 572 <= npairs.min() and npairs.max() <= 600
        rin = np.stack([po.R for po in poses]).astype(np.float32)
        tin = np.stack([po.t for po in poses]).astype(np.float32)
        _DEVICE[rho, iterations] = scenes, refined, e.refine_pose(src, dst, npairs, rin, tin, reproj_threshold=THR)
    return _DEVICE[rho, iterations]


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_explicit_call_agrees_with_the_restatement(vga, rho, iterations):  # noqa: F811
    scenes, refined, got = _device_refined(vga, rho, iterations)
    worst, other = np.zeros(3), []
    for f, (scene, want) in enumerate(zip(scenes, refined)):
        assert not want.failed and got[2][f] > 0, f
        dr, dt, dx, same = _compare(got, f, len(scene[0]), want, (rho, f))
        if same:
            worst = np.maximum(worst, (dr, dt, dx))
        else:
            other.append((f, got[5][f].tolist(), want.stats.tolist(), dr, dt, dx))
    print("rho %.1f: worst device - restatement difference on the same path: R %.3e, t %.3e, xyz %.3e relative; frames on "
          "another accept path: %s" % (rho, *worst, other))


@pytest.mark.parametrize("rho,iterations", ROUNDED_SETS)
def test_device_meets_the_planted_truth_conditions(vga, rho, iterations):  # noqa: F811
    scenes, refined, got = _device_refined(vga, rho, iterations)
    _, poses, _ = refined_poses(rho, iterations)
    before, after = [], []
    for f, (scene, po) in enumerate(zip(scenes, poses)):
        m = len(scene[0])
        errs = check_refined_pose(got[0][f], got[1][f], got[2][f], got[3][f, :m], got[4][f, :m], got[5][f], scene,
                                  (KINDS[f], f, rho))
        before.append(pose_errors(po.R, po.t, po.xyz, po.front, scene)[1])
        after.append(errs[1])
        print("rho %.1f frame %2d %-8s: rotation %.4f deg, direction %.4f deg, depth %.5f, stats %s"
              % (rho, f, KINDS[f], *errs, got[5][f].tolist()))
    print("rho %.1f: mean direction error %.4f -> %.4f deg" % (rho, np.mean(before), np.mean(after)))
    if rho > 0:
        assert np.mean(after) <= MEAN_DIRECTION_SHARE * np.mean(before)


def test_exact_pairs_reach_the_fp32_floor_on_the_device(vga):  # noqa: F811
    cases = [exact_case(kind, i) for kind, i in EXACT]
    src, dst, npairs = _pack([(c[0], c[1]) for c in cases], 640)
    rin, tin = np.stack([c[2] for c in cases]).astype(np.float32), np.stack([c[3] for c in cases]).astype(np.float32)
    got = vga.refine_pose(src, dst, npairs, rin, tin, reproj_threshold=8.0, iterations=8)
    for f, ((kind, i), c) in enumerate(zip(EXACT, cases)):
        assert got[2][f] >= 500, (kind, i, got[2][f])
        rot, direction = check_exact(got[0][f], got[1][f], got[5][f], c[4], (kind, i))
        print("%-8s %d: stats %s, rotation %.4f deg, direction %.4f deg" % (kind, i, got[5][f].tolist(), rot, direction))


def _raw_refine(e, src, dst, npairs, rin, tin, front=True, stats=True, alias=False, fill=0xFF, **params):
    """fpc_refine_pose into outputs pre-filled with `fill` bytes -> host arrays (R, t, nfront, xyz, front uint8, stats);
    alias: R_dev / t_dev are the input tensors."""
    import torch
    dev = e.torch_device
    n, stride = src.shape[0], src.shape[1]
    p = e._refine_params(None, None, params)
    ins = [torch.from_numpy(np.ascontiguousarray(v)).to(dev)
           for v in (src, dst, npairs, rin.reshape(n, 9).astype(np.float32), tin.reshape(n, 3).astype(np.float32))]
    outs = [torch.full(shape, fill, dtype=torch.uint8, device=dev)
            for shape in ((n, 36), (n, 12), (n, 4), (n, stride, 12), (n, stride), (n, 16))]
    if alias:
        outs[0], outs[1] = ins[3].view(torch.uint8), ins[4].view(torch.uint8)
    torch.cuda.synchronize()
    e._call("fpc_refine_pose", n, ins[0], ins[1], ins[2], stride, ins[3], ins[4], ctypes.byref(p), outs[0], outs[1], outs[2],
            outs[3], outs[4] if front else None, outs[5] if stats else None, inputs=ins)
    e.sync()
    rm, tv, nf, pts, fr, st = (o.cpu().numpy() for o in outs)
    return (rm.view(np.float32).reshape(n, 3, 3), tv.view(np.float32).reshape(n, 3), nf.view(np.int32).reshape(n),
            pts.view(np.float32).reshape(n, stride, 3), fr, st.view(np.float32).reshape(n, 4))


def test_tails_of_the_pair_list_and_of_the_outputs(vga):  # noqa: F811
    """Pair counts 0, 7, 8, 255, 256, 257 and 1 100 at stride 1 280: the workgroup's stride of 256 and the 1 024-record chunk of
    the pair list."""
    e = vga
    stride = 1280
    assert e.capacity >= stride
    s, d, _, _, _, r, t, _ = pose_scene("general", 2, 0.0, stride)
    counts = (0, 7, 8, 255, 256, 257, 1100)
    lists = [(s[:c], d[:c]) for c in counts]
    src, dst, npairs = _pack(lists, stride)
    rin = np.repeat(r[None].astype(np.float32), len(lists), 0)
    tin = np.repeat((t / np.linalg.norm(t))[None].astype(np.float32), len(lists), 0)
    got = _raw_refine(e, src, dst, npairs, rin, tin, reproj_threshold=3.0, min_front=8)
    rm, tv, nf, xyz, front, stats = got
    assert set(np.unique(front).tolist()) <= {0, 1}                                  # no 0xFF left: every row was written
    assert all(np.isfinite(v).all() for v in (xyz, rm, tv, stats))
    for f, (a, b) in enumerate(lists):
        want = refine_rule(a, b, rin[f], tin[f], thr=3.0, min_front=8)
        assert want.failed == (counts[f] < 8), f
        _compare(got, f, len(a), want, ("tails", f))
        assert not front[f, counts[f]:].any() and not xyz[f, counts[f]:].view(np.uint32).any()   # rows past the count: zero bytes
        assert nf[f] == front[f].sum()
    assert nf[2] == 8 and nf[3] >= 0.95 * 255 and nf[6] >= 0.95 * 1100 and front[6, 1024:1100].sum() >= 0.95 * 76
    # without front / stats the other outputs are what they were
    for kw in (dict(front=False), dict(stats=False)):
        raw = _raw_refine(e, src, dst, npairs, rin, tin, reproj_threshold=3.0, min_front=8, **kw)
        for k in (0, 1, 3):
            _bits(raw[k], got[k])
        np.testing.assert_array_equal(raw[2], nf)
        assert (raw[4] == 0xFF).all() if "front" in kw else (raw[5].view(np.uint32) == 0xFFFFFFFF).all()
    # R_dev / t_dev aliasing the inputs: the same bits
    raw = _raw_refine(e, src, dst, npairs, rin, tin, alias=True, reproj_threshold=3.0, min_front=8)
    for a, b in zip(raw, got):
        np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    # failed inputs fail their frame only: a zero R, a NaN in t, |t| = 0
    bad_r, bad_t = rin.copy(), tin.copy()
    bad_r[3] = 0.0
    bad_t[4, 1] = np.nan
    bad_t[5] = 0.0
    raw = _raw_refine(e, src, dst, npairs, bad_r, bad_t, reproj_threshold=3.0, min_front=8)
    for f in (3, 4, 5):
        assert not any(v[f].any() for v in raw), f
    for a, b in zip(raw, got):
        np.testing.assert_array_equal(np.ascontiguousarray(a[6]).view(np.uint8), np.ascontiguousarray(b[6]).view(np.uint8))
    assert e.check_guards() == 0


def test_frames_variant_is_bit_identical_to_explicit_pairs_and_calls_repeat(qvga):  # noqa: F811
    e, res = qvga
    cap = e.capacity
    plan = (e.plan_hash(), e.packed_size())
    key, key_pts = e.keep_frame(5), e.keep_frame_points(5)
    cams = dict(K_query=KQVGA, K_train=KQVGA)
    params = dict(min_front=1, min_parallax_deg=0.0, **cams)
    xy = [r[0] for r in res]
    counts = np.array([len(v) for v in xy])
    m, _ = e.match_frames_async(N, key=key, pairing="key", cross_check=True)
    fm, _, _ = e.fundamental_frames_async(N, m, key_xy=key_pts, pairing="key", iterations=256, seed=11)
    lin = e.pose_frames_async(N, m, fm, key_xy=key_pts, pairing="key", min_front=1, **cams)
    got = e.refine_pose_frames(N, m, lin[0], lin[1], key_xy=key_pts, pairing="key", **params)
    assert (got[2] > 0).any() and (got[5][:, 3] >= 1).any()
    again = e.refine_pose_frames(N, m, lin[0], lin[1], key_xy=key_pts, pairing="key", **params)
    for a, b in zip(got, again):                                                     # two calls: the same bits
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    src, dst, npairs, rows = _host_pairs(m.cpu().numpy(), xy, counts, lambda f: res[5][0], cap)
    rm, tv, nf, xyz, front, stats = e.refine_pose(src, dst, npairs, lin[0], lin[1], **params)
    _bits(got[0], rm)
    _bits(got[1], tv)
    _bits(got[5], stats)
    np.testing.assert_array_equal(got[2], nf)
    for f in range(N):
        back_f, back_x = np.zeros(cap, bool), np.zeros((cap, 3), np.float32)
        back_f[rows[f]], back_x[rows[f]] = front[f, :npairs[f]], xyz[f, :npairs[f]]
        np.testing.assert_array_equal(got[4][f], back_f)
        _bits(got[3][f], back_x)
    assert plan == (e.plan_hash(), e.packed_size()) and e.check_guards() == 0


@pytest.mark.parametrize("fmt", ["f32", "bf16"])
def test_bank_variant_is_bit_identical_to_the_frames_variant(qvga, fmt):  # noqa: F811
    e, res = qvga
    slots = 3
    e.bank_create(slots, e.capacity, format=fmt)
    try:
        for s in range(slots):
            e.bank_store(s + 1, s)
        e.detect(synth.make_batch(400, N, H, W))                                     # another batch against the stored frames
        _, best, m, _ = e.match_bank_async(N, cross_check=True, max_dist=0.9)
        slot = best.clone()
        slot[1], slot[4] = -1, slots
        cams = dict(K_query=KQVGA, K_train=KQVGA)
        params = dict(min_front=1, min_parallax_deg=0.0, **cams)
        fm, _, _ = e.fundamental_bank_async(N, best, m, iterations=256, seed=4)
        lin = e.pose_bank_async(N, best, m, fm, min_front=1, **cams)                # a pose for every frame: it is the slot that fails two
        got = e.refine_pose_bank(N, slot, m, lin[0], lin[1], **params)
        sl = slot.cpu().numpy()
        for v in got:
            assert not v[[1, 4]].any()                                               # no slot: the frame fails with zeros
        assert set(sl.tolist()) - {-1, slots} and (got[2] > 0).any()
        _, bx, bc = e.bank_view()
        for s in sorted(set(sl.tolist()) - {-1, slots}):
            rows_of = np.flatnonzero(sl == s)
            ref = e.refine_pose_frames(N, m, lin[0], lin[1], key_xy=(bx[s].clone(), bc[s:s + 1].clone()), pairing="key", **params)
            for a, b in zip(got, ref):
                np.testing.assert_array_equal(a[rows_of].view(np.uint8), b[rows_of].view(np.uint8))
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()
        e.detect(synth.make_batch(300, N, H, W))                                    # (the module's later tests see batch 1 again)


def test_chain_end_to_end_into_the_banks_landmarks():
    """Keypoints and descriptors planted on a scene with depth: fpc_bank_store_rows (the key frame), fpc_match_bank,
    fpc_fundamental_bank, fpc_pose_bank, fpc_refine_pose_bank, fpc_bank_store + fpc_bank_store_landmarks (xyz[0] and front[0]
    as they are), with no host call in between; then the bank's landmarks are the refined points."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(FRAME_H, FRAME_W, 2, max_keypoints=1024)
    try:
        cap = e.capacity
        scene = pose_scene("general", 3, 0.0)
        s, d = scene[0], scene[1]
        m = len(s)
        rng = np.random.Generator(np.random.PCG64(9))
        rows = rng.normal(size=(m, e.desc_dim))
        rows = (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)
        order = rng.permutation(m)                                                   # the key frame holds the rows in another order
        desc, xy = np.zeros((2, cap, e.desc_dim), np.float32), np.zeros((2, cap, 2), np.int32)
        desc[0, :m], xy[0, :m] = rows, s
        plant(e, dict(desc=desc, xy=xy, counts=np.array([m, 0])))
        e.bank_create(2, cap)
        assert e.bank_landmarks_reserve() > 0
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the landmarks are read
        e.bank_store_rows(0, rows[order], d[order].astype(np.int32))
        _, best, match, _ = e.match_bank_async(2, cross_check=True)
        fm, ni, _ = e.fundamental_bank_async(2, best, match, iterations=256, seed=5, reproj_threshold=THR)
        lin = e.pose_bank_async(2, best, match, fm, K_query=KVEC, K_train=KVEC, reproj_threshold=THR)
        got = e.refine_pose_bank_async(2, best, match, lin[0], lin[1], K_query=KVEC, K_train=KVEC, reproj_threshold=THR)
        e.bank_store(0, 1)                                                           # the query frame becomes slot 1 ...
        e.bank_store_landmarks(1, got[3][0], got[4][0])                              # ... with its refined landmarks
        lm = e.bank_landmarks()
        best, match, ni, lm = e._host((best, match, ni, lm))
        lin, got = e._host(lin), e._host(got)
        assert best[0] == 0 and best[1] == -1 and (match[0, :m] == np.argsort(order)).all() and ni[0] >= 0.9 * m
        for v in got:
            assert not v[1].any()                                                    # the frame without a slot
        front = got[4][0]
        assert got[2][0] >= 0.9 * m and not front[m:].any()
        np.testing.assert_array_equal(lm[1, :, :3][front].view(np.uint32), got[3][0][front].view(np.uint32))
        np.testing.assert_array_equal(lm[1, :, 3] != 0, front)
        assert not lm[1, :, :3][~front].any()
        want = refine_rule(s, d, lin[0][0], lin[1][0], thr=THR)
        _compare(got, 0, m, want, "chain")
        errs = check_refined_pose(got[0][0], got[1][0], got[2][0], got[3][0, :m], front[:m], got[5][0], scene, "chain")
        print("chain: rotation %.4f deg, direction %.4f deg, depth %.5f, stats %s" % (*errs, got[5][0].tolist()))
        assert e.check_guards() == 0
    finally:
        e.close()


def test_homography_solutions_go_in_through_which(vga):  # noqa: F811
    """A [n,2,3,3] / [n,2,3] input with which= selects a solution on the device: the same bits as the slice passed in."""
    cases = [exact_case(kind, i) for kind, i in EXACT[:2]]
    src, dst, npairs = _pack([(c[0], c[1]) for c in cases], 640)
    rin, tin = np.stack([c[2] for c in cases]).astype(np.float32), np.stack([c[3] for c in cases]).astype(np.float32)
    two_r, two_t = np.stack([np.zeros_like(rin), rin], 1), np.stack([np.zeros_like(tin), tin], 1)
    ref = vga.refine_pose(src, dst, npairs, rin, tin, reproj_threshold=8.0)
    got = vga.refine_pose(src, dst, npairs, two_r, two_t, which=1, reproj_threshold=8.0)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    assert (ref[2] > 0).all()
    zero = vga.refine_pose(src, dst, npairs, two_r, two_t, which=0, reproj_threshold=8.0)       # a solution that does not exist
    assert not any(v.any() for v in zero)
    with pytest.raises(ValueError):
        vga.refine_pose(src, dst, npairs, two_r, two_t, reproj_threshold=8.0)
    with pytest.raises(ValueError):
        vga.refine_pose(src, dst, npairs, rin, tin, which=1, reproj_threshold=8.0)


def test_bad_arguments_are_refused(qvga):  # noqa: F811
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
    rin = torch.eye(3, dtype=torch.float32, device=dev).reshape(1, 9).repeat(N, 1).contiguous()
    tin = torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float32, device=dev).repeat(N, 1).contiguous()
    rm = torch.full((N, 9), 7.0, dtype=torch.float32, device=dev)
    tv = torch.full((N, 3), 7.0, dtype=torch.float32, device=dev)
    nf = torch.full((N,), 7, dtype=torch.int32, device=dev)
    xyz = torch.full((N, cap, 3), 7.0, dtype=torch.float32, device=dev)
    front = torch.full((N, cap), 7, dtype=torch.uint8, device=dev)
    stats = torch.full((N, 4), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sp, np_, mp, kp, op, lp, ri, ti = (t.data_ptr() for t in (src, npairs, match, key_pts, one, slot, rin, tin))
    rp, tp, ip, xp, bp, qp = (t.data_ptr() for t in (rm, tv, nf, xyz, front, stats))

    def params(**kw):
        p = _lib.FpcRefineParams()
        lib.fpc_default_refine_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return ctypes.byref(p)
    pf = lambda n, s, d, c, stride, r0, t0, p, r, t, i, x: lib.fpc_refine_pose(e._ctx, n, s, d, c, stride, r0, t0, p, r, t, i, x, bp, qp)   # noqa: E731
    ff = lambda n, pairing, k, kc, m, r0, t0, p, r, t, i, x: lib.fpc_refine_pose_frames(e._ctx, n, pairing, k, kc, m, r0, t0, p, r, t, i, x, bp, qp)   # noqa: E731
    fb = lambda n, s, m, r0, t0, p, r, t, i, x: lib.fpc_refine_pose_bank(e._ctx, n, s, m, r0, t0, p, r, t, i, x, bp, qp)   # noqa: E731
    ok = params()
    e.bank_create(2, cap)
    try:
        nan, inf = float("nan"), float("inf")
        bad = [params(q_fx=0.0), params(q_fy=-1.0), params(t_fx=0.0), params(t_fy=-500.0), params(q_fx=nan), params(t_fy=inf),
               params(q_cx=nan), params(q_cy=inf), params(t_cx=-inf), params(t_cy=nan), params(reproj_threshold=0.0),
               params(reproj_threshold=-1.0), params(reproj_threshold=nan), params(reproj_threshold=2e18),
               params(min_front=0), params(min_front=-3), params(iterations=0), params(iterations=17), params(iterations=-1),
               params(lambda0=0.0), params(lambda0=-1e-3), params(lambda0=nan), params(lambda0=inf),
               params(min_parallax_deg=-0.5), params(min_parallax_deg=90.0), params(min_parallax_deg=nan), None]
        for p in bad:
            assert pf(N, sp, sp, np_, cap, ri, ti, p, rp, tp, ip, xp) == FPC_E_INVALID
            assert ff(N, 0, kp, op, mp, ri, ti, p, rp, tp, ip, xp) == FPC_E_INVALID
            assert fb(N, lp, mp, ri, ti, p, rp, tp, ip, xp) == FPC_E_INVALID
        for k in range(11):                                                          # a NULL in any pointer but front / stats
            if k == 3:
                continue
            a = [sp, sp, np_, cap, ri, ti, ok, rp, tp, ip, xp]
            a[k] = None
            assert pf(N, *a) == FPC_E_INVALID, k
        assert pf(0, sp, sp, np_, cap, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        assert pf(N + 1, sp, sp, np_, cap, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID     # above max_batch
        assert pf(N, sp, sp, np_, cap + 1, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID     # stride above capacity
        assert pf(N, sp, sp, np_, 0, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        assert ff(N, 2, kp, op, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID             # pairing
        assert ff(N, 0, None, None, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID         # FPC_PAIR_KEY without key points
        assert ff(N, 0, kp, None, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID           # key points without their count
        for k in range(3, 11):
            a = [0, kp, op, mp, ri, ti, ok, rp, tp, ip, xp]
            a[k] = None
            assert ff(N, *a) == FPC_E_INVALID, k
        assert ff(0, 0, kp, op, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        assert ff(N + 1, 0, kp, op, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        for k in range(9):
            a = [lp, mp, ri, ti, ok, rp, tp, ip, xp]
            a[k] = None
            assert fb(N, *a) == FPC_E_INVALID, k
        assert fb(0, lp, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        assert fb(N + 1, lp, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        e.sync()
        e.detect(synth.make_batch(300, 2, H, W))                                    # a detect of fewer frames bounds n
        assert ff(3, 0, kp, op, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        assert fb(3, lp, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID
        e.sync()
        # nothing was written by any refused call
        for t in (rm, tv, xyz, stats):
            assert (t.cpu() == 7.0).all()
        assert (nf.cpu() == 7).all() and (front.cpu() == 7).all()
        assert ff(2, 0, kp, op, mp, ri, ti, ok, rp, tp, ip, xp) == 0
        assert ff(2, 1, None, None, mp, ri, ti, ok, rp, tp, ip, xp) == 0             # PREVIOUS needs no key
        assert fb(2, lp, mp, ri, ti, ok, rp, tp, ip, xp) == 0
        assert pf(N, sp, sp, np_, cap, ri, ti, ok, rp, tp, ip, xp) == 0
        e.sync()
        # no match (frames, bank), or ten pairs of equal pixels under a sideways pose, which have no parallax (explicit): every
        # frame fails with zeros
        for t in (rm, tv, nf, xyz, front, stats):
            assert not t.cpu().numpy().any()
    finally:
        e.bank_destroy()
    assert fb(2, lp, mp, ri, ti, ok, rp, tp, ip, xp) == FPC_E_INVALID                # no bank
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))                                        # (the module's later tests see batch 1 again)
    with pytest.raises(ValueError):
        e.refine_pose_frames(N, match, rin, tin, key_xy=key_pts, pairing="next")
    with pytest.raises(TypeError):
        e.refine_pose(src, src, npairs, rin, tin, refits=2)
    with pytest.raises(ValueError):
        e.refine_pose(src, src, npairs, rin, tin, K_query=np.ones((3, 3)))
    with pytest.raises(ValueError):
        e.refine_pose_bank(N, slot, match, rin, tin)
