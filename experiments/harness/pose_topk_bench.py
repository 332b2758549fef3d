"""The pose and epipolar top-K calls (fpc_pnp_bank_topk, fpc_p3p_bank_topk, fpc_fundamental_bank_topk,
fpc_essential_bank_topk) beside k successive calls of the single-slot call each generalises (fpc_pnp_bank, fpc_p3p_bank,
fpc_fundamental_bank, fpc_essential_bank) on the same inputs in the same process, DESIGN.md section 7.  32 VGA frames whose
keypoints are planted as in pnp_bench.py: every frame holds exactly M rows, each matched to one row of a key frame that
carries a 3-D point and a pixel, pixels rounded, a fifth of the matches replaced by wrong ones.  The bank holds k = 4 slots
of M rows: slot 0 is that key frame, slots 1 .. 3 carry its rows at scrambled pixels and landmarks -- one right candidate
and three wrong ones per frame, the shortlist a relocaliser sees; every candidate's table is the frame's.  M = 200 and
1000, every model at its default parameters (1024 iterations).
    python experiments/harness/pose_topk_bench.py [reps] [runs]
prints one JSON line per M: per model the top-K call and the k single-slot calls from HIP events on the ctx stream (median,
min and max over `runs` runs of `reps` back-to-back calls, after a warm-up), their ratio, and the picked slots.  These are
event times around loops of host calls, four calls a repetition against one: for the short calls the k-calls side may
include the host's launch rate, so the ratio is what a caller sees, not a ratio of device times.  The per-kernel split
needs a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/pose_topk_bench.py 20 1"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import _lib
from fpc_amd.engine import Engine

H, W, B, K = 480, 640, 32, 4
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def timed(e, fn):
    for _ in range(3):
        fn()
    e.sync()
    st, out = e.torch_stream(), []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        for _ in range(reps):
            fn()
        t1.record(st)
        e.sync()
        out.append(t0.elapsed_time(t1) / reps)
    return [round(float(v), 4) for v in (np.median(out), min(out), max(out))]


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def project(x):
    return np.round(np.stack([FX * x[:, 0] / x[:, 2] + CX, FY * x[:, 1] / x[:, 2] + CY], 1)).astype(np.int32)


for M in (200, 1000):
    e = Engine(H, W, max_batch=B, max_keypoints=1024)
    cap, D = e.capacity, e.desc_dim
    prob = torch.zeros((B, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((B, D, H // 8, W // 8)))          # B frames of keypoints; the planted rows take their place
    rng = np.random.default_rng(M)
    # the key frame: M landmarks in its camera frame (in front of both views) and their pixels
    px = np.stack([rng.uniform(100, W - 100, M), rng.uniform(80, H - 80, M)], 1)
    z = rng.uniform(4.0, 12.0, M)
    key_xyz = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1).astype(np.float32)
    key_xy = project(key_xyz.astype(np.float64))
    hx, hm = np.zeros((B, cap, 2), np.int32), np.full((B, cap), -1, np.int32)
    for f in range(B):
        r = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 8.0)))
        t = rng.normal(size=3) * 0.5
        order = rng.permutation(M)
        hx[f, :M] = np.clip(project(key_xyz[order].astype(np.float64) @ r.T + t), 0, [W - 1, H - 1])
        hm[f, :M] = order
        wrong = rng.choice(M, M // 5, replace=False)
        hm[f, wrong] = rng.integers(0, M, len(wrong))
    xy, count = e._points_view()
    xy[:B].copy_(torch.from_numpy(hx))
    count[:B].fill_(M)
    # the bank: slot 0 the key frame, the others its rows at scrambled pixels and landmarks
    e.bank_create(K)
    e.bank_landmarks_reserve()
    e.bank_topk_reserve(K)
    e.pnp_reserve()
    e.pnp_topk_reserve()
    desc = rng.normal(size=(M, D))
    desc = (desc / np.linalg.norm(desc, axis=1, keepdims=True)).astype(np.float32)
    pad = np.zeros((cap, 3), np.float32)
    for sl in range(K):
        o = np.arange(M) if sl == 0 else rng.permutation(M)
        e.bank_store_rows(sl, desc, key_xy[o])
        pad[:M] = key_xyz[o]
        e.bank_store_landmarks(sl, pad.copy())
    cand = torch.arange(K, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous()             # [B][K]
    m = torch.from_numpy(np.repeat(hm[:, None], K, 1)).cuda().contiguous()                          # [B][K][cap]
    cols = [(cand[:, j].contiguous(), m[:, j].contiguous()) for j in range(K)]
    torch.cuda.synchronize()
    lib, ctx = e._l, e._ctx

    def out(*shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device="cuda")
    rm, tv, em, ni, mask = out(B, K, 9), out(B, K, 3), out(B, K, 9), out(B, K, dtype=torch.int32), out(B, K, cap, dtype=torch.uint8)
    pick, best, br, bt = out(B, dtype=torch.int32), out(B, dtype=torch.int32), out(B, 9), out(B, 3)
    rm1, tv1, em1, ni1, mask1 = out(B, 9), out(B, 3), out(B, 9), out(B, dtype=torch.int32), out(B, cap, dtype=torch.uint8)
    rp, pp, ep = _lib.FpcRansacParams(), _lib.FpcPnpParams(), _lib.FpcEssentialParams()
    lib.fpc_default_ransac_params(ctypes.byref(rp))
    lib.fpc_default_pnp_params(ctypes.byref(pp))
    lib.fpc_default_essential_params(ctypes.byref(ep))

    def topk(model):
        if model in ("pnp", "p3p"):
            fn = lib.fpc_pnp_bank_topk if model == "pnp" else lib.fpc_p3p_bank_topk
            return lambda: fn(ctx, B, K, cand.data_ptr(), m.data_ptr(), ctypes.byref(pp), rm.data_ptr(), tv.data_ptr(),
                              ni.data_ptr(), mask.data_ptr(), pick.data_ptr(), best.data_ptr(), br.data_ptr(), bt.data_ptr())
        if model == "fundamental":
            return lambda: lib.fpc_fundamental_bank_topk(ctx, B, K, cand.data_ptr(), m.data_ptr(), ctypes.byref(rp), rm.data_ptr(),
                                                         ni.data_ptr(), mask.data_ptr(), pick.data_ptr(), best.data_ptr(),
                                                         br.data_ptr())
        return lambda: lib.fpc_essential_bank_topk(ctx, B, K, cand.data_ptr(), m.data_ptr(), ctypes.byref(ep), rm.data_ptr(),
                                                   em.data_ptr(), ni.data_ptr(), mask.data_ptr(), pick.data_ptr(), best.data_ptr(),
                                                   br.data_ptr())

    def single(model, slot, match):
        if model in ("pnp", "p3p"):
            fn = lib.fpc_pnp_bank if model == "pnp" else lib.fpc_p3p_bank
            return fn(ctx, B, slot.data_ptr(), match.data_ptr(), ctypes.byref(pp), rm1.data_ptr(), tv1.data_ptr(), ni1.data_ptr(),
                      mask1.data_ptr())
        if model == "fundamental":
            return lib.fpc_fundamental_bank(ctx, B, slot.data_ptr(), match.data_ptr(), ctypes.byref(rp), rm1.data_ptr(),
                                            ni1.data_ptr(), mask1.data_ptr())
        return lib.fpc_essential_bank(ctx, B, slot.data_ptr(), match.data_ptr(), ctypes.byref(ep), rm1.data_ptr(), em1.data_ptr(),
                                      ni1.data_ptr(), mask1.data_ptr())

    row = {"M": M, "k": K, "frames": B, "iterations": int(pp.iterations)}
    for model in ("pnp", "p3p", "fundamental", "essential"):
        one = topk(model)

        def one_call():
            assert one() == 0

        def k_calls():
            for slot, match in cols:
                assert single(model, slot, match) == 0

        a, b = timed(e, one_call), timed(e, k_calls)
        e.sync()
        row[model] = {"topk_ms": a, "k_single_slot_calls_ms": b, "topk_over_k_calls": round(a[0] / b[0], 3),
                      "picked_slot_0": int((best == 0).sum()), "mean_inliers_slot_0": round(float(ni[:, 0].float().mean()), 1),
                      "max_inliers_wrong_slots": int(ni[:, 1:].max())}
    print(json.dumps(row), flush=True)
    e.close()
