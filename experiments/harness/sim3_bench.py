"""Sim(3) alignment (fpc_sim3_frames) beside RANSAC PnP (fpc_pnp_frames) at the same T and M in the same process, DESIGN.md
section 7.  32 VGA frames whose keypoints are planted as in pnp_bench.py: every frame holds exactly M rows, each matched to
one row of a key frame that carries a 3-D point, a fifth of the matches replaced by wrong ones; for the Sim(3) call every row
also carries a landmark of its own, the key's point under the frame's planted similarity (scale 0.6 .. 1.8) with a relative
depth error of 0.2 %.  T = 1024 hypotheses, M = 200 and 1000, the default refits of either call.
    python experiments/harness/sim3_bench.py [reps] [runs]
prints one JSON line per M: the two calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up), and the mean inlier counts.  The per-kernel split needs a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/sim3_bench.py 20 1
(sim3_gather_kernel, sim3_score_kernel, sim3_refit_kernel beside pnp_gather_kernel, pnp_score_kernel, pnp_refit_kernel)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import _lib
from fpc_amd.engine import Engine

H, W, B, T = 480, 640, 32, 1024
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
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
    e = Engine(H, W, max_batch=B, descriptor_enabled=False, max_keypoints=1024)
    e.pnp_reserve()
    cap = e.capacity
    prob = torch.zeros((B, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob)                                              # B frames of keypoints; the planted rows take their place
    rng = np.random.default_rng(M)
    # the key frame: M landmarks in its camera frame (in front of both views)
    px = np.stack([rng.uniform(100, W - 100, M), rng.uniform(80, H - 80, M)], 1)
    z = rng.uniform(4.0, 12.0, M)
    key_xyz = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1).astype(np.float32)
    hx, hm, hq = np.zeros((B, cap, 2), np.int32), np.full((B, cap), -1, np.int32), np.zeros((B, cap, 3), np.float32)
    for f in range(B):
        r = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 8.0)))
        t = rng.normal(size=3) * 0.5
        s = rng.uniform(0.6, 1.8)
        order = rng.permutation(M)
        xc = key_xyz[order].astype(np.float64) @ r.T + t
        hx[f, :M] = np.clip(project(xc), 0, [W - 1, H - 1])
        hq[f, :M] = s * xc * (1.0 + 0.002 * rng.normal(size=(M, 1)))
        hm[f, :M] = order
        wrong = rng.choice(M, M // 5, replace=False)
        hm[f, wrong] = rng.integers(0, M, len(wrong))
    xy, count = e._points_view()
    xy[:B].copy_(torch.from_numpy(hx))
    count[:B].fill_(M)
    m = torch.from_numpy(hm).cuda()
    kxyz, qxyz = torch.from_numpy(key_xyz).cuda(), torch.from_numpy(hq).cuda()
    kcount = torch.tensor([M], dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    lib, ctx = e._l, e._ctx
    sv = torch.empty((B,), dtype=torch.float32, device="cuda")
    rm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
    tv = torch.empty((B, 3), dtype=torch.float32, device="cuda")
    ni = torch.empty((B,), dtype=torch.int32, device="cuda")
    ns = torch.empty((B,), dtype=torch.int32, device="cuda")
    mask = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    q = _lib.FpcPnpParams()
    lib.fpc_default_pnp_params(ctypes.byref(q))
    q.iterations = T
    p = _lib.FpcSim3Params()
    lib.fpc_default_sim3_params(ctypes.byref(p))
    p.iterations = T

    def pnp():
        assert lib.fpc_pnp_frames(ctx, B, kxyz.data_ptr(), None, kcount.data_ptr(), m.data_ptr(), ctypes.byref(q),
                                  rm.data_ptr(), tv.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def sim3():
        assert lib.fpc_sim3_frames(ctx, B, qxyz.data_ptr(), None, kxyz.data_ptr(), None, kcount.data_ptr(), m.data_ptr(),
                                   ctypes.byref(p), sv.data_ptr(), rm.data_ptr(), tv.data_ptr(), ns.data_ptr(),
                                   mask.data_ptr()) == 0

    pms, sms = timed(e, pnp), timed(e, sim3)
    row = {"M": M, "T": T, "frames": B, "sim3_frames_ms": sms, "pnp_frames_ms": pms,
           "sim3_mean_inliers": round(float(ns.float().mean()), 1), "sim3_failed_frames": int((ns == 0).sum()),
           "pnp_mean_inliers": round(float(ni.float().mean()), 1), "pnp_failed_frames": int((ni == 0).sum()),
           "sim3_over_pnp": round(sms[0] / pms[0], 3)}
    print(json.dumps(row), flush=True)
    e.close()
