"""Minimal-sample absolute pose (fpc_p3p_frames) beside the 6-point DLT (fpc_pnp_frames) in the same process, DESIGN.md section
7.  pnp_bench.py's planted workload -- 32 VGA frames of exactly M rows, each matched to one row of a key frame that carries a
3-D point, pixels rounded, a fifth of the matches replaced by wrong ones, M = 200 and 1000 -- once with the key's landmarks in
a box ("box") and once with the same pixels' landmarks on one plane through depth 8, tilted 25 degrees ("planar").
fpc_p3p_frames runs at T = 256 and T = 1024, fpc_pnp_frames at T = 1024, the default refits of either call.
    python experiments/harness/p3p_bench.py [reps] [runs]
prints one JSON line per workload and M: the three calls from HIP events on the ctx stream (median, min and max over `runs`
runs of `reps` back-to-back calls, after a warm-up), the mean inlier counts and the number of frames each call solved.  The
per-kernel split needs a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/p3p_bench.py 20 1
(pnp_gather_kernel, p3p_score_kernel, p3p_refit_kernel beside pnp_score_kernel, pnp_refit_kernel; in that table the P3P
kernels' rows mix T = 256 and T = 1024 -- P3P_BENCH_T=1024 in the environment leaves only the T = 1024 calls)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import _lib
from fpc_amd.engine import Engine

H, W, B = 480, 640, 32
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
P3P_T = [int(v) for v in os.environ.get("P3P_BENCH_T", "256,1024").split(",")]


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


for workload in ("box", "planar"):
    for M in (200, 1000):
        e = Engine(H, W, max_batch=B, descriptor_enabled=False, max_keypoints=1024)
        e.pnp_reserve()
        cap = e.capacity
        prob = torch.zeros((B, H, W))
        prob[:, 40, 40] = 0.5
        e.get_points(prob)                                          # B frames of keypoints; the planted rows take their place
        rng = np.random.default_rng(M)
        # the key frame: M landmarks in its camera frame (in front of both views)
        px = np.stack([rng.uniform(100, W - 100, M), rng.uniform(80, H - 80, M)], 1)
        z = rng.uniform(4.0, 12.0, M)
        if workload == "planar":
            tilt = np.deg2rad(25.0)
            nrm = np.array([np.sin(tilt) * np.cos(0.7), np.sin(tilt) * np.sin(0.7), np.cos(tilt)])
            z = 8.0 * nrm[2] / (np.stack([(px[:, 0] - CX) / FX, (px[:, 1] - CY) / FY, np.ones(M)], 1) @ nrm)
        key_xyz = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1).astype(np.float32)
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
        m = torch.from_numpy(hm).cuda()
        kxyz = torch.from_numpy(key_xyz).cuda()
        kcount = torch.tensor([M], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lib, ctx = e._l, e._ctx
        rm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
        tv = torch.empty((B, 3), dtype=torch.float32, device="cuda")
        ni = torch.empty((B,), dtype=torch.int32, device="cuda")
        mask = torch.empty((B, cap), dtype=torch.uint8, device="cuda")

        def call(name, iterations):
            q = _lib.FpcPnpParams()
            lib.fpc_default_pnp_params(ctypes.byref(q))
            q.iterations = iterations

            def fn():
                assert getattr(lib, name)(ctx, B, kxyz.data_ptr(), None, kcount.data_ptr(), m.data_ptr(), ctypes.byref(q),
                                          rm.data_ptr(), tv.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0
            return fn

        row = {"workload": workload, "M": M, "frames": B}
        calls = [("p3p_T%d" % t, "fpc_p3p_frames", t) for t in P3P_T]
        if "P3P_BENCH_T" not in os.environ:
            calls.append(("pnp_T1024", "fpc_pnp_frames", 1024))
        for tag, name, iterations in calls:
            row[tag + "_ms"] = timed(e, call(name, iterations))
            row[tag + "_mean_inliers"] = round(float(ni.float().mean()), 1)
            row[tag + "_solved_frames"] = int((ni != 0).sum())
        print(json.dumps(row), flush=True)
        e.close()
