"""Minimal-sample relative pose (fpc_essential_frames) beside the 8-point (fpc_fundamental_frames) in the same process,
DESIGN.md section 7.  32 VGA frames of exactly M rows, each matched to one row of a key frame; both views see points at
depths 4 .. 8 ("box") or on a plane through depth 6 tilted 25 degrees ("planar") under a rotation of 2 .. 10 degrees and a
baseline of 0.5, pixels rounded, 60 % of the matches replaced by wrong ones, M = 200 and 1000.  Both calls run at T = 1024,
and at the budgets the float64 restatements needed on the 60 % scenes of tests/test_essential_ransac.py: 1024 for this
model, 4096 for the 8-point.
    python experiments/harness/essential_bench.py [reps] [runs]
prints one JSON line per workload and M: the calls from HIP events on the ctx stream (median, min and max over `runs` runs of
`reps` back-to-back calls, after a warm-up; the runs of the calls ALTERNATE, so that a drift of the clocks meets them all),
the mean inlier counts and the number of frames each call solved.  The per-kernel split needs a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/essential_bench.py 20 1
(hf_gather_kernel, essential_score_kernel, essential_refit_kernel beside fm_score_kernel, fm_refit_kernel)."""
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


def timed_alternating(e, fns):
    for fn in fns:
        for _ in range(3):
            fn()
    e.sync()
    st, out = e.torch_stream(), [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            for _ in range(reps):
                fn()
            t1.record(st)
            e.sync()
            out[k].append(t0.elapsed_time(t1) / reps)
    return [[round(float(v), 4) for v in (np.median(o), min(o), max(o))] for o in out]


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def project(x):
    return np.round(np.stack([FX * x[:, 0] / x[:, 2] + CX, FY * x[:, 1] / x[:, 2] + CY], 1)).astype(np.int32)


for workload in ("box", "planar"):
    for M in (200, 1000):
        e = Engine(H, W, max_batch=B, descriptor_enabled=False, max_keypoints=1024)
        cap = e.capacity
        prob = torch.zeros((B, H, W))
        prob[:, 40, 40] = 0.5
        e.get_points(prob)                                          # B frames of keypoints; the planted rows take their place
        rng = np.random.default_rng(M)
        px = np.stack([rng.uniform(100, W - 100, M), rng.uniform(80, H - 80, M)], 1)
        z = rng.uniform(4.0, 8.0, M)
        if workload == "planar":
            tilt = np.deg2rad(25.0)
            nrm = np.array([np.sin(tilt) * np.cos(0.7), np.sin(tilt) * np.sin(0.7), np.cos(tilt)])
            z = 6.0 * nrm[2] / (np.stack([(px[:, 0] - CX) / FX, (px[:, 1] - CY) / FY, np.ones(M)], 1) @ nrm)
        key_xyz = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FY * z, z], 1)
        key_xy = np.round(px).astype(np.int32)
        hx, hm = np.zeros((B, cap, 2), np.int32), np.full((B, cap), -1, np.int32)
        for f in range(B):
            r = rotation(rng.normal(size=3), np.deg2rad(rng.uniform(2.0, 10.0)))
            t = rng.normal(size=3)
            t = 0.5 * t / np.linalg.norm(t)
            order = rng.permutation(M)
            hx[f, :M] = np.clip(project(key_xyz[order] @ r.T + t), 0, [W - 1, H - 1])
            hm[f, :M] = order
            wrong = rng.choice(M, (3 * M) // 5, replace=False)
            hm[f, wrong] = rng.integers(0, M, len(wrong))
        xy, count = e._points_view()
        xy[:B].copy_(torch.from_numpy(hx))
        count[:B].fill_(M)
        m = torch.from_numpy(hm).cuda()
        kxy = torch.from_numpy(key_xy).cuda()
        kcount = torch.tensor([M], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        lib, ctx = e._l, e._ctx
        fm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
        em = torch.empty((B, 9), dtype=torch.float32, device="cuda")
        ni = torch.empty((B,), dtype=torch.int32, device="cuda")
        mask = torch.empty((B, cap), dtype=torch.uint8, device="cuda")

        def essential(iterations):
            q = _lib.FpcEssentialParams()
            lib.fpc_default_essential_params(ctypes.byref(q))
            q.iterations = iterations

            def fn():
                assert lib.fpc_essential_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(q),
                                                fm.data_ptr(), em.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0
            return fn

        def fundamental(iterations):
            q = _lib.FpcRansacParams()
            lib.fpc_default_ransac_params(ctypes.byref(q))
            q.iterations = iterations

            def fn():
                assert lib.fpc_fundamental_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(q),
                                                  fm.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0
            return fn

        calls = [("essential_T256", essential(256)), ("essential_T1024", essential(1024)),
                 ("fundamental_T1024", fundamental(1024)), ("fundamental_T4096", fundamental(4096))]
        row = {"workload": workload, "M": M, "frames": B}
        for (tag, fn), ms in zip(calls, timed_alternating(e, [fn for _, fn in calls])):
            row[tag + "_ms"] = ms
            fn()
            e.sync()
            row[tag + "_mean_inliers"] = round(float(ni.float().mean()), 1)
            row[tag + "_solved_frames"] = int((ni != 0).sum())
        print(json.dumps(row), flush=True)
        e.close()
