"""Two-view bundle adjustment (fpc_refine_pose_frames) beside the linear pose it refines (fpc_pose_frames) on the same pair
lists in the same process, alternating, DESIGN.md section 7.  32 VGA frames of K = 500, 1000, 2000 pairs each: a planted scene
with depth (random points 2 .. 8 units away, a rotation of 2 .. 12 degrees, a translation), both views rounded to integer
pixels and written in place of every frame's keypoints and of the key set, matched row to row -- so nearly every pair is a
member and a call has the most work it can have.  The pose call reads the exact F of the planted motion; the refine call
starts from that call's R, t and runs up to 8 attempts.
    python experiments/harness/refine_pose_bench.py [reps] [runs]
prints one JSON line per K: both calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up; the runs of the two calls alternate), the mean members, attempts and accepted steps, and
the refine call's time per attempt.  The kernels' own times need a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/refine_pose_bench.py 20 1
(refine_pose_kernel beside pose_kernel and hf_gather_kernel)."""
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
KVEC = (500.0, 500.0, 320.0, 240.0)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
KM = np.array([[KVEC[0], 0, KVEC[2]], [0, KVEC[1], KVEC[3]], [0, 0, 1.0]])


def scene(rng, k):
    """K pairs of one planted motion -> (query pixels, train pixels int32 [K,2], the exact F [9])."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = np.deg2rad(rng.uniform(2, 12))
    ax = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + np.sin(ang) * ax + (1 - np.cos(ang)) * ax @ ax
    t = rng.uniform(-0.6, 0.6, 3)
    pts = np.stack([rng.uniform(-3, 3, k), rng.uniform(-2, 2, k), rng.uniform(2, 8, k)], 1)
    a, b = pts @ KM.T, (pts @ r.T + t) @ KM.T
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    f = np.linalg.inv(KM).T @ tx @ r @ np.linalg.inv(KM)
    return np.rint(a[:, :2] / a[:, 2:]).astype(np.int32), np.rint(b[:, :2] / b[:, 2:]).astype(np.int32), (f / np.abs(f).max()).ravel()


def timed_pair(e, fns):
    """The calls of `fns`, alternating run by run -> per call [median, min, max] ms."""
    for fn in fns:
        for _ in range(3):
            fn()
    e.sync()
    st, out = e.torch_stream(), [[] for _ in fns]
    for _ in range(runs):
        for fn, o in zip(fns, out):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(st)
            for _ in range(reps):
                fn()
            t1.record(st)
            e.sync()
            o.append(t0.elapsed_time(t1) / reps)
    return [[round(float(v), 4) for v in (np.median(o), min(o), max(o))] for o in out]


for K in (500, 1000, 2000):
    e = Engine(H, W, max_batch=B, descriptor_enabled=False, max_keypoints=K)
    lib, ctx, cap = e._l, e._ctx, e.capacity
    assert cap >= K
    rng = np.random.Generator(np.random.PCG64(K))
    # one key set serves every frame of a call, so the 32 frames hold the same planted scene: 32 workgroups of equal work
    q0, t0, f0 = scene(rng, K)
    xy, count = e._points_view()
    prob = torch.zeros((B, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob)                                               # the context holds B frames of results
    xy[:B, :K].copy_(torch.from_numpy(np.repeat(q0[None], B, 0)))
    count[:B].fill_(K)
    kxy = torch.from_numpy(t0).cuda().contiguous()
    kcount = torch.tensor([K], dtype=torch.int32, device="cuda")
    m = torch.full((B, cap), -1, dtype=torch.int32, device="cuda")
    m[:, :K] = torch.arange(K, dtype=torch.int32, device="cuda")
    fm = torch.from_numpy(np.repeat(f0[None], B, 0).astype(np.float32)).cuda().contiguous()
    rm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
    tv = torch.empty((B, 3), dtype=torch.float32, device="cuda")
    nf = torch.empty((B,), dtype=torch.int32, device="cuda")
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device="cuda")
    front = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    r2, t2 = torch.empty_like(rm), torch.empty_like(tv)
    n2 = torch.empty_like(nf)
    xyz2, front2 = torch.empty_like(xyz), torch.empty_like(front)
    stats = torch.empty((B, 4), dtype=torch.float32, device="cuda")
    q = _lib.FpcPoseParams()
    lib.fpc_default_pose_params(ctypes.byref(q))
    p = _lib.FpcRefineParams()
    lib.fpc_default_refine_params(ctypes.byref(p))
    p.iterations = 8
    torch.cuda.synchronize()

    def pose():
        assert lib.fpc_pose_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), fm.data_ptr(), ctypes.byref(q),
                                   rm.data_ptr(), tv.data_ptr(), nf.data_ptr(), xyz.data_ptr(), front.data_ptr()) == 0

    def refine():
        assert lib.fpc_refine_pose_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), rm.data_ptr(),
                                          tv.data_ptr(), ctypes.byref(p), r2.data_ptr(), t2.data_ptr(), n2.data_ptr(),
                                          xyz2.data_ptr(), front2.data_ptr(), stats.data_ptr()) == 0

    pose()
    e.sync()
    pose_ms, refine_ms = timed_pair(e, (pose, refine))
    st = stats.cpu().numpy()
    attempts = float(st[:, 2].mean())
    row = {"K": K, "frames": B, "iterations": p.iterations, "pose_frames_ms": pose_ms, "refine_pose_frames_ms": refine_ms,
           "pose_mean_front": round(float(nf.float().mean()), 1), "refine_mean_front": round(float(n2.float().mean()), 1),
           "mean_attempts": round(attempts, 2), "mean_accepted": round(float(st[:, 3].mean()), 2),
           "rms_before_px": round(float(st[:, 0].mean()), 4), "rms_after_px": round(float(st[:, 1].mean()), 4),
           "refine_us_per_attempt": round(1e3 * refine_ms[0] / max(attempts, 1.0), 2),
           "refine_over_pose": round(refine_ms[0] / pose_ms[0], 2)}
    print(json.dumps(row), flush=True)
    e.close()
