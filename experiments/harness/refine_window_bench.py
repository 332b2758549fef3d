"""Local bundle adjustment (fpc_refine_window_frames) beside the two calls a mapper has without it, on the same scenes in
the same process, alternating: fpc_pnp_frames (one pose per frame, the landmarks held fixed) and fpc_refine_pose_frames (two
views per problem), DESIGN.md section 7.  Windows of 4 and 16 VGA frames over 200 and 1 000 landmarks: the planted box scenes
of tests/test_refine_window.py (depth 3 .. 8, pixels rounded to integers, start 0.12 degrees / 1 % off), written in place of
every frame's keypoints and matched against the key by a table.
    python experiments/harness/refine_window_bench.py [reps] [runs] [frames landmarks]
prints one JSON line per (frames, landmarks): the three calls from HIP events on the ctx stream (median, min and max over `runs`
runs of `reps` back-to-back calls, after a warm-up; the runs of the calls alternate), the window call's attempts, accepted
steps and rms, and its launches per call (6 + 5 per attempt of `iterations`, 2 or 3 memsets).  How much of the call is launch
gaps needs a kernel trace of its own, which gives the kernels' own times:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/refine_window_bench.py 20 1 16 1000
(the rw_*_kernel rows; the call's time less their sum per call is what the stream spent between launches)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import _lib
from fpc_amd.engine import Engine
from tests.test_refine_window import KVEC, box_scene

H, W, B = 480, 640, 16
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cases = [(int(sys.argv[3]), int(sys.argv[4]))] if len(sys.argv) > 4 else [(4, 200), (16, 200), (4, 1000), (16, 1000)]


def timed(e, fns):
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


for n, L in cases:
    e = Engine(H, W, max_batch=B, descriptor_enabled=False, max_keypoints=max(L, 256))
    lib, ctx, cap = e._l, e._ctx, e.capacity
    assert cap >= L
    e.pnp_reserve()
    e.window_reserve()
    sc = box_scene(1000 * n + L, n, landmarks=L, stride=cap)
    xy, count = e._points_view()
    prob = torch.zeros((B, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob)                                               # the context holds B frames of results
    xy[:n].copy_(torch.from_numpy(sc.xy.astype(np.int32)))
    count[:n].copy_(torch.from_numpy(sc.nobs.astype(np.int32)))
    dev = "cuda"
    match = torch.from_numpy(sc.idx.astype(np.int32)).to(dev)
    kxy = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    kxy[:L] = torch.from_numpy(sc.key_xy.astype(np.int32)).to(dev)
    kxyz = torch.zeros((cap, 3), dtype=torch.float32, device=dev)
    kxyz[:L] = torch.from_numpy(sc.x0.astype(np.float32)).to(dev)
    kcount = torch.tensor([L], dtype=torch.int32, device=dev)
    rin = torch.from_numpy(sc.r0.astype(np.float32).reshape(n, 9)).to(dev)
    tin = torch.from_numpy(sc.t0.astype(np.float32)).to(dev)
    # the same poses the other way round, |t| = 1: the pose calls' convention, for fpc_refine_pose_frames
    rinv = np.transpose(sc.r0, (0, 2, 1))
    tinv = -np.einsum("fij,fj->fi", rinv, sc.t0)
    rp = torch.from_numpy(rinv.astype(np.float32).reshape(n, 9)).to(dev)
    tp = torch.from_numpy((tinv / np.linalg.norm(tinv, axis=1, keepdims=True)).astype(np.float32)).to(dev)
    f32, i32, u8 = torch.float32, torch.int32, torch.uint8
    R, t, nobs = torch.empty((n, 9), dtype=f32, device=dev), torch.empty((n, 3), dtype=f32, device=dev), torch.empty((n,), dtype=i32, device=dev)
    xyz, kind = torch.empty((cap, 3), dtype=f32, device=dev), torch.empty((cap,), dtype=u8, device=dev)
    obs, stats = torch.empty((n, cap), dtype=u8, device=dev), torch.empty((4,), dtype=f32, device=dev)
    R2, t2, n2 = torch.empty_like(R), torch.empty_like(t), torch.empty_like(nobs)
    xyz2, front2 = torch.empty((n, cap, 3), dtype=f32, device=dev), torch.empty((n, cap), dtype=u8, device=dev)
    stats2 = torch.empty((n, 4), dtype=f32, device=dev)
    R3, t3, n3, in3 = torch.empty_like(R), torch.empty_like(t), torch.empty_like(nobs), torch.empty((n, cap), dtype=u8, device=dev)
    wp = _lib.FpcWindowParams()
    lib.fpc_default_window_params(ctypes.byref(wp))
    rpar = _lib.FpcRefineParams()
    lib.fpc_default_refine_params(ctypes.byref(rpar))
    ppar = _lib.FpcPnpParams()
    lib.fpc_default_pnp_params(ctypes.byref(ppar))
    torch.cuda.synchronize()

    def window():
        assert lib.fpc_refine_window_frames(ctx, n, kxy.data_ptr(), kcount.data_ptr(), kxyz.data_ptr(), None, match.data_ptr(),
                                            rin.data_ptr(), tin.data_ptr(), ctypes.byref(wp), R.data_ptr(), t.data_ptr(),
                                            nobs.data_ptr(), xyz.data_ptr(), kind.data_ptr(), obs.data_ptr(), stats.data_ptr()) == 0

    def refine():
        assert lib.fpc_refine_pose_frames(ctx, n, 0, kxy.data_ptr(), kcount.data_ptr(), match.data_ptr(), rp.data_ptr(),
                                          tp.data_ptr(), ctypes.byref(rpar), R2.data_ptr(), t2.data_ptr(), n2.data_ptr(),
                                          xyz2.data_ptr(), front2.data_ptr(), stats2.data_ptr()) == 0

    def pnp():
        assert lib.fpc_pnp_frames(ctx, n, kxyz.data_ptr(), None, kcount.data_ptr(), match.data_ptr(), ctypes.byref(ppar),
                                  R3.data_ptr(), t3.data_ptr(), n3.data_ptr(), in3.data_ptr()) == 0

    w_ms, r_ms, p_ms = timed(e, (window, refine, pnp))
    st = stats.cpu().numpy()
    row = {"frames": n, "landmarks": L, "iterations": wp.iterations, "refine_window_frames_ms": w_ms,
           "refine_pose_frames_ms": r_ms, "pnp_frames_ms": p_ms, "observations": int(nobs.sum()),
           "refined": int((kind == 1).sum()), "attempts": int(st[2]), "accepted": int(st[3]),
           "rms_before_px": round(float(st[0]), 4), "rms_after_px": round(float(st[1]), 4),
           "launches_per_call": 6 + 5 * wp.iterations + 1, "window_us_per_launch": round(1e3 * w_ms[0] / (7 + 5 * wp.iterations), 2)}
    print(json.dumps(row), flush=True)
    e.close()
