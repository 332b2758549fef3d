"""Relative pose (fpc_pose_frames) beside the RANSAC fundamental matrices it consumes (fpc_fundamental_frames) on the same
pair lists in the same process, DESIGN.md section 7.  32 VGA frames; max_keypoints K = 500, 1000, 2000 with a low confidence
threshold, so every frame holds exactly K keypoints; matched without the cross check against frame 0, so every frame has
exactly K pairs; T = 1024 hypotheses for the F.  The pose call reads the F that call wrote, at a threshold of 3 px and at one
beyond the frame (every pair used: the most work the kernel can have), with and without the xyz / front outputs.
    python experiments/harness/pose_bench.py [reps] [runs]
prints one JSON line per K: the calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up), and the mean counts.  The kernels' own times need a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/pose_bench.py 20 1
(pose_kernel beside fm_refit_kernel and hf_gather_kernel)."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import _lib, synth
from fpc_amd.engine import Engine

H, W, B = 480, 640, 32
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sd = synth.make_state_dict(0, dustbin_bias=7.0)
frames = torch.from_numpy(synth.make_batch(0, B, H, W)).cuda().contiguous()


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


for K in (500, 1000, 2000):
    e = Engine(H, W, max_batch=B, conf_thresh=1e-6, max_keypoints=K)
    e.load_state_dict(sd)
    torch.cuda.synchronize()
    e.detect_async(frames, B)
    assert (e.counts(B)[0] == K).all()
    lib, ctx, cap = e._l, e._ctx, e.capacity
    key, kcount = e.keep_frame(0)
    kxy = e.keep_frame_points(0)
    e.sync()
    m = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    fm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
    ni = torch.empty((B,), dtype=torch.int32, device="cuda")
    mask = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    rm = torch.empty((B, 9), dtype=torch.float32, device="cuda")
    tv = torch.empty((B, 3), dtype=torch.float32, device="cuda")
    nf = torch.empty((B,), dtype=torch.int32, device="cuda")
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device="cuda")
    front = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    p = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(p))
    p.iterations = 1024
    q = _lib.FpcPoseParams()
    lib.fpc_default_pose_params(ctypes.byref(q))
    q.min_front = 1
    assert lib.fpc_match_frames(ctx, B, 0, key.data_ptr(), kcount.data_ptr(), 0, 0.0, 0.0, m.data_ptr(), None) == 0
    e.sync()
    assert int((m >= 0).sum()) == B * K

    def fundamental():
        assert lib.fpc_fundamental_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(p),
                                          fm.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def pose(points=True):
        assert lib.fpc_pose_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), fm.data_ptr(), ctypes.byref(q),
                                   rm.data_ptr(), tv.data_ptr(), nf.data_ptr(), xyz.data_ptr() if points else None,
                                   front.data_ptr() if points else None) == 0

    fms = timed(e, fundamental)
    row = {"K": K, "T": p.iterations, "frames": B, "fundamental_frames_ms": fms,
           "fundamental_mean_inliers": round(float(ni.float().mean()), 1)}
    for name, thr in (("3px", 3.0), ("all_pairs", 1e6)):
        q.reproj_threshold = thr
        row["pose_frames_%s_ms" % name] = timed(e, pose)
        row["pose_frames_%s_no_points_ms" % name] = timed(e, lambda: pose(False))
        row["pose_%s_mean_front" % name] = round(float(nf.float().mean()), 1)
    row["pose_over_fundamental"] = round(row["pose_frames_3px_ms"][0] / fms[0], 3)
    print(json.dumps(row), flush=True)
    e.close()
