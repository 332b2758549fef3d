"""Relative pose from a homography (fpc_pose_homography_frames) beside the RANSAC homographies it consumes
(fpc_homography_frames) and beside the epipolar pose call (fpc_pose_frames, with the F of fpc_fundamental_frames) on the same
rows in the same process, DESIGN.md section 7.  pose_bench.py's setup: 32 VGA frames; max_keypoints K = 500, 1000, 2000 with a
low confidence threshold, so every frame holds exactly K keypoints; matched without the cross check against frame 0, so every
frame has exactly K pairs; T = 1024 hypotheses for H and F.  The homography-pose call reads the H that call wrote, at 3 px and
at a threshold beyond the frame (every pair counts for every candidate: the most work the kernel can have), with and without
the xyz / front outputs.
    python experiments/harness/pose_homography_bench.py [reps] [runs]
prints one JSON line per K: the calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up), the kinds and the mean counts.  The kernels' own times need a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/pose_homography_bench.py 20 1
(pose_homography_kernel beside pose_kernel, ransac_refit_kernel and hf_gather_kernel)."""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
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
    dev = "cuda"
    m = torch.empty((B, cap), dtype=torch.int32, device=dev)
    hm, fm = (torch.empty((B, 9), dtype=torch.float32, device=dev) for _ in range(2))
    ni = torch.empty((B,), dtype=torch.int32, device=dev)
    mask = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    kind = torch.empty((B,), dtype=torch.int32, device=dev)
    rm2, rm = torch.empty((B, 18), dtype=torch.float32, device=dev), torch.empty((B, 9), dtype=torch.float32, device=dev)
    tv2, tv = torch.empty((B, 6), dtype=torch.float32, device=dev), torch.empty((B, 3), dtype=torch.float32, device=dev)
    plane = torch.empty((B, 8), dtype=torch.float32, device=dev)
    nf2, npl = (torch.empty((B, 2), dtype=torch.int32, device=dev) for _ in range(2))
    nf = torch.empty((B,), dtype=torch.int32, device=dev)
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device=dev)
    front = torch.empty((B, cap), dtype=torch.uint8, device=dev)
    p = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(p))
    p.iterations = 1024
    q = _lib.FpcPoseHomographyParams()
    lib.fpc_default_pose_homography_params(ctypes.byref(q))
    q.min_front = 1
    r = _lib.FpcPoseParams()
    lib.fpc_default_pose_params(ctypes.byref(r))
    r.min_front = 1
    assert lib.fpc_match_frames(ctx, B, 0, key.data_ptr(), kcount.data_ptr(), 0, 0.0, 0.0, m.data_ptr(), None) == 0
    e.sync()
    assert int((m >= 0).sum()) == B * K
    src = (0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr())

    def homography():
        assert lib.fpc_homography_frames(ctx, B, *src, ctypes.byref(p), hm.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def fundamental():
        assert lib.fpc_fundamental_frames(ctx, B, *src, ctypes.byref(p), fm.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def pose_h(points=True):
        assert lib.fpc_pose_homography_frames(ctx, B, *src, hm.data_ptr(), ctypes.byref(q), kind.data_ptr(), rm2.data_ptr(),
                                              tv2.data_ptr(), plane.data_ptr(), nf2.data_ptr(), npl.data_ptr(),
                                              xyz.data_ptr() if points else None, front.data_ptr() if points else None) == 0

    def pose_f():
        assert lib.fpc_pose_frames(ctx, B, *src, fm.data_ptr(), ctypes.byref(r), rm.data_ptr(), tv.data_ptr(), nf.data_ptr(),
                                   xyz.data_ptr(), front.data_ptr()) == 0

    fundamental()
    row = {"K": K, "T": p.iterations, "frames": B, "pose_frames_3px_ms": timed(e, pose_f),
           "pose_mean_front": round(float(nf.float().mean()), 1), "homography_frames_ms": timed(e, homography),
           "homography_mean_inliers": round(float(ni.float().mean()), 1)}
    for name, thr in (("3px", 3.0), ("all_pairs", 1e6)):
        q.reproj_threshold = thr
        row["pose_homography_frames_%s_ms" % name] = timed(e, pose_h)
        row["pose_homography_frames_%s_no_points_ms" % name] = timed(e, lambda: pose_h(False))
        row["pose_homography_%s_kinds" % name] = np.bincount(kind.cpu().numpy(), minlength=4).tolist()
        row["pose_homography_%s_mean_support" % name] = [round(float(v), 1) for v in nf2.float().mean(0)]
    row["pose_homography_over_pose"] = round(row["pose_homography_frames_3px_ms"][0] / row["pose_frames_3px_ms"][0], 3)
    row["pose_homography_over_homography"] = round(row["pose_homography_frames_3px_ms"][0] / row["homography_frames_ms"][0], 3)
    print(json.dumps(row), flush=True)
    e.close()
