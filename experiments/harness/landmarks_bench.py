"""Map growth (fpc_landmarks_frames) beside the relative pose call (fpc_pose_frames) on the same match table in the same
process, DESIGN.md section 7.  pose_bench.py's setup: 32 VGA frames; max_keypoints K = 500, 1000, 2000 with a low confidence
threshold, so every frame holds exactly K keypoints; matched without the cross check against frame 0, so every frame has
exactly K rows with a match.  The pose call reads the F of fpc_fundamental_frames (T = 1024) at 3 px; the landmarks call runs
under one fixed pose (a sideways step: what the kernel computes per row does not depend on whether the row passes) against
the key without landmarks (every row triangulated), with a landmark on every row (every row carried over) and on every other
row.  The expectation to report against: one pass over the rows, so no more than the pose call, which makes two passes and a
decomposition.
    python experiments/harness/landmarks_bench.py [reps] [runs]
prints one JSON line per K: the calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up), and the mean counts.  The kernels' own times need a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/landmarks_bench.py 20 1
(landmarks_kernel beside pose_kernel and hf_gather_kernel)."""
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
    counts = torch.empty((B, 2), dtype=torch.int32, device="cuda")
    # the landmarks call's pose and the key's landmarks: the key's own pixels at depth 6, so that a row matched to itself
    # is carried over under the identity
    pose_r = torch.eye(3, device="cuda").reshape(1, 9).repeat(B, 1).contiguous()
    pose_t = torch.tensor([0.5, 0.0, 0.0], device="cuda").repeat(B, 1).contiguous()
    kz = torch.stack([(kxy[:, 0].float() - 320.0) / 500.0 * 6.0, (kxy[:, 1].float() - 240.0) / 500.0 * 6.0,
                      torch.full((cap,), 6.0, device="cuda")], 1).contiguous()
    every_other = (torch.arange(cap, device="cuda") % 2).to(torch.uint8).contiguous()
    p = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(p))
    p.iterations = 1024
    q = _lib.FpcPoseParams()
    lib.fpc_default_pose_params(ctypes.byref(q))
    q.min_front = 1
    lp = _lib.FpcLandmarkParams()
    lib.fpc_default_landmark_params(ctypes.byref(lp))
    assert lib.fpc_match_frames(ctx, B, 0, key.data_ptr(), kcount.data_ptr(), 0, 0.0, 0.0, m.data_ptr(), None) == 0
    e.sync()
    assert int((m >= 0).sum()) == B * K
    assert lib.fpc_fundamental_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(p),
                                      fm.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def pose():
        assert lib.fpc_pose_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), fm.data_ptr(), ctypes.byref(q),
                                   rm.data_ptr(), tv.data_ptr(), nf.data_ptr(), xyz.data_ptr(), front.data_ptr()) == 0

    def landmarks(key_xyz, key_valid):
        assert lib.fpc_landmarks_frames(ctx, B, kxy.data_ptr(), kcount.data_ptr(), key_xyz, key_valid, m.data_ptr(),
                                        pose_r.data_ptr(), pose_t.data_ptr(), ctypes.byref(lp), xyz.data_ptr(),
                                        front.data_ptr(), counts.data_ptr()) == 0

    row = {"K": K, "frames": B, "pose_frames_3px_ms": timed(e, pose), "pose_mean_front": round(float(nf.float().mean()), 1)}
    for name, args in (("triangulate", (None, None)), ("transfer", (kz.data_ptr(), None)),
                       ("mixed", (kz.data_ptr(), every_other.data_ptr()))):
        row["landmarks_frames_%s_ms" % name] = timed(e, lambda: landmarks(*args))
        row["landmarks_%s_mean_counts" % name] = [round(float(v), 1) for v in counts.float().mean(0)]
    row["landmarks_over_pose"] = round(max(row["landmarks_frames_%s_ms" % n][0] for n in ("triangulate", "transfer", "mixed"))
                                       / row["pose_frames_3px_ms"][0], 3)
    print(json.dumps(row), flush=True)
    e.close()
