"""RANSAC fundamental matrices (fpc_fundamental_frames) beside RANSAC homographies (fpc_homography_frames) on the same pair
lists in the same process, DESIGN.md section 7.  32 VGA frames; max_keypoints K = 500, 1000, 2000, 4500 with a low
confidence threshold, so every frame holds exactly K keypoints; matched without the cross check against frame 0, so every
frame has exactly K pairs; T = 256, 1024, 4096 hypotheses.
    python experiments/harness/fundamental_bench.py [reps] [runs]
prints one JSON line per (K, T): both calls from HIP events on the ctx stream (median, min and max over `runs` runs of `reps`
back-to-back calls, after a warm-up), their ratio, and the mean inlier counts.  The per-kernel times need a run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/fundamental_bench.py 20 1
(the dispatches of fm_score_kernel come in (K, T) order, 3 + reps per pair)."""
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


for K in (500, 1000, 2000, 4500):
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
    out = torch.empty((B, 9), dtype=torch.float32, device="cuda")
    ni = torch.empty((B,), dtype=torch.int32, device="cuda")
    mask = torch.empty((B, cap), dtype=torch.uint8, device="cuda")
    p = _lib.FpcRansacParams()
    lib.fpc_default_ransac_params(ctypes.byref(p))
    assert lib.fpc_match_frames(ctx, B, 0, key.data_ptr(), kcount.data_ptr(), 0, 0.0, 0.0, m.data_ptr(), None) == 0
    e.sync()
    assert int((m >= 0).sum()) == B * K

    def homography():
        assert lib.fpc_homography_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(p),
                                         out.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    def fundamental():
        assert lib.fpc_fundamental_frames(ctx, B, 0, kxy.data_ptr(), kcount.data_ptr(), m.data_ptr(), ctypes.byref(p),
                                          out.data_ptr(), ni.data_ptr(), mask.data_ptr()) == 0

    for T in (256, 1024, 4096):
        p.iterations = T
        hms = timed(e, homography)
        hin = round(float(ni.float().mean()), 1)
        fms = timed(e, fundamental)
        print(json.dumps({"K": K, "T": T, "frames": B, "homography_frames_ms": hms, "fundamental_frames_ms": fms,
                          "ratio": round(fms[0] / hms[0], 2), "hypothesis_pair_tests": B * T * K,
                          "gtests_per_s": round(B * T * K / fms[0] / 1e6, 1), "homography_mean_inliers": hin,
                          "fundamental_mean_inliers": round(float(ni.float().mean()), 1)}), flush=True)
    e.close()
