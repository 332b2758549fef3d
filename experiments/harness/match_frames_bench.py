"""Batched descriptor matching (fpc_match_frames) against today's best caller path (fpc_get_counts + one fpc_match per
frame), DESIGN.md section 7.  32 VGA frames; max_keypoints K = 500, 1000, 2000, 4500 with a low confidence threshold, so
every frame holds exactly K keypoints; matched (cross check on) against a K-row key (frame 0's descriptors).
    python experiments/harness/match_frames_bench.py [reps]
prints one JSON line per K: the batched call from HIP events on the ctx stream and wall-clock to a synchronised result,
the per-frame loop wall-clock (it synchronises inside fpc_get_counts), and 2 * sum(nq * nt * D), the FLOPs the MFMAs
execute.  The executed-MFMA fraction needs the kernel's own duration:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python experiments/harness/match_frames_bench.py 20
then match_frames_kernel's mean duration per K (its dispatches come in K order, 2 * reps + 3 per K) against 157.3 TF."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd import synth
from fpc_amd.engine import Engine

H, W, B = 480, 640, 32
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
sd = synth.make_state_dict(0, dustbin_bias=7.0)
frames = torch.from_numpy(synth.make_batch(0, B, H, W)).cuda().contiguous()
for K in (500, 1000, 2000, 4500):
    e = Engine(H, W, max_batch=B, conf_thresh=1e-6, max_keypoints=K)
    e.load_state_dict(sd)
    torch.cuda.synchronize()
    e.detect_async(frames, B)
    cnt = e.counts(B)[0]
    assert (cnt == K).all(), cnt
    lib, ctx, cap, dim = e._l, e._ctx, e.capacity, e.desc_dim
    key, kcount = e.keep_frame(0)
    e.sync()
    m = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    d = torch.empty((B, cap), dtype=torch.float32, device="cuda")
    desc = e._results_view()[0]
    kp, cp, mp, dp = key.data_ptr(), kcount.data_ptr(), m.data_ptr(), d.data_ptr()

    def batched():
        assert lib.fpc_match_frames(ctx, B, 0, kp, cp, 1, 0.0, 0.0, mp, dp) == 0

    def loop():
        cnt = np.zeros(B, np.int32)
        assert lib.fpc_get_counts(ctx, B, cnt.ctypes.data, None) == 0
        for f in range(B):
            assert lib.fpc_match(ctx, desc[f].data_ptr(), int(cnt[f]), kp, K, 1, 0.0, m[f].data_ptr(), d[f].data_ptr()) == 0

    for fn in (batched, loop):
        for _ in range(3):
            fn()
        e.sync()
    st = e.torch_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(st)
    for _ in range(reps):
        batched()
    t1.record(st)
    e.sync()
    ev_ms = t0.elapsed_time(t1) / reps
    w = time.perf_counter()
    for _ in range(reps):
        batched()
        e.sync()
    wall_ms = (time.perf_counter() - w) * 1e3 / reps
    w = time.perf_counter()
    for _ in range(reps):
        loop()
        e.sync()
    loop_ms = (time.perf_counter() - w) * 1e3 / reps
    flops = 2.0 * B * K * K * dim
    print(json.dumps({"K": K, "frames": B, "batched_events_ms": round(ev_ms, 4), "batched_wall_ms": round(wall_ms, 4),
                      "loop_wall_ms": round(loop_ms, 4), "speedup_wall": round(loop_ms / wall_ms, 2),
                      "mfma_flops": flops, "tflops_events": round(flops / ev_ms / 1e9, 2)}), flush=True)
    e.close()
