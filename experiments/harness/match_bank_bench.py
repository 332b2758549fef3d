"""One fpc_match_bank call against what the library offered before it for the same answer: S calls
of fpc_match_frames with slot s as the key, the per-slot count of matches and the arg-max with torch on the device, and
the host read of the winning slot that flow needs before it can go on (the bank call needs none; its wall-clock figure
synchronises all the same, so that both sides end with the answer on the host).
n = 1 and 32 VGA frames; max_keypoints K = 500, 1000, 2000, 4500 with a low confidence threshold, so every frame and every
slot holds exactly K rows; S = 16 and 64 slots; cross check on, max_dist 0.7.
    python experiments/harness/match_bank_bench.py [reps] [--format {f32,bf16}]
prints one JSON line per (n, K, S): the median of 5 runs of `reps` calls each with the runs' min and max, the bank call
from HIP events on the ctx stream and wall-clock, the loop wall-clock; the bank's chunk and bytes; and
2 * n * S * K * K * D, the FLOPs the score pass's MFMAs execute.  With --format bf16 (fpc_bank_create_ex, FPC_BANK_BF16) every
point times the fp32 bank first and the bf16 bank of the same frames right after it, in the same process on the same inputs,
and prints both with their ratio and whether the two banks name the same slots; the loop (which needs fp32 rows) is left out.
The executed-MFMA fraction needs the kernel's own duration:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/match_bank_bench.py 3
then bank_score_kernel's mean duration per case against 157.3 TF (bank_score_bf16_kernel: against 2 516 TF)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import torch

from fpc_amd import synth
from fpc_amd.engine import Engine

H, W = 480, 640
RUNS = 5
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=5)
ap.add_argument("--format", choices=("f32", "bf16"), default="f32")
args = ap.parse_args()
reps = args.reps
sd = synth.make_state_dict(0, dustbin_bias=7.0)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


for n in (1, 32):
    frames = torch.from_numpy(synth.make_batch(0, n, H, W)).cuda().contiguous()
    for K in (500, 1000, 2000, 4500):
        e = Engine(H, W, max_batch=n, conf_thresh=1e-6, max_keypoints=K)
        e.load_state_dict(sd)
        torch.cuda.synchronize()
        e.detect_async(frames, n)
        cnt = e.counts(n)[0]
        assert (cnt == K).all(), cnt
        lib, ctx, cap, dim = e._l, e._ctx, e.capacity, e.desc_dim
        st = e.torch_stream()
        for S in (16, 64):
            if args.format == "bf16":
                out = {"frames": n, "K": K, "slots": S}
                answers = []
                for fmt in ("f32", "bf16"):
                    e.bank_create(S, K, format=fmt)
                    for s in range(S):
                        e.bank_store(s % n, s)
                    score, best, m, d = e.match_bank_async(n, cross_check=True, max_dist=0.7)
                    e.sync()
                    answers.append(best.cpu())

                    def bank():
                        assert lib.fpc_match_bank(ctx, n, 1, 0.7, 0.0, 0, score.data_ptr(), best.data_ptr(), m.data_ptr(),
                                                  d.data_ptr()) == 0

                    bank()
                    e.sync()
                    ev = []
                    for _ in range(RUNS):
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record(st)
                        for _ in range(reps):
                            bank()
                        t1.record(st)
                        e.sync()
                        ev.append(t0.elapsed_time(t1) / reps)
                    info = e.bank_info()
                    out[fmt] = {"chunk": info["chunk"], "bank_bytes": info["bytes"], "bank_events_ms": spread(ev)}
                    e.bank_destroy()
                out["f32_over_bf16"] = round(out["f32"]["bank_events_ms"]["median"] / out["bf16"]["bank_events_ms"]["median"], 2)
                # beyond the runs' spread: the slower bf16 run against the faster fp32 run
                out["bf16_not_slower"] = out["bf16"]["bank_events_ms"]["min"] <= out["f32"]["bank_events_ms"]["max"]
                out["same_best"] = bool((answers[0] == answers[1]).all())
                out["score_mfma_flops"] = 2.0 * n * S * K * K * dim
                print(json.dumps(out), flush=True)
                continue
            e.bank_create(S, K)
            for s in range(S):
                e.bank_store(s % n, s)
            e.sync()
            info = e.bank_info()
            bd, _, bc = e.bank_view()
            score = torch.empty((n, S), dtype=torch.int32, device="cuda")
            best = torch.empty((n,), dtype=torch.int32, device="cuda")
            m = torch.empty((n, cap), dtype=torch.int32, device="cuda")
            d = torch.empty((n, cap), dtype=torch.float32, device="cuda")
            m_all = torch.empty((S, n, cap), dtype=torch.int32, device="cuda")
            d_all = torch.empty((S, n, cap), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def bank():
                assert lib.fpc_match_bank(ctx, n, 1, 0.7, 0.0, 0, score.data_ptr(), best.data_ptr(), m.data_ptr(),
                                          d.data_ptr()) == 0

            def loop():
                for s in range(S):
                    assert lib.fpc_match_frames(ctx, n, 0, bd[s].data_ptr(), bc[s:s + 1].data_ptr(), 1, 0.7, 0.0,
                                                m_all[s].data_ptr(), d_all[s].data_ptr()) == 0
                with torch.cuda.stream(st):
                    sc = (m_all >= 0).sum(dim=2).t()
                    b = sc.argmax(dim=1)
                    return b.cpu()                  # the host needs the slot to pick the table and the key coordinates

            for fn in (bank, loop):
                for _ in range(2):
                    fn()
                e.sync()
            ev, wall, lp = [], [], []
            for _ in range(RUNS):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(st)
                for _ in range(reps):
                    bank()
                t1.record(st)
                e.sync()
                ev.append(t0.elapsed_time(t1) / reps)
                w = time.perf_counter()
                for _ in range(reps):
                    bank()
                    e.sync()
                wall.append((time.perf_counter() - w) * 1e3 / reps)
                w = time.perf_counter()
                for _ in range(reps):
                    loop()
                lp.append((time.perf_counter() - w) * 1e3 / reps)
            flops = 2.0 * n * S * K * K * dim
            print(json.dumps({"frames": n, "K": K, "slots": S, "chunk": info["chunk"], "bank_bytes": info["bytes"],
                              "bank_events_ms": spread(ev), "bank_wall_ms": spread(wall), "loop_wall_ms": spread(lp),
                              "speedup_wall": round(statistics.median(lp) / statistics.median(wall), 2),
                              "score_mfma_flops": flops,
                              "tflops_events": round(flops / statistics.median(ev) / 1e9, 2)}), flush=True)
            e.bank_destroy()
        e.close()
