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
With --topk K [K ...] every point times verified relocalisation instead: fpc_match_bank_topk + fpc_homography_bank_topk (k = K)
against the host loop of existing calls they replace -- fpc_match_bank for the scores, then for each j < K one
fpc_match_bank_guided (identity H, a radius beyond the frame) and one fpc_homography_bank with column j of the candidates
(taken from the new call and laid out per round before the clock starts, which favours the loop) -- on the same inputs in the
same process, HIP events on the ctx stream, the median of 5 runs with min and max; n = 1 and 32, max_keypoints 1000 and 2000,
S = 16.  not_slower: the new calls' fastest run against the loop's slowest, i.e. beyond the runs' spread.
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
ap.add_argument("--topk", type=int, nargs="+", default=None, metavar="K")
args = ap.parse_args()
reps = args.reps
sd = synth.make_state_dict(0, dustbin_bias=7.0)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}




def events_ms(e, st, fn):
    """The median, min and max over RUNS runs of `reps` calls of fn, from HIP events on the ctx stream."""
    fn()
    e.sync()
    ev = []
    for _ in range(RUNS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(st)
        for _ in range(reps):
            fn()
        t1.record(st)
        e.sync()
        ev.append(t0.elapsed_time(t1) / reps)
    return spread(ev)


def topk_point(e, n, K, S):
    """One (n, K, S) point of --topk: the bank of `format`, one JSON line per k."""
    import ctypes
    lib, ctx, cap = e._l, e._ctx, e.capacity
    st = e.torch_stream()
    e.bank_create(S, K, format=args.format)
    for s in range(S):
        e.bank_store(s % n, s)
    ws_bytes = e.bank_topk_reserve(max(args.topk))
    params = e._ransac_params({})
    ident = torch.eye(3, device="cuda").reshape(1, 9).repeat(n, 1).contiguous()
    score = torch.empty((n, S), dtype=torch.int32, device="cuda")
    best = torch.empty((n,), dtype=torch.int32, device="cuda")
    for k in args.topk:
        cs = torch.empty((n, k), dtype=torch.int32, device="cuda")
        csc = torch.empty((n, k), dtype=torch.int32, device="cuda")
        m = torch.empty((n, k, cap), dtype=torch.int32, device="cuda")
        d = torch.empty((n, k, cap), dtype=torch.float32, device="cuda")
        hm = torch.empty((n, k, 9), dtype=torch.float32, device="cuda")
        ni = torch.empty((n, k), dtype=torch.int32, device="cuda")
        mask = torch.empty((n, k, cap), dtype=torch.uint8, device="cuda")
        pick = torch.empty((n,), dtype=torch.int32, device="cuda")
        m1 = torch.empty((k, n, cap), dtype=torch.int32, device="cuda")
        d1 = torch.empty((k, n, cap), dtype=torch.float32, device="cuda")
        h1 = torch.empty((k, n, 9), dtype=torch.float32, device="cuda")
        n1 = torch.empty((k, n), dtype=torch.int32, device="cuda")
        k1 = torch.empty((k, n, cap), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def new():
            assert lib.fpc_match_bank_topk(ctx, n, k, 1, 0.7, 0.0, 0, score.data_ptr(), cs.data_ptr(), csc.data_ptr(),
                                           m.data_ptr(), d.data_ptr()) == 0
            assert lib.fpc_homography_bank_topk(ctx, n, k, cs.data_ptr(), m.data_ptr(), ctypes.byref(params), hm.data_ptr(),
                                                ni.data_ptr(), mask.data_ptr(), pick.data_ptr(), best.data_ptr()) == 0

        new()
        e.sync()
        cols = cs.t().contiguous()                      # the candidates of round j, as the loop's slot_dev
        torch.cuda.synchronize()

        def rounds():
            for j in range(k):
                assert lib.fpc_match_bank_guided(ctx, n, cols[j].data_ptr(), ident.data_ptr(), 1e4, 1, 0.7, 0.0,
                                                 m1[j].data_ptr(), d1[j].data_ptr()) == 0
                assert lib.fpc_homography_bank(ctx, n, cols[j].data_ptr(), m1[j].data_ptr(), ctypes.byref(params),
                                               h1[j].data_ptr(), n1[j].data_ptr(), k1[j].data_ptr()) == 0

        def loop():
            assert lib.fpc_match_bank(ctx, n, 1, 0.7, 0.0, 0, score.data_ptr(), best.data_ptr(), None, None) == 0
            rounds()

        t_new, t_loop, t_rounds = events_ms(e, st, new), events_ms(e, st, loop), events_ms(e, st, rounds)
        same = bool((h1.permute(1, 0, 2).view(torch.int32) == hm.view(torch.int32)).all()) and \
            bool((m1.permute(1, 0, 2) == m).all()) and bool((n1.t() == ni).all())
        print(json.dumps({"frames": n, "K": K, "slots": S, "format": args.format, "topk": k, "workspace_bytes": ws_bytes,
                          "new_ms": t_new, "loop_ms": t_loop, "loop_rounds_only_ms": t_rounds,
                          "loop_over_new": round(t_loop["median"] / t_new["median"], 2),
                          "not_slower": t_new["min"] <= t_loop["max"], "same_bits": same}), flush=True)
    e.bank_destroy()


for n in (1, 32):
    frames = torch.from_numpy(synth.make_batch(0, n, H, W)).cuda().contiguous()
    for K in ((1000, 2000) if args.topk else (500, 1000, 2000, 4500)):
        e = Engine(H, W, max_batch=n, conf_thresh=1e-6, max_keypoints=K)
        e.load_state_dict(sd)
        torch.cuda.synchronize()
        e.detect_async(frames, n)
        cnt = e.counts(n)[0]
        assert (cnt == K).all(), cnt
        lib, ctx, cap, dim = e._l, e._ctx, e.capacity, e.desc_dim
        st = e.torch_stream()
        for S in (16, 64):
            if args.topk:
                if S == 16:
                    topk_point(e, n, K, S)
                continue
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
