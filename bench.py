#!/usr/bin/env python3
"""Headline benchmark: VGA SuperPoint forward + NMS + descriptors, frames/s.

    python bench.py --gpus 1 --steps 100 --warmup 30      (the defaults: 0.4 s timed after 0.1 s of warm-up, so that the
                                                          clock has settled; any K / W works)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus N                              (no launcher: bench.py starts the N ranks itself, _self_launch)
    python bench.py --full                                (the headline and every figure listed below beside it)
    python bench.py --dump-outputs DIR                    (also writes what the last timed step returned, as .npy)

One "step" = one pass of the whole hot path (fpc_detect: network, exp-softmax,
depth-to-space, threshold, greedy NMS, sort, border crop, descriptor sampling) over
one batch of 32 synthetic 640x480 frames that is already resident in HBM
(BASELINE.json configs[1]).  With N ranks every rank runs its own 32-frame batch
(weak scaling; configs[2] = 256 frames over 8 GPUs); the only collective is the
start-up broadcast of the packed weights.  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line: `value`, `ms_per_step` and the cheap facts of
the set-up (`create`, `weights_broadcast_ms`, `keypoints_per_frame`, ...).  Its timed region carries no HIP events.

With --full the line also holds, from HIP events in the timed steps and passes of their own after
them:
  roofline          the dominant kernel symbol of the step against its roof, `frac` <= 1 by construction:
                    bound "mfma" (fp32 workloads): achieved = FLOPs the matrix cores EXECUTED per launch (padding
                    included, a Winograd 3x3 at its reduced count) / the launch's duration / the fp32 matrix peak.
                    The duration is the kernel's own: the one-stream pass inside this run (the kernel alone on the GPU;
                    HIP events on its stream -- where they and rocprofv3's AverageNs agree); what the events bracket
                    inside the timed region, where two contexts share the GPU, is kept as `in_timed_region`.
                    `frac_algorithmic` = the direct convolution's FLOPs priced the same way: it exceeds 1 by
                    design for the Winograd kernels (`algorithmic_ceiling`).
                    hd64-bf16: `frac_hbm` (HBM bytes BY THE PMC COUNTERS / duration / 8 TB/s) and `frac_mfma`; `bound` =
                    the larger.  `traffic` = those counter bytes per launch (profiles/*pmc_summary*.csv, looked up by
                    symbol and scaled to the launch's frames); null when no committed profile holds the symbol.
  whole_path        the whole step against both roofs (executed-MFMA FLOPs and counter bytes per step / ms_per_step).
  kernels_serial    every kernel symbol alone on the GPU: frac_mfma (<= 1), frac_algorithmic, frac_hbm.
  steady_state      the same loop run for >= 2 s right after the K timed steps (clock settled).
  latency_ms_b1     one frame, one call at a time (BASELINE.json configs[0]'s use case).
  cpu_baseline      SURVEY 8(d): the torch.nn.functional CPU restatement of the path (oracle/torch_cpu.py + the C
                    oracle's post-processing) on this host: the MEDIAN of three passes over 100 frames (min / max
                    beside it), one thread and batch 32 as side figures; bounded.
  also              single_context, latency_b1, host_fed, other_workloads, the other fp32 modes, layer_ms_*; the
                    --no-* options drop single passes of a --full run.

--dump-outputs DIR (rank 0): what Engine.detect would have returned for the timed path's last step -- per frame the
keypoints' (x, y), confidences, descriptors and candidate counts -- as float32 / float64 .npy files, at most 64 MB in
all (dump_outputs).  Frames and checkpoint are seeded: the same arguments give the same inputs on every run and build.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def _self_launch():
    """`python bench.py --gpus N` with N > 1 and no launcher around it (WORLD_SIZE unset): start the N ranks here.

    The parent has not imported torch or the HIP library yet and never touches the GPU: it starts N fresh children
    (`sys.executable bench.py <same arguments>` with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*; never os.exec*), lets
    them share its stdout (only rank 0 prints the JSON line), and exits with the first non-zero child status -- the
    remaining ranks are then terminated instead of waiting in a collective for the backend's time-out.  Under
    torch.distributed.run (WORLD_SIZE set) this function does nothing."""
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--gpus", type=int, default=1)
    n = pre.parse_known_args()[0].gpus
    if n <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    live = list(procs)
    while live and rc == 0:
        time.sleep(0.05)
        for p in list(live):
            c = p.poll()
            if c is not None:
                live.remove(p)
                rc = rc or c
    if rc != 0:
        sys.stderr.write("bench.py: a rank exited with status %d; stopping the other %d\n" % (rc, len(live)))
        for p in live:
            p.terminate()
        deadline = time.time() + 10.0
        for p in live:
            try:
                p.wait(max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                p.kill()
    sys.exit(rc if 0 <= rc < 256 else 1)


if __name__ == "__main__":
    _self_launch()
    # (HIP multiplexes streams onto 4 hardware queues by default, a new stream onto the least-used one.  More queues
    # (GPU_MAX_HW_QUEUES=5, 6, 8) were measured again in round 4, with the streams probed: the device-resident headline loses
    # 5 %, the host-fed legs 5-25 %.  Left at the default; what matters is WHICH streams share a queue -- fpc_create and
    # fpc_upload_stream see to that: csrc/queue_map.h.)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import fpc_amd  # noqa: E402,F401
from fpc_amd import arch, dist as fdist, synth  # noqa: E402
from fpc_amd.engine import Engine  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3    # MI355X_MICROARCH.md: FP32 matrix peak (dense, f32 in / f32 acc)
PEAK_BF16_MFMA_TFLOPS = 2516.8  # ibid.: BF16 MFMA dense = 16x the FP32 matrix rate (~2.5 PF)
PEAK_HBM_GBS = 8000.0           # ibid.: HBM3E 8.0 TB/s (spec; 6.3 TB/s measured with a float4 copy)
H, W, BATCH = 480, 640, 32


class Mode:
    """What bounds the selected workload and the peaks to price it against."""

    def __init__(self, dtype, workload):
        self.dtype = dtype
        self.bound = "hbm" if workload == "hd64-bf16" else "mfma"
        # ceiling for ALGORITHMIC flops (one product = 1 fp32 MFMA / 6 bf16 / 3 fp16 / 1 bf16 MFMA) and for issued MFMAs
        self.peak_algorithmic = {"f32": PEAK_F32_MFMA_TFLOPS, "f32_split": PEAK_BF16_MFMA_TFLOPS / 6.0,
                                 "f32_split_f16": PEAK_BF16_MFMA_TFLOPS / 3.0, "bf16": PEAK_BF16_MFMA_TFLOPS}[dtype]
        self.peak_issued = PEAK_F32_MFMA_TFLOPS if dtype == "f32" else PEAK_BF16_MFMA_TFLOPS


# ----------------------------------------------------------------------------------------------------------------
# measured HBM traffic: the newest committed PMC summary (profiles/*pmc_summary*.csv) that holds the symbol
# ----------------------------------------------------------------------------------------------------------------
def load_traffic_table(dtype):
    """kernel symbol (template arguments included, 'void ' and argument list stripped) ->
    (HBM bytes per FRAME, file).  Files are written by profiles/summarize_pmc.py from three rocprofv3 --pmc passes
    (FETCH_SIZE x 2 -- the gfx950 correction of MI355X_MICROARCH.md -- + WRITE_SIZE, KiB -> bytes)."""
    table = {}
    tag = {"f32": "", "bf16": "bf16", "f32_split": "f32_split", "f32_split_f16": "f32_split_f16"}[dtype]
    def age(f):
        # rNN[letter]_...: later rounds win; within a round the set WITHOUT a letter is the round's final one (letters are
        # intermediate builds kept for DESIGN.md's history: `r02o_` is older than `r02_`) and wins over every letter
        m = re.match(r"r(\d+)([a-z]*)_", os.path.basename(f))
        return (int(m.group(1)), m.group(2) == "", m.group(2)) if m else (-1, False, "")
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*pmc_summary*.csv")), key=age)
    for f in files:   # the newest profile that holds a symbol wins
        base = os.path.basename(f)
        is_mode = base.rsplit("pmc_summary", 1)[1].replace(".csv", "").replace("_serial", "").strip("_")
        if is_mode != tag and not (tag == "f32_split" and is_mode == "f32_split_f16"):   # the bf16-term twins move the same bytes
            continue
        try:
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    sym = row["kernel"].replace("void ", "").split("(")[0].replace("fpc::", "").strip()
                    frames = float(row.get("frames_per_dispatch") or 32)
                    if tag == "f32_split" and is_mode == "f32_split_f16":
                        sym = sym.replace("block_h2_kernel", "block_x3_kernel")
                    table[sym] = (float(row["hbm_bytes_per_dispatch"]) / frames, "profiles/" + base, age(f))
        except (OSError, KeyError, ValueError):
            continue
    return table


def lookup_traffic(table, sym):
    """Exact symbol, or the same kernel name where one side carries no template arguments (the engine reports
    `stem_pool_kernel`, rocprofv3 `stem_pool_kernel<3>`); among several candidates the newest profile wins."""
    cands = [(v[2], k == sym, v) for k, v in table.items()
             if k == sym or (k.split("<")[0] == sym.split("<")[0] and ("<" not in sym or "<" not in k))]
    return max(cands)[2][:2] if cands else None


# ----------------------------------------------------------------------------------------------------------------
# CPU baseline
# ----------------------------------------------------------------------------------------------------------------
def cpu_core_budget():
    """The host cores this process is entitled to: min(scheduler affinity, cgroup CPU quota, 64) -- the same rule on
    every box.  (A GPU box reports 128-256 hardware threads but the container's quota is a fraction of them, and
    eager torch with more threads than CPUs runs several times SLOWER than with one.)"""
    n = len(os.sched_getaffinity(0))
    for path in ("/sys/fs/cgroup/cpu.max", ):
        try:
            quota, period = open(path).read().split()
            if quota != "max":
                n = min(n, max(1, int(int(quota) / int(period))))
        except (OSError, ValueError):
            pass
    try:   # cgroup v1
        q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0 and per > 0:
            n = min(n, max(1, q // per))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 64))


def cpu_baseline(state_dict, frames, budget_s=22.0, descriptor=True):
    """The path on this host's cores: forward = oracle/torch_cpu.py (torch.nn.functional, eager, fp32: what the
    reference's CPU path is), post-processing = the C oracle's get_points + get_descriptors (nms.py's Python loops
    restated in C -- faster than the reference's, so the figure errs in the baseline's favour).  All cores and ONE
    thread; batch 1 (the reference's facade) and batch 32 forward; bounded by `budget_s` of CPU time in total.

    `cores` = n = cpu_core_budget() threads; {n, n/2, n/4} are probed (median of three forwards after a warm-up one, a
    candidate whose warm-up forward takes over a second is dropped there and then) and reported as `thread_probe_ms`
    (round 2 probed up to 256 threads without a bound -- 43 s of a 65 s run -- and took the winner, which flipped
    between boxes)."""
    from oracle import oracle, torch_cpu
    sd = torch_cpu.to_torch(state_dict)
    x = torch.from_numpy(np.ascontiguousarray(frames))
    n = x.shape[0]
    h, w = x.shape[2], x.shape[3]
    t_start = time.perf_counter()
    ncap = cpu_core_budget()
    probe = {}
    for th in sorted({ncap, max(1, ncap // 2), max(1, ncap // 4)}, reverse=True):
        torch.set_num_threads(th)
        t0 = time.perf_counter()
        torch_cpu.forward(x[:1], sd, descriptor)
        if time.perf_counter() - t0 > 1.0 and probe:      # (the first candidate is kept whatever it costs: one is needed)
            continue
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            torch_cpu.forward(x[:1], sd, descriptor)
            ts.append(time.perf_counter() - t0)
        probe[th] = float(np.median(ts))
    # `cores` is the core budget itself -- the same rule on every box.  (Picking the fastest probe flipped between 8 and
    # 16 threads from one box to the next on timings 5 % apart; the probe stays in the line as information.)
    all_threads = ncap if ncap in probe else min(probe, key=probe.get)

    def run(threads, warm, want, share):
        """batch-1 loop: returns (frames, forward seconds, post-processing seconds)."""
        torch.set_num_threads(threads)
        oracle.set_threads(threads)
        for i in range(warm):
            torch_cpu.forward(x[i % n:i % n + 1], sd, descriptor)
        tf = tp = 0.0
        k = 0
        deadline = time.perf_counter() + share
        while k < want and (k < 3 or time.perf_counter() < deadline):
            i = k % n
            t0 = time.perf_counter()
            prob, desc, _ = torch_cpu.forward(x[i:i + 1], sd, descriptor)
            t1 = time.perf_counter()
            xs, ys, _, _ = oracle.get_points(prob[0].numpy())
            if descriptor:
                oracle.get_descriptors(desc[0].numpy(), xs, ys, h, w)
            t2 = time.perf_counter()
            tf += t1 - t0
            tp += t2 - t1
            k += 1
        return k, tf, tp

    # 8(d): warm-up, then THREE passes of up to 100 timed iterations each (time-bounded); `value` is the median pass,
    # min / max are reported (round 3 reported one pass: 47 frames/s on one box, 67 on the next)
    passes = []
    for pi_ in range(3):
        passes.append(run(all_threads, 5 if pi_ == 0 else 1, 100, budget_s * 0.2))
    rates = sorted(k_ / (f_ + p_) for k_, f_, p_ in passes)
    ka, fa, pa = sorted(passes, key=lambda t: t[0] / (t[1] + t[2]))[1]
    torch.set_num_threads(all_threads)
    nb = min(n, 32)
    torch_cpu.forward(x[:nb], sd, descriptor)
    t0 = time.perf_counter()
    reps = 0
    while reps < 1 or (reps < 10 and time.perf_counter() - t0 < budget_s * 0.1):
        torch_cpu.forward(x[:nb], sd, descriptor)
        reps += 1
    fb = (time.perf_counter() - t0) / reps
    k1, f1, p1 = run(1, 1, 12, budget_s * 0.15)
    torch.set_num_threads(all_threads)
    oracle.set_threads(oracle.max_threads())
    spent = time.perf_counter() - t_start
    r3 = lambda v: round(v, 3)   # noqa: E731
    return {"value": r3(rates[1]), "unit": "frames/s", "cores": all_threads, "kind": "port",
            "passes": 3, "min": r3(rates[0]), "max": r3(rates[2]), "spread": r3((rates[2] - rates[0]) / rates[1]),
            "sample": "median of 3 passes, each %d of the bench's %dx%d frames one at a time (5 warm-up frames before the first): "
                      "forward by the torch.nn.functional restatement oracle/torch_cpu.py (eager fp32, %d threads) + "
                      "post-processing (get_points + get_descriptors) by the C oracle; %.1f s of CPU work in all legs"
                      % (ka, w, h, all_threads, spent),
            "core_budget": ncap, "thread_probe_ms": {str(k): r3(v * 1e3) for k, v in sorted(probe.items())},
            "note": "the GPU boxes give a container a CPU quota (16) out of 256 shared logical CPUs: the multi-thread figure "
                    "moves 3-5 % inside a run (min / max) and 33-66 frames/s from box to box; `single_thread` is the stable "
                    "one (10.3-10.5 frames/s on every box measured)",
            "forward_ms": r3(fa / ka * 1e3), "postproc_ms": r3(pa / ka * 1e3),
            "forward_only_frames_per_s": r3(ka / fa),
            "batch%d_forward_frames_per_s" % nb: r3(nb / fb),
            "single_thread": {"value": r3(k1 / (f1 + p1)), "frames": k1, "forward_ms": r3(f1 / k1 * 1e3),
                              "postproc_ms": r3(p1 / k1 * 1e3)}}


def cpu_baseline_vgg_reference(sd, frames):
    """kind "reference": the reference's own cpp/src/model.cc (oracle/_ref/ref_vgg_forward, built by
    oracle/Makefile.ref) timed on this host's cores -- the forward pass only, which is all of cpp/ that can be built."""
    import importlib.util
    path = os.path.join(ROOT, "tests", "golden", "make_golden_vgg.py")
    spec = importlib.util.spec_from_file_location("make_golden_vgg", path)
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    if not os.path.exists(mg.BIN):
        return None
    n, reps = frames.shape[0], 3
    _, _, err = mg.run_reference(sd, frames, repeats=reps)
    kv = dict(ln.split() for ln in err.strip().splitlines() if len(ln.split()) == 2)
    sec = float(kv["forward_seconds"])
    return {"value": round(n / sec, 3), "unit": "frames/s", "cores": int(kv.get("threads", 0)), "kind": "reference",
            "sample": "%d of the bench's %dx%d gray frames, SPModel::forward only (cpp/src/model.cc compiled unmodified "
                      "with libtorch CPU, %d runs of %.2f s); the rest of cpp/ needs TRTorch/OpenCV" % (n, W, H, reps, sec)}


def host_fed_rates(sd, frames_np, local, dtype, steps=36):
    """H2D-inclusive rates (the second figure, never `value`): every step uploads its batch from pinned host
    memory and runs the path.  (a) the reference's input, fp32 RGB [n,3,H,W]; (b) 8-bit RGB HWC frames converted on
    the device (fpc_detect_u8).

    The pipeline a serving loop would run: ONE dedicated copy stream (its uploads never queue behind a compute launch),
    THREE device buffers, two contexts in turn, each computing a whole batch on one stream.  Events do the hand-offs:
    a context waits for `uploaded[b]`, the copy stream waits for `consumed[b]` before it overwrites buffer b.
    (Round 2 uploaded on the context's own stream: a context's copy never overlapped its own compute, and with
    2 x 4 streams on 4 hardware queues uploads also queued behind the other context's launches: 6.3 GB/s of a link that
    does 25, 77 % of the device-resident rate.)"""
    dev = torch.device("cuda", local)
    res = {}
    u8 = np.clip(np.rint(frames_np.transpose(0, 2, 3, 1) * 255.0), 0, 255).astype(np.uint8)
    nbuf = 3
    for tag, host in (("f32_rgb_nchw", torch.from_numpy(frames_np).pin_memory()),
                      ("u8_rgb_hwc", torch.from_numpy(np.ascontiguousarray(u8)).pin_memory())):
        # The loop's three streams -- two contexts, one upload -- sit on three different hardware queues because the LIBRARY
        # places them (csrc/queue_map.h): a context's main stream avoids the queues of the other live contexts' main
        # streams, and fpc_upload_stream hands out a stream beside both.  (Round 4 picked torch streams here with a
        # host-clock probe of its own; with torch's pooled streams as they come, which stream shared a queue with which
        # was the process's history: fp32 frames read 69 % of the device-resident rate and 8-bit ones 95 %, and after an
        # unrelated change the other way round.)  NMS in line: a context is ONE stream then, and nothing of it is left
        # to land on the upload stream's queue.
        ctxs = []
        for _ in range(2):
            e = Engine(H, W, max_batch=BATCH, device=local, dtype=dtype, num_streams=1, plan_flags=["nms_in_line"])
            e.load_state_dict(sd)
            ctxs.append((e.torch_stream(), e))
        copy_stream = ctxs[0][1].upload_stream()
        placement = [e.stream_report()["streams"] for _, e in ctxs]
        bufs = [torch.empty_like(host, device=dev) for _ in range(nbuf)]
        uploaded = [torch.cuda.Event() for _ in range(nbuf)]
        consumed = [torch.cuda.Event() for _ in range(nbuf)]

        def step(i):
            b = i % nbuf
            st, e = ctxs[i % 2]
            with torch.cuda.stream(copy_stream):
                if i >= nbuf:
                    copy_stream.wait_event(consumed[b])
                bufs[b].copy_(host, non_blocking=True)
                uploaded[b].record(copy_stream)
            with torch.cuda.stream(st):
                st.wait_event(uploaded[b])
                if tag == "u8_rgb_hwc":
                    e.detect_u8_async(bufs[b], BATCH, "rgb_hwc")
                else:
                    e.detect_async(bufs[b], BATCH)
                consumed[b].record(st)
        attempts = 0
        while True:
            attempts += 1
            for i in range(6):
                step(i)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(6, 6 + steps):
                step(i)
            torch.cuda.synchronize(dev)
            dt = time.perf_counter() - t0
            # the link alone: the same uploads with nothing else on the GPU
            t1 = time.perf_counter()
            with torch.cuda.stream(copy_stream):
                for i in range(8):
                    bufs[i % nbuf].copy_(host, non_blocking=True)
            torch.cuda.synchronize(dev)
            dc = (time.perf_counter() - t1) / 8
            # the contexts alone: the same calls on resident buffers
            t1 = time.perf_counter()
            for i in range(8):
                st, e = ctxs[i % 2]
                with torch.cuda.stream(st):
                    (e.detect_u8_async(bufs[i % nbuf], BATCH, "rgb_hwc") if tag == "u8_rgb_hwc" else e.detect_async(bufs[i % nbuf], BATCH))
            torch.cuda.synchronize(dev)
            dk = (time.perf_counter() - t1) / 8
            # A step that costs compute + more than half an upload has its uploads in a row with a context's launches (round 4:
            # one run in five of the full default run).  Said, not hidden: the leg is repeated, `attempts` reported.
            if dt / steps < dk + 0.5 * dc or attempts >= 3:
                break
        nbytes = host.numel() * host.element_size()
        res[tag] = {"value": round(BATCH * steps / dt, 2), "unit": "frames/s", "steps": steps, "attempts": attempts,
                    "stream_queues": placement,
                    "compute_alone_ms_per_batch": round(dk * 1e3, 3),
                    "h2d_bytes_per_frame": int(host[0].numel() * host.element_size()),
                    "h2d_gbytes_per_s": round(nbytes * steps / dt / 1e9, 2),
                    "upload_alone_ms_per_batch": round(dc * 1e3, 3), "link_gbytes_per_s_alone": round(nbytes / dc / 1e9, 2),
                    "ms_per_step": round(dt / steps * 1e3, 4)}
        for _, e in ctxs:
            e.close()
        del bufs
    return res


def symbol_stats(timings, steps):
    """kernel symbol -> dict(mean launch ms, algorithmic / MFMA-issued FLOPs and algorithmic bytes per launch, ...)."""
    by, layers = {}, {}
    for name, kern, ms, fl, mf, nbytes in timings:
        by.setdefault(kern, []).append((ms, fl, mf, nbytes))
        layers.setdefault(kern, set()).add(name)
    out = {}
    for k, v in by.items():
        out[k] = {"avg_launch_ms": float(np.mean([r[0] for r in v])), "flops": float(np.mean([r[1] for r in v])),
                  "mfma_flops": float(np.mean([r[2] for r in v])), "bytes": float(np.mean([r[3] for r in v])),
                  "launches_per_step": len(v) // max(1, steps), "layers": len(layers[k]),
                  "total_ms": float(np.sum([r[0] for r in v])) / max(1, steps)}
    return out


def roofline_entry(mode, sym, st, step_ms, traffic_table, batch=None, duration_source=""):
    """One kernel symbol against its roof.  `frac` is a fraction of a ROOF and therefore <= 1:

    bound "mfma":  achieved = FLOPs the matrix cores EXECUTED for one launch (MFMA instructions x their FLOPs: tile and
                   channel padding included, a Winograd 3x3 at 16/36 or 36/144 of the direct convolution's count) / the
                   launch's duration / the dense MFMA peak of the dtype.  `frac_algorithmic` beside it prices the
                   direct-convolution FLOPs of SURVEY 8(d) the same way and EXCEEDS 1 BY DESIGN for the Winograd kernels
                   (`algorithmic_ceiling` = algorithmic / executed FLOPs says how far it may go).
    bound "hbm":   achieved = HBM bytes of one launch BY THE PMC COUNTERS (profiles/*pmc_summary*.csv: 2 x FETCH_SIZE +
                   WRITE_SIZE, per frame x the launch's frames) / duration / 8 TB/s.
    For hd64-bf16 both fractions are reported (`frac_hbm`, `frac_mfma`) and `bound` names the larger one.
    `duration_source` says which clock `avg_launch_ms` is (the kernel alone on the GPU, or inside the timed region)."""
    sec = st["avg_launch_ms"] * 1e-3
    frames = (batch or BATCH) * st["layers"] / max(1, st["launches_per_step"])      # frames one launch covers (a sub-batch)
    alg_tf = st["flops"] / sec / 1e12
    exe_tf = st["mfma_flops"] / sec / 1e12
    tr = lookup_traffic(traffic_table, sym)
    traffic = tr[0] * frames if tr else None
    frac_mfma = exe_tf / mode.peak_issued
    frac_hbm = (traffic / sec / 1e9 / PEAK_HBM_GBS) if traffic else None
    e = {"kernel": sym}
    bound = mode.bound
    if mode.bound == "hbm":     # the configuration SURVEY 8(d) calls HBM-bound: whichever roof the kernel is closer to
        bound = "hbm" if (frac_hbm is not None and frac_hbm >= frac_mfma) else "mfma"
    if bound == "hbm":
        e.update(bound="hbm", achieved=round(traffic / sec / 1e9, 1), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(frac_hbm, 4))
    else:
        e.update(bound="mfma", achieved=round(exe_tf, 3), peak=mode.peak_issued, unit="TFLOP/s", frac=round(frac_mfma, 4))
    e["traffic"] = round(traffic) if traffic else None
    e["traffic_source"] = tr[1] if tr else None
    e.update(
        duration_source=duration_source,
        avg_launch_ms=round(st["avg_launch_ms"], 4), frames_per_launch=frames,
        frac_mfma=round(frac_mfma, 4), frac_hbm=round(frac_hbm, 4) if frac_hbm is not None else None,
        executed_mfma_flops_per_launch=st["mfma_flops"],
        # the direct-convolution count of SURVEY 8(d) (what the reference's library computes): may exceed the roof
        algorithmic_flops_per_launch=st["flops"], achieved_algorithmic=round(alg_tf, 3),
        frac_algorithmic=round(alg_tf / mode.peak_algorithmic, 4),
        frac_algorithmic_note="direct-convolution FLOPs / duration / peak: exceeds 1 by design where the 3x3 runs as Winograd",
        algorithmic_ceiling=round(st["flops"] / st["mfma_flops"] * mode.peak_issued / mode.peak_algorithmic, 3) if st["mfma_flops"] else None,
        algorithmic_bytes_per_launch=st["bytes"],
        traffic_over_algorithmic_bytes=round(traffic / st["bytes"], 3) if (traffic and st["bytes"]) else None,
        launches_per_step=st["launches_per_step"], share_of_step=round(st["total_ms"] / step_ms, 3))
    return e


def side_workload(name, sd, local, budget_s=4.0):
    """BASELINE.json configs[3] / configs[4] inside the default run, so that the driver's clock brackets them too:
    a bounded pass (a few warm-up steps, then timed steps for about budget_s / 2 seconds, HIP events on) of
    `qvga32-magicpoint` (32 x 240x320, detector only, fp32) or `hd64-bf16` (64 x 1280x960, bf16).  Same synthetic
    frames and checkpoint recipe as `--workload <name>`; `value` of the line stays configs[1]."""
    if name == "hd64-bf16":
        h, w, batch, dtype, desc = 960, 1280, 64, "bf16", True
    else:
        h, w, batch, dtype, desc = 240, 320, 32, "f32", False
    mode = Mode(dtype, name)
    dev = torch.device("cuda", local)
    e = Engine(h, w, max_batch=batch, device=local, dtype=dtype, descriptor_enabled=desc)
    e.load_state_dict(sd)
    nbase = batch if h * w <= 480 * 640 else 8
    fr = synth.make_batch(100, nbase, h, w)
    if nbase < batch:
        fr = np.concatenate([np.roll(fr, 16 * k, axis=3) for k in range(batch // nbase)], 0)
    frames = torch.from_numpy(fr).to(dev)
    del fr
    for _ in range(3):
        e.detect_async(frames, batch)
    e.sync()
    t0 = time.perf_counter()
    for _ in range(3):
        e.detect_async(frames, batch)
    e.sync()
    per = (time.perf_counter() - t0) / 3
    # (as the headline's `warmup_extra_steps`: keep warming, untimed, until 0.4 s have passed -- six steps end before the
    # clock has settled and the bounded pass then reads 3 % under the same workload's own run)
    tw = time.perf_counter()
    while time.perf_counter() - tw < 0.4:
        for _ in range(4):
            e.detect_async(frames, batch)
        e.sync()
    cnt, ncand = e.counts(batch)
    k = int(min(200, max(5, budget_s * 0.5 / max(per, 1e-6))))
    every = 4                  # (events on one call in four, as in the headline's timed region: on every call they are 7 % of
    e.set_timing(every)        # this pass's frame rate at QVGA -- 49 400 against 52 800 frames/s -- and 0.5 % at HD)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(k):
        e.detect_async(frames, batch)
    e.sync()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    tim = e.timings()
    e.set_timing(False)
    e.close()
    step_ms = dt / k * 1e3
    stats = symbol_stats(tim, len(range(0, k, every)))
    # the same kernels alone on the GPU (one stream), a few steps: the durations the roofline fractions are priced on
    e1 = Engine(h, w, max_batch=batch, device=local, dtype=dtype, descriptor_enabled=desc, num_streams=1, plan_flags=["nms_in_line"])
    e1.load_state_dict(sd)
    for _ in range(2):
        e1.detect_async(frames, batch)
    e1.sync()
    e1.set_timing(True)
    ks = 5
    t1 = time.perf_counter()
    for _ in range(ks):
        e1.detect_async(frames, batch)
    e1.sync()
    serial_ms = (time.perf_counter() - t1) / ks * 1e3
    sstats = symbol_stats(e1.timings(), ks)
    e1.close()
    del frames
    torch.cuda.empty_cache()
    key = "bytes" if mode.bound == "hbm" else "flops"
    sym = max((s_ for s_ in sstats if sstats[s_][key] > 0), key=lambda s_: sstats[s_]["total_ms"])
    table = load_traffic_table(dtype) if mode.bound == "hbm" else {}      # (the committed PMC summaries are VGA fp32 and HD bf16)
    roof = roofline_entry(mode, sym, sstats[sym], serial_ms, table, batch,
                          "HIP events on the launch stream, one stream: the kernel alone on the GPU (%d steps)" % ks)
    if sym in stats:
        roof["in_timed_region"] = {"avg_launch_ms": round(stats[sym]["avg_launch_ms"], 4),
                                   "note": "streams share the GPU here: a launch's bracket includes the time it shares"}
    out = {"value": round(batch * k / dt, 2), "unit": "frames/s", "steps": k, "warmup": 6, "ms_per_step": round(step_ms, 4),
           "ms_per_step_one_stream": round(serial_ms, 4),
           "frames_per_step": batch, "height": h, "width": w, "dtype": dtype,
           "keypoints_per_frame": round(float(np.mean(cnt)), 1), "candidates_per_frame": round(float(np.mean(ncand)), 1),
           "roofline": roof}
    out["whole_path"] = whole_path_fractions(mode, tim, len(range(0, k, every)), step_ms, batch, table)
    return out


def whole_path_fractions(mode, timings, steps, step_ms, batch, table):
    """The whole step against both roofs: executed-MFMA FLOPs and HBM bytes per step / ms_per_step.  HBM bytes: by the
    PMC counters where a committed summary holds every kernel symbol of the step (`hbm_bytes_source` "pmc"), else the
    algorithmic bytes (every launch's input read once + output written once)."""
    sec = step_ms * 1e-3
    exe = sum(t[4] for t in timings) / steps
    alg = sum(t[3] for t in timings) / steps
    alg_bytes = sum(t[5] for t in timings) / steps
    syms = {}
    for name, kern, ms, fl, mf, nb in timings:
        syms.setdefault(kern, set()).add(name)
    launches = {}
    for name, kern, ms, fl, mf, nb in timings:
        launches[kern] = launches.get(kern, 0) + 1
    pmc_bytes, missing = 0.0, []
    for kern in syms:
        parts = kern.split("+") if "+" in kern else [kern]      # (the NMS launches are reported as one joined symbol)
        got = [lookup_traffic(table, p_) for p_ in parts]
        if any(g is None for g in got):
            missing.append(kern)
            continue
        # bytes per frame of the symbol (all its launches of a step summed by the profile's per-dispatch mean x dispatches
        # per step): the table holds bytes per FRAME and per DISPATCH, so x frames x layers of that symbol
        pmc_bytes += sum(g[0] for g in got) * batch * len(syms[kern])
    r = {"executed_mfma_tflops": round(exe / sec / 1e12, 3), "frac_mfma": round(exe / sec / 1e12 / mode.peak_issued, 4),
         "algorithmic_tflops": round(alg / sec / 1e12, 3),
         "algorithmic_bytes_per_frame": round(alg_bytes / batch)}
    if not missing and pmc_bytes > 0:
        r.update(hbm_bytes_source="pmc", hbm_bytes_per_frame=round(pmc_bytes / batch),
                 hbm_gbytes_per_s=round(pmc_bytes / sec / 1e9, 1), frac_hbm=round(pmc_bytes / sec / 1e9 / PEAK_HBM_GBS, 4))
    else:
        r.update(hbm_bytes_source="algorithmic (no committed PMC summary holds: %s)" % ", ".join(missing[:3]),
                 hbm_gbytes_per_s=round(alg_bytes / sec / 1e9, 1), frac_hbm=round(alg_bytes / sec / 1e9 / PEAK_HBM_GBS, 4))
    r["bound"] = "hbm" if r["frac_hbm"] >= r["frac_mfma"] else "mfma"
    return r


def aggregate_over_ranks(world, my_dt, dt, bcast_ms, steps, batch):
    """The contract's timing rule: `dt` = MAX over ranks of the barrier-to-barrier time of the K steps; `value` = frames of
    ALL ranks / that time.  Also gathers every rank's own rate and start-up time (`per_rank`).  One place, so that the
    gloo rehearsal (FPC_BENCH_RENDEZVOUS_ONLY, tests/test_dist_gloo.py) runs the very code an 8-GPU lease will run."""
    dt = fdist.max_over_ranks(dt)
    per_rank = None
    if world > 1:
        import torch.distributed as tdist
        coll_dev = "cuda" if tdist.get_backend() == "nccl" else "cpu"
        mine = torch.tensor([batch * steps / my_dt, bcast_ms], dtype=torch.float64, device=coll_dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        tdist.all_gather(allr, mine)
        per_rank = [[round(float(v), 2) for v in r.cpu()] for r in allr]
    value = batch * steps * world / dt
    return dt, value, per_rank


def rank_frame_seed(rank, batch):
    """First seed of a rank's synthetic frames: 100 + batch * rank (seeds 100..355 over 8 GPUs)."""
    return 100 + batch * rank


def bind_cpu_threads(world):
    """N ranks on one node share the host: each takes cores // N threads for its host-side work (frame synthesis, the
    host-fed legs, torch's intra-op pool), so 8 ranks do not oversubscribe the box.  Returns the thread count."""
    n = max(1, cpu_core_budget() // max(1, world))
    torch.set_num_threads(n)
    return n


DUMP_BYTES = 64 << 20
DUMP_DESC_ROWS = 32768      # a seeded sample of the descriptor rows: all of them are 65 MB for 32 VGA frames


def dump_outputs(path, eng, n):
    """--dump-outputs: the last step's results as a caller of the path receives them (Engine.fetch, which is what
    Engine.detect returns), the frames' keypoints concatenated in frame order:
      keypoints_per_frame [n], candidates_per_frame [n]     float32
      keypoints_xy [K,2] (x, y pixels), keypoints_conf [K]  float32
      descriptor_rows [S]                                   float64: the rows of `descriptors`, sorted; all K when
                                                            K <= DUMP_DESC_ROWS, else a sample drawn with seed 0
      descriptors [S,D]                                     float32 (not written when the descriptor head is off)"""
    res = eng.fetch(n)
    out = {"keypoints_per_frame": np.array([len(r[1]) for r in res], np.float32),
           "candidates_per_frame": np.array([r[3] for r in res], np.float32),
           "keypoints_xy": np.concatenate([r[0] for r in res]).astype(np.float32),
           "keypoints_conf": np.concatenate([r[1] for r in res]).astype(np.float32)}
    if res[0][2] is not None:
        desc = np.concatenate([r[2] for r in res])
        k = desc.shape[0]
        rows = np.arange(k) if k <= DUMP_DESC_ROWS else np.sort(np.random.default_rng(0).choice(k, DUMP_DESC_ROWS, replace=False))
        out["descriptor_rows"] = rows.astype(np.float64)
        out["descriptors"] = np.ascontiguousarray(desc[rows], np.float32)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_BYTES:
        raise SystemExit("--dump-outputs: %d bytes exceed the %d-byte budget" % (total, DUMP_BYTES))
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--contexts", type=int, default=int(os.environ.get("FPC_BENCH_CONTEXTS", "0")),
                    help="fpc contexts used round-robin (double buffering: batch k+1 starts while batch k drains).  Default "
                         "(0): 2 for the fp32 VGA workload, each running its batch as ONE sub-batch -- a 32-frame launch of "
                         "the F(4x4,3x3) blocks is 640 tiles = 2.5 rounds of the 256 CUs, which only a second independent "
                         "batch can fill -- and 1 elsewhere.  `single_context` in the line is the same loop on one context.")
    ap.add_argument("--gray", action="store_true",
                    help="feed gray frames [n,1,H,W] (in_channels=1: stem filters summed over the input channels); "
                         "default is the reference network's 3-channel input")
    ap.add_argument("--no-serial-pass", action="store_true", help="skip the extra one-stream pass that gives clean per-kernel durations")
    ap.add_argument("--no-timing-events", action="store_true",
                    help="do not bracket launches with HIP events (roofline then comes from a separate pass)")
    ap.add_argument("--workload", choices=["vga32", "hd64-bf16", "qvga32-magicpoint"], default="vga32",
                    help="vga32 = BASELINE.json configs[1] (the headline; default); hd64-bf16 = configs[4]: 64 frames of "
                         "1280x960 per step, bf16 activations / weights with fp32 accumulation")
    ap.add_argument("--dtype", choices=["f32", "f32_split", "f32_split_f16"], default="f32",
                    help="vga32 only. f32 (default): fp32 MFMA (v_mfma_f32_32x32x2_f32, Winograd where it pays). "
                         "f32_split: fp32 tensors, every product as six bf16 MFMAs on exactly split operands "
                         "(block_x3.h) -- same 1e-4 parity bar, reported beside the headline as `split_operand_mode`. "
                         "f32_split_f16: the same with two fp16 terms per operand and three MFMAs per product")
    ap.add_argument("--arch", choices=["resnet", "vgg"], default="resnet",
                    help="resnet (default): the Python network of BASELINE.json's configs. vgg: the cpp/ frontend's "
                         "superpoint::SPModel (SURVEY 8f rank 4), gray frames, 52 GFLOP per VGA frame")
    ap.add_argument("--no-host-fed", action="store_true", help="skip the host-fed (H2D-inclusive) passes")
    ap.add_argument("--no-alt-pass", action="store_true", help="skip the extra passes in the other fp32 arithmetic modes")
    ap.add_argument("--no-steady-state", action="store_true", help="skip the >= 2 s steady-state pass")
    ap.add_argument("--no-latency", action="store_true", help="skip the single-frame latency pass")
    ap.add_argument("--only-timed", action="store_true", help="the timed region and nothing else (profiling runs)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="skip the bounded passes of BASELINE.json configs[3] / configs[4] reported beside the headline")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beside the headline (HIP events in the timed region, roofline, steady state, "
                         "one context, latency, the other fp32 modes, configs[3] / configs[4], host-fed rates, CPU "
                         "baseline); without it a run sets up, warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what their last step returned (rank 0's batch) to DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        args.no_cpu_baseline = args.no_serial_pass = args.no_host_fed = args.no_alt_pass = True
        args.no_steady_state = args.no_latency = args.no_other_workloads = args.no_timing_events = True
    if args.only_timed:
        args.no_cpu_baseline = args.no_serial_pass = args.no_host_fed = args.no_alt_pass = True
        args.no_steady_state = args.no_latency = args.no_other_workloads = True
    global H, W, BATCH
    dtype = args.dtype
    magic = args.workload == "qvga32-magicpoint"   # configs[3]: detector only, 240x320, NMS r = 4
    if magic:
        H, W = 240, 320
        args.no_host_fed = True
    if args.workload == "hd64-bf16":
        H, W, BATCH, dtype = 960, 1280, 64, "bf16"
        args.no_host_fed = True
    mode = Mode(dtype, args.workload)
    auto_ctx = args.contexts <= 0
    if auto_ctx:
        args.contexts = 2 if (args.workload == "vga32" and dtype == "f32" and args.arch == "resnet") else 1

    rank, world, local = fdist.init_from_env()
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    host_threads = bind_cpu_threads(world)
    if os.environ.get("FPC_BENCH_RENDEZVOUS_ONLY") == "1":
        # test hook (tests/test_dist_gloo.py): the launch + rendezvous + timing reduction of the N > 1 path without a
        # GPU.  FPC_BENCH_FAKE_STEP_MS="3.0,3.5,..." gives every rank a pretended time per step; the reduction below is
        # aggregate_over_ranks -- the function the real run calls.
        import torch.distributed as tdist
        mine = torch.tensor([rank], dtype=torch.int64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            tdist.all_gather(allr, mine)
            fdist.barrier()
        # what every rank of the real run derives from its rank: its frames' first seed (seeds
        # 100 .. 355 over 8 GPUs = 100 + 32 * rank) and, for a caller that shards ONE batch of 32 * world frames instead
        # (configs[2]: 256 frames on 8 GPUs), its contiguous shard -- gathered in rank order
        lo, hi = fdist.shard_range(BATCH * world, world, rank)
        facts = torch.tensor([rank, rank_frame_seed(rank, BATCH), lo, hi, host_threads], dtype=torch.int64)
        allf = [torch.zeros_like(facts) for _ in range(world)]
        if world > 1:
            tdist.all_gather(allf, facts)
        else:
            allf = [facts]
        rec = {"rendezvous": "ok", "world": world, "ranks": [int(t.item()) for t in allr] if world > 1 else [0],
               "backend": tdist.get_backend() if world > 1 else None, "host_threads_per_rank": host_threads,
               "frame_seed0": [int(f[1]) for f in allf], "shards": [[int(f[2]), int(f[3])] for f in allf],
               "host_threads": [int(f[4]) for f in allf]}
        fake = os.environ.get("FPC_BENCH_FAKE_STEP_MS")
        if fake:
            ms = [float(v) for v in fake.split(",")]
            my_dt = ms[rank % len(ms)] * 1e-3 * args.steps
            dt, value, per_rank = aggregate_over_ranks(world, my_dt, my_dt, 10.0 + rank, args.steps, BATCH)
            rec.update(value=round(value, 2), ms_per_step=round(dt / args.steps * 1e3, 4), n_gpus=world, steps=args.steps,
                       per_rank={"frames_per_s": [r[0] for r in per_rank], "weights_start_up_ms": [r[1] for r in per_rank]} if per_rank else None)
        if rank == 0:
            print(json.dumps(rec))
        if world > 1:
            tdist.destroy_process_group()
        return
    local = local % max(1, torch.cuda.device_count())   # (a gloo rehearsal may put several ranks on one GPU)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    # synthetic checkpoint in the reference's layout; rank 0 packs and broadcasts it
    vgg = args.arch == "vgg"
    if vgg:
        args.gray, args.no_host_fed, args.no_alt_pass = True, True, True
    sd = (synth.make_vgg_state_dict(0, dustbin_bias=5.5) if vgg else synth.make_state_dict(0, dustbin_bias=7.0)) if rank == 0 else None
    cin = 1 if args.gray else 3
    kw = dict(device=local, in_channels=cin, dtype=dtype, arch=args.arch, descriptor_enabled=not magic)
    kw1 = dict(kw)                       # a context on its own: the library's default plan (two sub-batches on two streams)
    if args.contexts > 1 and "FPC_STREAMS" not in os.environ:
        kw["num_streams"] = 1            # contexts in turn: each runs its whole batch as one sub-batch
    tc0 = time.perf_counter()
    eng = Engine(H, W, max_batch=BATCH, **kw)
    first_create_ms = (time.perf_counter() - tc0) * 1e3   # the process's first fpc_create: code object load, anchor search, workspace
    fdist.barrier()
    tb0 = time.perf_counter()
    fdist.broadcast_packed_weights(eng, sd)
    torch.cuda.synchronize(dev)
    bcast_ms = (time.perf_counter() - tb0) * 1e3      # rank 0: parse + pack + broadcast; others: wait + receive + import
    engs = [eng]
    create_ms = None
    for _ in range(1, max(1, args.contexts)):
        tc0 = time.perf_counter()
        e2 = Engine(H, W, max_batch=BATCH, **kw)
        create_ms = (time.perf_counter() - tc0) * 1e3       # a later fpc_create: stream placement + workspace only
        e2.import_packed_device(eng.packed_view())          # device to device
        engs.append(e2)
    stream_reports = [e_.stream_report() for e_ in engs]
    # this rank's frames: seeds 100 + 32*rank ... (configs[2]: seeds 100..355 over 8 GPUs)
    nbase = BATCH if H * W <= 480 * 640 else 8      # HD: 8 distinct frames, shifted copies fill the batch
    frames_np = synth.make_batch(rank_frame_seed(rank, BATCH), nbase, H, W, gray=args.gray)
    if nbase < BATCH:
        frames_np = np.concatenate([np.roll(frames_np, 16 * k, axis=3) for k in range(BATCH // nbase)], 0)
    if args.gray:
        frames_np = np.ascontiguousarray(frames_np[:, :1])
    frames = torch.from_numpy(frames_np).to(dev)
    torch.cuda.synchronize(dev)

    def loop(k):
        for i in range(k):
            engs[i % len(engs)].detect_async(frames, BATCH)
        for e_ in engs:
            e_.sync()

    tw0 = time.perf_counter()
    loop(args.warmup)
    # The W warm-up steps of a short run (the driver's W = 5 is 16 ms) end before the clock has settled, and the timed
    # K steps would then measure the ramp: keep warming, untimed, until 0.3 s have passed (reported as warmup_extra_steps).
    extra = 0
    while not args.only_timed and time.perf_counter() - tw0 < 0.3:
        loop(4 * len(engs))
        extra += 4 * len(engs)
    cnt, ncand = eng.counts(BATCH)

    # events on ONE call in EVERY (round 4: two event records per launch on every call were 0.7 % of the frame rate --
    # 11 300 against 11 390 frames/s, two runs each; sampled they still span the whole timed region)
    use_events = not args.no_timing_events
    EVERY = 4
    for e_ in engs:
        e_.set_timing(EVERY if use_events else 0)
    timed_calls = sum(len(range(0, len(range(j, args.steps, len(engs))), EVERY)) for j in range(len(engs)))
    fdist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    loop(args.steps)
    torch.cuda.synchronize(dev)
    my_dt = time.perf_counter() - t0
    fdist.barrier()
    dt = time.perf_counter() - t0
    timed_timings = [t for e_ in engs for t in e_.timings()] if use_events else []
    for e_ in engs:
        e_.set_timing(False)
    dt, value_all, per_rank = aggregate_over_ranks(world, my_dt, dt, bcast_ms, args.steps, BATCH)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, engs[(args.steps - 1) % len(engs)], BATCH)

    # steady state: the same loop for >= 2 s (the K timed steps of the contract last well under DVFS settling time)
    steady = None
    if not args.no_steady_state:
        ks = max(args.steps, int(np.ceil(2.2 / max(1e-6, my_dt / args.steps))))
        fdist.barrier()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        loop(ks)
        torch.cuda.synchronize(dev)
        fdist.barrier()
        d1 = fdist.max_over_ranks(time.perf_counter() - t1)
        steady = {"value": round(BATCH * ks * world / d1, 2), "unit": "frames/s", "steps": ks, "seconds": round(d1, 3),
                  "ms_per_step": round(d1 / ks * 1e3, 4)}

    single = rank == 0 and world == 1
    single_ctx = None
    if args.contexts > 1 and args.full and not args.only_timed:
        # the same loop on ONE context with the library's default plan (every rank; not part of `value`)
        e0 = Engine(H, W, max_batch=BATCH, **kw1)
        e0.import_packed(eng.export_packed())
        for _ in range(min(10, args.warmup)):
            e0.detect_async(frames, BATCH)
        e0.sync()
        ks = max(args.steps, 50)
        fdist.barrier()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for _ in range(ks):
            e0.detect_async(frames, BATCH)
        e0.sync()
        torch.cuda.synchronize(dev)
        fdist.barrier()
        d1 = fdist.max_over_ranks(time.perf_counter() - t1)
        single_ctx = {"value": round(BATCH * ks * world / d1, 2), "unit": "frames/s", "steps": ks, "ms_per_step": round(d1 / ks * 1e3, 4),
                      "plan": "one context, the library's default plan (two sub-batches of 16 frames on two streams)"}
        e0.close()
    serial = None
    if use_events and single and not args.no_serial_pass:
        # same kernels, one stream: clean per-kernel durations (not part of `value`)
        e1 = Engine(H, W, max_batch=BATCH, num_streams=1, plan_flags=["nms_in_line"], **kw1)
        e1.import_packed(eng.export_packed())
        for _ in range(2):
            e1.detect_async(frames, BATCH)
        e1.sync()
        e1.set_timing(True)
        ks = min(10, args.steps)
        t1 = time.perf_counter()
        for _ in range(ks):
            e1.detect_async(frames, BATCH)
        e1.sync()
        d1 = time.perf_counter() - t1
        serial = (symbol_stats(e1.timings(), ks), d1 / ks * 1e3, e1.timings(), ks)
        e1.close()
    latency = None
    if single and not args.no_latency:
        el = Engine(H, W, max_batch=1, **kw1)
        el.import_packed(eng.export_packed())
        one = frames[:1].contiguous()
        for _ in range(20):
            el.detect_async(one, 1)
            el.sync()
        lat = []
        for _ in range(200):
            t1 = time.perf_counter()
            el.detect_async(one, 1)
            el.sync()
            lat.append((time.perf_counter() - t1) * 1e3)
        latency = {"median": round(float(np.median(lat)), 4), "p10": round(float(np.percentile(lat, 10)), 4),
                   "p90": round(float(np.percentile(lat, 90)), 4), "calls": len(lat)}
        el.close()
    alt = {}
    if single and not args.no_alt_pass and args.workload == "vga32" and not vgg:
        # the other fp32 arithmetic modes on the same frames (not part of `value`)
        for adt in ("f32", "f32_split", "f32_split_f16"):
            if adt == dtype:
                continue
            ea = Engine(H, W, max_batch=BATCH, device=local, in_channels=cin, dtype=adt)
            ea.load_state_dict(sd)
            for _ in range(3):
                ea.detect_async(frames, BATCH)
            ea.sync()
            ks = min(20, max(5, args.steps))
            t1 = time.perf_counter()
            for _ in range(ks):
                ea.detect_async(frames, BATCH)
            ea.sync()
            d1 = time.perf_counter() - t1
            acnt, _ = ea.counts(BATCH)
            key = {"f32": "plain_f32_mfma_mode", "f32_split": "split_operand_mode", "f32_split_f16": "split_operand_fp16_mode"}[adt]
            alt[key] = {"dtype": adt, "value": round(BATCH * ks / d1, 2), "unit": "frames/s", "steps": ks,
                        "ms_per_step": round(d1 / ks * 1e3, 4), "keypoints_per_frame": round(float(np.mean(acnt)), 1),
                        "same_keypoint_counts_as_headline_mode": bool(np.array_equal(acnt, cnt))}
            ea.close()
    other = {}
    if single and not args.no_other_workloads and args.workload == "vga32" and dtype == "f32" and not vgg and not args.gray:
        for e_ in engs:      # the headline engines are done: give their slabs back before the HD one is carved
            e_.close()
        del frames
        torch.cuda.empty_cache()
        for wl_name in ("qvga32-magicpoint", "hd64-bf16"):
            try:
                other[wl_name] = side_workload(wl_name, sd, local)
            except Exception as ex:   # a side pass must never cost the headline line
                other[wl_name] = {"error": "%s: %s" % (type(ex).__name__, ex)}
    host_fed = None
    if single and not args.no_host_fed and args.workload == "vga32" and not args.gray:
        host_fed = host_fed_rates(sd, frames_np, local, dtype)
    total_frames = BATCH * args.steps * world

    if rank == 0:
        value = value_all
        assert abs(value - total_frames / dt) <= 1e-6 * value
        step_ms = dt / args.steps * 1e3
        flops_frame = 2.0 * (arch.vgg_conv_macs(H, W) if vgg else arch.conv_macs(H, W, descriptor=not magic))
        wl = ("batch=32 640x480 frames per GPU, super_point checkpoint layout, fp32 "
              "(BASELINE.json configs[1]; configs[2] when n_gpus=8)" +
              ("; products as six bf16 MFMAs on exactly split fp32 operands" if dtype == "f32_split" else
               "; products as three fp16 MFMAs on two-term split fp32 operands" if dtype == "f32_split_f16" else "")
              ) if dtype != "bf16" else (
              "batch=64 1280x960 frames per GPU, super_point checkpoint layout, bf16 activations/weights, fp32 "
              "accumulation, fp32 post-processing (BASELINE.json configs[4])")
        if magic:
            wl = "batch=32 240x320 frames per GPU, detector only (MagicPoint), NMS r=4, " + dtype + " (BASELINE.json configs[3])"
        if vgg:
            wl = "batch=32 640x480 gray frames per GPU, the cpp/ frontend's network (superpoint::SPModel, 256-D), " + dtype
        out = {
            "metric": "frames/sec (%s) SuperPoint fwd+NMS+descriptors" % ("QVGA 320x240, detector only" if magic else "VGA 640x480" if dtype != "bf16" else "HD 1280x960"),
            "value": round(value, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "warmup_extra_steps": extra, "ms_per_step": round(step_ms, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"f32": "f32", "bf16": "bf16", "f32_split": "f32 (3 x bf16 split operands, 6 MFMA per product, f32 accumulate)",
                      "f32_split_f16": "f32 (2 x fp16 split operands, 3 MFMA per product, f32 accumulate)"}[dtype],
            "data": "synthetic (seeded frames + seeded checkpoint in the reference's layout)",
            "config": {"workload": wl, "frames_per_step_per_gpu": BATCH, "height": H, "width": W, "input_channels": cin,
                       "parallelism": "frame-sharded x%d, no data-path collective" % world},
            "frames_per_sec_per_gpu": round(value / world, 2),
            "whole_path_tflops": round(value * flops_frame / 1e12, 3),
            "whole_path_frac_of_%s_mfma_peak" % ("f32" if dtype == "f32" else "bf16"): round(
                value / world * flops_frame * {"f32_split": 6.0, "f32_split_f16": 3.0}.get(dtype, 1.0) / 1e12 /
                (PEAK_F32_MFMA_TFLOPS if dtype == "f32" else PEAK_BF16_MFMA_TFLOPS), 4),
            "keypoints_per_frame": round(float(np.mean(cnt)), 1),
            "candidates_per_frame": round(float(np.mean(ncand)), 1),
            "weights_broadcast_ms": round(bcast_ms, 2),
            "host_threads_per_rank": host_threads,
            # what fpc_create costs (include/fpc.h: fpc_stream_report): the process's first one carries the code object's
            # load and the search for one anchor stream per hardware queue; a later one only places its own streams
            "create": {"first_create_ms": round(first_create_ms, 2), "create_ms": round(create_ms, 2) if create_ms is not None else None,
                       "stream_placement": stream_reports},
        }
        out["config"]["contexts"] = args.contexts
        out["config"]["batches_in_flight"] = ("%d contexts in turn, each a whole 32-frame batch per call on one stream: batch k+1 starts while "
                                              "batch k drains" % args.contexts) if args.contexts > 1 else "1 context"
        if single_ctx is not None:
            out["single_context"] = single_ctx
        if per_rank is not None:
            out["per_rank"] = {"frames_per_s": [r[0] for r in per_rank], "weights_start_up_ms": [r[1] for r in per_rank]}
        if steady is not None:
            out["steady_state"] = steady
        if latency is not None:
            out["latency_ms_b1"] = latency["median"]
            out["latency_b1"] = latency
        if timed_timings:
            # dominant kernel = the kernel SYMBOL (as rocprofv3 aggregates) with the largest share of the step.  In the
            # timed region several streams run concurrently, so a launch's duration includes the time it shares the GPU;
            # `roofline_serial` repeats the measurement with one stream (kernels alone on the GPU).
            table = load_traffic_table(dtype) if (H, W) == (480, 640) or mode.bound == "hbm" else {}
            stats = symbol_stats(timed_timings, timed_calls)
            key = "bytes" if mode.bound == "hbm" else "flops"
            sym = max((k for k in stats if stats[k][key] > 0), key=lambda k: stats[k]["total_ms"])
            if args.contexts == 1 and os.environ.get("FPC_STREAMS") == "1":
                timed_src = "HIP events on the launch stream inside the timed region (one context, FPC_STREAMS=1: the kernel alone on the GPU)"
            else:
                timed_src = ("HIP events on the launch streams inside the timed region, on one call in %d (%d context%s: launches of "
                             "different streams share the GPU, a launch's bracket includes that time)"
                             % (EVERY, args.contexts, "s" if args.contexts > 1 else ""))
            timed_roof = roofline_entry(mode, sym, stats[sym], step_ms, table, None, timed_src)
            if serial is not None:
                # `roofline` = the dominant kernel priced on ITS OWN duration (the one-stream pass: the kernel alone on the
                # GPU, where HIP events and rocprofv3's AverageNs agree -- profiles/README.md); the timed region's bracket,
                # which includes the time a launch shares the GPU with the other context's, is kept beside it.
                sstats, sms, stim, ks = serial
                out["roofline"] = roofline_entry(mode, sym, sstats[sym], sms, table, None,
                                                 "HIP events on the launch stream, one-stream pass inside this run (%d steps): the "
                                                 "kernel alone on the GPU" % ks)
                out["roofline"]["in_timed_region"] = {k_: timed_roof[k_] for k_ in ("avg_launch_ms", "frac", "frac_mfma", "frac_algorithmic",
                                                                                   "share_of_step", "duration_source")}
                out["roofline"]["ms_per_step_one_stream"] = round(sms, 4)
            else:
                out["roofline"] = timed_roof
            per_layer = {}
            for name, kern, ms, fl, mf, nb in timed_timings:
                per_layer.setdefault(name, []).append((ms, mf, nb))
            out["layer_ms_per_step_concurrent"] = {k: round(float(np.sum([m for m, _, _ in v])) / timed_calls, 4) for k, v in per_layer.items()}
            out["whole_path"] = whole_path_fractions(mode, timed_timings, timed_calls, step_ms, BATCH, table)
            if serial is not None:
                sstats, sms, stim, ks = serial
                lay = {}
                for name, kern, ms, fl, mf, nb in stim:
                    lay.setdefault(name, []).append(ms)
                out["layer_ms_serial"] = {k: round(float(np.mean(v)), 4) for k, v in lay.items()}
                # every kernel symbol of the plan, alone on the GPU: executed-MFMA fraction (<= 1), the algorithmic one
                # (may exceed 1: Winograd) and the HBM fraction by counter bytes where a committed PMC summary holds the symbol
                ks_out = {}
                for k, v in sorted(sstats.items(), key=lambda kv: -kv[1]["total_ms"]):
                    sec_ = v["avg_launch_ms"] * 1e-3
                    tr_ = lookup_traffic(table, k)
                    fr_ = BATCH * v["layers"] / max(1, v["launches_per_step"])
                    ks_out[k] = {"avg_launch_ms": round(v["avg_launch_ms"], 4), "launches_per_step": v["launches_per_step"],
                                 "frac_mfma": round(v["mfma_flops"] / sec_ / 1e12 / mode.peak_issued, 4),
                                 "frac_algorithmic": round(v["flops"] / sec_ / 1e12 / mode.peak_algorithmic, 4),
                                 "frac_hbm": round(tr_[0] * fr_ / sec_ / 1e9 / PEAK_HBM_GBS, 4) if tr_ else None,
                                 "traffic_over_algorithmic_bytes": round(tr_[0] * fr_ / v["bytes"], 3) if (tr_ and v["bytes"]) else None}
                out["kernels_serial"] = ks_out
        if host_fed is not None:
            for v in host_fed.values():
                v["fraction_of_device_resident"] = round(v["value"] / value, 4)
            out["host_fed"] = host_fed
        if other:
            out["other_workloads"] = other
        out.update(alt)
        if world == 1 and not args.no_cpu_baseline and vgg:
            cb = cpu_baseline_vgg_reference(sd, frames_np[:4])
            if cb is not None:
                out["cpu_baseline"] = cb
        elif world == 1 and not args.no_cpu_baseline:
            ncb = 32 if H * W <= 480 * 640 else 4
            cb_frames = frames_np[:ncb] if not args.gray else np.repeat(frames_np[:ncb], 3, axis=1)
            out["cpu_baseline"] = cpu_baseline(sd, cb_frames, descriptor=not magic)
        print(json.dumps(out))
    for e_ in engs:
        e_.close()
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
