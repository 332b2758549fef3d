"""fpc_match_frames_guided against fpc_match_frames on the same inputs, in the same run.
32 VGA frames of exactly K = 500, 1000, 2000, 4500 rows against a key frame of K rows, cross check on: the key is K random
integer pixels with random unit descriptors, frame f the key's pixels under a planted homography (a rotation, a scale, a
shift and a little perspective that grow with f), rounded, rows that leave the frame replaced by unrelated ones, in random
order (device results are sorted by confidence, which is no spatial order either).  The rows are written into the
library's device results behind a fpc_get_points call.  Radii 4, 16 and 1e4 px under the planted H.
    python experiments/harness/match_guided_bench.py [reps] [--cells]
prints one JSON line per (K, radius): the median of 5 runs of `reps` (default 50) calls each by HIP events on the ctx stream
with the runs' min and max, for the guided call and for fpc_match_frames; the share of (64-row strip, 64-row train tile)
pairs without a candidate (counted on the host from the gate, frames 0, 11, 21, 31), which is the share of tiles the
kernel skips, and its complement, the fraction of fpc_match_frames' MFMAs the guided kernel executes.
--cells adds fpc_match_frames_guided_cells beside them (same inputs, same run, interleaved): its time, its ratio to the
guided call, and the share of (strip, tile) pairs it visited, from the call's own counters over all 32 frames."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd.engine import Engine

H, W, N = 480, 640, 32
RUNS = 5
CELLS = "--cells" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--cells"]
reps = int(argv[0]) if argv else 50


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def homography(f):
    a, s = 0.004 * f, 1.0 + 0.003 * f
    c = np.array([[1, 0, W / 2], [0, 1, H / 2], [0, 0, 1.0]])
    r = np.array([[s * np.cos(a), -s * np.sin(a), 0.7 * f], [s * np.sin(a), s * np.cos(a), -0.4 * f], [2e-6 * f, -1e-6 * f, 1]])
    return c @ r @ np.linalg.inv(c)


def scene(K, dim, rng):
    flat = rng.permutation(W * H)[:K]
    key_xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    key = unit(rng.normal(size=(K, dim)))
    desc, xy, hs = np.zeros((N, K, dim), np.float32), np.zeros((N, K, 2), np.int32), np.zeros((N, 9), np.float32)
    for f in range(N):
        g = homography(f)
        p = np.concatenate([key_xy, np.ones((K, 1))], 1) @ g.T
        p = np.rint(p[:, :2] / p[:, 2:])
        out = (p[:, 0] < 0) | (p[:, 0] > W - 1) | (p[:, 1] < 0) | (p[:, 1] > H - 1)
        d = unit(key + rng.normal(0, 0.02, key.shape))
        d[out] = unit(rng.normal(size=(int(out.sum()), dim)))
        p[out] = np.stack([rng.integers(0, W, int(out.sum())), rng.integers(0, H, int(out.sum()))], 1)
        o = rng.permutation(K)
        desc[f], xy[f] = d[o], p[o]
        gi = np.linalg.inv(g)
        hs[f] = (gi / gi[2, 2]).astype(np.float32).reshape(9)
    return key, key_xy, desc, xy, hs


def skipped_share(xy, key_xy, hs, radius, frames=(0, 11, 21, 31)):
    """The share of (64-row strip, 64-row train tile) pairs without a candidate: include/fpc.h's gate in float64."""
    skipped = total = 0
    u, v = key_xy[None, :, 0].astype(np.float64), key_xy[None, :, 1].astype(np.float64)
    for f in frames:
        h = hs[f].astype(np.float64)
        x, y = xy[f, :, 0:1].astype(np.float64), xy[f, :, 1:2].astype(np.float64)
        w = h[6] * x + h[7] * y + h[8]
        ex, ey = h[0] * x + h[1] * y + h[2] - w * u, h[3] * x + h[4] * y + h[5] - w * v
        cand = (w > 0) & (ex * ex + ey * ey < float(radius) ** 2 * w * w)
        k = cand.shape[0]
        pad = -k % 64
        t = np.pad(cand, ((0, pad), (0, pad))).reshape((k + pad) // 64, 64, (k + pad) // 64, 64).any(axis=(1, 3))
        skipped, total = skipped + int((~t).sum()), total + t.size
    return skipped / total


for K in (500, 1000, 2000, 4500):
    e = Engine(H, W, max_batch=N, max_keypoints=K)
    cap, dim = e.capacity, e.desc_dim
    assert cap == K, (cap, K)
    key, key_xy, desc, xy, hs = scene(K, dim, np.random.Generator(np.random.PCG64(K)))
    prob = torch.zeros((N, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((N, dim, H // 8, W // 8)))
    rd, rc = e._results_view()
    rx, _ = e._points_view()
    rd[:N].copy_(torch.from_numpy(desc))
    rx[:N].copy_(torch.from_numpy(xy))
    rc[:N].fill_(K)
    kd, kc = e._key(key)
    kx, _ = e._key_xy(key_xy)
    hdev = torch.from_numpy(hs).cuda()
    m = torch.empty((N, cap), dtype=torch.int32, device="cuda")
    d = torch.empty((N, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib, ctx, st = e._l, e._ctx, e.torch_stream()

    def plain():
        assert lib.fpc_match_frames(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), 1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

    for radius in (4.0, 16.0, 1e4):
        def guided():
            assert lib.fpc_match_frames_guided(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(), hdev.data_ptr(), radius,
                                               1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

        def cells():
            assert lib.fpc_match_frames_guided_cells(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(), hdev.data_ptr(),
                                                     radius, 1, 0.0, 0.0, m.data_ptr(), d.data_ptr(), None) == 0

        calls = (("guided", guided), ("plain", plain)) + ((("cells", cells),) if CELLS else ())
        for _, fn in calls:
            for _ in range(3):
                fn()
        e.sync()
        times = {name: [] for name, _ in calls}
        for _ in range(RUNS):
            for name, fn in calls:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(st)
                for _ in range(reps):
                    fn()
                t1.record(st)
                e.sync()
                times[name].append(t0.elapsed_time(t1) / reps)
        share = skipped_share(xy, key_xy, hs, radius)
        row = {"frames": N, "K": K, "radius": radius, "guided_ms": spread(times["guided"]),
               "match_frames_ms": spread(times["plain"]),
               "ratio": round(statistics.median(times["guided"]) / statistics.median(times["plain"]), 3),
               "tiles_skipped": round(share, 4), "executed_mfma_fraction": round(1.0 - share, 4)}
        if CELLS:
            _, _, stats = e.match_frames_guided_cells_async(N, hdev, radius, key=(kd, kc), key_xy=(kx, kc), stats=True)
            e.sync()
            stats = stats.cpu().numpy().astype(np.int64)
            row.update({"cells_ms": spread(times["cells"]),
                        "cells_over_guided": round(statistics.median(times["cells"]) / statistics.median(times["guided"]), 3),
                        "cells_visited_share": round(float(stats[:, 0].sum()) / float(stats[:, 1].sum()), 4)})
        print(json.dumps(row), flush=True)
    e.close()
