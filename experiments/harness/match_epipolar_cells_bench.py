"""fpc_match_frames_guided_epipolar_cells beside fpc_match_frames and fpc_match_frames_guided_epipolar on the same inputs, in
the same process.
32 VGA frames of exactly K = 500, 1000, 2000, 4500 rows against a key frame of K rows, cross check on.  The key is K random
integer pixels with random unit descriptors and a depth of 2 .. 8 units each (K = diag(500, 500), centre (320, 240)); frame f
sees those 3-D points from a planted camera of one of two kinds -- `general`: a rotation of 2 .. 11 degrees about a slanted
axis and a translation with all three components, `sideways`: a pure x translation -- so its rows follow a planted
fundamental matrix.  Pixels are rounded, rows that leave the frame are replaced by unrelated ones, in random order (device
results are sorted by confidence, which is no spatial order either).  The rows are written into the library's device results
behind a fpc_get_points call.
    python experiments/harness/match_epipolar_cells_bench.py [reps]
prints one JSON line per (camera, K, radius), radius 2 / 4 / 8 px: the median of 5 runs of `reps` (default 50) calls each by
HIP events on the ctx stream with the runs' min and max, for fpc_match_frames, fpc_match_frames_guided_epipolar (the
yardstick) and fpc_match_frames_guided_epipolar_cells; the ratio of the new call to the yardstick; whether the two calls'
min -- max brackets overlap; the share of (strip, tile) pairs the new call visited, from its stats_dev; and whether its
tables equal the yardstick's bit for bit on these inputs."""
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
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
KMAT = np.array([[500.0, 0, W / 2], [0, 500.0, H / 2], [0, 0, 1]])


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def camera(kind, f):
    """Frame f's camera, X_f = R X + t."""
    if kind == "sideways":
        return np.eye(3), np.array([(1.0 if f % 2 else -1.0) * (0.3 + 0.0125 * f), 0.0, 0.0])
    axis = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    a = np.deg2rad(2.0 + 0.3 * f)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k), np.array([0.3, -0.2, 0.25]) * (0.5 + f / N)


def scene(kind, K, dim, rng):
    flat = rng.permutation(W * H)[:K]
    key_xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    key = unit(rng.normal(size=(K, dim)))
    ki = np.linalg.inv(KMAT)
    pts = (np.concatenate([key_xy, np.ones((K, 1))], 1) @ ki.T) * rng.uniform(2, 8, K)[:, None]
    desc, xy = np.zeros((N, K, dim), np.float32), np.zeros((N, K, 2), np.int32)
    fs = np.zeros((N, 9), np.float32)
    for f in range(N):
        r, t = camera(kind, f)
        p = (pts @ r.T + t) @ KMAT.T
        p = np.rint(p[:, :2] / p[:, 2:])
        out = (p[:, 0] < 0) | (p[:, 0] > W - 1) | (p[:, 1] < 0) | (p[:, 1] > H - 1)
        d = unit(key + rng.normal(0, 0.02, key.shape))
        d[out] = unit(rng.normal(size=(int(out.sum()), dim)))
        p[out] = np.stack([rng.integers(0, W, int(out.sum())), rng.integers(0, H, int(out.sum()))], 1)
        o = rng.permutation(K)
        desc[f], xy[f] = d[o], p[o]
        # query = frame f, train = the key: X_key = R^T X_f - R^T t, F = K^-T [t']x R' K^-1
        r2, t2 = r.T, -r.T @ t
        fm = ki.T @ np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]]) @ r2 @ ki
        fs[f] = (fm / np.sqrt((fm * fm).sum())).astype(np.float32).reshape(9)
    return key, key_xy, desc, xy, fs


for K in (500, 1000, 2000, 4500):
    e = Engine(H, W, max_batch=N, max_keypoints=K)
    cap, dim = e.capacity, e.desc_dim
    assert cap == K, (cap, K)
    prob = torch.zeros((N, H, W))
    prob[:, 40, 40] = 0.5
    e.get_points(prob, torch.ones((N, dim, H // 8, W // 8)))
    rd, rc = e._results_view()
    rx, _ = e._points_view()
    m = torch.empty((N, cap), dtype=torch.int32, device="cuda")
    d = torch.empty((N, cap), dtype=torch.float32, device="cuda")
    m2, d2 = torch.empty_like(m), torch.empty_like(d)
    stats = torch.zeros((N, 2), dtype=torch.int32, device="cuda")
    lib, ctx, st = e._l, e._ctx, e.torch_stream()
    for kind in ("general", "sideways"):
        key, key_xy, desc, xy, fs = scene(kind, K, dim, np.random.Generator(np.random.PCG64([K, len(kind)])))
        rd[:N].copy_(torch.from_numpy(desc))
        rx[:N].copy_(torch.from_numpy(xy))
        rc[:N].fill_(K)
        kd, kc = e._key(key)
        kx, _ = e._key_xy(key_xy)
        fdev = torch.from_numpy(fs).cuda()
        torch.cuda.synchronize()

        def plain():
            assert lib.fpc_match_frames(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), 1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

        for radius in (2.0, 4.0, 8.0):
            def epipolar():
                assert lib.fpc_match_frames_guided_epipolar(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(),
                                                            fdev.data_ptr(), radius, 1, 0.0, 0.0, m.data_ptr(),
                                                            d.data_ptr()) == 0

            def cells():
                assert lib.fpc_match_frames_guided_epipolar_cells(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(),
                                                                  fdev.data_ptr(), radius, 1, 0.0, 0.0, m2.data_ptr(),
                                                                  d2.data_ptr(), stats.data_ptr()) == 0

            calls = (("epipolar", epipolar), ("cells", cells), ("plain", plain))
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
            epipolar()
            cells()
            e.sync()
            same = bool(torch.equal(m, m2) and torch.equal(d.view(torch.int32), d2.view(torch.int32)))
            sh = stats.cpu().numpy().astype(np.int64)
            med = {name: statistics.median(v) for name, v in times.items()}
            apart = max(times["cells"]) < min(times["epipolar"]) or min(times["cells"]) > max(times["epipolar"])
            print(json.dumps({"camera": kind, "frames": N, "K": K, "radius": radius, "match_frames_ms": spread(times["plain"]),
                              "guided_epipolar_ms": spread(times["epipolar"]),
                              "guided_epipolar_cells_ms": spread(times["cells"]),
                              "cells_over_epipolar": round(med["cells"] / med["epipolar"], 3),
                              "brackets_overlap": not apart,
                              "visited_share": round(float(sh[:, 0].sum()) / float(sh[:, 1].sum()), 4),
                              "matched": int((m2 >= 0).sum().item()), "bit_identical": same}), flush=True)
    e.close()
