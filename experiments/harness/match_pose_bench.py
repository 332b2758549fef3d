"""fpc_match_frames_guided_pose beside fpc_match_frames, fpc_match_frames_guided and fpc_match_frames_guided_epipolar on the
same inputs, in the same process.
The scene, the points and the method are match_epipolar_bench.py's: 32 VGA frames of exactly K = 500, 1000, 2000, 4500 rows
against a key frame of K rows, cross check on; the key is K random integer pixels with random unit descriptors, back-projected
(K = diag(500, 500), centre (320, 240)) onto a slanted plane 5 units in front of the key camera; frame f sees the plane from
a camera rotated and translated a little more with every f, so its rows follow a planted homography, a planted fundamental
matrix AND a planted pose, the back-projected points being the key's landmarks.  Pixels are rounded, rows that leave the
frame are replaced by unrelated ones, in random order.  The rows are written into the library's device results behind a
fpc_get_points call.
    python experiments/harness/match_pose_bench.py [reps]
prints one JSON line per (K, radius), radius 2 / 4 / 8 px: the median of 5 runs of `reps` (default 50) calls each by HIP
events on the ctx stream with the runs' min and max, for the four calls, interleaved; the ratios of the new call and of the
epipolar call to fpc_match_frames_guided (the yardstick: parent code with the same per-pair operation count and the same
disc-shaped gate); and per gate the share of (64-row strip, 64-row train tile) pairs without a candidate (counted on the host
from the gates of include/fpc.h, frames 0, 11, 21, 31), which is the share of tiles the kernel skips."""
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
FX, FY, CX, CY = 500.0, 500.0, W / 2, H / 2
KMAT = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
PLANE_N, PLANE_D = np.array([0.1, -0.05, 1.0]), 5.0               # n . X = d in the key camera's coordinates


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def camera(f):
    """Frame f's camera, X_f = R X + t: a rotation about (0.2, 1, 0.1) and a translation that grow with f."""
    axis = np.array([0.2, 1.0, 0.1]) / np.linalg.norm([0.2, 1.0, 0.1])
    a = 0.002 * (f + 1)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * (k @ k), np.array([0.02, -0.01, 0.005]) * (f + 1)


def scene(K, dim, rng):
    flat = rng.permutation(W * H)[:K]
    key_xy = np.stack([flat % W, flat // W], 1).astype(np.int32)
    key = unit(rng.normal(size=(K, dim)))
    ki = np.linalg.inv(KMAT)
    rays = np.concatenate([key_xy, np.ones((K, 1))], 1) @ ki.T
    key_xyz = (rays * (PLANE_D / (rays @ PLANE_N))[:, None]).astype(np.float32)      # the plane's points: the landmarks
    desc, xy = np.zeros((N, K, dim), np.float32), np.zeros((N, K, 2), np.int32)
    hs, fs = np.zeros((N, 9), np.float32), np.zeros((N, 9), np.float32)
    rs, ts = np.zeros((N, 9), np.float32), np.zeros((N, 3), np.float32)
    for f in range(N):
        r, t = camera(f)
        g = KMAT @ (r + np.outer(t, PLANE_N) / PLANE_D) @ ki             # key pixel -> frame pixel, over the plane
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
        # query = frame f, train = the key: X_key = R^T X_f - R^T t, F = K^-T [t']x R' K^-1
        r2, t2 = r.T, -r.T @ t
        fm = ki.T @ np.array([[0, -t2[2], t2[1]], [t2[2], 0, -t2[0]], [-t2[1], t2[0], 0]]) @ r2 @ ki
        fs[f] = (fm / np.sqrt((fm * fm).sum())).astype(np.float32).reshape(9)
        rs[f], ts[f] = r.reshape(9), t                                   # landmark frame (the key camera) -> frame f
    return key, key_xy, key_xyz, desc, xy, hs, fs, rs, ts


def gate_h(f, x, y, radius):
    h, u, v = f["m"], f["u"], f["v"]
    w = h[6] * x + h[7] * y + h[8]
    ex, ey = h[0] * x + h[1] * y + h[2] - w * u, h[3] * x + h[4] * y + h[5] - w * v
    return (w > 0) & (ex * ex + ey * ey < float(radius) ** 2 * w * w)


def gate_f(f, x, y, radius):
    m, u, v = f["m"], f["u"], f["v"]
    l0, l1, l2 = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5], m[6] * x + m[7] * y + m[8]
    m0, m1 = m[0] * u + m[3] * v + m[6], m[1] * u + m[4] * v + m[7]
    e = l0 * u + l1 * v + l2
    return e * e < float(radius) ** 2 * (l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1)


def gate_p(f, x, y, radius):
    r, t, p = f["m"], f["t"], f["xyz"]
    a = r[0] * p[:, 0] + r[1] * p[:, 1] + r[2] * p[:, 2] + t[0]
    b = r[3] * p[:, 0] + r[4] * p[:, 1] + r[5] * p[:, 2] + t[1]
    c = (r[6] * p[:, 0] + r[7] * p[:, 1] + r[8] * p[:, 2] + t[2])[None]
    ex, ey = FX * a[None] - (x - CX) * c, FY * b[None] - (y - CY) * c
    return (c > 0) & (ex * ex + ey * ey < float(radius) ** 2 * c * c)


def skipped_share(gate, xy, key_xy, key_xyz, ms, ts, radius, frames=(0, 11, 21, 31)):
    """The share of (64-row strip, 64-row train tile) pairs without a candidate: include/fpc.h's gates in float64."""
    skipped = total = 0
    u, v = key_xy[None, :, 0].astype(np.float64), key_xy[None, :, 1].astype(np.float64)
    for f in frames:
        x, y = xy[f, :, 0:1].astype(np.float64), xy[f, :, 1:2].astype(np.float64)
        cand = gate(dict(m=ms[f].astype(np.float64), t=ts[f].astype(np.float64), u=u, v=v, xyz=key_xyz.astype(np.float64)),
                    x, y, radius)
        k = cand.shape[0]
        pad = -k % 64
        t = np.pad(cand, ((0, pad), (0, pad))).reshape((k + pad) // 64, 64, (k + pad) // 64, 64).any(axis=(1, 3))
        skipped, total = skipped + int((~t).sum()), total + t.size
    return skipped / total


for K in (500, 1000, 2000, 4500):
    e = Engine(H, W, max_batch=N, max_keypoints=K)
    cap, dim = e.capacity, e.desc_dim
    assert cap == K, (cap, K)
    key, key_xy, key_xyz, desc, xy, hs, fs, rs, ts = scene(K, dim, np.random.Generator(np.random.PCG64(K)))
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
    kl = torch.from_numpy(key_xyz).cuda()
    hdev, fdev = torch.from_numpy(hs).cuda(), torch.from_numpy(fs).cuda()
    rdev, tdev = torch.from_numpy(rs).cuda(), torch.from_numpy(ts).cuda()
    m = torch.empty((N, cap), dtype=torch.int32, device="cuda")
    d = torch.empty((N, cap), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib, ctx, st = e._l, e._ctx, e.torch_stream()

    def plain():
        assert lib.fpc_match_frames(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), 1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

    for radius in (2.0, 4.0, 8.0):
        def guided():
            assert lib.fpc_match_frames_guided(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(), hdev.data_ptr(), radius,
                                               1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

        def epipolar():
            assert lib.fpc_match_frames_guided_epipolar(ctx, N, 0, kd.data_ptr(), kc.data_ptr(), kx.data_ptr(),
                                                        fdev.data_ptr(), radius, 1, 0.0, 0.0, m.data_ptr(), d.data_ptr()) == 0

        def pose():
            assert lib.fpc_match_frames_guided_pose(ctx, N, kd.data_ptr(), kc.data_ptr(), kl.data_ptr(), None, rdev.data_ptr(),
                                                    tdev.data_ptr(), FX, FY, CX, CY, radius, 1, 0.0, 0.0, m.data_ptr(),
                                                    d.data_ptr()) == 0

        calls = (("guided", guided), ("epipolar", epipolar), ("pose", pose), ("plain", plain))
        for _, fn in calls:
            for _ in range(3):
                fn()
        e.sync()
        matched = int((m.cpu().numpy() >= 0).sum())                     # (of the last warm-up call: plain)
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
        pose()
        e.sync()
        matched_pose = int((m.cpu().numpy() >= 0).sum())
        med = {name: statistics.median(v) for name, v in times.items()}
        print(json.dumps({"frames": N, "K": K, "radius": radius, "match_frames_ms": spread(times["plain"]),
                          "guided_h_ms": spread(times["guided"]), "guided_epipolar_ms": spread(times["epipolar"]),
                          "guided_pose_ms": spread(times["pose"]),
                          "pose_over_guided_h": round(med["pose"] / med["guided"], 3),
                          "epipolar_over_guided_h": round(med["epipolar"] / med["guided"], 3),
                          "pose_over_match_frames": round(med["pose"] / med["plain"], 3),
                          "tiles_skipped_h": round(skipped_share(gate_h, xy, key_xy, key_xyz, hs, ts, radius), 4),
                          "tiles_skipped_epipolar": round(skipped_share(gate_f, xy, key_xy, key_xyz, fs, ts, radius), 4),
                          "tiles_skipped_pose": round(skipped_share(gate_p, xy, key_xy, key_xyz, rs, ts, radius), 4),
                          "rows_matched_plain": matched, "rows_matched_pose": matched_pose}), flush=True)
    e.close()
