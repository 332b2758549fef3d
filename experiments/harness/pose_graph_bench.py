"""Pose-graph optimisation (fpc_graph_optimise) on planted rings, DESIGN.md section 7: rings of 64, 256 and 1 024 nodes with
2 x nodes edges (the odometry, the loop edge and exact chords of tests/test_pose_graph.py's ring_scene: a scale drift of
1 + 0.3 / N per edge, 2 mrad and 0.01 of noise, the start composed from the odometry), the reservation sized to the ring.
    python experiments/harness/pose_graph_bench.py [reps] [runs] [nodes]
prints one JSON line per ring and parameter set: the call from HIP events on the ctx stream (median, min and max over `runs`
runs of `reps` back-to-back calls, after a warm-up), the attempts made and accepted, the cost before and after, the time per
attempt, and the launches per call (5 + 6 per attempt of `iterations`, less one).  Every timed call starts from the same
nodes: a fpc_graph_set_nodes launch in front of it is part of the figure.  Parameter sets: the defaults (16 attempts of at
most 256 CG iterations) and the same with cg_iterations = 32, which shows what the single-workgroup solve costs.  The kernels'
own times need a kernel trace of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python experiments/harness/pose_graph_bench.py 20 1 1024
(the pg_*_kernel rows; the call's time less their sum per call is what the stream spent between launches)."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from fpc_amd.engine import Engine
from tests.test_pose_graph import ring_scene

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sizes = [int(sys.argv[3])] if len(sys.argv) > 3 else [64, 256, 1024]

for n in sizes:
    sc = ring_scene(n, True, n, 100 + n, edges_cap=2 * n)
    g = sc.graph
    assert g.count == 2 * n and g.dropped == 0
    e = Engine(64, 96, max_batch=1, descriptor_enabled=False, max_keypoints=64)
    nbytes = e.graph_reserve(n, 2 * n)
    dev = e.torch_device
    s0, r0, t0 = (torch.from_numpy(v).to(dev) for v in (g.s, g.R, g.t))
    e.graph_set_nodes(0, r0, t0, s0)
    e.graph_add_edges_async(g.efrom, g.eto, g.eR, g.et, g.es)
    fixed = torch.zeros(1, dtype=torch.int32, device=dev)
    for params in ({}, {"cg_iterations": 32}):
        def call():
            e.graph_set_nodes(0, r0, t0, s0)
            return e.graph_optimise_async(fixed, **params)

        for _ in range(3):
            stats = call()
        e.sync()
        stats = stats.cpu().numpy()
        st, ms = e.torch_stream(), []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            for _ in range(reps):
                call()
            b.record(st)
            e.sync()
            ms.append(a.elapsed_time(b) / reps)
        it = 16
        print(json.dumps({"nodes": n, "edges": 2 * n, "params": params or "defaults", "reservation_bytes": nbytes,
                          "ms_per_call": [round(float(v), 4) for v in (np.median(ms), min(ms), max(ms))],
                          "attempts": int(stats[2]), "accepted": int(stats[3]),
                          "ms_per_attempt": round(float(np.median(ms)) / max(int(stats[2]), 1), 4),
                          "cost": [float(stats[0]), float(stats[1])], "launches_per_call": 1 + 5 + 6 * it - 1}), flush=True)
    e.close()
