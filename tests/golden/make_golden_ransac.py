#!/usr/bin/env python3
"""Fixture ransac_pins.json: what tests/test_gpu_ransac_pins.py pins -- per case the bit patterns of the models (H, F, or R
and t), the inlier counts and the hashes of the masks.  Needs the GPU and a built libfpc.so (FPC_LIB_PATH picks another
build than the tree's):

    python tests/golden/make_golden_ransac.py [output.json]

Run it on the build whose results are meant to be the pinned ones: for a change that must not move them, that is the build
of the commit BEFORE the change, never the changed one.

Before it writes, it checks that the planted inputs give the fixture something to pin: every frame that is not degenerate
by construction has inliers, the degenerate ones have none, the min_inliers case rejects a frame that has a best
hypothesis and keeps another, and in every family one refit changes the model (refits = 1 against refits = 0).
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import fpc_amd  # noqa: E402,F401
from tests.test_gpu_ransac_pins import FAMILIES, FIXTURE, Rig, cases, record  # noqa: E402


def check(pins):
    for fam, (threads, sample, _, _) in FAMILIES.items():
        base = "%s-a-T%d-r%%d-m%d" % (fam, threads, sample)
        r0, r1, rej = pins[base % 0], pins[base % 1], pins["%s-a-T%d-r1-m600" % (fam, threads)]
        model = lambda r: r["R"] + r["t"] if fam == "pnp" else r["model"]       # noqa: E731
        assert model(r0) != model(r1), "%s: one refit changed nothing" % fam
        assert r1["ninliers"][2] > 0 and rej["ninliers"][2] == 0 and rej["ninliers"][3] >= 600, (fam, r1["ninliers"], rej["ninliers"])
        for name, rec in pins.items():
            if not name.startswith(fam + "-"):
                continue
            ni = rec["ninliers"]
            if "-a-" in name:                               # sample - 1, sample, 257, 1 024 pairs
                assert ni[0] == 0 and ni[3] > 500, (name, ni)
                assert "-m600" in name or (ni[1] == sample and ni[2] > 100), (name, ni)
            else:                                           # 1 025, capacity, outliers only, collinear
                assert ni[0] > 500 and ni[1] > 500 and ni[2] < 30 and ni[3] == 0, (name, ni)
    for name, rec in pins.items():
        if name.startswith("gather-"):
            counts = rec.get("ninliers", rec.get("nfront"))
            assert sum(1 for v in counts if v > 0) >= 2, (name, counts)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    pins = {}
    rig = Rig()
    try:
        for case in cases():
            pins[case[0]] = record(rig, *case[1:])
            print(case[0], {k: v for k, v in pins[case[0]].items() if k in ("ninliers", "nfront", "pick", "best")}, flush=True)
    finally:
        rig.close()
    try:
        check(pins)
    except AssertionError:
        out += ".rejected"                                  # (kept to be looked at, never the fixture)
        raise
    finally:
        with open(out, "w") as f:
            json.dump(pins, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", out, len(pins), "cases")
