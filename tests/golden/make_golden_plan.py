#!/usr/bin/env python3
"""Fixture plan_pins.json: what tests/test_gpu_plan_pins.py pins -- per case the plan hash, the packed size, the
SHA-256 of the blob packed from seed-0 weights and the (layer name, kernel symbol) lists of a one-frame and a
four-frame fpc_forward.  Needs the GPU and a built libfpc.so (FPC_LIB_PATH picks another build than the tree's):

    python tests/golden/make_golden_plan.py [output.json]

Run it on the build whose plan is meant to be the pinned one: for a change that must not move the plan, that is the
build of the commit BEFORE the change, never the changed one.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import fpc_amd  # noqa: E402,F401
from tests.test_gpu_plan_pins import FIXTURE, cases, dump_pins, record  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    pins = {}
    for case in cases():
        pins[case[0]] = record(*case[1:])
        print(case[0], pins[case[0]]["plan_hash"], pins[case[0]]["packed_size"], len(pins[case[0]]["launches_1"]),
              len(pins[case[0]]["launches_4"]), flush=True)
    dump_pins(pins, out)
    print("wrote", out, len(pins), "cases")
