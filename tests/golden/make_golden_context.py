#!/usr/bin/env python3
"""Fixture context_pins.json: what tests/test_gpu_context_pins.py pins -- per case the streams a context opens, its
packed size and the bytes each reserving call reports.  Needs the GPU and a built libfpc.so (FPC_LIB_PATH picks another
build than the tree's):

    python tests/golden/make_golden_context.py [output.json]

Run it on the build whose allocations are meant to be the pinned ones: for a change that must not move them, that is
the build of the commit BEFORE the change, never the changed one.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import fpc_amd  # noqa: E402,F401
from tests.test_gpu_context_pins import FIXTURE, cases, record  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    pins = {}
    for case in cases():
        rec = record(*case[1:])
        assert rec.pop("guards_bad", 0) == 0, case[0]
        pins[case[0]] = rec
        print(case[0], json.dumps(rec, sort_keys=True), flush=True)
    with open(out, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, len(pins), "cases")
