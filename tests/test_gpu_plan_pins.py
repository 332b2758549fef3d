"""The launch plan, the packed blob and the kernels each launch names, pinned to tests/golden/plan_pins.json.

The host code between a checkpoint and a launch (the plan builders, the weight packers, the launch functions of
csrc/fpc_api.hip) can be reorganised without touching a kernel; this test is what says such a change moved nothing:
for every case the plan hash, the packed size, the SHA-256 of the blob packed from seed-0 weights, and the
(layer name, kernel symbol) list of a one-frame and of a four-frame fpc_forward equal the fixture.

A pull request that MEANS to change the plan (a new kernel instance, another tile, another fragment layout)
regenerates the fixture with tests/golden/make_golden_plan.py and says so; any other pull request passes this test
with the fixture as it is."""
import hashlib
import json
import os

import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_pins.json")
GEOMETRIES = ((32, 48), (160, 64))     # ragged tiles both ways; a 20-row 1/8 map (the stacked Winograd walk from two frames up)
MAX_BATCH = 4
DTYPES = {"resnet": ("f32", "bf16", "f32_split", "f32_split_f16"), "vgg": ("f32", "f32_split", "f32_split_f16")}
F32_PLANS = ("winograd_gen1", "winograd_gen2", "no_fused_blocks", "tiles_round5")


def cases():
    """(id, arch, dtype, plan flag or None, height, width): the default plan of each architecture x dtype, and the
    Python network's FPC_F32 plan under the flags that change its kernels or its blob, at both geometries."""
    out = []
    for h, w in GEOMETRIES:
        for arch, dtypes in DTYPES.items():
            out += [("%s-%s-%dx%d" % (arch, dt, h, w), arch, dt, None, h, w) for dt in dtypes]
        out += [("resnet-f32-%s-%dx%d" % (flag, h, w), "resnet", "f32", flag, h, w) for flag in F32_PLANS]
    return out


_cache = {}


def _shared(key, make, *args, **kw):
    if key not in _cache:
        _cache[key] = make(*args, **kw)
    return _cache[key]


def record(arch, dtype, flag, h, w):
    """What the fixture holds for one case, from the library the package loads."""
    from fpc_amd.engine import Engine

    vgg = arch == "vgg"
    eng = Engine(h, w, max_batch=MAX_BATCH, in_channels=1 if vgg else 3, dtype=dtype, arch=arch,
                 plan_flags=[flag] if flag else ())
    try:
        eng.load_state_dict(_shared(("sd", arch), synth.make_vgg_state_dict if vgg else synth.make_state_dict, seed=0))
        frames = _shared(("frames", vgg, h, w), synth.make_batch, 11, MAX_BATCH, h, w, gray=vgg)[:, :1 if vgg else 3].copy()
        rec = {"plan_hash": "%016x" % eng.plan_hash(), "packed_size": int(eng.packed_size()),
               "blob_sha256": hashlib.sha256(eng.export_packed().tobytes()).hexdigest()}
        for n in (1, MAX_BATCH):
            eng.set_timing(True)
            eng.forward(frames[:n])
            rec["launches_%d" % n] = [[name, symbol] for name, symbol, _, _, _, _ in eng.timings()]
            eng.set_timing(False)
    finally:
        eng.close()
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_plan_pins(case):
    with open(FIXTURE) as f:
        want = json.load(f)[case[0]]
    got = record(*case[1:])
    for key in want:
        assert got[key] == want[key], "%s: %s differs from tests/golden/plan_pins.json" % (case[0], key)
    assert sorted(got) == sorted(want)
