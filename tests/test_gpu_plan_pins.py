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
# Created with min_sub_batch = 2, so that the four-frame call is a LARGE call (n >= 2 * min_sub_batch) and launches the
# large-call variants of the plan -- the default min_sub_batch of 8 makes both pinned calls of the cases above few-frame
# calls.  (arch, dtype, plan flags, further Engine keyword arguments): the builder branches the cases above never enter.
LARGE_CALL = (
    [("resnet", "f32", (), {})] +
    [("resnet", "f32", flags, {}) for flags in (
        ("no_latency_tiles",), ("no_winograd",), ("no_winograd", "layer1_tile_8x16"), ("no_winograd_detector",),
        ("no_winograd_layer_in1",), ("detector_gen1",), ("w36_one_wave",), ("conv_round1",), ("stem_round3",))] +
    [("resnet", "f32", (), {"descriptor_enabled": False}), ("resnet", "f32", (), {"in_channels": 1}),
     ("resnet", "bf16", (), {}), ("resnet", "bf16", ("convt_phases",), {}), ("resnet", "bf16", ("no_fused_softmax",), {}),
     ("resnet", "bf16", (), {"descriptor_enabled": False}), ("resnet", "f32_split", (), {}),
     ("vgg", "f32", (), {}), ("vgg", "f32", (), {"descriptor_enabled": False})])


def cases():
    """(id, arch, dtype, plan flags, height, width, Engine keyword arguments): the default plan of each architecture x
    dtype, the Python network's FPC_F32 plan under the flags that change its kernels or its blob, and the large-call
    cases, at both geometries."""
    out = []
    for h, w in GEOMETRIES:
        for arch, dtypes in DTYPES.items():
            out += [("%s-%s-%dx%d" % (arch, dt, h, w), arch, dt, (), h, w, {}) for dt in dtypes]
        out += [("resnet-f32-%s-%dx%d" % (flag, h, w), "resnet", "f32", (flag,), h, w, {}) for flag in F32_PLANS]
        for arch, dt, flags, kw in LARGE_CALL:
            tags = list(flags) + ["%s_%d" % (k, int(v)) for k, v in sorted(kw.items())]
            out.append(("-".join([arch, dt, "sub2"] + tags + ["%dx%d" % (h, w)]), arch, dt, flags, h, w,
                        dict(kw, min_sub_batch=2)))
    return out


def load_pins(path=FIXTURE):
    """Case id -> record.  The file holds the records of the few-frame cases in full, as it always has; those of the
    large-call cases sit under "large_call" with their launch lists as indexes into ONE table of (layer name, kernel
    symbol) pairs -- the same lists, a line per case."""
    with open(path) as f:
        pins = json.load(f)
    packed = pins.pop("large_call", {"launch_table": [], "cases": {}})
    table = packed["launch_table"]
    for cid, rec in packed["cases"].items():
        pins[cid] = {k: [table[i] for i in v] if k.startswith("launches_") else v for k, v in rec.items()}
    return pins


def dump_pins(pins, path=FIXTURE):
    """The inverse of load_pins (tests/golden/make_golden_plan.py)."""
    large = {c[0] for c in cases() if "min_sub_batch" in c[6]}
    table = sorted({tuple(l) for cid in large for k, v in pins[cid].items() if k.startswith("launches_") for l in v})
    index = {l: i for i, l in enumerate(table)}
    text = json.dumps({cid: rec for cid, rec in pins.items() if cid not in large}, indent=1, sort_keys=True)
    rows = ["   %s: %s" % (json.dumps(cid), json.dumps(
        {k: [index[tuple(l)] for l in v] if k.startswith("launches_") else v for k, v in pins[cid].items()}, sort_keys=True))
        for cid in sorted(large)]
    with open(path, "w") as f:
        f.write(text[:text.rindex("}")].rstrip("\n") + ',\n "large_call": {\n  "launch_table": [\n' +
                ",\n".join("   " + json.dumps(list(l)) for l in table) + '\n  ],\n  "cases": {\n' + ",\n".join(rows) + "\n  }\n }\n}\n")


_cache = {}


def _shared(key, make, *args, **kw):
    if key not in _cache:
        _cache[key] = make(*args, **kw)
    return _cache[key]


def record(arch, dtype, flags, h, w, kw, env=None):
    """What the fixture holds for one case, from the library the package loads.  `env`: variables set while the context
    is created (fpc_create reads them) and restored behind it."""
    from fpc_amd.engine import Engine

    vgg = arch == "vgg"
    kw = dict(kw)
    cin = kw.pop("in_channels", 1 if vgg else 3)
    old = {k: os.environ.get(k) for k in env or {}}
    os.environ.update(env or {})
    try:
        eng = Engine(h, w, max_batch=MAX_BATCH, in_channels=cin, dtype=dtype, arch=arch, plan_flags=list(flags), **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        eng.load_state_dict(_shared(("sd", arch), synth.make_vgg_state_dict if vgg else synth.make_state_dict, seed=0))
        frames = _shared(("frames", cin == 1, h, w), synth.make_batch, 11, MAX_BATCH, h, w, gray=cin == 1)[:, :cin].copy()
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
    want = _shared("pins", load_pins)[case[0]]
    got = record(*case[1:])
    for key in want:
        assert got[key] == want[key], "%s: %s differs from tests/golden/plan_pins.json" % (case[0], key)
    assert sorted(got) == sorted(want)


# An FPC_* variable set instead of its plan flag gives the flag's plan: (variables, the flags whose record it must equal,
# whether that record is a large-call one, dtype).  No fixture data of their own.
SUB2 = {"min_sub_batch": 2}
VARIABLE_FOR_FLAG = (
    ({"FPC_WINOGRAD_GEN": "1"}, ("winograd_gen1",), {}, "f32"),
    ({"FPC_WINOGRAD_GEN": "2"}, ("winograd_gen2",), {}, "f32"),
    ({"FPC_FUSE": "0"}, ("no_fused_blocks",), {}, "f32"),
    ({"FPC_TILES_ROUND6": "0"}, ("tiles_round5",), {}, "f32"),
    ({"FPC_LATENCY_TILES": "0"}, ("no_latency_tiles",), SUB2, "f32"),
    ({"FPC_WINOGRAD": "0"}, ("no_winograd",), SUB2, "f32"),
    ({"FPC_WINOGRAD": "0", "FPC_L1_T816": "0"}, ("no_winograd", "layer1_tile_8x16"), SUB2, "f32"),   # (set at all: on)
    ({"FPC_WINOGRAD_DET": "0"}, ("no_winograd_detector",), SUB2, "f32"),
    ({"FPC_WINOGRAD_IN1": "0"}, ("no_winograd_layer_in1",), SUB2, "f32"),
    ({"FPC_WINOGRAD_DET_GEN": "1"}, ("detector_gen1",), SUB2, "f32"),
    ({"FPC_W36_PAIRED": "0"}, ("w36_one_wave",), SUB2, "f32"),
    ({"FPC_CONV_LEAN": "0"}, ("conv_round1",), SUB2, "f32"),
    ({"FPC_STEM_LEAN": "0"}, ("stem_round3",), SUB2, "f32"),
    ({"FPC_CONVT_FUSED": "0"}, ("convt_phases",), SUB2, "bf16"),
    ({"FPC_FUSE_SOFTMAX": "0"}, ("no_fused_softmax",), SUB2, "bf16"),
    ({"FPC_MIN_SUB": "2"}, (), SUB2, "f32"),                                                         # (no min_sub_batch)
)


@pytest.mark.gpu
@pytest.mark.parametrize("env,flags,kw,dtype", VARIABLE_FOR_FLAG, ids=["+".join("%s=%s" % i for i in v[0].items()) for v in VARIABLE_FOR_FLAG])
def test_variable_gives_its_flags_plan(env, flags, kw, dtype):
    h, w = GEOMETRIES[0]
    cid = "-".join(["resnet", dtype] + (["sub2"] if kw else []) + list(flags) + ["%dx%d" % (h, w)])
    want = _shared("pins", load_pins)[cid]
    got = record("resnet", dtype, (), h, w, {} if "FPC_MIN_SUB" in env else kw, env=env)
    assert got == want, "%s does not give the plan of %s" % (env, cid)
