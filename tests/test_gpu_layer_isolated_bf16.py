"""Layer-isolated parity of the bf16 mode's kernels (pytest -m gpu): tests/test_gpu_layer_isolated.py for dtype="bf16".

After a forward, every tensor of Engine.ACTIVATIONS is read back, every layer is computed once more from the DEVICE'S OWN
input tensor(s) with the mode's roundings put where the kernels put them (oracle.bf16_layer_parts, double accumulation), and
EVERY element of EVERY frame must lie in the interval that fp32 accumulation order leaves open around that value
(oracle/layer_check.py::compare_bf16_layer: no allowance for a share of elements; tests/test_layer_oracle_bf16.py shows on
the CPU that it flags one element off by one bf16 ulp).  A failure names the layer, its kernel, the frame and the position in
the tile.

The bf16 kernels run a persistent grid: XCD k -- the workgroups with blockIdx.x & 7 == k -- walks the tiles [k T / 8,
(k + 1) T / 8) of a launch, workgroup j of `per` = grid / 8 taking every per-th from the j-th on, and the walk carries state
from tile to tile (the next tile's first halo chunk, the weight-fragment ring, tiles past the last made "not live").  The
default grid has a few hundred workgroups, so a small call never makes one walk two tiles: FPC_BF16_GRID caps the grid, and
every case computes from its geometry (TILES below, from FPC_BF16_KINDS) how many tiles each workgroup of each launch walks
and asserts the regime it is there for -- and, by symbol, the instance that wrote each tensor.

Weights: seed 3, dustbin_bias 4.0; frames: synth.make_batch(11, n, h, w); forward, not detect (detect writes no logits here).
"""
import os
import re

import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth
from oracle import layer_check

pytestmark = pytest.mark.gpu

SD = synth.make_state_dict(3, dustbin_bias=4.0)

# tensor -> (TH, TW of the instance's tile, the map it tiles as a divisor of the frame, gridDim.y): FPC_BF16_KINDS, stem_bf16.h
TILES = {"pool": (8, 7, 4, 1), "layer1.0": (8, 32, 4, 1), "layer1.1": (8, 32, 4, 1), "layer2.0": (6, 20, 8, 1), "layer2.1": (8, 16, 8, 1),
         "det.0": (8, 16, 8, 1), "det.1": (8, 16, 8, 1), "desc_in.0": (3, 20, 16, 1), "desc_in.1": (4, 16, 16, 1),
         "up": (8, 16, 16, 2),      # 8 x 16 on its 1/16 INPUT (16 x 32 of the output); two output-channel parts
         "desc_out.0": (8, 16, 8, 1), "desc_out.1": (8, 16, 8, 1)}
SYMBOLS = {"pool": "stem_bf16_kernel",
           "layer1.0": "block_bf16_one_kernel<8, 32, 1, 3, 64, 2, 2, 4, 1, 64>", "layer1.1": "block_bf16_one_kernel<8, 32, 1, 3, 64, 2, 2, 4, 1, 64>",
           "layer2.0": "block_bf16_one_kernel<6, 20, 2, 3, 64, 2, 2, 2, 2, 128>", "layer2.1": "block_bf16_one_kernel<8, 16, 1, 3, 128, 1, 4, 4, 1, 128>",
           "det.0": "block_bf16_one_kernel<8, 16, 1, 3, 128, 1, 4, 4, 1, 80>", "det.1": "block_bf16_one_kernel<8, 16, 1, 3, 80, 4, 1, 1, 3, 80>",
           "desc_in.0": "block_bf16_one_kernel<3, 20, 2, 3, 128, 1, 4, 2, 2, 256>", "desc_in.1": "block_bf16_two_kernel<4, 16, 1, 3, 128, 1, 4, 2, 2, 256>",
           "up": "convt_bf16_kernel<8, 16, 1, 2, 64, 2, 2, 2, 1, 128>",
           "desc_out.0": "block_bf16_kernel<8, 16, 1, 3, 64, 1, 4, 4, 1, 128>", "desc_out.1": "block_bf16_one_kernel<8, 16, 1, 3, 128, 1, 4, 4, 1, 128>"}
CONVT_PHASE = "block_bf16_kernel<8, 16, 1, 2, 64, 1, 4, 4, 1, 128>"      # FPC_PLAN_CONVT_PHASES: four launches of it, gridDim.y 1
DESCRIPTOR_HEAD = ("desc_in.0", "desc_in.1", "up", "desc_out.0", "desc_out.1")
QUARTER, EIGHTH = ("pool", "layer1.0", "layer1.1"), ("layer2.0", "layer2.1", "det.0", "det.1", "desc_out.0", "desc_out.1")

# id -> (h, w, frames, Engine keywords, FPC_BF16_GRID or None)
CASES = {
    "walk_one_per_xcd": (160, 192, 5, dict(), 8),
    "walk_two_per_xcd": (176, 208, 6, dict(), 16),
    "empty_xcd_ranges": (48, 80, 1, dict(), None),
    "default_grid": (160, 192, 5, dict(), None),
    "convt_phases": (176, 208, 5, dict(plan_flags=["convt_phases"]), 8),
    "no_fused_softmax": (160, 192, 2, dict(plan_flags=["no_fused_softmax"]), None),
    "gray": (160, 192, 5, dict(in_channels=1), 8),
    "detector_only": (160, 192, 5, dict(descriptor_enabled=False), 8),
}
_frames = {}
_launches = {}     # case id -> [(op name, kernel symbol)] of its forward


def frames_of(h, w, n, channels=3):
    if (h, w) not in _frames or len(_frames[(h, w)]) < n:
        _frames[(h, w)] = synth.make_batch(11, n, h, w)
    f = _frames[(h, w)][:n]
    return f if channels == 3 else f[:, :1].copy()


def tiles_of(name, h, w, n):
    """T of the launch that writes `name` for n frames of h x w."""
    th, tw, div, _ = TILES[name]
    return -(-(h // div) // th) * -(-(w // div) // tw) * n


def grid_of(name, T, cap, cus):
    """gridDim.x of that launch: plan_options.h's bf16_persistent_grid; with no cap, what it is AT LEAST (one resident
    workgroup per CU; the instances hold more)."""
    parts = TILES[name][3]
    return min((T + 7) // 8 * 8, max(8, (cap or cus) // parts // 8 * 8))


def walk(T, grid):
    """Tiles walked by each workgroup of a launch, [xcd][j]: block_bf16.h / stem_bf16.h / convt_bf16.h."""
    per = grid // 8
    out = []
    for xcd in range(8):
        first, end = xcd * T // 8, (xcd + 1) * T // 8
        out.append([max(0, -(-(end - first - j) // per)) for j in range(per)])
    return out


def engine_of(cid):
    from fpc_amd.engine import Engine
    h, w, n, kw, cap = CASES[cid]
    env = {} if cap is None else {"FPC_BF16_GRID": str(cap)}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine(h, w, max_batch=n, dtype="bf16", **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.load_state_dict(SD)
    return e


def launches_of(engine, frames):
    engine.set_timing(True)
    engine.forward(frames)
    engine.sync()
    out = [(op, sym) for op, sym, _, _, _, _ in engine.timings()]
    engine.set_timing(False)
    return out


def launches_of_case(cid, engine=None):
    """The launches of case `cid`: as recorded when it ran, or (the case deselected) from a forward of its own."""
    if cid not in _launches:
        h, w, n, kw = CASES[cid][:4]
        e = engine or engine_of(cid)
        try:
            _launches[cid] = launches_of(e, frames_of(h, w, n, kw.get("in_channels", 3)))
        finally:
            if engine is None:
                e.close()
    return _launches[cid]


def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(cid, symbols=SYMBOLS, absent=()):
    """Asserts the instance that wrote each tensor, runs a forward, checks every layer and frame.  -> {tensor: (T, grid,
    walk)} of the case's launches, for the caller's assertions about the regime."""
    h, w, n, kw, cap = CASES[cid]
    frames = frames_of(h, w, n, kw.get("in_channels", 3))
    e = engine_of(cid)
    try:
        launches = launches_of_case(cid, e)
        kernels = [s for _, s in launches]
        wrote = layer_check.layer_kernels(launches)
        names = [t for t in e.ACTIVATIONS if e.descriptor_enabled or t not in DESCRIPTOR_HEAD]
        for t in names:
            assert wrote[t] == symbols[t], (cid, t, wrote[t])
        for k in absent:
            assert k not in kernels, (cid, k)
        if not e.descriptor_enabled:
            assert not any(wrote[t] != "?" for t in DESCRIPTOR_HEAD), (cid, wrote)
        e.forward(frames)
        layer_check.check_bf16_layers(e, frames, SD, "%s %dx%dx%d" % (cid, h, w, n), launches=launches,
                                      tiles={t: (TILES[t][0] * (2 if t == "up" else 1), TILES[t][1] * (2 if t == "up" else 1)) for t in names})
    finally:
        e.close()
    cus = cu_count()
    regime = {}
    for t in names:
        T = tiles_of(t, h, w, n)
        g = grid_of(t, T, cap, cus)
        regime[t] = (T, g, walk(T, g))
    return regime


def test_walk_one_workgroup_per_xcd():
    """160 x 192, five frames, FPC_BF16_GRID=8: one workgroup per XCD, every launch with more than 8 tiles (pool 175,
    layer1 50, ..., up 10) -- some workgroup of EVERY instance walks two tiles or more; layer1, the 128-channel and the
    detector instances three or more.  40 x 48 maps under 8 x 32 tiles and 20 x 24 under 8 x 16: partial tiles on the right
    and bottom edges."""
    regime = run_case("walk_one_per_xcd")
    assert len(regime) == 12 and regime["pool"][0] == 175 and regime["layer1.0"][0] == 50 and regime["up"][0] == 10
    for t, (T, g, per_wg) in regime.items():
        assert g == 8 and T > 8 and max(max(x) for x in per_wg) >= 2 and sum(sum(x) for x in per_wg) == T, (t, T, g, per_wg)
    for t in ("layer1.0", "layer1.1", "layer2.1", "det.0", "det.1", "desc_out.0", "desc_out.1"):
        assert max(max(x) for x in regime[t][2]) >= 3, (t, regime[t])
    assert (192 // 4) % 32 and (160 // 8) % 8 and (192 // 8) % 16


def test_walk_two_workgroups_per_xcd():
    """176 x 208, six frames, FPC_BF16_GRID=16: two workgroups per XCD take every other tile of its range (tcur += per), each
    with two or more on the 1/4- and 1/8-resolution layers; 11 x 13 maps at 1/16 (the two parts of `up` share the 16: 8 each)."""
    regime = run_case("walk_two_per_xcd")
    for t in QUARTER + EIGHTH:
        T, g, per_wg = regime[t]
        assert g == 16 and all(len(x) == 2 and min(x) >= 2 for x in per_wg), (t, T, g, per_wg)
    assert regime["up"][1] == 8 and regime["up"][0] == 12
    assert (176 // 16, 208 // 16) == (11, 13)


def test_empty_xcd_ranges():
    """48 x 80, one frame, the default grid: fewer than 8 tiles on every layer, so XCDs with an empty range -- XCD 0 among
    them, whose workgroup's first tile is already not live -- next to XCDs with one tile."""
    regime = run_case("empty_xcd_ranges")
    for t, (T, g, per_wg) in regime.items():
        assert T < 8 and g == 8 and per_wg[0] == [0] and sorted(set(x[0] for x in per_wg)) == [0, 1], (t, T, g, per_wg)
    assert regime["layer2.0"][0] == 1 and regime["pool"][0] == 6


def test_default_grid():
    """160 x 192, five frames, the default grid (a workgroup per tile: every launch has fewer tiles than CUs): the regime
    every earlier small test ran in, at this bar."""
    regime = run_case("default_grid")
    for t, (T, g, per_wg) in regime.items():
        assert g == (T + 7) // 8 * 8 and max(max(x) for x in per_wg) == 1, (t, T, g)


def test_convt_phases():
    """176 x 208, five frames, FPC_PLAN_CONVT_PHASES, FPC_BF16_GRID=8: `up` written by four launches of block_bf16_kernel<8,
    16, 1, 2, ...> (10 tiles each: a workgroup walks two), convt_bf16_kernel absent."""
    regime = run_case("convt_phases", symbols=dict(SYMBOLS, up=CONVT_PHASE), absent=[SYMBOLS["up"]])
    assert [s for _, s in launches_of_case("convt_phases")].count(CONVT_PHASE) == 4
    T, g, per_wg = regime["up"]
    assert T == 10 and g == 8 and max(max(x) for x in per_wg) == 2


def test_no_fused_softmax():
    """160 x 192, two frames, FPC_PLAN_NO_FUSED_SOFTMAX: the detector's second block without its softmax epilogue compiled
    in the plan, the exp-softmax a launch of its own."""
    run_case("no_fused_softmax")
    assert any(s.startswith("softmax") for _, s in launches_of_case("no_fused_softmax"))


def test_gray_stem():
    """160 x 192, five gray frames (in_channels=1), FPC_BF16_GRID=8: stem_bf16_kernel's one-plane instance (the library
    reports both instances under one symbol; the context's in_channels decides) against the stem with the three filters
    summed before their rounding to bf16, 175 tiles on 8 workgroups."""
    regime = run_case("gray")
    assert regime["pool"][:2] == (175, 8)


def test_detector_only():
    """160 x 192, five frames, descriptor_enabled=False, FPC_BF16_GRID=8: no launch of the descriptor head, its tensors not
    asked for; the seven others as in walk_one_per_xcd."""
    regime = run_case("detector_only")
    assert sorted(regime) == sorted(t for t in SYMBOLS if t not in DESCRIPTOR_HEAD)


def test_every_kernel_of_a_vga_call_is_covered():
    """Every convolution, block and stem symbol that a VGA call of 32 bf16 frames or of one frame launches (forwards only)
    is exercised by a case above."""
    from fpc_amd.engine import Engine
    need = set()
    for n in (32, 1):
        e = Engine(480, 640, max_batch=n, dtype="bf16")
        try:
            e.load_state_dict(SD)
            need |= set(e.kernel_names(synth.make_batch(11, n, 480, 640)))
        finally:
            e.close()
    need = {k for k in need if not re.match(r"softmax|nms|descriptor16", k)}
    assert any(k.startswith("stem_bf16") for k in need) and any(k.startswith("convt_bf16") for k in need), sorted(need)
    covered = set()
    for cid in CASES:
        covered |= {s for _, s in launches_of_case(cid)}
    assert need <= covered, sorted(need - covered)
