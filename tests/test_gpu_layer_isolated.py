"""Layer-isolated float64 parity of the fp32 network kernels (pytest -m gpu): the fp32 counterpart of
tests/test_gpu_parity.py::_check_bf16_layers.

After a forward, every tensor of Engine.ACTIVATIONS is read back, every layer is computed once more from the DEVICE'S OWN
input tensor(s) by oracle.f32_layer / oracle.f32_stem (folded float weights, double accumulation), and the device's output
must agree within 1e-4 at every element of EVERY frame (oracle/layer_check.py; tests/test_layer_oracle.py shows on the CPU
that this comparison flags a dropped column, row, K-chunk, a leak across a stacked seam and a wrong 65th channel).  A
failure names the layer, its kernel, the frame and the position in the tile, the stacked image and the channel chunks.

Each case sits at the smallest geometry that reaches the kernel it is there for, and asserts that this kernel ran.  Bit
equality with "tiles_round5" (tests/test_gpu_round6_tiles.py) stays the bar for a change of tiling; this is the bar a change
of arithmetic order answers to.  Every case also prints, per layer, the device's error over the error of the same layer in
plain fp32 on the CPU (E_ref); nothing is asserted from that ratio -- DESIGN.md keeps the measured table.

Weights: seed 3, dustbin_bias 4.0; frames: synth.make_batch(11, n, h, w); fp32, arch "resnet".
"""
import os
import re

import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth
from oracle import layer_check

pytestmark = pytest.mark.gpu

SD = synth.make_state_dict(3, dustbin_bias=4.0)
NLT = "no_latency_tiles"
STACKED = "wblock36s_kernel<2, 4, 4>"
CONV82 = "wconv36p_kernel<8, 2, 3>"
BLOCK416 = "block_mfma_kernel<4, 16, 2, 32, 1, 4, 2, 1, 128>"
PAIRED64 = "wblock36p_kernel<4, 4, 3>"

_frames = {}


def frames_of(h, w, n):
    if (h, w) not in _frames or len(_frames[(h, w)]) < n:
        _frames[(h, w)] = synth.make_batch(11, n, h, w)
    return _frames[(h, w)][:n]


def flag_of(define):
    """The name in _lib.PLAN_FLAGS of include/fpc.h's FPC_PLAN_<define>."""
    name = define.lower()
    assert name in _lib.PLAN_FLAGS, define
    return name


def launches_of(engine, frames):
    """[(op name, kernel symbol)] of one forward over `frames`: Engine.kernel_names with the op names kept."""
    engine.set_timing(True)
    engine.forward(frames)
    engine.sync()
    out = [(op, sym) for op, sym, _, _, _, _ in engine.timings()]
    engine.set_timing(False)
    assert sorted(s for _, s in out) == sorted(engine.kernel_names(frames))
    return out


def ran(kernels, want):
    """`want` names a symbol, or "head*tail" a family of instances."""
    head, _, tail = want.partition("*")
    return any(k == want or ("*" in want and k.startswith(head) and k.endswith(tail)) for k in kernels)


L1 = ("layer1.0", "layer1.1")
C128 = ("layer2.1", "desc_out.0", "desc_out.1")
DET = ("det.0", "det.1")
# id -> (h, w, frames, Engine keywords, {kernel the case is there for: the tensors it must have written}, kernels that must NOT run
#        [, environment of the Engine's creation])
W36_8, W36_16 = {"FPC_W36_CUS": "8"}, {"FPC_W36_CUS": "16"}
CASES = {
    "stacked_walk": (160, 192, 5, dict(plan_flags=[NLT]), {STACKED: C128, "wblock36p_dust_kernel<2, 8, 3>": DET}, []),
    "stacked_walk_other_seams": (224, 192, 4, dict(plan_flags=[NLT]), {STACKED: C128, "wblock36p_dust_kernel<4, 4, 3>": DET}, []),
    "frame_by_frame_128": (224, 192, 3, dict(plan_flags=[NLT]), {"wblock36_kernel<2, 4, 4>": C128}, [STACKED]),
    "conv_8x2_tiles": (288, 128, 1, dict(plan_flags=[NLT]), {CONV82: ("desc_in.1",), "wblock36p_kernel<2, 8, 3>": L1}, []),
    "paired_64": (224, 160, 1, dict(plan_flags=[NLT]), {PAIRED64: L1 + ("desc_in.1",)}, [CONV82]),
    "block_4x16": (176, 208, 2, dict(plan_flags=[NLT]), {BLOCK416: ("layer2.0",), "wblock36_kernel<2, 2, 8>": C128}, []),
    "latency_160x192": (160, 192, 1, dict(), {"wblock16_kernel<4, *": L1, "wblock16_kernel<8, *": C128 + ("desc_in.1",),
                                              "wblock_mfma_kernel<*, 3, 72>": DET, "stem_pool2_kernel": ("pool",),
                                              "conv2_mfma_kernel<*": ("desc_in.1", "up")}, []),
    "latency_176x208": (176, 208, 2, dict(), {"wblock16_kernel<4, *": L1, "wblock16_kernel<8, *": C128 + ("desc_in.1",),
                                              "wblock_mfma_kernel<*, 3, 72>": DET, "stem_pool_kernel": ("pool",),
                                              "conv2_mfma_kernel<*": ("desc_in.1", "up")}, []),
    "two_sub_batches": (160, 192, 7, dict(plan_flags=[NLT], min_sub_batch=2), {STACKED: C128}, []),
    "split_bf16x3": (176, 208, 3, dict(dtype="f32_split"), {"block_x3_kernel<*": L1 + C128 + DET + ("layer2.0", "desc_in.0", "desc_in.1", "up"),
                                                            "stem_pool_x3_kernel": ("pool",)}, []),
    "split_fp16x2": (176, 208, 3, dict(dtype="f32_split_f16"), {"block_h2_kernel<*": L1 + C128 + DET + ("layer2.0", "desc_in.0", "desc_in.1", "up"),
                                                                "stem_pool_x3_kernel": ("pool",)}, []),
    # the kernels still shipped behind a plan flag
    "winograd_gen1": (176, 208, 2, dict(plan_flags=["winograd_gen1"]), {"wblock_mfma_kernel<32, 2, 64>": L1, "wblock_mfma_kernel<32, 4, 128>": C128}, []),
    "winograd_gen2": (176, 208, 2, dict(plan_flags=["winograd_gen2", NLT]), {"wblock16_kernel<8, 8>": C128}, []),
    "no_winograd": (176, 208, 2, dict(plan_flags=["no_winograd"]), {"block_mfma_kernel<16, 16, *": L1, "block_mfma_kernel<6, 20, 1, 64, 2, *": C128,
                                                                    "block_mfma_kernel<6, 20, 1, *, 72>": DET}, ["w*"]),
    "no_fused_blocks": (176, 208, 2, dict(plan_flags=["no_fused_blocks"]), {"conv_mfma_kernel<8, 16, 1, 3, *": L1, "conv_mfma_kernel<6, 20, 2, 3, *": ("layer2.0", "desc_in.0"),
                                                                            "conv_mfma_kernel<6, 20, 1, 3, 72, *": ("det.1",)}, ["w*", "block*"]),
    "tiles_round5": (176, 208, 2, dict(plan_flags=["tiles_round5", NLT]), {"block_mfma_kernel<6, 20, 2, 32, 2, 2, 2, 2, 128>": ("layer2.0",)}, [BLOCK416]),
    "w36_one_wave": (176, 208, 2, dict(plan_flags=[flag_of("W36_ONE_WAVE"), NLT]), {"wblock36_kernel<1, 4, 4>": L1 + ("desc_in.1",), "wblock36_dust_kernel<2, 8>": DET}, []),
    "w36_one_wave_other_tiles": (288, 128, 1, dict(plan_flags=[flag_of("W36_ONE_WAVE"), NLT]), {"wblock36_kernel<1, 2, 8>": L1, "wblock36_dust_kernel<4, 4>": DET}, []),
    "detector_gen1": (176, 208, 2, dict(plan_flags=[flag_of("DETECTOR_GEN1"), NLT]), {"wblock_mfma_kernel<*, 3, 72>": DET, PAIRED64: L1}, ["wblock36p_dust*", "wblock36_dust*"]),
    "stem_round3": (160, 192, 1, dict(plan_flags=[flag_of("STEM_ROUND3")]), {"stem_pool_kernel": ("pool",)}, ["stem_pool2_kernel"]),
    "conv_round1": (176, 208, 2, dict(plan_flags=[flag_of("CONV_ROUND1")]), {"conv_mfma_kernel<3, 20, 1, 1, *": ("desc_in.1",), "conv_mfma_kernel<3, 20, 1, 2, *": ("up",)}, ["conv2_mfma*"]),
    # the F(4x4,3x3) kernels' XCD-chunked tile walk: FPC_W36_CUS caps a launch at 8 (16) workgroups, one (two) per XCD, and
    # every launch named here has more tiles than that (run_case asserts it from the geometry), so its workgroups walk
    # several.  (wconv36p_kernel<8, 2, 3> and the 1/16-resolution maps have one or two tiles at these sizes: not named.)
    "stacked_walk_w36_8": (160, 192, 5, dict(plan_flags=[NLT]), {STACKED: C128, "wblock36p_dust_kernel<2, 8, 3>": DET}, [], W36_8),
    "frame_by_frame_128_w36_8": (224, 192, 3, dict(plan_flags=[NLT]), {"wblock36_kernel<2, 4, 4>": C128}, [STACKED], W36_8),
    "paired_64_w36_8": (224, 160, 1, dict(plan_flags=[NLT]), {PAIRED64: L1}, [CONV82], W36_8),
    "conv_8x2_tiles_w36_8": (288, 128, 1, dict(plan_flags=[NLT]), {"wblock36p_kernel<2, 8, 3>": L1}, [], W36_8),
    "w36_one_wave_w36_8": (176, 208, 3, dict(plan_flags=[flag_of("W36_ONE_WAVE"), NLT]), {"wblock36_kernel<1, 4, 4>": L1, "wblock36_dust_kernel<2, 8>": DET}, [], W36_8),
    "stacked_walk_w36_16": (160, 192, 8, dict(plan_flags=[NLT]), {STACKED: C128, "wblock36p_dust_kernel<2, 8, 3>": DET}, [], W36_16),
    # wblock16_kernel's persistent walk (persist_min_tiles: from one tile per CU on) on layer 1 of the latency plan
    "latency_persistent_layer1": (176, 208, 11, dict(), {"wblock16_kernel<4, *": L1}, []),
}
MAP_DIVISOR = {t: 4 for t in L1}
MAP_DIVISOR.update({t: 8 for t in C128 + DET})


def tiles_of(sym, tensor, h, w, n):
    """Tiles of the launch of `sym` that writes `tensor` for n frames of h x w: a generation-3 workgroup takes 16 Winograd
    tiles of 4 x 4 pixels arranged TYT x TXT (wblock36s_kernel: of the n frames stacked into one image); wblock16_kernel<NCG,
    TH> takes TH x 16 pixels."""
    mh, mw = h // MAP_DIVISOR[tensor], w // MAP_DIVISOR[tensor]
    nums = [int(v) for v in re.findall(r"\d+", sym.partition("<")[2])]
    if sym.startswith("wblock16_kernel"):
        return -(-mh // nums[1]) * -(-mw // 16) * n
    tyt, txt = nums[1:3] if sym.startswith(("wblock36_kernel", "wblock36s_kernel")) else nums[0:2]
    if sym.startswith("wblock36s_kernel"):
        return -(-n * mh // (4 * tyt)) * -(-mw // (4 * txt))
    return -(-mh // (4 * tyt)) * -(-mw // (4 * txt)) * n


def engine_of(cid):
    """The Engine of case `cid`, created under the case's environment (read at creation), weights loaded."""
    from fpc_amd.engine import Engine
    h, w, n, kw = CASES[cid][:4]
    env = CASES[cid][6] if len(CASES[cid]) > 6 else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = Engine(h, w, max_batch=n, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.load_state_dict(SD)
    return e
_launches = {}     # case id -> [(op name, kernel symbol)] of its forward


def launches_of_case(cid, engine=None):
    """The launches of case `cid`: as recorded when it ran, or (the case deselected) from a forward of its own."""
    if cid not in _launches:
        h, w, n = CASES[cid][:3]
        e = engine or engine_of(cid)
        try:
            _launches[cid] = launches_of(e, frames_of(h, w, n))
        finally:
            if engine is None:
                e.close()
    return _launches[cid]


def run_case(cid, more_tiles_than=0):
    """`more_tiles_than`: every launch the case is there for must have more tiles than that, by tiles_of."""
    h, w, n, kw, there_for, absent = CASES[cid][:6]
    frames = frames_of(h, w, n)
    e = engine_of(cid)
    try:
        launches = launches_of_case(cid, e)
        kernels = [s for _, s in launches]
        wrote = layer_check.layer_kernels(launches)
        for k, tensors in there_for.items():
            assert ran(kernels, k), (cid, k, sorted(set(kernels)))
            for t in tensors:
                assert ran(wrote[t].split(" + "), k), (cid, k, t, wrote[t])
                if more_tiles_than:
                    sym = next(x for x in wrote[t].split(" + ") if ran([x], k))
                    assert tiles_of(sym, t, h, w, n) > more_tiles_than, (cid, sym, t, tiles_of(sym, t, h, w, n))
        for k in absent:
            assert not ran(kernels, k), (cid, k)
        e.forward(frames)
        layer_check.check_layers(e, frames, SD, "%s %dx%dx%d" % (cid, h, w, n), launches=launches)
    finally:
        e.close()


# ---------------------------------------------------------------- the batch plan ("no_latency_tiles": calls of a few frames reach it)
def test_stacked_walk():
    """160 x 192, five frames: wblock36s_kernel<2, 4, 4> on the three 128-channel blocks.  20 x 24 maps, 100 stacked rows:
    seams 4, 8 and 12 rows into a tile and on a tile edge (row 80), a partial tile column, a last tile row of 4 rows; 10 x 12
    maps at 1/16.  The detector's blocks run wblock36p_dust_kernel<2, 8, 3> here (64 + 1 channels on 8 x 32 pixels)."""
    run_case("stacked_walk")


def test_stacked_walk_other_seams():
    """224 x 192, four frames: 28-row maps, 112 stacked rows = 7 tile rows instead of 8, seams 12, 8 and 4 rows in.  The
    detector's blocks run wblock36p_dust_kernel<4, 4, 3> here."""
    run_case("stacked_walk_other_seams")


def test_frame_by_frame_128_channel_block():
    """224 x 192, three frames: 84 rows are 6 tile rows either way, so wblock36_kernel<2, 4, 4> walks frame by frame."""
    run_case("frame_by_frame_128")


def test_conv_8x2_tiles():
    """288 x 128: layer_in.1's conv1 on wconv36p_kernel<8, 2, 3>, 18 x 8 maps (partial rows); the 72 x 32 maps of layer1 put
    its blocks on wblock36p_kernel<2, 8, 3>, the arrangement a VGA batch takes."""
    run_case("conv_8x2_tiles")


def test_paired_64_channel_block():
    """224 x 160: a 14 x 10 map stays on wblock36p_kernel<4, 4, 3> (one 16 x 16 tile against two 32 x 8)."""
    run_case("paired_64")


def test_block_4x16():
    """176 x 208, two frames: layer2.0 on block_mfma_kernel<4, 16, ...>, 22 x 26 output with partial tiles both ways; 22 and
    26 are no multiples of 4, so every Winograd layer has a partial tile too (the 128-channel ones on 2 x 8 tiles)."""
    run_case("block_4x16")


def test_two_sub_batches():
    """160 x 192, seven frames as two sub-batches (min_sub_batch=2): each launch stacks its own frames; all seven checked."""
    run_case("two_sub_batches")


# ---------------------------------------------------------------- the latency plan (the default for calls of a few frames)
@pytest.mark.parametrize("cid", ["latency_160x192", "latency_176x208"])
def test_latency_plan(cid):
    """wblock16_kernel (64- and 128-channel instances), the detector on wblock_mfma_kernel<..., 3, 72>, conv2_mfma_kernel
    (ConvTranspose, layer_in.1's 1 x 1) and the stem: stem_pool2_kernel where the stem's 80 x 96 map is whole 16 x 16 tiles,
    stem_pool_kernel where it is not (88 x 104)."""
    run_case(cid)


# ---------------------------------------------------------------- the persistent tile walks: workgroups that take several tiles
@pytest.mark.parametrize("cid", ["stacked_walk_w36_8", "frame_by_frame_128_w36_8", "paired_64_w36_8", "conv_8x2_tiles_w36_8",
                                 "w36_one_wave_w36_8", "stacked_walk_w36_16"])
def test_w36_tile_walk(cid):
    """Cases above once more with FPC_W36_CUS = 8 (one of them 16): a generation-3 launch then has 8 (16) workgroups, XCD k's
    walking the tiles [k ceil(T / 8), (k + 1) ceil(T / 8)) -- several each, the last XCDs fewer or none -- where every other
    case of this file gives each workgroup one tile.  w36_one_wave runs three frames here: the detector's 8 x 32 tiles are 3
    per frame on a 22 x 26 map."""
    cap = int(CASES[cid][6]["FPC_W36_CUS"])
    run_case(cid, more_tiles_than=cap)


def test_latency_plan_persistent_layer1():
    """176 x 208, eleven frames on the default (latency) plan: wblock16_kernel<4, 8> on layer 1 has 6 x 4 tiles of 8 x 16 per
    44 x 52 map, 264 in the launch -- at least one per CU, from where the launch is persistent (persist_min_tiles = 1): one
    workgroup per CU, the first ones walking a second tile."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    run_case("latency_persistent_layer1", more_tiles_than=cus - 1)


# ---------------------------------------------------------------- kernels still shipped behind a flag
@pytest.mark.parametrize("cid", ["winograd_gen1", "winograd_gen2", "no_winograd", "no_fused_blocks", "tiles_round5", "w36_one_wave",
                                 "w36_one_wave_other_tiles", "detector_gen1", "stem_round3", "conv_round1"])
def test_alternative_plans(cid):
    """176 x 208, two frames, one flag each -- except where the flag alone does not reach its kernel there:
    FPC_PLAN_W36_ONE_WAVE and FPC_PLAN_DETECTOR_GEN1 act on the batch plan, which a two-frame call reaches with
    "no_latency_tiles" (as "winograd_gen2" and "tiles_round5" do); FPC_PLAN_STEM_ROUND3 acts only where stem_pool2_kernel
    would run, whole 16 x 16 tiles of the stem's map, so it runs at 160 x 192 x 1; and the one-wave kernels' other two
    instances (wblock36_kernel<1, 2, 8>, wblock36_dust_kernel<4, 4>) need maps such as 72 x 32 and 36 x 16: 288 x 128 x 1."""
    run_case(cid)


# ---------------------------------------------------------------- the split-operand modes (README: the same 1e-4)
@pytest.mark.parametrize("cid", ["split_bf16x3", "split_fp16x2"])
def test_split_operand_modes(cid):
    """176 x 208, three frames: dtype "f32_split" on block_x3_kernel, "f32_split_f16" on the same template's two-plane fp16
    instantiation, which the library names block_h2_kernel; both on stem_pool_x3_kernel."""
    run_case(cid)


# ---------------------------------------------------------------- the detector's 64 + 1 channels
def test_detector_65_channel_kernels_are_among_the_cases():
    """det.0 and det.1 are written by wblock36p_dust_kernel in both arrangements and by wblock36_dust_kernel in both in
    cases above (a failure there names channel 64 as chunk 1, lane 0: tests/test_layer_oracle.py)."""
    want = {"wblock36p_dust_kernel<2, 8, 3>": "stacked_walk", "wblock36p_dust_kernel<4, 4, 3>": "stacked_walk_other_seams",
            "wblock36_dust_kernel<2, 8>": "w36_one_wave", "wblock36_dust_kernel<4, 4>": "w36_one_wave_other_tiles"}
    for sym, cid in want.items():
        wrote = layer_check.layer_kernels(launches_of_case(cid))
        assert wrote["det.0"] == sym and wrote["det.1"] == sym, (cid, wrote["det.0"], wrote["det.1"])


# ---------------------------------------------------------------- coverage
def test_every_kernel_of_a_vga_call_is_covered():
    """Every convolution, block and stem symbol that a VGA call of 32 frames or of one frame launches on the default fp32
    plan (forwards only, no oracle) is exercised by a case above -- so no VGA-sized case is needed: the instances depend on
    the maps' tile counts, not on their size."""
    from fpc_amd.engine import Engine
    need = set()
    for n in (32, 1):
        e = Engine(480, 640, max_batch=n)
        try:
            e.load_state_dict(SD)
            need |= set(e.kernel_names(synth.make_batch(11, n, 480, 640)))
        finally:
            e.close()
    need = {k for k in need if not re.match(r"softmax|nms|descriptor16", k)}
    assert any(k.startswith("stem") for k in need) and any(k.startswith("wblock36s") for k in need), sorted(need)
    covered = set()
    for cid in CASES:
        covered |= {s for _, s in launches_of_case(cid)}
    assert need <= covered, sorted(need - covered)


