"""Layer-isolated float64 parity of the C++ network's kernels (arch="vgg", pytest -m gpu): tests/test_gpu_layer_isolated.py
for superpoint::SPModel.

After a forward, every tensor of Engine.VGG_ACTIVATIONS is read back, every layer is computed once more from the DEVICE'S
OWN input tensor by oracle.vgg_layer (double accumulation; the pools exact; the descriptor's norm in double), and the
device's output must agree within 1e-4 at every element of EVERY frame (layer_check.check_vgg_layers;
tests/test_layer_oracle_vgg.py shows on the CPU that this comparison flags a dropped column, row or K-chunk, a leak across
a stacked seam, a misplaced 64-channel part, a pool that skips a row, a missing normalisation, a wrong padding and a wrong
65th channel).  Three max-pools and the ReLUs behind the full-resolution layers can hide such a fault from a bound at the
heads; here nothing compounds across layers.

Each case sits at the smallest geometry that reaches the kernel it is there for, and asserts that this kernel wrote the
tensors named.  Every case prints, per layer, the device's error over the error of the same layer in plain fp32 on the CPU
(E_ref); nothing is asserted from that ratio -- DESIGN.md keeps the measured table.

Weights: synth.make_vgg_state_dict(8, 3.0); frames: the gray plane of synth.make_batch(11, n, h, w, gray=True); fp32.
"""
import re

import numpy as np
import pytest
import torch

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth
from oracle import layer_check, oracle

pytestmark = pytest.mark.gpu

SD = synth.make_vgg_state_dict(8, 3.0)
NLT = "no_latency_tiles"
INVALID = -1                             # FPC_E_INVALID (include/fpc.h)
W64 = "wblock36p_kernel<4, 4, 3>"        # generation 3, conv-only, 64 channels: 4 x 4 Winograd tiles ...
W64_2X8 = "wblock36p_kernel<2, 8, 3>"    # ... and 2 x 8
W128 = "wblock36_kernel<2, 4, 4>"
W128_2X8 = "wblock36_kernel<2, 2, 8>"
STACKED = "wblock36s_kernel<2, 4, 4>"
DET_1X1 = "conv_mfma_kernel<6, 20, 1, 1, 64, 4, 1, 1, 3>"
DESC_1X1 = "conv_mfma_kernel<6, 20, 1, 1, 64, 2, 2, 2, 2>"

_frames = {}


def frames_of(h, w, n):
    if (h, w) not in _frames or len(_frames[(h, w)]) < n:
        _frames[(h, w)] = synth.make_batch(11, n, h, w, gray=True)[:, :1].copy()
    return _frames[(h, w)][:n]


def vgg_engine(h, w, n, **kw):
    from fpc_amd.engine import Engine
    return Engine(h, w, max_batch=n, in_channels=1, arch="vgg", **kw)


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


FULL = ("conv0_b",)                          # 64 channels on the frame's own size
HALF = ("conv1_a", "conv1_b")                # 64 channels at 1/2
C64 = FULL + HALF
QUARTER = ("conv2_a", "conv2_b")             # 128 channels at 1/4
EIGHTH = ("conv3_a", "conv3_b")              # 128 channels at 1/8
HEADS = ("det_a", "desc_a")                  # 256 channels at 1/8, in parts
C128 = QUARTER + EIGHTH + HEADS
POOLS = ("pool0", "pool1", "pool2")
OWN = {"vgg_conv0_kernel": ("conv0_a",), "maxpool2_kernel": POOLS, "l2norm256_kernel": ("desc_b",)}
ONE = {DET_1X1: ("det_b",), DESC_1X1: ("desc_b",)}
TWO_PARTS = {t: ("2 parts of 128 channels",) for t in HEADS}     # ONE launch, gridDim.y = 2
FOUR_PARTS = {t: ("4 parts of 64 channels",) for t in HEADS}
# id -> (h, w, frames, Engine keywords, {kernel the case is there for: the tensors it must have written}, kernels that must
#        NOT run, {tensor: what the op names of its launches must say, one entry per launch})
CASES = {
    "stacked": (160, 192, 5, dict(plan_flags=[NLT]), {W64: C64, STACKED: EIGHTH + HEADS, "wblock36*_kernel<2, 4, 4>": QUARTER, **OWN, **ONE}, [], TWO_PARTS),
    "ragged": (176, 208, 2, dict(plan_flags=[NLT]), {W64: C64, W128: QUARTER, W128_2X8: EIGHTH + HEADS, **OWN, **ONE}, [STACKED], TWO_PARTS),
    "ragged_8": (168, 200, 2, dict(plan_flags=[NLT]), {W64: C64, W128: QUARTER, W128_2X8: EIGHTH + HEADS, **OWN, **ONE}, [STACKED], TWO_PARTS),
    "four_parts": (64, 96, 2, dict(plan_flags=[NLT]), {W64: C64 + HEADS, W128: QUARTER + EIGHTH, **OWN, **ONE}, [], FOUR_PARTS),
    "tiles_2x8": (144, 64, 1, dict(plan_flags=[NLT]), {W64_2X8: HALF, W64: FULL, **OWN}, [], {}),
    "tiles_2x8_128": (288, 128, 1, dict(plan_flags=[NLT]), {W128_2X8: QUARTER, W64: C64, W128: EIGHTH + HEADS, **OWN}, [W64_2X8], TWO_PARTS),
    "latency_1": (160, 192, 1, dict(), {"wblock16_kernel<4, 8>": C64, "wblock16_kernel<8, 8>": C128, **OWN, **ONE}, ["wblock36*"], TWO_PARTS),
    "latency_2": (176, 208, 2, dict(), {"wblock16_kernel<4, 8>": C64, "wblock16_kernel<8, 8>": C128, **OWN, **ONE}, ["wblock36*"], TWO_PARTS),
    "winograd_gen1": (176, 208, 2, dict(plan_flags=["winograd_gen1"]), {"wblock_mfma_kernel<32, 2, 64>": C64, "wblock_mfma_kernel<32, 4, 128>": C128, **OWN},
                      ["wblock36*", "wblock16*"], {t: ("channels 0..127", "channels 128..255") for t in HEADS}),
    "winograd_gen2": (176, 208, 2, dict(plan_flags=["winograd_gen2", NLT]), {"wblock16_kernel<4, 8>": C64, "wblock16_kernel<8, 8>": C128, **OWN}, ["wblock36*"], TWO_PARTS),
    "no_winograd": (176, 208, 2, dict(plan_flags=["no_winograd"]), {"conv_mfma_kernel<8, 16, 1, 3, *": C64, "conv_mfma_kernel<6, 20, 1, 3, *": C128, **OWN, **ONE}, ["w*"], {}),
    "split_bf16x3": (176, 208, 3, dict(dtype="f32_split"), {"block_x3_kernel<8, 16, 1, 3, *": C64, "block_x3_kernel<6, 20, 1, 3, *": QUARTER + EIGHTH,
                                                            "block_x3_kernel<3, 20, 1, 3, *": HEADS, "block_x3_kernel<6, 20, 1, 1, *": ("det_b",),
                                                            "block_x3_kernel<3, 20, 1, 1, *": ("desc_b",), **OWN}, ["w*", "conv_mfma*"], {}),
    "split_fp16x2": (176, 208, 3, dict(dtype="f32_split_f16"), {"block_h2_kernel<8, 16, 1, 3, *": C64, "block_h2_kernel<6, 20, 1, 3, *": QUARTER + EIGHTH,
                                                                "block_h2_kernel<3, 20, 1, 3, *": HEADS, "block_h2_kernel<6, 20, 1, 1, *": ("det_b",),
                                                                "block_h2_kernel<3, 20, 1, 1, *": ("desc_b",), **OWN}, ["w*", "conv_mfma*"], {}),
    "no_descriptor": (168, 200, 2, dict(plan_flags=[NLT], descriptor_enabled=False), {W64: C64, W128_2X8: EIGHTH + ("det_a",), DET_1X1: ("det_b",),
                                                                                      "vgg_conv0_kernel": ("conv0_a",), "maxpool2_kernel": POOLS},
                      ["l2norm256_kernel"], {"det_a": ("2 parts of 128 channels",)}),
}
_launches = {}     # case id -> [(op name, kernel symbol)] of its forward


def launches_of_case(cid, engine=None):
    """The launches of case `cid`: as recorded when it ran, or (the case deselected) from a forward of its own."""
    if cid not in _launches:
        h, w, n, kw = CASES[cid][:4]
        e = engine or vgg_engine(h, w, n, **kw)
        try:
            if engine is None:
                e.load_state_dict(SD)
            _launches[cid] = launches_of(e, frames_of(h, w, n))
        finally:
            if engine is None:
                e.close()
    return _launches[cid]


def run_case(cid):
    h, w, n, kw, there_for, absent, op_says = CASES[cid]
    frames = frames_of(h, w, n)
    e = vgg_engine(h, w, n, **kw)
    try:
        e.load_state_dict(SD)
        launches = launches_of_case(cid, e)
        kernels = [s for _, s in launches]
        wrote, ops = layer_check.vgg_layer_kernels(launches), layer_check.vgg_layer_ops(launches)
        wrong = []       # every finding of the case in one failure: which kernel wrote what, then the numbers
        for k, tensors in there_for.items():
            if not ran(kernels, k):
                wrong.append("%s: %s did not run: %s" % (cid, k, sorted(set(kernels))))
            wrong += ["%s: %s was written by %s, not by %s" % (cid, t, wrote[t], k) for t in tensors if not ran(wrote[t].split(" + "), k)]
        wrong += ["%s: %s ran" % (cid, k) for k in absent if ran(kernels, k)]
        for t, says in op_says.items():      # a layer in parts is ONE launch (gridDim.y parts) whose op name counts them
            if len(ops[t]) != len(says) or not all(s in op for s, op in zip(says, ops[t])):
                wrong.append("%s: %s by the launches %s, expected %s" % (cid, t, ops[t], says))
        names = e.VGG_ACTIVATIONS
        if not kw.get("descriptor_enabled", True):
            names = tuple(t for t in names if not t.startswith("desc"))
            for t in ("desc_a", "desc_b"):
                with pytest.raises(_lib.FpcError) as refused:
                    e.activation(t, 0, 1)
                assert refused.value.code == INVALID
        e.forward(frames)
        try:
            layer_check.check_vgg_layers(e, frames, SD, "%s %dx%dx%d" % (cid, h, w, n), launches=launches, names=names)
        except AssertionError as failed:
            wrong.append(str(failed))
        assert not wrong, "\n".join(wrong)
    finally:
        e.close()


# ---------------------------------------------------------------- the taps themselves
def test_taps_shapes_and_the_two_outputs():
    """All 15 names with the shapes of the reference's modules; "det_b" is bit-equal to forward's logits and "desc_b" to
    its descriptor map, for a frame range that does not start at 0 too; unknown names and the Python network's names are
    refused, and so are this network's names on a Python-network engine."""
    from fpc_amd.engine import Engine
    h, w, n = 64, 96, 3
    frames = frames_of(h, w, n)
    e = vgg_engine(h, w, n)
    try:
        e.load_state_dict(SD)
        _, desc, logits = e.forward(frames)
        shapes = {}
        for lv, (a, b, p, c) in enumerate((("conv0_a", "conv0_b", "pool0", 64), ("conv1_a", "conv1_b", "pool1", 64),
                                           ("conv2_a", "conv2_b", "pool2", 128), ("conv3_a", "conv3_b", None, 128))):
            shapes[a] = shapes[b] = (c, h >> lv, w >> lv)
            if p:
                shapes[p] = (c, h >> (lv + 1), w >> (lv + 1))
        shapes.update(det_a=(256, h // 8, w // 8), desc_a=(256, h // 8, w // 8), det_b=(65, h // 8, w // 8), desc_b=(256, h // 8, w // 8))
        assert tuple(shapes) and set(shapes) == set(Engine.VGG_ACTIVATIONS) and len(Engine.VGG_ACTIVATIONS) == 15
        for name in Engine.VGG_ACTIVATIONS:
            assert tuple(e.activation(name, 0, n).shape) == (n,) + shapes[name], name
            assert tuple(e.activation(name, 2, 1).shape) == (1,) + shapes[name], name
        for f0, k in ((0, n), (1, 2)):
            assert torch.equal(e.activation("det_b", f0, k).view(torch.int32), logits[f0:f0 + k].view(torch.int32))
            assert torch.equal(e.activation("desc_b", f0, k).view(torch.int32), desc[f0:f0 + k].view(torch.int32))
        for bad in Engine.ACTIVATIONS + ("conv4_a", "", "conv0_a "):
            with pytest.raises(_lib.FpcError, match=r"\(-1\)"):
                e.activation(bad, 0, 1)
        with pytest.raises(_lib.FpcError, match=r"\(-1\)"):
            e.activation("conv0_a", 2, 2)        # frames 2 and 3 of a 3-frame context
    finally:
        e.close()
    r = Engine(64, 96, max_batch=1)
    try:
        for bad in Engine.VGG_ACTIVATIONS:
            with pytest.raises(_lib.FpcError, match=r"\(-1\)"):
                r.activation(bad, 0, 1)
    finally:
        r.close()


# ---------------------------------------------------------------- the batch plan ("no_latency_tiles": calls of a few frames reach it)
def test_stacked_walk():
    """160 x 192, five frames: conv-only 64-channel generation-3 launches on 160 x 192 and 80 x 96 maps, 128-channel ones on
    40 x 48, and the 20 x 24 maps of conv3_a / conv3_b and of the heads' 3 x 3 layers walked stacked (100 rows: seams 4, 8
    and 12 rows into a tile); det_a and desc_a as ONE launch of two 128-channel parts each."""
    run_case("stacked")


def test_ragged_on_every_level():
    """176 x 208, two frames: maps of 176 x 208, 88 x 104, 44 x 52 and 22 x 26 -- partial 16 x 16 tiles on three levels, and
    22 x 26 on 8 x 32 tiles partial both ways."""
    run_case("ragged")


def test_ragged_multiples_of_8():
    """168 x 200, two frames: multiples of 8 but not of 16, so the full-resolution 64-channel walk has partial tiles too;
    maps down to 21 x 25 (odd both ways)."""
    run_case("ragged_8")


def test_four_parts_of_64_channels():
    """64 x 96, two frames: the 8 x 12 map is one 16 x 16 tile, where det_a and desc_a run as FOUR 64-channel parts in one
    launch of the 64-channel instance.  Every channel of every part is compared: parts 1..3 writing over part 0, or a part
    landing 64 channels off, fails channels 0..63 or the part's own (tests/test_layer_oracle_vgg.py plants exactly that)."""
    run_case("four_parts")


@pytest.mark.parametrize("cid", ["tiles_2x8", "tiles_2x8_128"])
def test_2x8_tile_arrangement_of_a_72x32_map(cid):
    """A 72 x 32 map is 9 tiles of 8 x 32 against 10 of 16 x 16.  At 144 x 64 it is the 64-channel map of conv1_a / conv1_b:
    the only conv-only launches on wblock36p_kernel<2, 8, 3>.  At 288 x 128 -- where the Python network's 64-channel
    layer1 takes that arrangement -- this network's 72 x 32 map is the 128-channel one of conv2_a / conv2_b
    (wblock36_kernel<2, 2, 8>), and its 64-channel maps, 288 x 128 and 144 x 64, tie and stay on 4 x 4."""
    run_case(cid)


# ---------------------------------------------------------------- the latency plan (the default for calls of a few frames)
@pytest.mark.parametrize("cid", ["latency_1", "latency_2"])
def test_latency_plan(cid):
    """Default flags, one frame at 160 x 192 and two at 176 x 208: the conv-only generation-2 instances, 64 and 128
    channels, the heads' 3 x 3 layers as two 128-channel parts."""
    run_case(cid)


# ---------------------------------------------------------------- kernels still shipped behind a flag, the split-operand modes, no descriptor head
@pytest.mark.parametrize("cid", ["winograd_gen1", "winograd_gen2", "no_winograd", "split_bf16x3", "split_fp16x2", "no_descriptor"])
def test_alternative_plans_and_modes(cid):
    """176 x 208: generation 1 (a 256-channel layer as two launches), generation 2 on the batch plan, the plain
    conv_mfma_kernel 3 x 3 and both of its 1 x 1 instances, the split-operand add_fconv instances (3 x 3 with 64, 128 and
    256 outputs, 1 x 1 with 65 and 256); 168 x 200 with the descriptor head disabled: the desc_* taps are refused, the
    other thirteen checked."""
    run_case(cid)


# ---------------------------------------------------------------- more than one launch per layer
def test_full_resolution_layer_in_two_launches():
    """960 x 1280, eight frames in one sub-batch: a frame's 64-channel full-resolution tensor is 314 572 800 bytes, of which
    (0x7fffff00 - 1) // 314 572 800 = 6 fit generation 3's 32-bit offsets, so encoder_conv0_b runs as launches of 6 + 2
    frames -- the second launch (and any g0 > 0 of launch_wblock's loop) is reached by nothing smaller.  Frames 5 (the
    first launch's last), 6 and 7 (the second launch's) are checked: conv0_a and conv0_b in three 24-row bands each (top,
    middle, bottom; layer_check.compare_band), and the final logits bit for bit against frame-by-frame calls."""
    h, w, n, band = 960, 1280, 8, 24
    assert (0x7fffff00 - 1) // (h * w * 64 * 4) == 6
    base = synth.make_batch(11, 1, h, w, gray=True)[:, :1]
    frames = np.concatenate([np.roll(base, (37 * i, 91 * i), axis=(2, 3)) for i in range(n)])     # eight different frames
    e = vgg_engine(h, w, n, plan_flags=[NLT], min_sub_batch=n)
    try:
        e.load_state_dict(SD)
        launches = launches_of(e, frames)
        wrote = layer_check.vgg_layer_kernels(launches)
        assert wrote["conv0_b"] == W64 and wrote["conv0_a"] == "vgg_conv0_kernel", wrote
        logits = e.forward(frames)[2][5:].cpu().numpy()
        failures = []
        for f in (5, 6, 7):
            a_dev = e.activation("conv0_a", f, 1)
            b_dev = e.activation("conv0_b", f, 1)
            for a in (0, (h - band) // 2, h - band):
                b = a + band
                x0, x1, x2 = frames[f:f + 1, :, a:b], a_dev[:, :, a:b].cpu().numpy(), b_dev[:, :, a:b].cpu().numpy()
                for name, x, got in (("conv0_a", x0, x1), ("conv0_b", x1, x2)):
                    rep = layer_check.compare_band(name, got, oracle.vgg_layer(name, [x], SD), a, b, h)
                    print("layer-isolated | two_launches 960x1280x8 frame %d rows %d..%d | %s | %s | max err %.3e | rel %.3e" % (
                        f, a, b - 1, name, wrote[name], rep["max_err"], rep["rel"]))
                    if not rep["ok"]:
                        failures.append("frame %d [%s]: %s" % (f, wrote[name], rep["message"]))
            del a_dev, b_dev
        assert not failures, "\n".join(failures)
        for f in (5, 6, 7):
            one = e.forward(frames[f:f + 1])[2].cpu().numpy()
            assert np.array_equal(one.view(np.int32), logits[f - 5:f - 4].view(np.int32)), f
    finally:
        e.close()


def test_generation_2_plan_beyond_its_32_bit_offsets_is_refused():
    """wblock16_kernel addresses its input from the batch's frame 0 with unsigned 32-bit byte offsets: at 256 bytes per
    frame pixel, thirteen 960 x 1280 frames are in reach and the fourteenth is not.  A "winograd_gen2" context of 14 such
    frames is refused by fpc_create before anything is allocated; so is the default plan where one frame is too large for
    generation 3 (2896 x 3328: 9.6 M pixels x 256 bytes) and two of them are beyond generation 2."""
    assert 0xfffffff0 // (960 * 1280 * 256) == 13
    with pytest.raises(_lib.FpcError, match=r"\(-1\)"):
        vgg_engine(960, 1280, 14, plan_flags=["winograd_gen2"])
    assert 2896 * 3328 * 256 >= 0x7fffff00 and 2 * 2896 * 3328 * 256 > 0xfffffff0
    with pytest.raises(_lib.FpcError, match=r"\(-1\)"):
        vgg_engine(2896, 3328, 2)


# ---------------------------------------------------------------- coverage
def test_every_kernel_of_a_vga_call_is_covered():
    """Every convolution, pool and normalisation symbol that a VGA call of 32 frames or of one frame launches on the
    default fp32 plan (forwards only, no oracle) is exercised by a case above: the instances depend on the maps' tile
    counts, not on their size."""
    need = set()
    for n in (32, 1):
        e = vgg_engine(480, 640, n)
        try:
            e.load_state_dict(SD)
            need |= set(e.kernel_names(frames_of(480, 640, n)))
        finally:
            e.close()
    need = {k for k in need if not re.match(r"softmax|nms|descriptor16", k)}
    assert {"vgg_conv0_kernel", "maxpool2_kernel", "l2norm256_kernel"} <= need and any(k.startswith("wblock36s") for k in need), sorted(need)
    covered = set()
    for cid in CASES:
        covered |= {s for _, s in launches_of_case(cid)}
    assert need <= covered, sorted(need - covered)
