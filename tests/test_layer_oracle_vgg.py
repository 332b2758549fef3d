"""The layer-isolated reference of the C++ network (oracle.vgg_layer over oracle.VGG_LAYERS) and its comparator
(layer_check.check_vgg_layers / compare_band), pinned on the CPU: the chained layers agree with the whole-network oracle
and with fixture F7 (the reference binary's own output), and the comparison that tests/test_gpu_layer_isolated_vgg.py
applies to the device flags every planted fault at the right layer, frames and position.  CPU only."""
import math
import os

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import arch, synth
from oracle import layer_check, oracle

SPEC = arch.vgg_state_dict_spec()
SD = synth.make_vgg_state_dict(8, 3.0)
NAMES = tuple(k for k, _ in oracle.VGG_LAYERS)
GRAPH = dict(oracle.VGG_LAYERS)

_taps = {}


def gray(seed, n, h, w):
    return synth.make_batch(seed, n, h, w, gray=True)[:, :1].copy()


def chain(frames, sd):
    """Every tensor of VGG_LAYERS, each layer fed with the previous one's output."""
    tp = {"frames": frames}
    for name, ins in oracle.VGG_LAYERS:
        tp[name] = oracle.vgg_layer(name, [tp[i] for i in ins], sd)
    return tp


def taps_of(h, w, n):
    """The chained tensors of `n` frames, computed once per geometry and never written to."""
    if (h, w, n) not in _taps:
        tp = chain(gray(11, n, h, w), SD)
        for a in tp.values():
            a.setflags(write=False)
        _taps[(h, w, n)] = tp
    return _taps[(h, w, n)]


def test_the_names_are_the_engines():
    from fpc_amd.engine import Engine
    assert NAMES == Engine.VGG_ACTIVATIONS
    assert GRAPH["conv0_a"] == ("frames",) and GRAPH["det_a"] == GRAPH["desc_a"] == ("conv3_b",)
    for name, ins in oracle.VGG_LAYERS:     # every input is the frames or an earlier tensor
        assert all(i == "frames" or NAMES.index(i) < NAMES.index(name) for i in ins), name


@pytest.mark.parametrize("h,w,n", [(32, 48, 1), (176, 208, 2)])
def test_chained_layers_agree_with_the_whole_network_oracle(h, w, n):
    """Chained from the frames, the layers give oracle.vgg_forward's logits and descriptors within 1 ulp of the tensor's
    largest magnitude.  Measured: 0 at both sizes -- the whole-network oracle runs the same convolution, the same float
    bias and the same division by the float of a double norm, so nothing but the order of two float operations could
    differ; 1 ulp is the smallest bound that still says "the same arithmetic" without demanding bit equality."""
    tp = taps_of(h, w, n)
    _, desc, logits = oracle.vgg_forward(np.array(tp["frames"]), SD, SPEC)
    for name, want in (("det_b", logits), ("desc_b", desc)):
        got = tp[name]
        assert got.shape == want.shape, name
        bound = 2.0 ** -23 * 2.0 ** math.floor(math.log2(float(np.abs(want).max())))
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        print("%-7s max |tensor| %.3g  error %.3g  bound %.3g" % (name, np.abs(want).max(), err, bound))
        assert err <= bound, (name, err, bound)


def test_chained_layers_agree_with_the_reference_binary(golden_dir):
    """Fixture F7 (32 x 48) is the output of the reference's own C++ network: the chain reproduces its logits and
    descriptors within the project's 1e-4."""
    g = np.load(os.path.join(golden_dir, "f7_vgg_32x48.npz"))
    sd = synth.make_vgg_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    tp = chain(gray(int(g["seed_frame"]), 1, 32, 48), sd)
    np.testing.assert_allclose(tp["det_b"], g["logits"], rtol=0, atol=layer_check.ATOL)
    np.testing.assert_allclose(tp["desc_b"], g["desc"], rtol=0, atol=layer_check.ATOL)


def test_the_reference_stays_inside_the_range_of_the_bar():
    """The absolute 1e-4 applies while max |reference| <= 40: every layer of both weight sets the GPU tests may use stays
    between 2 and 8 there, and the smallest descriptor norm before normalisation is above 3."""
    for sd in (SD, synth.make_vgg_state_dict(3, 4.0)):
        tp = chain(gray(11, 2, 160, 192), sd)
        for name in NAMES:
            if name != "desc_b":
                assert 2.0 < float(np.abs(tp[name]).max()) < 8.0, (name, float(np.abs(tp[name]).max()))
        p, k, _ = oracle._VGG_CONVS["desc_b"]
        raw = oracle._conv2d(tp["desc_a"], sd[p + ".weight"], 1, 0) + oracle._bias(sd[p + ".bias"])
        assert float(np.linalg.norm(raw.astype(np.float64), axis=1).min()) > 3.0


class _TapEngine:
    """Stands in for an arch="vgg" Engine whose last forward left `taps` in its workspace."""
    VGG_ACTIVATIONS = NAMES

    class _Tensor:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    def __init__(self, taps):
        self.taps = taps

    def activation(self, name, frame0=0, n=1):
        return self._Tensor(np.array(self.taps[name][frame0:frame0 + n]))


def _last_col(a):
    a[..., -1] = 0


def _last_row(a):
    a[..., -1, :] = 0


def _seam(a):
    a[1, :, 0, :] = a[0, :, -1, :]


def _k_chunk(a):
    a[:, 64:128] = 0


def _from_damaged_input(name, tp, damage):
    x = np.array(tp[GRAPH[name][0]])
    damage(x)
    return oracle.vgg_layer(name, [x], SD)


def test_comparator_flags_every_planted_fault():
    """160 x 192, three frames.  The clean tensors pass check_vgg_layers on a stand-in engine with zero elements over the
    bar; each planted fault is reported with its layer, frames and position: an output computed from an input whose last
    column or row is zeroed (a full-resolution layer and a 1/8 one), from a row leaked across the stacked seam, from input
    channels 64..127 zeroed; a 256-output layer whose channels 64..127 repeat channels 0..63 (a misplaced part); a pool
    that ignores the odd row; desc_b left un-normalised; conv0_a with replicated padding; det_b's channel 64 repeating
    channel 63."""
    n, h, w = 3, 160, 192
    tp = taps_of(h, w, n)
    rows = []
    launches = [("encoder_conv0_a [conv+bias+relu, 1 input channel]", "c0_k"), ("encoder_conv0_b [winograd conv+bias+relu]", "w_k"),
                ("max_pool2d(2,2) after encoder_conv0_b", "pool_k"), ("max_pool2d(2,2) after encoder_conv1_b", "pool_k"),
                ("detector_conv_a [winograd conv+bias+relu, channels 0..127]", "p_k"),
                ("detector_conv_a [winograd conv+bias+relu, channels 128..255]", "p_k"),
                ("descriptor_conv_a [winograd conv+bias+relu, 4 parts of 64 channels]", "q_k"),
                ("descriptor_conv_b [conv+bias]", "one_k"), ("descriptor L2 normalisation over channels", "norm_k")]
    layer_check.check_vgg_layers(_TapEngine(tp), np.array(tp["frames"]), SD, "clean", launches=launches, rows=rows)
    assert [r["layer"] for r in rows] == list(NAMES)
    kern = {r["layer"]: r["kernel"] for r in rows}
    assert kern["conv0_a"] == "c0_k" and kern["conv0_b"] == "w_k" and kern["pool0"] == kern["pool1"] == "pool_k"
    assert kern["det_a"] == "p_k" and kern["desc_b"] == "one_k + norm_k" and kern["pool2"] == kern["conv1_a"] == "?"
    assert layer_check.vgg_layer_ops(launches)["desc_a"] == ["descriptor_conv_a [winograd conv+bias+relu, 4 parts of 64 channels]"]
    for r in rows:     # a plain fp32 re-computation is itself inside the bar; the clean tensors ARE the reference
        assert r["e_ref"] < layer_check.ATOL and r["max_err"] == 0.0, r
        assert (r["e_ref"] > 0) == (not r["layer"].startswith("pool")), r

    def flagged(name, got, frames=None):
        rep = layer_check.compare_layer(name, got, tp[name])
        tag = "%s: %s" % (name, rep["message"])
        assert not rep["ok"] and rep["n_over"] > 0 and rep["layer"] == name and rep["message"].startswith(name + ":"), tag
        assert rep["frames_over"] == (list(range(n)) if frames is None else frames), tag
        f, c, y, x = rep["worst"]
        assert "y mod 16 = %d, x mod 16 = %d" % (y % 16, x % 16) in rep["message"], tag
        return rep, tag

    for name in ("conv0_b", "conv3_b", "det_a"):       # a full-resolution layer and two at 1/8
        ho, wo = tp[name].shape[2:]
        rep, tag = flagged(name, _from_damaged_input(name, tp, _last_col))
        assert rep["worst"][3] >= wo - 2, tag
        rep, tag = flagged(name, _from_damaged_input(name, tp, _last_row))
        assert rep["worst"][2] >= ho - 2, tag
        rep, tag = flagged(name, _from_damaged_input(name, tp, _seam), frames=[1])
        assert rep["worst"][0] == 1 and rep["worst"][2] <= 1, tag
        assert "row %d of the stacked image" % (ho + rep["worst"][2]) in rep["message"], tag
    for name in ("conv2_b", "conv3_a", "det_a", "det_b", "desc_b"):   # every K >= 128, 3 x 3 and 1 x 1
        flagged(name, _from_damaged_input(name, tp, _k_chunk))
    for name in ("det_a", "desc_a"):
        got = np.array(tp[name])
        got[:, 64:128] = got[:, 0:64]
        rep, tag = flagged(name, got)
        assert 64 <= rep["worst"][1] < 128 and "(chunk of 64: 1, lane %d)" % (rep["worst"][1] - 64) in rep["message"], tag
        over = np.abs(got - tp[name]) > layer_check.ATOL
        assert not over[:, :64].any() and not over[:, 128:].any()
    for name in ("pool0", "pool2"):
        x = tp[GRAPH[name][0]]
        flagged(name, np.maximum(x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2]))
    p = oracle._VGG_CONVS["desc_b"][0]
    flagged("desc_b", oracle._conv2d(tp["desc_a"], SD[p + ".weight"], 1, 0) + oracle._bias(SD[p + ".bias"]))
    edge = np.pad(np.array(tp["frames"]), ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
    q = oracle._VGG_CONVS["conv0_a"][0]
    got = oracle._relu(oracle._conv2d(edge, SD[q + ".weight"], 1, 0) + oracle._bias(SD[q + ".bias"]))
    rep, tag = flagged("conv0_a", got)
    f, c, y, x = rep["worst"]
    assert y in (0, h - 1) or x in (0, w - 1), tag
    inner = np.abs(got - tp["conv0_a"])[:, :, 1:-1, 1:-1]
    assert float(inner.max()) == 0.0
    got = np.array(tp["det_b"])
    got[:, 64] = got[:, 63]
    rep, tag = flagged("det_b", got)
    assert rep["worst"][1] == 64 and "channel 64 (chunk of 64: 1, lane 0)" in rep["message"], tag


def test_band_comparison():
    """compare_band: a reference computed from rows [a, b) of the input alone agrees with the whole layer on the rows whose
    3 x 3 support lies inside the band or on the frame's true edge -- and on no more: the band's first and last row do
    not (unless they are the frame's), so a band check that compared them would fail on a correct tensor.  A fault inside
    the compared rows is reported at its frame row."""
    tp = taps_of(160, 192, 3)
    h = 160
    assert layer_check.band_rows(0, 24, h) == (0, 23) and layer_check.band_rows(68, 92, h) == (69, 91)
    assert layer_check.band_rows(136, 160, h) == (137, 160)
    for name in ("conv0_a", "conv0_b"):
        x, full = tp[GRAPH[name][0]], tp[name]
        for a, b in ((0, 24), (68, 92), (136, 160)):
            want = oracle.vgg_layer(name, [x[:, :, a:b]], SD)
            rep = layer_check.compare_band(name, full[:, :, a:b], want, a, b, h)
            assert rep["ok"] and rep["max_err"] == 0.0 and rep["rows"] == layer_check.band_rows(a, b, h), rep["message"]
            whole = layer_check.compare_layer(name, full[:, :, a:b], want)
            assert not whole["ok"] and whole["worst"][2] in ([b - a - 1] if a == 0 else [0] if b == h else [0, b - a - 1])
            lo, hi = rep["rows"]
            bad = np.array(full[:, :, a:b])
            bad[2, 5, hi - 1 - a, 7] += 1.0
            rep = layer_check.compare_band(name, bad, want, a, b, h)
            assert not rep["ok"] and rep["n_over"] == 1 and rep["worst"] == (2, 5, hi - 1, 7) and rep["frames_over"] == [2], rep["message"]
    wrong = layer_check.compare_band("conv0_a", np.zeros((1, 64, 23, 8), np.float32), np.zeros((1, 64, 24, 8), np.float32), 0, 24, h)
    assert not wrong["ok"] and "shape" in wrong["message"]
