"""The layer-isolated bf16 check (oracle.bf16_layer_parts, oracle/layer_check.py::compare_bf16_layer / check_bf16_layers),
pinned on the CPU: the parts reproduce the emulation bit for bit, two stand-in devices -- the same layers in plain fp32, each
with an h rounded from its own accumulation -- pass every layer and frame with nothing over, and every planted fault is
reported at the right layer and frame: a mutation check of the check that tests/test_gpu_layer_isolated_bf16.py applies to the
device.  The last two faults are the gain over tests/test_gpu_parity.py::_check_bf16_layers: they fit inside its allowance
for a share of elements and are reported here.  CPU only."""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth
from oracle import layer_check, oracle

SD = synth.make_state_dict(3, dustbin_bias=4.0)
NAMES = ("pool",) + tuple(k for k, _ in oracle.BF16_LAYERS)
GRAPH = dict(oracle.BF16_LAYERS, pool=("frames",))
GEOMETRIES = [(160, 192, 2), (48, 80, 1)]
# tests/test_gpu_parity.py::_check_bf16_layers, its three constants
OLD_REL, OLD_EXACT, OLD_FLIPS = 1.25 * 2.0 ** -7, 1e-4, 0.005

_standins = {}


def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


def standin_of(h, w, n, quarters):
    """(frames, taps) of a stand-in device: every layer in plain torch fp32 (conv1 in `quarters` K-chunks) from the
    stand-in's OWN previous tensors, stored as the mode stores them.  Computed once, never written to."""
    key = (h, w, n, quarters)
    if key not in _standins:
        frames = synth.make_batch(11, n, h, w)
        taps = {"frames": frames}
        for name in NAMES:
            ins = [taps[i] for i in GRAPH[name]]
            out_f32 = name != "pool" and oracle._BF16_BLOCKS.get(name, (0, 0, 0, False))[3]
            taps[name] = layer_check.bf16_output_of(name, layer_check.torch_bf16_parts(name, ins, SD, quarters=quarters), out_f32)
        _standins[key] = (frames, _frozen(taps))
    return _standins[key]


class _TapEngine:
    """Stands in for a dtype="bf16" Engine whose last forward left `taps` in its workspace."""
    ACTIVATIONS = NAMES

    class _Tensor:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    def __init__(self, taps, descriptor_enabled=True):
        self.taps = taps
        self.descriptor_enabled = descriptor_enabled

    def activation(self, name, frame0=0, n=1):
        return self._Tensor(np.array(self.taps[name][frame0:frame0 + n]))


# ---------------------------------------------------------------- the parts are the emulation
def _stem_as_it_stood(image, sd):
    """oracle.bf16_emulated_stem before bf16_layer_parts, statement by statement."""
    image = np.ascontiguousarray(image, np.float32)
    s, t = oracle._fold(sd, "encoder.bn1")
    st = oracle._relu(oracle._conv2d(oracle.round_bf16(image), oracle._wq(sd["encoder.conv1.weight"], s), 2, 3) + oracle._bias(t))
    return oracle.maxpool3s2(st)


def _layer_as_it_stood(name, inputs, sd):
    """oracle.bf16_emulated_layer before bf16_layer_parts, statement by statement."""
    rb, conv, wq, fold, bias = oracle.round_bf16, oracle._conv2d, oracle._wq, oracle._fold, oracle._bias
    x = rb(np.ascontiguousarray(np.concatenate(inputs, 1) if len(inputs) > 1 else inputs[0], np.float32))
    if name == "up":
        s, t = fold(sd, "descriptor.bn")
        wt = rb((sd["descriptor.up_sample.weight"].astype(np.float64) * s[None, :, None, None]).astype(np.float32))
        bt = (sd["descriptor.up_sample.bias"].astype(np.float64) * s + t).astype(np.float32)
        b, _, h, w = x.shape
        up = np.empty((b, 128, 2 * h, 2 * w), np.float32)
        oracle.lib().oracle_conv_transpose2d(oracle._p(x), oracle._p(np.ascontiguousarray(wt)), oracle._p(bt), oracle._p(up), b, 256, h, w, 128)
        return rb(oracle._relu(up))
    p, stride, proj, out_f32 = oracle._BF16_BLOCKS[name]
    s1, t1 = fold(sd, p + ".bn1")
    s2, t2 = fold(sd, p + ".bn2")
    h = rb(oracle._relu(conv(x, wq(sd[p + ".conv1.weight"], s1), stride, 1) + bias(t1)))
    y = conv(h, wq(sd[p + ".conv2.weight"], s2), 1, 0)
    if proj:
        sp, tp = fold(sd, p + ".identity_downsample.1")
        y = y + conv(x, wq(sd[p + ".identity_downsample.0.weight"], sp), stride, 0) + bias(t2 + tp)
    else:
        y = y + bias(t2) + x
    y = oracle._relu(y)
    return y if out_f32 else rb(y)


@pytest.mark.parametrize("h,w,n", GEOMETRIES)
def test_parts_are_the_emulation_bit_for_bit(h, w, n):
    """bf16_emulated_stem / bf16_emulated_layer come out of bf16_layer_parts exactly as they stood before it, and the
    parts are consistent: h = round_bf16(relu(v)), the stored value = (round_bf16 of) relu(y), max-pooled for the stem."""
    frames, taps = standin_of(h, w, n, 1)
    for name in NAMES:
        ins = [np.array(taps[i]) for i in GRAPH[name]]
        parts = oracle.bf16_layer_parts(name, ins, SD)
        if name == "pool":
            now, then = oracle.bf16_emulated_stem(ins[0], SD), _stem_as_it_stood(ins[0], SD)
            from_parts = oracle.maxpool3s2(np.maximum(parts["y"], np.float32(0)))
        else:
            now, then = oracle.bf16_emulated_layer(name, ins, SD), _layer_as_it_stood(name, ins, SD)
            from_parts = np.maximum(parts["y"], np.float32(0))
            from_parts = from_parts if parts["out_f32"] else oracle.round_bf16(from_parts)
        assert now.dtype == then.dtype == np.float32 and now.shape == then.shape, name
        assert np.array_equal(now.view(np.uint32), then.view(np.uint32)), name
        assert np.array_equal(now.view(np.uint32), from_parts.view(np.uint32)), name
        assert parts["out_f32"] == (name == "det.1"), name
        if "h" in parts:
            assert np.array_equal(parts["h"], oracle.round_bf16(np.maximum(parts["v"], np.float32(0)))), name
            assert parts["w2"].shape[2:] == (1, 1) and parts["w2"].shape[1] == parts["h"].shape[1], name
            assert np.array_equal(parts["w2"], oracle.round_bf16(parts["w2"])), name
        else:
            assert name in ("pool", "up") and "v" not in parts, name


# ---------------------------------------------------------------- two stand-in devices pass, and not vacuously
@pytest.mark.parametrize("quarters", [1, 4])
@pytest.mark.parametrize("h,w,n", GEOMETRIES)
def test_standin_devices_pass_every_layer(h, w, n, quarters):
    """Plain torch fp32, and torch fp32 with conv1 accumulated in four K-quarters, each with h rounded from its own
    accumulation: zero elements outside their interval in every layer and frame (through check_bf16_layers itself); every EPS
    under the 1e-4 ceiling, at most 10 % of a bf16 layer's elements ambiguous, the logits' median delta under 1e-4."""
    frames, taps = standin_of(h, w, n, quarters)
    rows = []
    launches = [("encoder.conv1+bn1+relu+max_pool", "stem_k"), ("encoder.layer1.0", "a_k"), ("descriptor.up_sample", "u_k")]
    layer_check.check_bf16_layers(_TapEngine(taps), frames, SD, "stand-in q%d %dx%dx%d" % (quarters, h, w, n), launches=launches, rows=rows)
    assert [r["layer"] for r in rows] == list(NAMES)
    assert rows[0]["kernel"] == "stem_k" and rows[1]["kernel"] == "a_k" and rows[NAMES.index("up")]["kernel"] == "u_k" and rows[2]["kernel"] == "?"
    for r in rows:
        assert r["ok"] and r["n_over"] == 0 and r["frames_over"] == [], r["message"]
        assert 0 < r["eps_y"] <= layer_check.ATOL and r["eps_h"] <= layer_check.ATOL, r
        assert r["eps_y"] == layer_check.BF16_EPS_MARGIN * r["e_ref_y"] and r["eps_h"] == layer_check.BF16_EPS_MARGIN * r["e_ref_h"], r
        assert (r["eps_h"] > 0) == (r["layer"] not in ("pool", "up")), r
        if r["layer"] == "det.1":
            assert r["ambiguous"] is None and r["median_delta"] <= layer_check.ATOL and r["max_err"] <= layer_check.ATOL, r
        else:
            assert 0 < r["ambiguous"] <= layer_check.BF16_MAX_AMBIGUOUS and r["flips"] <= r["ambiguous"], r
    # a detector-only context: the descriptor head's tensors are not asked for
    rows = []
    det_only = {k: v for k, v in taps.items() if not (k.startswith("desc") or k == "up")}
    layer_check.check_bf16_layers(_TapEngine(det_only, descriptor_enabled=False), frames, SD, "detector only", rows=rows)
    assert [r["layer"] for r in rows] == ["pool", "layer1.0", "layer1.1", "layer2.0", "layer2.1", "det.0", "det.1"]


# ---------------------------------------------------------------- planted faults
def _trunc_bf16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def _bf16_ulp_up(x):
    """The next bf16 value above a positive bf16 value."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) + np.uint32(0x10000)).view(np.float32)


def _checked(name, ins):
    parts = oracle.bf16_layer_parts(name, ins, SD)
    eps_h, eps_y, _, _ = layer_check.bf16_eps(name, ins, SD, parts)
    return parts, eps_h, eps_y


def _standin_output(name, ins, parts):
    return layer_check.bf16_output_of(name, layer_check.torch_bf16_parts(name, ins, SD), parts["out_f32"])


def _old_check_passes(got, want):
    """The arithmetic of tests/test_gpu_parity.py::_check_bf16_layers on one layer."""
    rel = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)
    return float(rel.max()) < OLD_REL and float((rel > OLD_EXACT).mean()) < OLD_FLIPS


def test_comparator_flags_every_planted_fault():
    """160 x 192, two frames, every layer: an output computed from an input whose last column / last row is zeroed, two
    8 x 16 output tiles of frame 1 swapped, the two frames' outputs swapped, h truncated instead of rounded -- each is
    reported, with the layer, the frames and the position of the damage."""
    n = 2
    frames, taps = standin_of(160, 192, n, 1)
    for name in NAMES:
        ins = [np.array(taps[i]) for i in GRAPH[name]]
        parts, eps_h, eps_y = _checked(name, ins)
        clean = np.array(taps[name])
        rep = layer_check.compare_bf16_layer(name, clean, parts, eps_h, eps_y)
        assert rep["ok"] and rep["n_over"] == 0, rep["message"]
        ho, wo = clean.shape[2:]

        th, tw = min(8, ho // 2), min(16, wo // 2)     # 8 x 16 tiles where the map holds two each way (1/4 resolution)

        def failed(got, what, frames_over):
            rep = layer_check.compare_bf16_layer(name, got, parts, eps_h, eps_y, tile=(th, tw))
            tag = "%s, %s: %s" % (name, what, rep["message"])
            assert not rep["ok"] and rep["n_over"] > 0 and rep["layer"] == name and rep["message"].startswith(name + ":"), tag
            assert rep["frames_over"] == frames_over and rep["worst"][0] in frames_over, tag
            f, c, y, x = rep["worst"]
            for text in ("at frame %d channel %d (chunk of 64: %d, lane %d) y %d x %d" % (f, c, c // 64, c % 64, y, x),
                         "y mod 16 = %d, x mod 16 = %d" % (y % 16, x % 16), "accepted [", "emulation ",
                         "row %d col %d of %d x %d tile (%d, %d)" % (y % th, x % tw, th, tw, y // th, x // tw)):
                assert text in rep["message"], tag
            return rep

        for what, axis in (("last input column zeroed", 3), ("last input row zeroed", 2)):
            bad = [a.copy() for a in ins]
            for a in bad:
                a[(slice(None),) * axis + (-1,)] = 0
            rep = failed(_standin_output(name, bad, oracle.bf16_layer_parts(name, bad, SD)), what, [0, 1])
            # (the stem's 7 x 7 window and the pool reach two pooled cells in; a stride-1 layer one)
            assert rep["worst"][axis] >= (wo, ho)[axis == 2] - 3, (name, what, rep["message"])

        got = clean.copy()
        got[1, :, :th, :tw], got[1, :, th:2 * th, tw:2 * tw] = clean[1, :, th:2 * th, tw:2 * tw], clean[1, :, :th, :tw]
        rep = failed(got, "tiles (0, 0) and (1, 1) of frame 1 swapped", [1])
        assert (rep["worst"][2] // th, rep["worst"][3] // tw) in ((0, 0), (1, 1)), rep["message"]

        failed(np.ascontiguousarray(clean[::-1]), "frames 0 and 1 swapped", [0, 1])

        if "h" in parts:
            t = layer_check.torch_bf16_parts(name, ins, SD)
            t = layer_check.torch_bf16_parts(name, ins, SD, h=_trunc_bf16(np.maximum(t["v"], np.float32(0))))
            failed(layer_check.bf16_output_of(name, t, parts["out_f32"]), "h truncated instead of rounded", [0, 1])


def test_comparator_flags_a_swapped_k_chunk_and_the_65th_channel():
    frames, taps = standin_of(160, 192, 2, 1)
    # desc_out.0 reads [up | layer2.1], 256 channels: its first two 64-channel K-chunks swapped
    ins = [np.array(taps[i]) for i in GRAPH["desc_out.0"]]
    parts, eps_h, eps_y = _checked("desc_out.0", ins)
    x = np.concatenate(ins, 1)
    bad = np.concatenate([x[:, 64:128], x[:, 0:64], x[:, 128:]], 1)
    got = _standin_output("desc_out.0", [bad], parts)
    rep = layer_check.compare_bf16_layer("desc_out.0", got, parts, eps_h, eps_y)
    assert not rep["ok"] and rep["frames_over"] == [0, 1] and rep["n_over"] > got.size // 2, rep["message"]
    # the detector's 65th channel repeating its neighbour
    for name in ("det.0", "det.1"):
        ins = [np.array(taps[i]) for i in GRAPH[name]]
        parts, eps_h, eps_y = _checked(name, ins)
        got = np.array(taps[name])
        got[:, 64] = got[:, 63]
        rep = layer_check.compare_bf16_layer(name, got, parts, eps_h, eps_y)
        assert not rep["ok"] and rep["worst"][1] == 64 and rep["frames_over"] == [0, 1], rep["message"]
        assert "channel 64 (chunk of 64: 1, lane 0)" in rep["message"], rep["message"]


def test_faults_inside_the_old_allowance_are_reported():
    """On every bf16-stored block layer: the output truncated instead of rounded on 0.4 % of frame 1's elements, and one
    unambiguous element moved by one bf16 ulp.  Both pass the arithmetic of _check_bf16_layers (under its 0.5 % of elements,
    within its 1.25 * 2^-7 per element) and fail here, at frame 1 -- the second at exactly its element.  Shown through
    check_bf16_layers too, on the network's last tensor."""
    n = 2
    frames, taps = standin_of(160, 192, n, 1)
    rng = np.random.default_rng(5)
    for name in NAMES:
        if name in ("pool", "det.1"):   # (the stem's interval is pooled, the logits are fp32: no single bf16 rounding to plant)
            continue
        ins = [np.array(taps[i]) for i in GRAPH[name]]
        parts, eps_h, eps_y = _checked(name, ins)
        want = oracle.bf16_emulated_layer(name, ins, SD)
        clean = np.array(taps[name])
        assert _old_check_passes(clean, want), name

        # truncation on 0.4 % of one frame
        mine = np.maximum(layer_check.torch_bf16_parts(name, ins, SD)["y"], np.float32(0))
        pick = rng.random(clean[1].shape) < 0.004
        got = clean.copy()
        got[1][pick] = _trunc_bf16(mine[1])[pick]
        moved = int((got != clean).sum())
        # (half of the picked elements are zeros after the ReLU, half of the rest round down anyway)
        assert 20 <= moved <= pick.sum() <= 0.005 * clean[1].size, (name, moved)
        rep = layer_check.compare_bf16_layer(name, got, parts, eps_h, eps_y)
        assert _old_check_passes(got, want), name
        assert not rep["ok"] and rep["frames_over"] == [1] and 0.8 * moved <= rep["n_over"] <= moved, (name, moved, rep["message"])

        # one unambiguous element, one ulp
        delta = layer_check.bf16_delta(parts, eps_h, eps_y)
        lo = layer_check._rb_relu_outward(parts["y"], delta, False)
        hi = layer_check._rb_relu_outward(parts["y"], delta, True)
        cand = np.argwhere((lo[1] == hi[1]) & (clean[1] >= 0.5) & (clean[1] < 2.0))
        c, y, x = (int(v) for v in cand[len(cand) // 2])
        got = clean.copy()
        got[1, c, y, x] = _bf16_ulp_up(clean[1, c, y, x])[0]
        assert 0 < got[1, c, y, x] - clean[1, c, y, x] <= 2.0 ** -7
        rep = layer_check.compare_bf16_layer(name, got, parts, eps_h, eps_y)
        assert _old_check_passes(got, want), name
        assert not rep["ok"] and rep["n_over"] == 1 and rep["worst"] == (1, c, y, x) and rep["frames_over"] == [1], (name, rep["message"])

        if name == "desc_out.1":
            bad = dict(taps)
            bad[name] = got
            with pytest.raises(AssertionError) as exc:
                layer_check.check_bf16_layers(_TapEngine(bad), frames, SD, "one ulp", launches=[("descriptor.layer_out.1", "k_sym")])
            text = str(exc.value)
            assert text.startswith("one ulp [k_sym]: desc_out.1: 1 of ") and "frame(s) [1]" in text and text.count("\n") == 0, text


def test_what_the_check_refuses():
    """A reference outside the range the bar is stated for, a wrong shape, a value that is not finite, an EPS over the
    1e-4 ceiling, and a layer where too many intervals hold more than one bf16 value."""
    one = np.ones((1, 2, 2, 2), np.float32)
    parts = {"y": one.copy(), "out_f32": False}
    assert layer_check.compare_bf16_layer("up", one, parts, 0.0, 1e-6)["ok"]
    assert not layer_check.compare_bf16_layer("up", one * 41, {"y": one * 41, "out_f32": False}, 0.0, 1e-6)["ok"]
    assert not layer_check.compare_bf16_layer("up", np.ones((1, 2, 2, 3), np.float32), parts, 0.0, 1e-6)["ok"]
    for bad in (np.nan, np.inf, -np.inf):
        got = one.copy()
        got[0, 1, 1, 0] = bad
        for out_f32 in (False, True):
            rep = layer_check.compare_bf16_layer("up", got, dict(parts, out_f32=out_f32), 0.0, 1e-6)
            assert not rep["ok"] and rep["worst"] == (0, 1, 1, 0) and rep["n_over"] == 1, rep["message"]
    for eps_h, eps_y in ((0.0, 1.01e-4), (1.01e-4, 1e-6)):
        rep = layer_check.compare_bf16_layer("up", one, parts, eps_h, eps_y)
        assert not rep["ok"] and "ceiling" in rep["message"], rep["message"]
    # every y half-way between two bf16 values: every interval holds both, whatever the EPS
    mid = {"y": np.full((1, 2, 2, 2), 1.0 + 2.0 ** -8, np.float32), "out_f32": False}
    rep = layer_check.compare_bf16_layer("up", oracle.round_bf16(mid["y"]), mid, 0.0, 1e-6)
    assert not rep["ok"] and rep["n_over"] == 0 and rep["ambiguous"] == 1.0 and "too wide" in rep["message"], rep["message"]
    # the fp32 logits: |got - relu(y)| <= delta
    logit = {"y": one.copy(), "out_f32": True}
    assert layer_check.compare_bf16_layer("det.1", one + np.float32(5e-7), logit, 0.0, 1e-6)["ok"]
    assert not layer_check.compare_bf16_layer("det.1", one + np.float32(2e-6), logit, 0.0, 1e-6)["ok"]
