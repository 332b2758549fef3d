"""The layer-isolated fp32 reference (oracle.f32_stem / oracle.f32_layer) and its comparator (oracle/layer_check.py),
pinned on the CPU: the reference agrees with the whole-network oracle and with the source project's own forward hooks, and
the comparator that tests/test_gpu_layer_isolated.py applies to the device flags every planted fault at the right layer
and frame -- a mutation check of the check itself.  CPU only."""
import math
import os

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import arch, synth
from oracle import layer_check, oracle

SPEC = arch.state_dict_spec()
SD = synth.make_state_dict(3, dustbin_bias=4.0)

_taps = {}


def taps_of(h, w, n):
    """(frames, taps of the whole-network oracle), computed once per geometry and never written to."""
    if (h, w, n) not in _taps:
        frames = synth.make_batch(11, n, h, w)
        tp = oracle.forward(frames, SD, SPEC, with_taps=True)[3]
        for a in tp.values():
            a.setflags(write=False)
        frames.setflags(write=False)
        _taps[(h, w, n)] = (frames, tp)
    return _taps[(h, w, n)]


@pytest.mark.parametrize("h,w,n", [(32, 48, 1), (160, 192, 3), (176, 208, 2)])
def test_reference_agrees_with_the_whole_network_oracle(h, w, n):
    """Fed with the taps of oracle.forward, every layer reproduces the next tap within 4 ulp of the tensor's largest
    magnitude (2 measured): the only difference is BatchNorm folded into the weights against BatchNorm applied after the
    convolution."""
    frames, tp = taps_of(h, w, n)
    for name in ("pool",) + tuple(k for k, _ in oracle.LAYERS):
        ins = [frames] if name == "pool" else [tp[i] for i in dict(oracle.LAYERS)[name]]
        got = layer_check.reference_layer(name, ins, SD)
        want = tp[name]
        assert got.shape == want.shape, name
        bound = 4 * 2.0 ** -23 * 2.0 ** math.floor(math.log2(float(np.abs(want).max())))
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        print("%-10s max |tap| %.3g  error %.3g  bound %.3g" % (name, np.abs(want).max(), err, bound))
        assert err <= bound, (name, err, bound)


def test_reference_agrees_with_the_source_projects_taps(golden_dir):
    """Fixture F1 holds forward hooks on the source project's own modules: fed with its tap_* tensors, the reference
    reproduces every next one within the project's 1e-4."""
    g = np.load(os.path.join(golden_dir, "f1_layers_32x48.npz"))
    sd = synth.make_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    frame = synth.make_batch(int(g["seed_frame"]), 1, int(g["h"]), int(g["w"]))
    for name in ("pool",) + tuple(k for k, _ in oracle.LAYERS):
        ins = [frame] if name == "pool" else [g["tap_" + i] for i in dict(oracle.LAYERS)[name]]
        got = layer_check.reference_layer(name, ins, sd)
        want = g["tap_" + name]
        assert got.shape == want.shape, name
        np.testing.assert_allclose(got, want, rtol=0, atol=layer_check.ATOL, err_msg=name)


class _TapEngine:
    """Stands in for an Engine whose last forward left `taps` in its workspace."""
    ACTIVATIONS = ("pool",) + tuple(k for k, _ in oracle.LAYERS)

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


def _damages(x, first_has_channel_64):
    """name -> damaged copy of the input tensor list `x` ([n,C,h,w] each, n >= 2)."""
    def each(fn):
        out = [a.copy() for a in x]
        for a in out:
            fn(a)
        return out

    def seam(a):
        a[1, :, 0, :] = a[0, :, -1, :]

    def last_col(a):
        a[..., -1] = 0

    def last_row(a):
        a[..., -1, :] = 0

    d = {"last column zeroed": each(last_col), "last row zeroed": each(last_row), "seam leak into frame 1": each(seam)}
    if first_has_channel_64:
        out = [a.copy() for a in x]
        out[0][:, 64] = 0
        d["input channel 64 zeroed"] = out
    return d


def test_comparator_flags_every_planted_fault():
    """160 x 192, three frames.  The clean tensors pass with zero elements over the bar (through check_layers itself, on a
    stand-in engine); an output computed from a damaged input -- last column, last row, a row leaked across the stacked
    seam, a dropped K-chunk -- and a detector output whose 65th channel repeats its neighbour are each reported, with the
    layer, the frames and the position of the damage."""
    n = 3
    frames, tp = taps_of(160, 192, n)
    rows = []
    launches = [("encoder.conv1+bn1+relu", "stem_k"), ("encoder.layer1.0 [winograd x]", "a_k"), ("encoder.layer1.0.conv2", "b_k"),
                ("encoder.layer1.1 [x]", "c_k")]
    layer_check.check_layers(_TapEngine(tp), frames, SD, "clean", launches=launches, rows=rows)
    assert [r["layer"] for r in rows] == list(_TapEngine.ACTIVATIONS)
    assert rows[0]["kernel"] == "stem_k" and rows[1]["kernel"] == "a_k + b_k" and rows[2]["kernel"] == "c_k" and rows[3]["kernel"] == "?"
    for r in rows:     # a plain fp32 re-computation is itself inside the bar; the clean tensors are 2 ulp from the reference
        assert 0 < r["e_ref"] < layer_check.ATOL and r["max_err"] < 4e-6, r

    graph = dict(oracle.LAYERS)
    for name in _TapEngine.ACTIVATIONS:
        ins = [np.array(frames)] if name == "pool" else [np.array(tp[i]) for i in graph[name]]
        want = layer_check.reference_layer(name, ins, SD)
        clean = layer_check.compare_layer(name, tp[name], want)
        assert clean["ok"] and clean["n_over"] == 0 and clean["frames_over"] == [], clean["message"]
        ho, wo = want.shape[2:]
        for what, bad in _damages(ins, name != "pool" and ins[0].shape[1] > 64).items():
            rep = layer_check.compare_layer(name, layer_check.reference_layer(name, bad, SD), want)
            tag = "%s, %s: %s" % (name, what, rep["message"])
            assert not rep["ok"] and rep["n_over"] > 0 and rep["layer"] == name and rep["message"].startswith(name + ":"), tag
            f, c, y, x = rep["worst"]
            if what == "seam leak into frame 1":
                assert rep["frames_over"] == [1] and f == 1 and y <= 1, tag
                assert "row %d of the stacked image" % (ho + y) in rep["message"], tag
            else:
                assert rep["frames_over"] == list(range(n)), tag
            if what == "last column zeroed":
                assert x >= wo - 3, tag
            if what == "last row zeroed":
                assert y >= ho - 3, tag
            assert "y mod 16 = %d, x mod 16 = %d" % (y % 16, x % 16) in rep["message"], tag
        if name in ("det.0", "det.1"):
            got = want.copy()
            got[:, 64] = got[:, 63]
            rep = layer_check.compare_layer(name, got, want)
            assert not rep["ok"] and rep["worst"][1] == 64 and rep["frames_over"] == list(range(n)), rep["message"]
            assert "channel 64 (chunk of 64: 1, lane 0)" in rep["message"], rep["message"]
    # a reference outside the range the absolute bar is stated for is refused, a wrong shape and a NaN are failures
    big = np.full((1, 1, 2, 2), 41.0, np.float32)
    assert not layer_check.compare_layer("x", big, big)["ok"]
    assert not layer_check.compare_layer("x", np.zeros((1, 1, 2, 3), np.float32), np.zeros((1, 1, 2, 2), np.float32))["ok"]
    nan = np.zeros((1, 1, 2, 2), np.float32)
    nan[0, 0, 1, 1] = np.nan
    rep = layer_check.compare_layer("x", nan, np.zeros((1, 1, 2, 2), np.float32))
    assert not rep["ok"] and rep["worst"] == (0, 0, 1, 1)
