"""Layer-isolated float64 parity of the fp32 plans -- TEST INFRASTRUCTURE ONLY (tests/test_layer_oracle.py on the CPU,
tests/test_gpu_layer_isolated.py on the device; the C++ network: tests/test_layer_oracle_vgg.py and
tests/test_gpu_layer_isolated_vgg.py, through the *_vgg_* twins at the end of this file).

Every layer of the network is fed the input tensor(s) the device itself holds for it (fpc_read_activation) and computed
once more by oracle.f32_layer / oracle.f32_stem: folded float weights, double accumulation.  The device's output tensor
must agree within ATOL at EVERY element of EVERY frame.  Nothing compounds across layers, so a failure names a layer, a
frame and a position -- and says where that position lies in a 16-pixel tile, in the stacked image of the batch and in the
channel chunks, which is what tells a tile edge from a seam from a dropped K-chunk from the detector's 65th channel.

ATOL is the 1e-4 of BASELINE.json's north star, which tests/test_gpu_parity.py::test_f1_per_layer_taps_on_the_device
applies per layer already; the numerical contract of include/fpc.h keeps the absolute 1e-4 up to magnitude MAX_MAGNITUDE,
and compare_layer refuses to apply the bar to a reference tensor outside that range.
"""
import numpy as np

from . import oracle

ATOL = 1e-4
MAX_MAGNITUDE = 40.0

# tensor name -> the prefix of the op names (Engine.timings()) that write it
_OP_PREFIX = {name: blk[0] for name, blk in oracle._BLOCKS.items()}
_OP_PREFIX["up"] = "descriptor.up_sample"
_POOL_PREFIXES = ("encoder.conv1", "encoder.max_pool")


def layer_kernels(launches):
    """[(op name, kernel symbol), ...] of one forward (Engine.timings()) -> {tensor name: "symbol" or "symbol + symbol"},
    the kernels that wrote each of Engine.ACTIVATIONS, in launch order, each once."""
    out = {}
    for tensor in ("pool",) + tuple(n for n, _ in oracle.LAYERS):
        prefixes = _POOL_PREFIXES if tensor == "pool" else (_OP_PREFIX[tensor],)
        syms = []
        for op, sym in launches:
            if any(op == p or (op.startswith(p) and op[len(p)] in " .+[") for p in prefixes) and sym not in syms:
                syms.append(sym)
        out[tensor] = " + ".join(syms) if syms else "?"
    return out


def compare_layer(name, got, want, atol=ATOL):
    """One layer's device tensor `got` against its reference `want` (both [n,C,h,w]) -> a report (dict):
    ok, layer, message (one line; what a failing test shows), max_err, max_want, rel (max_err / max_want), n_over,
    frames_over (the frames with an element over the bar) and worst = (frame, channel, y, x).  A non-finite difference
    counts as over the bar."""
    got, want = np.asarray(got), np.asarray(want)
    rep = {"ok": False, "layer": name, "n_over": -1, "frames_over": [], "worst": None, "max_err": float("nan"),
           "max_want": float("nan"), "rel": float("nan")}
    if got.shape != want.shape:
        rep["message"] = "%s: shape %s on the device, %s in the reference" % (name, got.shape, want.shape)
        return rep
    n, _, h, w = want.shape
    max_want = float(np.max(np.abs(want)))
    rep["max_want"] = max_want
    if not max_want <= MAX_MAGNITUDE:
        rep["message"] = "%s: max |reference| = %g is outside the range (%g) the absolute %g bar is stated for" % (
            name, max_want, MAX_MAGNITUDE, atol)
        return rep
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    err = np.where(np.isfinite(err), err, np.inf)
    over = err > atol
    rep["max_err"] = float(err.max())
    rep["rel"] = rep["max_err"] / max(max_want, np.finfo(np.float32).tiny)
    rep["n_over"] = int(over.sum())
    i, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
    rep["worst"] = (i, c, y, x)
    rep["frames_over"] = [k for k in range(n) if over[k].any()]
    rep["ok"] = rep["n_over"] == 0
    if rep["ok"]:
        rep["message"] = "%s: max error %.3g (%.3g of max |reference| %.3g)" % (name, rep["max_err"], rep["rel"], max_want)
    else:
        rep["message"] = ("%s: %d of %d elements over %g in frame(s) %s; worst %.3g (device %r, reference %r) at frame %d "
                          "channel %d (chunk of 64: %d, lane %d) y %d x %d -- y mod 16 = %d, x mod 16 = %d, row %d of the "
                          "stacked image (%d rows per frame), map %d x %d" % (
                              name, rep["n_over"], err.size, atol, rep["frames_over"], rep["max_err"], float(got[i, c, y, x]),
                              float(want[i, c, y, x]), i, c, c // 64, c % 64, y, x, y % 16, x % 16, i * h + y, h, h, w))
    return rep


def reference_layer(name, inputs, sd):
    """The float64-accumulating reference of one tensor of Engine.ACTIVATIONS: "pool" from the frames, a layer from its
    input tensor(s)."""
    return oracle.f32_stem(inputs[0], sd) if name == "pool" else oracle.f32_layer(name, inputs, sd)


def torch_f32_layer(name, inputs, sd):
    """The same single layer with the same folded float weights in plain fp32 on the CPU (torch.nn.functional): what an
    fp32 implementation with no particular care costs against the double reference (E_ref in the tests' tables)."""
    import torch
    import torch.nn.functional as F

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.float32))

    with torch.no_grad():
        x = t(np.concatenate(inputs, 1) if len(inputs) > 1 else inputs[0])
        if name == "pool":
            w, b = oracle.f32_folded_weights("pool", sd)
            return F.max_pool2d(F.relu(F.conv2d(x, t(w), t(b), stride=2, padding=3)), 3, 2, 1).numpy()
        if name == "up":
            wt, bt = oracle.f32_folded_weights("up", sd)
            return F.relu(F.conv_transpose2d(x, t(wt), t(bt), stride=2, padding=1, output_padding=1)).numpy()
        (w1, b1, w2, wp, b2), stride = oracle.f32_folded_weights(name, sd)
        h = F.relu(F.conv2d(x, t(w1), t(b1), stride=stride, padding=1))
        y = F.conv2d(h, t(w2))
        bias = t(b2)[None, :, None, None]
        y = y + F.conv2d(x, t(wp), stride=stride) + bias if wp is not None else y + bias + x
        return F.relu(y).numpy()


def _check(engine, frames, sd, tag, launches, rows, names, graph, reference, torch_reference, kernels):
    """check_layers / check_vgg_layers: `names` in order, `graph` {tensor: its input tensors, "frames" = the frames}."""
    frames = np.ascontiguousarray(frames, np.float32)
    n = frames.shape[0]
    dev = {name: engine.activation(name, 0, n).cpu().numpy() for name in names}
    dev["frames"] = frames
    failures = []
    for name in names:
        inputs = [dev[i] for i in graph[name]]
        want = reference(name, inputs, sd)
        rep = compare_layer(name, dev[name], want)
        e_ref = float(np.max(np.abs(torch_reference(name, inputs, sd).astype(np.float64) - want)))
        # (an exact layer -- a max-pool -- has E_ref = 0: ratio 0 where the device is exact too)
        ratio = rep["max_err"] / e_ref if e_ref > 0 else 0.0 if rep["max_err"] == 0 else float("inf")
        print("layer-isolated | %s | %s | %s | max err %.3e | rel %.3e | E_ref %.3e | device / E_ref %.2f" % (
            tag, name, kernels[name], rep["max_err"], rep["rel"], e_ref, ratio))
        if rows is not None:
            rows.append({"tag": tag, "layer": name, "kernel": kernels[name], "max_err": rep["max_err"], "rel": rep["rel"],
                         "e_ref": e_ref, "ratio": ratio, "max_want": rep["max_want"]})
        if not rep["ok"]:
            failures.append("%s [%s]: %s" % (tag, kernels[name], rep["message"]))
    assert not failures, "\n".join(failures)


def check_layers(engine, frames, sd, tag, launches=None, rows=None):
    """Call after engine.forward(frames): every tensor of engine.ACTIVATIONS, every frame of the batch, against
    reference_layer on the device's own input tensor(s).  Prints one line per layer (kernel symbol, max error, max error
    relative to max |reference|, E_ref of torch_f32_layer on the same input and device error / E_ref), appends the same
    figures to `rows`, and raises AssertionError with every failing layer's message once all layers were looked at."""
    graph = dict(oracle.LAYERS)
    graph["pool"] = ("frames",)
    _check(engine, frames, sd, tag, launches, rows, engine.ACTIVATIONS, graph, reference_layer, torch_f32_layer,
           layer_kernels(launches or []))


# ---------------------------------------------------------------------------------------------------------------
# The C++ network (arch="vgg"): the same comparison over oracle.VGG_LAYERS / oracle.vgg_layer
# (tests/test_layer_oracle_vgg.py on the CPU, tests/test_gpu_layer_isolated_vgg.py on the device).
# ---------------------------------------------------------------------------------------------------------------
def _vgg_op_prefixes(tensor):
    """The prefixes of the op names (Engine.timings()) that write `tensor`."""
    if tensor.startswith("pool"):
        return ("max_pool2d(2,2) after " + oracle._VGG_CONVS["conv%s_b" % tensor[4:]][0],)
    if tensor == "desc_b":      # the 1 x 1 convolution, then l2norm256_kernel in place
        return (oracle._VGG_CONVS[tensor][0], "descriptor L2 normalisation")
    return (oracle._VGG_CONVS[tensor][0],)


def vgg_layer_kernels(launches):
    """layer_kernels for the C++ network: {tensor of Engine.VGG_ACTIVATIONS: "symbol" or "symbol + symbol"}."""
    out = {}
    for tensor, _ in oracle.VGG_LAYERS:
        syms = []
        for op, sym in launches:
            if any(op == p or (op.startswith(p) and op[len(p)] in " .+[") for p in _vgg_op_prefixes(tensor)) and sym not in syms:
                syms.append(sym)
        out[tensor] = " + ".join(syms) if syms else "?"
    return out


def vgg_layer_ops(launches):
    """{tensor: [op names that wrote it]} -- the op name of a layer computed in parts says how many and how wide."""
    return {tensor: [op for op, _ in launches if any(op == p or (op.startswith(p) and op[len(p)] in " .+[")
                                                      for p in _vgg_op_prefixes(tensor))] for tensor, _ in oracle.VGG_LAYERS}


def torch_vgg_layer(name, inputs, sd):
    """oracle.vgg_layer in plain fp32 on the CPU (torch.nn.functional): E_ref of the tests' tables."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(inputs[0], np.float32))
        if name.startswith("pool"):
            return F.max_pool2d(x, 2, 2).numpy()
        p, k, relu = oracle._VGG_CONVS[name]
        y = F.conv2d(x, torch.from_numpy(sd[p + ".weight"]), torch.from_numpy(sd[p + ".bias"]), padding=k // 2)
        if relu:
            y = F.relu(y)
        if name == "desc_b":
            y = y / torch.norm(y, 2, 1, keepdim=True)
        return y.numpy()


def check_vgg_layers(engine, frames, sd, tag, launches=None, rows=None, names=None):
    """check_layers for an arch="vgg" engine: every tensor of `names` (default engine.VGG_ACTIVATIONS; without the
    desc_* ones where the descriptor head is disabled), every frame, against oracle.vgg_layer on the device's own input."""
    _check(engine, frames, sd, tag, launches, rows, names or engine.VGG_ACTIVATIONS, dict(oracle.VGG_LAYERS), oracle.vgg_layer,
           torch_vgg_layer, vgg_layer_kernels(launches or []))


def band_rows(a, b, h):
    """The output rows [lo, hi) of a 3 x 3, padding-1 layer that input rows [a, b) of an h-row frame determine alone:
    those whose support lies inside the band or on the frame's true top / bottom edge (where the padding is the layer's)."""
    return (a if a == 0 else a + 1), (b if b == h else b - 1)


def compare_band(name, got, want, a, b, h, atol=ATOL):
    """compare_layer on a band of rows: `got` is rows [a, b) of the device's output tensor, `want` the reference computed
    from rows [a, b) of the input alone (its zero padding stands in for the rows outside the band, so its first / last
    row is wrong unless the band touches the frame's edge).  Only band_rows(a, b, h) are compared; worst's y and
    "rows" are frame rows, the message's y counts from row `lo`."""
    lo, hi = band_rows(a, b, h)
    got, want = np.asarray(got), np.asarray(want)
    assert 0 <= a < lo < hi <= b <= h or 0 == a == lo < hi <= b <= h, (a, b, h)
    assert want.shape[2] == b - a, (want.shape, a, b)
    if got.shape != want.shape:
        return compare_layer(name, got, want, atol)
    rep = compare_layer(name, got[:, :, lo - a:hi - a], want[:, :, lo - a:hi - a], atol)
    rep["rows"] = (lo, hi)
    if rep["worst"] is not None:
        f, c, y, x = rep["worst"]
        rep["worst"] = (f, c, y + lo, x)
    rep["message"] += " [rows %d..%d of the frame's %d, y counted from row %d]" % (lo, hi - 1, h, lo)
    return rep
