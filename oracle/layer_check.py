"""Layer-isolated float64 parity of the fp32 plans -- TEST INFRASTRUCTURE ONLY (tests/test_layer_oracle.py on the CPU,
tests/test_gpu_layer_isolated.py on the device; the bf16 mode: compare_bf16_layer / check_bf16_layers below; the C++ network: tests/test_layer_oracle_vgg.py and
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
# The bf16 mode (dtype="bf16"): the same layer-isolated comparison, per element, with no allowance for a share of elements
# (tests/test_layer_oracle_bf16.py on the CPU, tests/test_gpu_layer_isolated_bf16.py on the device).
#
# The emulation (oracle.bf16_layer_parts) puts the mode's roundings where the kernels put them and accumulates in double;
# the device accumulates in fp32, in another order.  The two can differ at an element only where that moved a value
# across a bf16 rounding boundary: at the output, or at an h = round_bf16(relu(conv1 + bias)) feeding it -- and conv2 of a
# block is 1 x 1, so the h's that feed an output element are the one pixel's channels.  With EPS_h / EPS_y the most an fp32
# accumulation of conv1 / of y may lie from the double one,
#     U     = max(rb(relu(v + EPS_h)) - h, h - rb(relu(v - EPS_h)))       the most a device h differs from the emulation's
#     delta = EPS_y + conv1x1(U, |w2|)                                    ("up" and the stem have no h: delta = EPS_y)
# a bf16-stored output is accepted iff rb(relu(y - delta)) <= got <= rb(relu(y + delta)) (the stem: both bounds max-pooled,
# the pool being monotone), the fp32 logits iff |got - relu(y)| <= delta.  EPS is BF16_EPS_MARGIN x E_ref, E_ref the
# largest error against the double value of the SAME computation in plain fp32 on the CPU (torch_bf16_parts: same bf16
# operands, same input, the emulation's h): DESIGN.md's table has the fp32-accumulating direct kernels at up to 4.56 x
# E_ref, and 8 is under twice that.  Each EPS must itself be <= ATOL.  So that wide intervals cannot make the check
# vacuous, at most BF16_MAX_AMBIGUOUS of a bf16 layer's elements may have an interval of more than one bf16 value, and
# the median delta of the logits must be <= ATOL.
# ---------------------------------------------------------------------------------------------------------------
BF16_EPS_MARGIN = 8.0
BF16_MAX_AMBIGUOUS = 0.10


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _conv_in_quarters(F, x, w, quarters, **kw):
    """conv2d / conv_transpose2d `F` with the input channels accumulated in `quarters` chunks, the partial sums added in
    float in order: another fp32 accumulation order of the same sum."""
    cin = x.shape[1]
    if quarters <= 1 or cin % quarters:
        return F(x, w, **kw)
    q = cin // quarters
    transposed = w.shape[0] == cin and F.__name__ == "conv_transpose2d"
    acc = None
    for k in range(quarters):
        wk = w[k * q:(k + 1) * q] if transposed else w[:, k * q:(k + 1) * q]
        part = F(x[:, k * q:(k + 1) * q], wk, **kw)
        acc = part if acc is None else acc + part
    return acc


def torch_bf16_parts(name, inputs, sd, h=None, quarters=1):
    """oracle.bf16_layer_parts in plain fp32 on the CPU (torch.nn.functional), same bf16-rounded operands -> dict with y
    and, for a block, v and h.  `h`: the h that conv2 reads (the emulation's, for E_ref of y alone); None: its own,
    round_bf16(relu(v)), as a device computes it.  `quarters` > 1: conv1 (the transposed convolution for "up") accumulated
    in that many chunks of input channels -- a second fp32 accumulation order."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = _t(oracle.round_bf16(np.concatenate(inputs, 1) if len(inputs) > 1 else inputs[0]))
        if name == "pool":
            w, b = oracle.bf16_folded_weights("pool", sd, gray=x.shape[1] == 1)
            return {"y": F.conv2d(x, _t(w), _t(b), stride=2, padding=3).numpy()}
        if name == "up":
            wt, bt = oracle.bf16_folded_weights("up", sd)
            y = _conv_in_quarters(F.conv_transpose2d, x, _t(wt), quarters, stride=2, padding=1, output_padding=1)
            return {"y": (y + _t(bt)[None, :, None, None]).numpy()}
        (w1, b1, w2, wp, b2), stride = oracle.bf16_folded_weights(name, sd)
        v = (_conv_in_quarters(F.conv2d, x, _t(w1), quarters, stride=stride, padding=1) + _t(b1)[None, :, None, None]).numpy()
        own = oracle.round_bf16(np.maximum(v, np.float32(0)))
        y = F.conv2d(_t(own if h is None else h), _t(w2))
        bias = _t(b2)[None, :, None, None]
        y = y + F.conv2d(x, _t(wp), stride=stride) + bias if wp is not None else y + bias + x
        return {"v": v, "h": own, "y": y.numpy()}


def bf16_output_of(name, parts, out_f32):
    """The tensor a device that computed `parts` (y before ReLU and rounding) stores: what the stand-in devices of
    tests/test_layer_oracle_bf16.py hand to the check."""
    y = np.maximum(np.asarray(parts["y"], np.float32), np.float32(0))
    if name == "pool":
        y = oracle.maxpool3s2(y)
    return y if out_f32 else oracle.round_bf16(y)


def bf16_eps(name, inputs, sd, parts):
    """(EPS_h, EPS_y, E_ref of conv1, E_ref of y) of one layer on these inputs; EPS_h is 0 where there is no h."""
    ref = torch_bf16_parts(name, inputs, sd, h=parts.get("h"))
    e_y = float(np.max(np.abs(ref["y"].astype(np.float64) - parts["y"])))
    e_h = float(np.max(np.abs(ref["v"].astype(np.float64) - parts["v"]))) if "v" in parts else 0.0
    return BF16_EPS_MARGIN * e_h, BF16_EPS_MARGIN * e_y, e_h, e_y


def _rb_relu_outward(v, eps, up):
    """round_bf16(relu(v +- eps)), the float sum nudged outward so that its own rounding cannot narrow the interval."""
    f = (v.astype(np.float64) + (eps if up else -eps)).astype(np.float32)
    f = np.nextafter(f, np.float32(np.inf if up else -np.inf))
    return oracle.round_bf16(np.maximum(f, np.float32(0)))


def bf16_delta(parts, eps_h, eps_y):
    """delta [n,C,h,w] (float64) of the rule above."""
    y = parts["y"]
    if "h" not in parts:
        return np.full(y.shape, eps_y, np.float64)
    h = parts["h"].astype(np.float64)
    u = np.maximum(_rb_relu_outward(parts["v"], eps_h, True) - h, h - _rb_relu_outward(parts["v"], eps_h, False))
    w2 = np.abs(parts["w2"].astype(np.float64))[:, :, 0, 0]
    return eps_y + np.einsum("oc,nchw->nohw", w2, u, optimize=True)


def compare_bf16_layer(name, got, parts, eps_h, eps_y, tile=None):
    """One tensor of the bf16 mode, the device's `got` [n,C,h,w] against oracle.bf16_layer_parts of its own input(s) ->
    a report like compare_layer's: ok, layer, message, n_over, frames_over, worst = (frame, channel, y, x), max_want,
    max_err (against the emulation's stored value), plus flips (share of elements != that value), ambiguous (share of
    elements whose accepted interval holds more than one bf16 value; None for the fp32 logits), median_delta, eps_h,
    eps_y.  Not ok: an element outside its interval or not finite, an EPS over ATOL, a layer over BF16_MAX_AMBIGUOUS
    (the logits: median delta over ATOL), a reference outside MAX_MAGNITUDE, a wrong shape.  `tile` = (TH, TW) of the
    kernel's output tile adds the position in that tile to a failure's message."""
    got = np.asarray(got)
    out_f32 = bool(parts["out_f32"])
    pool = name == "pool"
    want = bf16_output_of(name, parts, out_f32)
    rep = {"ok": False, "layer": name, "n_over": -1, "frames_over": [], "worst": None, "max_err": float("nan"),
           "max_want": float("nan"), "flips": float("nan"), "ambiguous": None, "median_delta": float("nan"),
           "eps_h": eps_h, "eps_y": eps_y}
    if got.shape != want.shape:
        rep["message"] = "%s: shape %s on the device, %s in the reference" % (name, got.shape, want.shape)
        return rep
    n, _, h, w = want.shape
    max_want = float(np.max(np.abs(want)))
    rep["max_want"] = max_want
    if not max_want <= MAX_MAGNITUDE:
        rep["message"] = "%s: max |reference| = %g is outside the range (%g) the absolute %g bar is stated for" % (
            name, max_want, MAX_MAGNITUDE, ATOL)
        return rep
    if not (eps_h <= ATOL and eps_y <= ATOL):
        rep["message"] = "%s: EPS_h %.3g / EPS_y %.3g over the %g ceiling" % (name, eps_h, eps_y, ATOL)
        return rep
    delta = bf16_delta(parts, eps_h, eps_y)
    rep["median_delta"] = float(np.median(delta))
    y = parts["y"]
    if out_f32:
        lo, hi = want.astype(np.float64) - delta, want.astype(np.float64) + delta
    else:
        lo, hi = _rb_relu_outward(y, delta, False), _rb_relu_outward(y, delta, True)
        if pool:
            lo, hi = oracle.maxpool3s2(lo), oracle.maxpool3s2(hi)
        rep["ambiguous"] = float(np.mean(lo != hi))
    g = got.astype(np.float64)
    dist = np.maximum(lo - g, g - hi)               # > 0: outside the interval by that much
    dist = np.where(np.isfinite(g), dist, np.inf)
    over = dist > 0
    err = np.abs(g - want)
    rep["max_err"] = float(np.where(np.isfinite(err), err, np.inf).max())
    rep["flips"] = float(np.mean(got != want))
    rep["n_over"] = int(over.sum())
    i, c, yy, x = (int(v) for v in np.unravel_index(int(np.argmax(dist)), dist.shape))
    rep["worst"] = (i, c, yy, x)
    rep["frames_over"] = [k for k in range(n) if over[k].any()]
    vacuous = (rep["median_delta"] > ATOL) if out_f32 else (rep["ambiguous"] > BF16_MAX_AMBIGUOUS)
    rep["ok"] = rep["n_over"] == 0 and not vacuous
    share = ("median delta %.3g" % rep["median_delta"]) if out_f32 else ("%.2f %% ambiguous" % (100 * rep["ambiguous"]))
    if rep["n_over"]:
        where = ""
        if tile:
            th, tw = tile
            where = ", row %d col %d of %d x %d tile (%d, %d)" % (yy % th, x % tw, th, tw, yy // th, x // tw)
        y_at = ("max-pooled from y around (%d, %d)" % (2 * yy, 2 * x)) if pool else ("y %r, delta %.3g" % (float(y[i, c, yy, x]), float(delta[i, c, yy, x])))
        rep["message"] = ("%s: %d of %d elements outside their interval in frame(s) %s; worst: device %r, accepted [%r, %r], "
                          "emulation %r (%s) at frame %d channel %d (chunk of 64: %d, lane %d) y %d x %d -- y mod 16 = %d, "
                          "x mod 16 = %d%s, row %d of the stacked image (%d rows per frame), map %d x %d; %s" % (
                              name, rep["n_over"], dist.size, rep["frames_over"], float(got[i, c, yy, x]), float(lo[i, c, yy, x]),
                              float(hi[i, c, yy, x]), float(want[i, c, yy, x]), y_at, i, c, c // 64, c % 64, yy, x, yy % 16, x % 16,
                              where, i * h + yy, h, h, w, share))
    elif vacuous:
        rep["message"] = "%s: the check is too wide to mean anything here: %s (EPS_h %.3g, EPS_y %.3g)" % (name, share, eps_h, eps_y)
    else:
        rep["message"] = "%s: every element inside its interval; %.3f %% differ from the emulation, max %.3g; %s" % (
            name, 100 * rep["flips"], rep["max_err"], share)
    return rep


def check_bf16_layers(engine, frames, sd, tag, launches=None, rows=None, tiles=None):
    """check_layers for a dtype="bf16" engine, after engine.forward(frames): every tensor of engine.ACTIVATIONS (without
    the descriptor head's where it is disabled), every frame, each from the device's own input tensor(s), by
    compare_bf16_layer with the EPS of bf16_eps on those inputs.  Prints one line per layer, appends the figures to `rows`,
    raises AssertionError with every failing layer's message.  `tiles`: {tensor: (TH, TW)} for the messages."""
    frames = np.ascontiguousarray(frames, np.float32)
    n = frames.shape[0]
    with_desc = getattr(engine, "descriptor_enabled", True)
    names = [t for t in engine.ACTIVATIONS if with_desc or not (t.startswith("desc") or t == "up")]
    dev = {name: engine.activation(name, 0, n).cpu().numpy() for name in names}
    dev["frames"] = frames
    graph = dict(oracle.BF16_LAYERS)
    graph["pool"] = ("frames",)
    kernels = layer_kernels(launches or [])
    failures = []
    for name in names:
        inputs = [dev[i] for i in graph[name]]
        parts = oracle.bf16_layer_parts(name, inputs, sd)
        eps_h, eps_y, e_h, e_y = bf16_eps(name, inputs, sd, parts)
        rep = compare_bf16_layer(name, dev[name], parts, eps_h, eps_y, tile=(tiles or {}).get(name))
        amb = "median delta %.3e" % rep["median_delta"] if rep["ambiguous"] is None else "ambiguous %.3f %%" % (100 * rep["ambiguous"])
        print("layer-isolated bf16 | %s | %s | %s | flips %.4f %% | %s | max err %.3e | E_ref h %.3e y %.3e | EPS h %.3e y %.3e" % (
            tag, name, kernels[name], 100 * rep["flips"], amb, rep["max_err"], e_h, e_y, eps_h, eps_y))
        if rows is not None:
            rows.append(dict(rep, tag=tag, kernel=kernels[name], e_ref_h=e_h, e_ref_y=e_y))
        if not rep["ok"]:
            failures.append("%s [%s]: %s" % (tag, kernels[name], rep["message"]))
    assert not failures, "\n".join(failures)


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
