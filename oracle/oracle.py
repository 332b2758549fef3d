"""ctypes binding of oracle/fpc_oracle.c -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this
module; the product package never does (tests/test_abi_and_host.py::test_product_never_imports_the_oracle).
"""
import ctypes
import os
import subprocess

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libfpc_oracle.so")
_lib = None

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)


def build(force=False):
    src = os.path.join(_DIR, "fpc_oracle.c")
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-s", "-C", _DIR, "-B", "libfpc_oracle.so"])
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_SO)
        _lib.oracle_forward.restype = ctypes.c_int
        _lib.oracle_get_points.restype = ctypes.c_int
        _lib.oracle_get_max_threads.restype = ctypes.c_int
    return _lib


def _p(a):
    return a.ctypes.data_as(_f32p)


def set_threads(n):
    lib().oracle_set_threads(ctypes.c_int(n))


def max_threads():
    return lib().oracle_get_max_threads()


TAP_NAMES = ["stem", "pool", "layer1.0", "layer1.1", "layer2.0", "layer2.1", "det.0", "det.1",
             "desc_in.0", "desc_in.1", "up", "desc_out.0", "desc_out.1"]


def tap_shapes(b, h, w):
    h2, w2, h4, w4, h8, w8, h16, w16 = h // 2, w // 2, h // 4, w // 4, h // 8, w // 8, h // 16, w // 16
    return [(b, 64, h2, w2), (b, 64, h4, w4), (b, 64, h4, w4), (b, 64, h4, w4), (b, 128, h8, w8),
            (b, 128, h8, w8), (b, 65, h8, w8), (b, 65, h8, w8), (b, 256, h16, w16),
            (b, 256, h16, w16), (b, 128, h8, w8), (b, 128, h8, w8), (b, 128, h8, w8)]


def weight_ptrs(state_dict, spec):
    """Array of 163 float* in state_dict order (NULL for the int64 counters)."""
    keep = []
    arr = (_f32p * len(spec))()
    for i, name in enumerate(spec):
        v = state_dict[name]
        if v.dtype == np.float32:
            v = np.ascontiguousarray(v)
            keep.append(v)
            arr[i] = _p(v)
        else:
            arr[i] = None
    return arr, keep


def forward(image, state_dict, spec, descriptor_enabled=True, with_taps=False):
    """image float32 [B,3,H,W] -> (prob_map [B,H,W], desc [B,128,H/8,W/8], logits [B,65,H/8,W/8][, taps])."""
    image = np.ascontiguousarray(image, dtype=np.float32)
    b, c, h, w = image.shape
    assert c == 3
    prob = np.empty((b, h, w), np.float32)
    desc = np.empty((b, 128, h // 8, w // 8), np.float32)
    logits = np.empty((b, 65, h // 8, w // 8), np.float32)
    wp, keep = weight_ptrs(state_dict, spec)
    taps = None
    tap_arr = None
    if with_taps:
        taps = [np.empty(s, np.float32) for s in tap_shapes(b, h, w)]
        tap_arr = (_f32p * len(taps))(*[_p(t) for t in taps])
    rc = lib().oracle_forward(_p(image), wp, b, h, w, int(bool(descriptor_enabled)), _p(prob),
                              _p(desc), _p(logits), tap_arr)
    if rc != 0:
        raise ValueError("oracle_forward: H and W must be multiples of 16")
    del keep
    if with_taps:
        return prob, desc, logits, dict(zip(TAP_NAMES, taps))
    return prob, desc, logits


# ---------------------------------------------------------------------------------------------------------------
# The same network with the roundings of the product's FPC_BF16 mode (BASELINE.json configs[4]) put where that mode
# puts them -- so that the bf16 path is held to a bound of a few fp32-accumulation ulps, not to "what 8 significant
# bits give" (round-1 VERDICT: a 0.25-absolute bound can hide a mis-rounded layer).  What is rounded to bf16
# (round-to-nearest-even): the frame; every BatchNorm-folded weight (fold in double, round to float, round to bf16);
# every tensor the mode keeps in bf16 -- h inside a block, block outputs, the transposed convolution's output.  What
# stays fp32: the stem output / pooled map (it is rounded when the first block reads it), biases, accumulation (here:
# double), the outputs of detector.layer.1 and descriptor.layer_out.1.  Convolutions are the oracle's own
# (oracle_conv2d / oracle_conv_transpose2d / oracle_maxpool3s2, double accumulation).
# ---------------------------------------------------------------------------------------------------------------
def round_bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(np.float32)


def _conv2d(x, w, stride, pad):
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    b, cin, h, wd = x.shape
    cout, _, k, _ = w.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    out = np.empty((b, cout, ho, wo), np.float32)
    lib().oracle_conv2d(_p(x), _p(w), _p(out), b, cin, h, wd, cout, k, stride, pad)
    return out


def _fold(sd, bn):
    s = sd[bn + ".weight"].astype(np.float64) / np.sqrt(sd[bn + ".running_var"].astype(np.float64) + 1e-5)
    t = sd[bn + ".bias"].astype(np.float64) - sd[bn + ".running_mean"].astype(np.float64) * s
    return s, t


def _wq(w, s):
    """BN-folded weight as the product packs it: (float)(w * s) in double, then bf16."""
    return round_bf16((w.astype(np.float64) * s[:, None, None, None]).astype(np.float32))


# (output tensor, input tensor(s)) of every layer of the bf16 plan, by the names of TAP_NAMES / fpc_read_activation
BF16_LAYERS = [("layer1.0", ("pool",)), ("layer1.1", ("layer1.0",)), ("layer2.0", ("layer1.1",)), ("layer2.1", ("layer2.0",)),
               ("det.0", ("layer2.1",)), ("det.1", ("det.0",)), ("desc_in.0", ("layer2.1",)), ("desc_in.1", ("desc_in.0",)),
               ("up", ("desc_in.1",)), ("desc_out.0", ("up", "layer2.1")), ("desc_out.1", ("desc_out.0",))]
_BF16_BLOCKS = {  # name -> (checkpoint prefix, stride, projection shortcut, fp32 output)
    "layer1.0": ("encoder.layer1.0", 1, True, False), "layer1.1": ("encoder.layer1.1", 1, False, False),
    "layer2.0": ("encoder.layer2.0", 2, True, False), "layer2.1": ("encoder.layer2.1", 1, False, False),
    "det.0": ("detector.layer.0", 1, True, False), "det.1": ("detector.layer.1", 1, False, True),
    "desc_in.0": ("descriptor.layer_in.0", 2, True, False), "desc_in.1": ("descriptor.layer_in.1", 1, False, False),
    "desc_out.0": ("descriptor.layer_out.0", 1, True, False),
    # (round 3: the mode stores the descriptor map as bf16 too -- descriptor sampling reads half the bytes; the logits stay fp32)
    "desc_out.1": ("descriptor.layer_out.1", 1, False, False)}


def _relu(v):
    return np.maximum(v, np.float32(0))


def _bias(t):
    return t.astype(np.float32)[None, :, None, None]


def maxpool3s2(a):
    """[B,C,h,w] float32 -> the 3 x 3, stride-2, padding-1 maximum [B,C,h/2,w/2] (exact)."""
    a = np.ascontiguousarray(a, np.float32)
    b, c, h, w = a.shape
    out = np.empty((b, c, h // 2, w // 2), np.float32)
    lib().oracle_maxpool3s2(_p(a), _p(out), b, c, h, w)
    return out


def bf16_folded_weights(name, sd, gray=False):
    """The BatchNorm-folded bf16 weights and float biases of one layer of the FPC_BF16 plan, as the product packs them.
    "pool": the stem's (w [64,3,7,7] -- [64,1,7,7], the three filters summed in double, for gray frames -- and bias [64]);
    "up": (wt [256,128,3,3], bias [128]); a block: (w1, b1, w2, wp or None, b2 (+ the projection's)), stride."""
    if name == "pool":
        s, t = _fold(sd, "encoder.bn1")
        w = sd["encoder.conv1.weight"]
        if gray:
            w = w.astype(np.float64)
            w = w[:, 0:1] + w[:, 1:2] + w[:, 2:3]
        return _wq(w, s), t.astype(np.float32)
    if name == "up":     # ConvTranspose2d(256, 128, 3, 2, 1, 1) + bias, bn, relu (superpoint.py:45-47,55-57)
        s, t = _fold(sd, "descriptor.bn")
        wt = round_bf16((sd["descriptor.up_sample.weight"].astype(np.float64) * s[None, :, None, None]).astype(np.float32))
        return wt, (sd["descriptor.up_sample.bias"].astype(np.float64) * s + t).astype(np.float32)
    p, stride, proj, _ = _BF16_BLOCKS[name]
    s1, t1 = _fold(sd, p + ".bn1")
    s2, t2 = _fold(sd, p + ".bn2")
    wp = None
    if proj:
        sp, tp = _fold(sd, p + ".identity_downsample.1")
        wp, t2 = _wq(sd[p + ".identity_downsample.0.weight"], sp), t2 + tp
    return (_wq(sd[p + ".conv1.weight"], s1), t1.astype(np.float32), _wq(sd[p + ".conv2.weight"], s2), wp,
            t2.astype(np.float32)), stride


def bf16_layer_parts(name, inputs, sd):
    """The pieces of ONE tensor of the FPC_BF16 plan on given input tensor(s) (oracle/layer_check.py::compare_bf16_layer
    bounds the device's tensor from them) -> dict:
      y        the output before ReLU and rounding (float, from double accumulation).  "pool": the stem's convolution + bias
               at half resolution, before ReLU and the max-pool; "up": the transposed convolution + bias;
      out_f32  whether the mode stores relu(y) as it is (det.1) or rounded to bf16;
      v, h, w2 (blocks only) conv1 + bias before ReLU, h = round_bf16(relu(v)), the folded bf16 weight [cout,cmid,1,1] of conv2.
    "pool" takes the frames ([B,3,H,W], or [B,1,H,W] gray); every other input is rounded to bf16 where the kernel reads it."""
    x = round_bf16(np.ascontiguousarray(np.concatenate(inputs, 1) if len(inputs) > 1 else inputs[0], np.float32))
    if name == "pool":
        w, t = bf16_folded_weights("pool", sd, gray=x.shape[1] == 1)
        return {"y": _conv2d(x, w, 2, 3) + t[None, :, None, None], "out_f32": False}
    if name == "up":
        wt, bt = bf16_folded_weights("up", sd)
        b, _, h, w = x.shape
        up = np.empty((b, 128, 2 * h, 2 * w), np.float32)
        lib().oracle_conv_transpose2d(_p(x), _p(np.ascontiguousarray(wt)), _p(bt), _p(up), b, 256, h, w, 128)
        return {"y": up, "out_f32": False}
    (w1, b1, w2, wp, b2), stride = bf16_folded_weights(name, sd)
    v = _conv2d(x, w1, stride, 1) + b1[None, :, None, None]
    h = round_bf16(_relu(v))
    y = _conv2d(h, w2, 1, 0)
    if wp is not None:
        # one fp32 accumulator over [h | x] on the device; here two double-accumulated halves added in float
        y = y + _conv2d(x, wp, stride, 0) + b2[None, :, None, None]
    else:
        y = y + b2[None, :, None, None] + x
    return {"v": v, "h": h, "y": y, "w2": w2, "out_f32": _BF16_BLOCKS[name][3]}


def bf16_emulated_stem(image, sd):
    """frames -> the pooled stem output ("pool") before it is stored (the device stores it as bf16: round_bf16 of
    this): bf16 frame and weights, fp32 accumulation / bias / ReLU / max-pool."""
    return maxpool3s2(_relu(bf16_layer_parts("pool", [image], sd)["y"]))


def bf16_emulated_layer(name, inputs, sd):
    """ONE layer of the FPC_BF16 plan on given input tensor(s) [B,C,h,w] (float32 arrays; values the mode keeps in bf16
    are rounded here where the kernel rounds them, so feeding the device's own tensors back in is exact)."""
    parts = bf16_layer_parts(name, inputs, sd)
    y = _relu(parts["y"])
    return y if parts["out_f32"] else round_bf16(y)


# ---------------------------------------------------------------------------------------------------------------
# The fp32 twins of the two functions above: ONE layer of the fp32 plans on given input tensor(s), nothing rounded to
# bf16.  Weights are BatchNorm-folded as weights.h packs them ((float)(w * s), the product taken in double), every
# convolution accumulates in double and is rounded to float once, bias / shortcut / ReLU are float.  Fed with a layer's
# own input as the device holds it, the result bounds that layer alone: nothing compounds across layers.
# ---------------------------------------------------------------------------------------------------------------
LAYERS = BF16_LAYERS        # the layer graph is the network's, not the mode's
_BLOCKS = _BF16_BLOCKS


def _wf(w, s):
    """BN-folded fp32 weight as the product packs it: (float)(w * s), the product in double."""
    return (w.astype(np.float64) * s[:, None, None, None]).astype(np.float32)


def f32_folded_weights(name, sd):
    """The folded float weights and biases f32_layer uses for `name`, for a caller that runs the same layer with another
    convolution (tests: torch's fp32 one).  "pool": the stem's (w [64,3,7,7], bias [64]); "up": (wt [256,128,3,3],
    bias [128]); a block: (w1, b1, w2, wp or None, b2 (+ the projection's)), stride."""
    if name == "pool":
        s, t = _fold(sd, "encoder.bn1")
        return _wf(sd["encoder.conv1.weight"], s), t.astype(np.float32)
    if name == "up":
        s, t = _fold(sd, "descriptor.bn")
        wt = (sd["descriptor.up_sample.weight"].astype(np.float64) * s[None, :, None, None]).astype(np.float32)
        return wt, (sd["descriptor.up_sample.bias"].astype(np.float64) * s + t).astype(np.float32)
    p, stride, proj, _ = _BLOCKS[name]
    s1, t1 = _fold(sd, p + ".bn1")
    s2, t2 = _fold(sd, p + ".bn2")
    wp = None
    if proj:
        sp, tp = _fold(sd, p + ".identity_downsample.1")
        wp, t2 = _wf(sd[p + ".identity_downsample.0.weight"], sp), t2 + tp
    return (_wf(sd[p + ".conv1.weight"], s1), t1.astype(np.float32), _wf(sd[p + ".conv2.weight"], s2), wp,
            t2.astype(np.float32)), stride


def f32_stem(image, sd):
    """frames [B,3,H,W] -> the pooled stem output ("pool") of the fp32 plans: 7 x 7 stride-2 convolution with folded
    weights (double accumulation), bias, ReLU, 3 x 3 stride-2 max-pool."""
    image = np.ascontiguousarray(image, np.float32)
    b, _, hh, ww = image.shape
    w, t = f32_folded_weights("pool", sd)
    st = _relu(_conv2d(image, w, 2, 3) + t[None, :, None, None])
    x0 = np.empty((b, 64, hh // 4, ww // 4), np.float32)
    lib().oracle_maxpool3s2(_p(np.ascontiguousarray(st)), _p(x0), b, 64, hh // 2, ww // 2)
    return x0


def f32_layer(name, inputs, sd):
    """ONE layer of the fp32 plans on given float32 input tensor(s) [B,C,h,w]: the ten ResNet blocks and "up"
    (ConvTranspose2d + bn + relu).  bf16_emulated_layer's structure without a single bf16 rounding."""
    x = np.ascontiguousarray(np.concatenate(inputs, 1) if len(inputs) > 1 else inputs[0], np.float32)
    if name == "up":
        wt, bt = f32_folded_weights(name, sd)
        b, _, h, w = x.shape
        up = np.empty((b, 128, 2 * h, 2 * w), np.float32)
        lib().oracle_conv_transpose2d(_p(x), _p(np.ascontiguousarray(wt)), _p(bt), _p(up), b, 256, h, w, 128)
        return _relu(up)
    (w1, b1, w2, wp, b2), stride = f32_folded_weights(name, sd)
    h = _relu(_conv2d(x, w1, stride, 1) + b1[None, :, None, None])
    y = _conv2d(h, w2, 1, 0)
    if wp is not None:
        y = y + _conv2d(x, wp, stride, 0) + b2[None, :, None, None]
    else:
        y = y + b2[None, :, None, None] + x
    return _relu(y)


# ---------------------------------------------------------------------------------------------------------------
# The C++ network (superpoint::SPModel, cpp/src/model.cc:61-93; vgg_forward below is the whole of it) one layer at a
# time, by the names of Engine.VGG_ACTIVATIONS / fpc_read_activation: (output tensor, input tensor(s)); "frames" is the
# gray plane [B,1,H,W].  No BatchNorm: weights and biases as the checkpoint holds them.
# ---------------------------------------------------------------------------------------------------------------
VGG_LAYERS = [("conv0_a", ("frames",)), ("conv0_b", ("conv0_a",)), ("pool0", ("conv0_b",)),
              ("conv1_a", ("pool0",)), ("conv1_b", ("conv1_a",)), ("pool1", ("conv1_b",)),
              ("conv2_a", ("pool1",)), ("conv2_b", ("conv2_a",)), ("pool2", ("conv2_b",)),
              ("conv3_a", ("pool2",)), ("conv3_b", ("conv3_a",)),
              ("det_a", ("conv3_b",)), ("det_b", ("det_a",)), ("desc_a", ("conv3_b",)), ("desc_b", ("desc_a",))]
_VGG_CONVS = {  # name -> (checkpoint prefix, kernel size, ReLU)
    "det_a": ("detector_conv_a", 3, True), "det_b": ("detector_conv_b", 1, False),
    "desc_a": ("descriptor_conv_a", 3, True), "desc_b": ("descriptor_conv_b", 1, False)}
_VGG_CONVS.update({"conv%d_%s" % (i, ab): ("encoder_conv%d_%s" % (i, ab), 3, True) for i in range(4) for ab in "ab"})


def vgg_layer(name, inputs, sd):
    """ONE layer of the C++ network on its float32 input tensor [B,C,h,w]: a convolution (double accumulation, rounded to
    float once) + bias (+ ReLU); "poolN": the exact 2 x 2 maximum; "desc_b": the 1 x 1 convolution + bias divided by its
    norm over the channels, the norm taken in double (model.cc:90-91: no epsilon)."""
    x = np.ascontiguousarray(inputs[0], np.float32)
    if name.startswith("pool"):
        b, c, h, w = x.shape
        return np.ascontiguousarray(x[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, c, h // 2, 2, w // 2, 2).max(axis=(3, 5)))
    p, k, relu = _VGG_CONVS[name]
    y = _conv2d(x, sd[p + ".weight"], 1, k // 2) + _bias(sd[p + ".bias"])
    if relu:
        y = _relu(y)
    if name == "desc_b":
        nrm = np.sqrt(np.sum(np.square(y.astype(np.float64)), axis=1, keepdims=True))
        y = y / nrm.astype(np.float32)
    return y


def forward_bf16_emulated(image, sd, descriptor_enabled=True, with_taps=False):
    """image float32 [B,3,H,W] -> (prob_map, desc, logits[, taps]) as `forward`, with FPC_BF16's roundings."""
    image = np.ascontiguousarray(image, np.float32)
    b, _, hh, ww = image.shape
    taps = {"pool": bf16_emulated_stem(image, sd)}
    for name, ins in BF16_LAYERS:
        if not descriptor_enabled and (name.startswith("desc") or name == "up"):
            continue
        taps[name] = bf16_emulated_layer(name, [taps[i] for i in ins], sd)
    logits = taps["det.1"]
    hc, wc = hh // 8, ww // 8
    desc = taps["desc_out.1"] if descriptor_enabled else np.zeros((b, 128, hc, wc), np.float32)
    # exp-softmax (+1e-5, no max-subtraction) and depth-to-space, superpoint.py:111-114, in float as `forward` does
    e = np.exp(logits.astype(np.float32))
    sm = e / (e.sum(1, keepdims=True, dtype=np.float32) + np.float32(.00001))
    prob = np.empty((b, hh, ww), np.float32)
    lib().oracle_restore_prob_map(_p(np.ascontiguousarray(sm.astype(np.float32))), _p(prob), b, hc, wc, 8)
    return (prob, desc, logits, taps) if with_taps else (prob, desc, logits)


def get_points(prob, conf_thresh=0.015, nms_dist=4, border_remove=4):
    """prob float32 [H,W] -> (xs int32[K], ys int32[K], conf float32[K], n_candidates)."""
    prob = np.ascontiguousarray(prob, dtype=np.float32)
    h, w = prob.shape
    cap = h * w
    xs = np.empty(cap, np.int32)
    ys = np.empty(cap, np.int32)
    conf = np.empty(cap, np.float32)
    ncand = ctypes.c_int(0)
    k = lib().oracle_get_points(_p(prob), h, w, ctypes.c_float(conf_thresh), nms_dist,
                                border_remove, xs.ctypes.data_as(_i32p), ys.ctypes.data_as(_i32p),
                                _p(conf), cap, ctypes.byref(ncand))
    return xs[:k].copy(), ys[:k].copy(), conf[:k].copy(), ncand.value


def get_descriptors(desc_map, xs, ys, h, w):
    """desc_map float32 [D,Hc,Wc], points -> float32 [K,D] unit-norm rows."""
    desc_map = np.ascontiguousarray(desc_map, dtype=np.float32)
    d, hc, wc = desc_map.shape
    xs = np.ascontiguousarray(xs, np.int32)
    ys = np.ascontiguousarray(ys, np.int32)
    k = len(xs)
    out = np.empty((k, d), np.float32)
    if k:
        lib().oracle_get_descriptors(_p(desc_map), d, hc, wc, h, w, xs.ctypes.data_as(_i32p),
                                     ys.ctypes.data_as(_i32p), k, _p(out))
    return out


def get_descriptors_at(desc_map, xs, ys, h, w):
    """As get_descriptors, at float64 points (fractional / outside the frame allowed)."""
    desc_map = np.ascontiguousarray(desc_map, dtype=np.float32)
    d, hc, wc = desc_map.shape
    xy = np.ascontiguousarray(np.stack([np.asarray(xs, np.float64), np.asarray(ys, np.float64)], 1))
    out = np.empty((len(xy), d), np.float32)
    if len(xy):
        lib().oracle_get_descriptors_at(_p(desc_map), d, hc, wc, h, w, xy.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                        len(xy), _p(out))
    return out


def match(query, train, cross_check=True, max_dist=0.0):
    """BFMatcher(NORM_L2, crossCheck).match restated (parity unpinned: cv2 is absent) -> (match, dist)."""
    q = np.ascontiguousarray(query, np.float32)
    t = np.ascontiguousarray(train, np.float32)
    m = np.full(len(q), -1, np.int32)
    d = np.zeros(len(q), np.float32)
    if len(q):
        lib().oracle_match(_p(q), len(q), _p(t), len(t), q.shape[1], int(bool(cross_check)),
                           ctypes.c_float(max_dist), m.ctypes.data_as(_i32p), _p(d))
    return m, d


def first_within(key, cur, tolerance=0.8):
    """SearchKeyFrameCorrespondence (cpp/src/main.cc:18-29) restated -> first index or -1 per key descriptor."""
    k = np.ascontiguousarray(key, np.float32)
    c = np.ascontiguousarray(cur, np.float32)
    out = np.full(len(k), -1, np.int32)
    if len(k):
        lib().oracle_first_within(_p(k), len(k), _p(c), len(c), k.shape[1], ctypes.c_double(tolerance),
                                  out.ctypes.data_as(_i32p))
    return out


def u8_to_float(frames_u8, layout):
    """8-bit frames -> float frames [n,C,H,W] (camera.py:31, inferencewrapper.py:70-81, inference.py:79,
    cpp/src/camera.cc:17-18).  layout: 0 gray [n,H,W], 1 RGB HWC, 2 BGR HWC (swap), 3 BGR HWC -> gray."""
    a = np.ascontiguousarray(frames_u8, np.uint8)
    n, h, w = a.shape[0], a.shape[1], a.shape[2]
    cout = 1 if layout in (0, 3) else 3
    out = np.empty((n, cout, h, w), np.float32)
    lib().oracle_u8_to_float(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, h * w, int(layout), _p(out))
    return out


def vgg_forward(image, state_dict, spec):
    """The reference's C++ network (cpp/src/model.cc:61-93) restated: image float32 [B,1,H,W] ->
    (prob_map [B,H,W], desc [B,256,H/8,W/8] unit-norm over channels, logits [B,65,H/8,W/8])."""
    image = np.ascontiguousarray(image, dtype=np.float32)
    b, c, h, w = image.shape
    assert c == 1
    prob = np.empty((b, h, w), np.float32)
    desc = np.empty((b, 256, h // 8, w // 8), np.float32)
    logits = np.empty((b, 65, h // 8, w // 8), np.float32)
    wp, keep = weight_ptrs(state_dict, spec)
    rc = lib().oracle_vgg_forward(_p(image), wp, b, h, w, _p(prob), _p(desc), _p(logits))
    if rc != 0:
        raise ValueError("oracle_vgg_forward: H and W must be multiples of 8")
    del keep
    return prob, desc, logits


def warp_perspective(planes, coeffs, nearest=False):
    """functional_tensor.perspective restated (homographies.py:215-216): planes float32 [P,H,W], coeffs 8 floats."""
    a = np.ascontiguousarray(planes, np.float32)
    p, h, w = a.shape
    k = np.ascontiguousarray(coeffs, np.float32).ravel()
    out = np.empty_like(a)
    lib().oracle_warp_perspective(_p(a), p, h, w, _p(k), int(bool(nearest)), _p(out))
    return out


def erode_ellipse(plane, r):
    """cv2.erode with the MORPH_ELLIPSE (2r, 2r) element, constant border 0 (homographies.py:238-247) restated."""
    a = np.ascontiguousarray(plane, np.float32)
    h, w = a.shape
    out = np.empty_like(a)
    lib().oracle_erode_ellipse(_p(a), h, w, int(r), _p(out))
    return out


def invert_homography(h):
    """invert_homography (homographies.py:185-209) in double."""
    m = np.append(np.asarray(h, np.float64).ravel(), 1.0).reshape(3, 3)
    inv = np.linalg.inv(m)
    return (inv / inv[2, 2]).ravel()[:8].astype(np.float32)


def homography_adaptation(frames, forward_fn, homographies, inverses=None, erosion_radius=8, aggregation="sum"):
    """homography_adaptation (homographies.py:250-324) restated; forward_fn(frames [n,C,H,W]) -> prob maps [n,H,W]."""
    frames = np.ascontiguousarray(frames, np.float32)
    n, c, h, w = frames.shape
    probs = [forward_fn(frames)]
    counts = [np.ones((h, w), np.float32)]
    ones = np.ones((1, h, w), np.float32)
    for i, hm in enumerate(homographies):
        hinv = inverses[i] if inverses is not None else invert_homography(hm)
        warped = warp_perspective(frames.reshape(n * c, h, w), hm).reshape(n, c, h, w)
        count = warp_perspective(ones, hinv, nearest=True)[0]
        mask = warp_perspective(ones, hm, nearest=True)[0]
        if erosion_radius:
            count, mask = erode_ellipse(count, erosion_radius), erode_ellipse(mask, erosion_radius)
        wp = forward_fn(warped) * mask[None]
        probs.append(warp_perspective(wp, hinv) * count[None])
        counts.append(count)
    total = np.sum(np.stack(counts, -1), -1, dtype=np.float32)
    stack = np.stack(probs, -1)
    agg = stack.max(-1) if aggregation == "max" else stack.sum(-1, dtype=np.float32) / total[None]
    return np.where(total[None] >= len(homographies) // 3, agg, 0.0).astype(np.float32)


def resize_crop_u8(frames_u8, h, w, swap_rb=False):
    """make_query_image (inference.py:72-85) on camera.py:31 frames: uint8 [n,sh,sw,3] -> float32 [n,3,h,w]."""
    a = np.ascontiguousarray(frames_u8, np.uint8)
    n, sh, sw, _ = a.shape
    out = np.empty((n, 3, h, w), np.float32)
    rc = lib().oracle_resize_crop_u8(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, sh, sw, h, w, int(bool(swap_rb)), _p(out))
    if rc != 0:
        raise ValueError("target larger than the resized frame")
    return out
