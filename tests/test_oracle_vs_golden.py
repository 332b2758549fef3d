"""Pins the CPU oracle (oracle/fpc_oracle.c) against the golden vectors produced by the
reference's own python modules (tests/golden/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import arch, synth
from oracle import oracle

SPEC = arch.state_dict_spec()


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_spec_matches_survey_table_w():
    assert len(SPEC) == 163
    assert sum(int(np.prod(s)) for s in SPEC.values()) == 2352378
    assert arch.conv_macs(480, 640) == 8304897600
    assert abs(arch.conv_macs(240, 320, descriptor=False) * 2 / 1e9 - 2.127) < 1e-3


def test_f1_per_layer_activations(golden_dir):
    g = load(golden_dir, "f1_layers_32x48.npz")
    sd = synth.make_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    frame = synth.make_frame(int(g["seed_frame"]), int(g["h"]), int(g["w"]))
    prob, desc, logits, taps = oracle.forward(frame.transpose(2, 0, 1)[None], sd, SPEC, with_taps=True)
    for name in oracle.TAP_NAMES:
        ref = g["tap_" + name]
        got = taps[name]
        assert got.shape == ref.shape, name
        # the reference is fp32 (oneDNN); the oracle accumulates in double: a few 1e-7 relative
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5, err_msg=name)
    np.testing.assert_allclose(logits, g["logits"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(desc, g["desc_map"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(prob, g["prob"], rtol=2e-5, atol=1e-7)


def test_f2_restore_prob_map(golden_dir):
    g = load(golden_dir, "f2_restore_prob_map.npz")
    inp = np.ascontiguousarray(g["inp"])
    b, c, hc, wc = inp.shape
    out = np.empty((b, hc * 8, wc * 8), np.float32)
    oracle.lib().oracle_restore_prob_map(oracle._p(inp), oracle._p(out), b, hc, wc, 8)
    np.testing.assert_array_equal(out, g["out"])


F3_CASES = ["empty", "below_thresh", "single", "single_border", "pair_d4", "pair_d5", "pair_diag4",
            "chain", "border_suppresses", "corners", "dense_cluster", "threshold_edge",
            "rand_64x96", "rand_120x160", "rand_full_48x64"]


def f3_case(g, name):
    h, w = [int(v) for v in g[name + "_hw"]]
    pm = np.zeros(h * w, np.float32)
    pm[g[name + "_idx"]] = g[name + "_val"]
    return pm.reshape(h, w), g[name + "_out"]


@pytest.mark.parametrize("name", F3_CASES)
def test_f3_get_points(golden_dir, name):
    g = load(golden_dir, "f3_get_points.npz")
    pm, ref = f3_case(g, name)
    xs, ys, conf, _ = oracle.get_points(pm)
    assert ref.shape[0] == 3
    assert len(xs) == ref.shape[1]
    # integer work: exact
    np.testing.assert_array_equal(xs, ref[0].astype(np.int32))
    np.testing.assert_array_equal(ys, ref[1].astype(np.int32))
    np.testing.assert_array_equal(conf, ref[2].astype(np.float32))


def test_f4_get_descriptors(golden_dir):
    g = load(golden_dir, "f4_get_descriptors.npz")
    h, w = [int(v) for v in g["hw"]]
    pts = g["points"]
    out = oracle.get_descriptors(g["desc_map"][0], pts[0].astype(np.int32), pts[1].astype(np.int32), h, w)
    np.testing.assert_allclose(out.T, g["out"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(np.linalg.norm(out, axis=1), 1.0, rtol=1e-6)
    assert oracle.get_descriptors(g["desc_map"][0], [], [], h, w).shape == (0, 16)


@pytest.mark.parametrize("tag", ["qvga", "vga", "magicpoint_qvga", "gray_vga"])
def test_f5_end_to_end(golden_dir, tag):
    g = load(golden_dir, "f5_e2e_%s.npz" % tag)
    h, w = int(g["h"]), int(g["w"])
    sd = synth.make_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    frame = synth.make_frame(int(g["seed_frame"]), h, w, gray=tag.startswith("gray"))   # gray plane x3: dataset_utils.py:19-20
    de = bool(int(g["descriptor_enabled"]))
    prob, desc, logits = oracle.forward(frame.transpose(2, 0, 1)[None], sd, SPEC, descriptor_enabled=de)
    np.testing.assert_allclose(logits.ravel()[::7], g["logits_probe"], rtol=5e-5, atol=5e-5)
    np.testing.assert_allclose(desc.ravel()[::11], g["desc_map_probe"], rtol=5e-5, atol=5e-5)
    np.testing.assert_allclose(prob.ravel()[::13], g["prob_probe"], rtol=5e-5, atol=1e-7)
    xs, ys, conf, ncand = oracle.get_points(prob[0])
    # fixtures were chosen tie-safe (make_golden.py prints the margins): indices must be identical
    assert float(g["tie_margin"]) > 5e-6 and float(g["thresh_margin"]) > 1e-6
    assert ncand == int(g["n_candidates"])
    # The frames have flat regions, so distinct keypoints can carry bit-identical
    # confidences; the reference leaves the order among exact ties unspecified
    # (numpy's default argsort, nms.py:17,51), so the keypoint SET must be identical
    # and the order must agree wherever confidences differ.
    gx, gy, gc = g["points_x"].astype(np.int64), g["points_y"].astype(np.int64), g["points_conf"]
    assert len(xs) == len(gx)
    mine = np.sort(ys.astype(np.int64) * w + xs)
    theirs = np.sort(gy * w + gx)
    np.testing.assert_array_equal(mine, theirs)
    assert np.all(np.diff(conf) <= 0)
    lut = dict(zip((gy * w + gx).tolist(), gc.tolist()))
    ref_conf = np.array([lut[int(i)] for i in ys.astype(np.int64) * w + xs], np.float32)
    np.testing.assert_allclose(conf, ref_conf, rtol=2e-5)
    np.testing.assert_allclose(conf, gc, rtol=2e-5)      # same rank -> same confidence
    order = {int(i): k for k, i in enumerate((gy * w + gx).tolist())}
    perm = np.array([order[int(i)] for i in ys.astype(np.int64) * w + xs])
    if de:
        d = oracle.get_descriptors(desc[0], xs, ys, h, w)
        # row k of the reference's subset is its keypoint subset_idx[k]; find ours by pixel
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        np.testing.assert_allclose(d[inv[g["desc_subset_idx"]]], g["desc_subset"], rtol=0, atol=2e-5)
    else:
        assert not desc.any()


@pytest.mark.parametrize("tag", ["qvga", "gray_vga"])
def test_torch_cpu_restatement_against_the_reference(golden_dir, tag):
    """oracle/torch_cpu.py -- what bench.py times as the CPU baseline -- computes the reference's network."""
    import torch
    from oracle import torch_cpu
    g = load(golden_dir, "f5_e2e_%s.npz" % tag)
    h, w = int(g["h"]), int(g["w"])
    sd = synth.make_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    frame = synth.make_frame(int(g["seed_frame"]), h, w, gray=tag.startswith("gray"))
    prob, desc, logits = torch_cpu.forward(torch.from_numpy(frame.transpose(2, 0, 1)[None].copy()), torch_cpu.to_torch(sd))
    np.testing.assert_allclose(logits.numpy().ravel()[::7], g["logits_probe"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(desc.numpy().ravel()[::11], g["desc_map_probe"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(prob.numpy().ravel()[::13], g["prob_probe"], rtol=0, atol=1e-6)


def test_f6_u8_to_float(golden_dir):
    """8-bit frames -> float frames (camera.py:31, preprocess_coco.py:25, inferencewrapper.py:70-81,
    inference.py:79): the oracle against numpy's / torch's own evaluation of the reference's expressions."""
    g = np.load(os.path.join(golden_dir, "f6_u8_to_float.npz"))
    table = oracle.u8_to_float(np.arange(256, dtype=np.uint8).reshape(1, 16, 16), 0)
    np.testing.assert_array_equal(table.ravel(), g["table"])
    np.testing.assert_array_equal(oracle.u8_to_float(g["img"], 1), g["rgb"])
    np.testing.assert_array_equal(oracle.u8_to_float(g["img"], 2), g["bgr_swapped"])
    gray = oracle.u8_to_float(g["img"], 3)                 # OpenCV's 8-bit BGR2GRAY, restated (unpinned)
    assert gray.shape == (2, 1, 16, 24) and gray.min() >= 0.0 and gray.max() <= 1.0
    b, gch, r = (g["img"][..., i].astype(np.float64) for i in range(3))
    assert np.max(np.abs(gray[:, 0] * 255.0 - (0.114 * b + 0.587 * gch + 0.299 * r))) <= 0.51


def _gray(seed, h, w):
    return synth.make_batch(seed, 1, h, w, gray=True)[:, :1].copy()


def test_f7_vgg_network_against_the_reference_binary_outputs(golden_dir):
    """The reference's C++ network (superpoint::SPModel, cpp/src/model.cc) -- fixtures written by the
    reference's own source compiled unmodified (oracle/_ref/ref_vgg_forward, tests/golden/make_golden_vgg.py)."""
    spec = arch.vgg_state_dict_spec()
    names = [ln.split()[0] for ln in open(os.path.join(golden_dir, "f7_vgg_names.txt")).read().strip().splitlines()]
    assert names == list(spec.keys())
    g = np.load(os.path.join(golden_dir, "f7_vgg_32x48.npz"))
    sd = synth.make_vgg_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    prob, desc, logits = oracle.vgg_forward(_gray(int(g["seed_frame"]), 32, 48), sd, spec)
    np.testing.assert_allclose(logits, g["logits"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(desc, g["desc"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(desc, axis=1), 1.0, rtol=1e-5)
    assert prob.shape == (1, 32, 48) and 0.0 <= prob.min() and prob.max() <= 1.0
    g = np.load(os.path.join(golden_dir, "f7_vgg_qvga.npz"))
    sd = synth.make_vgg_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    prob, desc, logits = oracle.vgg_forward(_gray(int(g["seed_frame"]), int(g["h"]), int(g["w"])), sd, spec)
    np.testing.assert_allclose(logits.ravel()[::7], g["logits_probe"], rtol=0, atol=5e-5)
    np.testing.assert_allclose(desc.ravel()[::11], g["desc_probe"], rtol=0, atol=5e-6)
    assert abs(float(logits.astype(np.float64).sum()) - float(g["logits_sum"])) < 0.05


def test_vgg_oracle_against_live_reference_binary(golden_dir):
    """The reference itself on a seed of its own (fixture F7 48x64: what oracle/_ref/ref_vgg_forward returned for it)
    against the oracle; where that binary is built (oracle/Makefile.ref) and runs, also its output of now."""
    import importlib.util
    g = np.load(os.path.join(golden_dir, "f7_vgg_48x64.npz"))
    sd = synth.make_vgg_state_dict(int(g["seed_weights"]), float(g["dustbin_bias"]))
    fr = _gray(int(g["seed_frame"]), int(g["h"]), int(g["w"]))
    refs = [(g["logits"], g["desc"])]
    binpath = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_vgg_forward")
    if os.path.exists(binpath):
        specm = importlib.util.spec_from_file_location("make_golden_vgg", os.path.join(golden_dir, "make_golden_vgg.py"))
        mg = importlib.util.module_from_spec(specm)
        specm.loader.exec_module(mg)
        try:
            point, dref, _ = mg.run_reference(sd, fr)
            refs.append((point, dref))
        except Exception:  # e.g. libtorch missing on the machine running the tests: the stored outputs still hold
            pass
    prob, desc, logits = oracle.vgg_forward(fr, sd, arch.vgg_state_dict_spec())
    for point, dref in refs:
        np.testing.assert_allclose(logits, point, rtol=0, atol=2e-5)
        np.testing.assert_allclose(desc, dref, rtol=0, atol=2e-6)


def _f3b_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "f3b_get_points_random.npz"))
    for i in range(48):
        k = "c%02d" % i
        h, w = [int(v) for v in g[k + "_hw"]]
        pm = np.zeros(h * w, np.float32)
        pm[g[k + "_idx"]] = g[k + "_val"]
        yield k, pm.reshape(h, w), int(g[k + "_par"][0]), int(g[k + "_par"][1]), float(g[k + "_thr"]), g[k + "_out"]


def test_f3b_get_points_random_maps_and_settings(golden_dir):
    """48 random tie-free maps through the reference's get_points with varying nms_dist / border_remove /
    confidence_thresh (fixture F3b): indices and confidences exact."""
    n = 0
    for k, pm, nms, border, thr, ref in _f3b_cases(golden_dir):
        xs, ys, conf, _ = oracle.get_points(pm, conf_thresh=thr, nms_dist=nms, border_remove=border)
        assert len(xs) == ref.shape[1], k
        np.testing.assert_array_equal(xs, ref[0].astype(np.int32), err_msg=k)
        np.testing.assert_array_equal(ys, ref[1].astype(np.int32), err_msg=k)
        np.testing.assert_array_equal(conf, ref[2].astype(np.float32), err_msg=k)
        n += 1
    assert n == 48


def test_f4b_get_descriptors_geometries(golden_dir):
    """Fixture F4b: the reference's get_descriptors at D = 128 on wide / tall / HD-like maps."""
    g = np.load(os.path.join(golden_dir, "f4b_get_descriptors_random.npz"))
    for i in range(5):
        h, w = [int(v) for v in g["c%d_hw" % i]]
        pts = g["c%d_pts" % i]
        out = oracle.get_descriptors(g["c%d_map" % i][0], pts[0], pts[1], h, w)
        np.testing.assert_allclose(out.T, g["c%d_out" % i], rtol=0, atol=2e-6)


def test_f8_perspective_warp_against_torch_grid_sample(golden_dir):
    """Fixture F8: torch.nn.functional.grid_sample on grids built by the restated torchvision perspective formula
    (homographies.py:215-216).  Bilinear within fp32 noise; nearest identical except where the source coordinate
    lands within fp32 noise of a pixel boundary (the grid comes out of a BLAS product in torch)."""
    g = np.load(os.path.join(golden_dir, "f8_warp_perspective.npz"))
    img = g["img"]
    for i, hm in enumerate(g["homographies"]):
        got = oracle.warp_perspective(img, hm)
        np.testing.assert_allclose(got, g["bilinear_%d" % i], rtol=0, atol=2e-5)
        gn = oracle.warp_perspective(img, hm, nearest=True)
        assert np.mean(gn != g["nearest_%d" % i]) < 2e-3
    # identity homography: the identity up to the fp32 noise of the grid arithmetic (as in torch: case 0 above)
    np.testing.assert_allclose(oracle.warp_perspective(img, g["homographies"][0]), img, rtol=0, atol=1e-5)
    # erosion of an all-ones plane only eats the border (constant border 0), by the ellipse's extent
    er = oracle.erode_ellipse(np.ones((40, 56), np.float32), 4)
    assert er[4:-4, 4:-4].all() and not er[0].any() and not er[:, 0].any()
    assert er.sum() == (40 - 4 - 3) * (56 - 4 - 3)      # even-sized element, anchor (r, r): r rows/cols on one side, r - 1 on the other


def test_f9_query_image_resize_crop(golden_dir):
    """Fixture F9: make_query_image (inference.py:72-85) with torch's F.interpolate as the bilinear resize: geometry,
    BGR->RGB, crop and CHW layout of oracle_resize_crop_u8; values within the fp32 noise of the coordinate arithmetic
    (OpenCV forms the size ratio in double, torch in fp32)."""
    g = np.load(os.path.join(golden_dir, "f9_query_image.npz"))
    for i in range(4):
        th, tw = [int(v) for v in g["c%d_hw" % i]]
        got = oracle.resize_crop_u8(g["c%d_frame" % i][None], th, tw, swap_rb=True)[0]
        np.testing.assert_allclose(got, g["c%d_out" % i], rtol=0, atol=1e-5, err_msg="case %d" % i)
