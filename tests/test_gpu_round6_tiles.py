"""Round 6 (pytest -m gpu): tiles that fit the maps -- the stacked walk of the 128-channel Winograd blocks
(wblock36s_kernel), layer_in.1's conv1 on 8 x 2 Winograd tiles (wconv36p_kernel) and layer2.0 on 4 x 16 pixels
(block_mfma_kernel<4, 16, ...>) -- against round 5's tilings, which FPC_PLAN_TILES_ROUND5 ("tiles_round5") keeps.

Every Winograd tile and every output pixel sees the same operands in the same order under both plans, so the bar is BIT
EQUALITY of every activation and of the final keypoints and descriptors, not a tolerance.  All contexts run with
"no_latency_tiles", so that calls of a few frames reach the batch kernels; every case is run once more under
"guard_zones" (no store outside a tensor).  The plan hash and the packed blob are the same under both plans.
"""
import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth

pytestmark = pytest.mark.gpu

SD = synth.make_state_dict(3, dustbin_bias=4.0)
STACKED = "wblock36s_kernel<2, 4, 4>"
CONV82 = "wconv36p_kernel<8, 2, 3>"
BLOCK416 = "block_mfma_kernel<4, 16, 2, 32, 1, 4, 2, 1, 128>"
NEW = (STACKED, CONV82, BLOCK416)

_frames = {}


def frames_of(h, w, n):
    if (h, w) not in _frames or len(_frames[(h, w)]) < n:
        _frames[(h, w)] = synth.make_batch(11, n, h, w)
    return _frames[(h, w)][:n]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(frames, flags=(), want_kernels=True, **kw):
    """One detect call of `frames` on a fresh context -> dict(act: {name: [n,C,h,w]}, det: fetch(), kernels, hash, guards)."""
    from fpc_amd.engine import Engine
    n, _, h, w = frames.shape
    e = Engine(h, w, max_batch=n, plan_flags=["no_latency_tiles"] + list(flags), **kw)
    try:
        e.load_state_dict(SD)
        out = {"hash": e.plan_hash(), "blob": e.export_packed()}
        out["det"] = e.detect(frames)
        out["act"] = {name: e.activation(name, 0, n).cpu().numpy() for name in e.ACTIVATIONS}
        out["guards"] = e.check_guards() if "guard_zones" in flags else None
        out["kernels"] = set(e.kernel_names(frames)) if want_kernels else set()
    finally:
        e.close()
    return out


def assert_same_bits(got, want, what):
    assert got["hash"] == want["hash"], what
    for name in want["act"]:
        assert np.array_equal(bits(got["act"][name]), bits(want["act"][name])), (what, name)
    assert len(got["det"]) == len(want["det"])
    for f, (a, b) in enumerate(zip(got["det"], want["det"])):
        assert a[3] == b[3], (what, f)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2])), (what, f)


def check_against_round5(h, w, n, ran, not_ran=(), **kw):
    """The default plan against "tiles_round5" on the same frames, then once more under guard zones."""
    frames = frames_of(h, w, n)
    want = run(frames, ["tiles_round5"], **kw)
    assert not (want["kernels"] & set(NEW)), want["kernels"] & set(NEW)
    got = run(frames, **kw)
    for k in ran:
        assert k in got["kernels"], (k, sorted(got["kernels"]))
    for k in not_ran:
        assert k not in got["kernels"], k
    assert_same_bits(got, want, (h, w, n))
    assert np.array_equal(got["blob"], want["blob"])
    guarded = run(frames, ["guard_zones"], want_kernels=False, **kw)
    assert guarded["guards"] == 0
    assert_same_bits(guarded, want, (h, w, n, "guard_zones"))
    return got


# ---------------------------------------------------------------- 1. the stacked walk
@pytest.mark.parametrize("n", [5, 7])
def test_stacked_walk_20_row_maps(n):
    """160 x 192 images: layer2 maps of 20 x 24 (a partial tile column).  Five frames are 100 stacked rows -- seams 4, 8 and
    12 rows into a tile and on a tile edge (row 80), a last tile row of 4 rows; seven frames add seams at 100 .. 120."""
    check_against_round5(160, 192, n, [STACKED])


def test_stacked_walk_28_row_maps():
    """224 x 192 images, 28-row maps (seam offset 12).  Three frames are 84 rows = 6 tile rows either way, so the launch
    walks frame by frame; four frames are 112 rows = 7 tile rows instead of 8 and walk stacked (seams 12, 8 and 4 rows in)."""
    check_against_round5(224, 192, 3, [], [STACKED])
    check_against_round5(224, 192, 4, [STACKED])


def test_stacked_walk_two_sub_batches():
    """One call of seven frames as two sub-batches (4 + 3 frames on the default streams): each launch stacks its own frames."""
    check_against_round5(160, 192, 7, [STACKED], min_sub_batch=2)


def test_stacked_walk_each_frame_as_alone():
    """Every frame of a stacked batch against that frame run alone (one frame never stacks)."""
    n = 5
    frames = frames_of(160, 192, n)
    batch = run(frames)
    assert STACKED in batch["kernels"]
    for f in range(n):
        one = run(frames[f:f + 1], want_kernels=False)
        for name in one["act"]:
            assert np.array_equal(bits(batch["act"][name][f]), bits(one["act"][name][0])), (f, name)
        a, b = batch["det"][f], one["det"][0]
        assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2])), f


def test_stacked_walk_leaks_nothing_across_a_seam():
    """Frames of all ones next to frames of all zeros: a zero frame between two ones frames is, in every activation, the
    zero frame of an all-zeros batch -- a leak across a seam shows in its border rows -- and the batch equals round 5's."""
    n, h, w = 5, 160, 192
    mixed = np.zeros((n, 3, h, w), np.float32)
    mixed[0::2] = 1.0
    got = run(mixed)
    assert STACKED in got["kernels"]
    zeros = run(np.zeros((n, 3, h, w), np.float32), want_kernels=False)
    for name in got["act"]:
        for f in (1, 3):
            assert np.array_equal(bits(got["act"][name][f]), bits(zeros["act"][name][f])), (name, f)
        for f in (2, 4):      # ... and the ones frames among themselves (frame 0 has no frame above it)
            assert np.array_equal(bits(got["act"][name][f]), bits(got["act"][name][0])), (name, f)
    assert_same_bits(got, run(mixed, ["tiles_round5"], want_kernels=False), "ones next to zeros")


# ---------------------------------------------------------------- 2. layer_in.1's conv1 on 8 x 2 Winograd tiles
def test_conv_8x2_tiles_partial_rows():
    """288 x 128 images: layer_in maps of 18 x 8 -- one 32 x 8 tile (partial rows) instead of two 16 x 16."""
    check_against_round5(288, 128, 1, [CONV82])


def test_conv_8x2_tiles_30_row_maps():
    """480 x 128 images, two frames: 30 x 8 maps, one tile per frame instead of two."""
    check_against_round5(480, 128, 2, [CONV82])


def test_conv_8x2_tiles_not_chosen_where_they_do_not_win():
    """224 x 160 images: a 14 x 10 map is one 16 x 16 tile and two 32 x 8 tiles -- the paired block kernel's shape stays."""
    got = check_against_round5(224, 160, 1, [], [CONV82])
    assert "wblock36p_kernel<4, 4, 3>" in got["kernels"]


# ---------------------------------------------------------------- 3. layer2.0 on 4 x 16 pixels
def test_block_4x16_partial_tiles():
    """176 x 208 images, two frames: layer2.0's output is 22 x 26 -- partial tile rows and columns."""
    check_against_round5(176, 208, 2, [BLOCK416])


# ---------------------------------------------------------------- all three at the headline geometry
@pytest.mark.parametrize("n", [1, 2, 4])
def test_vga(n):
    """480 x 640: 60 x 80 and 30 x 40 maps.  Every call takes the 4 x 16 block and the 8 x 2 tiles; one frame never stacks,
    two frames are 120 rows = 8 tile rows either way, four are 240 rows = 15 tile rows instead of 16 and walk stacked."""
    check_against_round5(480, 640, n, [BLOCK416, CONV82] + ([STACKED] if n == 4 else []), [] if n == 4 else [STACKED])


# ---------------------------------------------------------------- the C++ network's conv-only 128-channel layers stack too
def test_stacked_walk_conv_only_layers_of_the_vgg_network():
    """arch="vgg": conv4a / conv4b are conv-only 128-channel launches on 20 x 24 maps at 160 x 192 -- five frames walk stacked
    (the conv-only store path behind the same halo).  Dense maps, keypoints and descriptors against "tiles_round5", bit for bit."""
    from fpc_amd.engine import Engine
    n, h, w = 5, 160, 192
    sd = synth.make_vgg_state_dict(8, 3.0)
    frames = synth.make_batch(21, n, h, w, gray=True)[:, :1].copy()
    out = {}
    for flags in (("tiles_round5",), (), ("guard_zones",)):
        e = Engine(h, w, max_batch=n, in_channels=1, arch="vgg", plan_flags=["no_latency_tiles"] + list(flags))
        try:
            e.load_state_dict(sd)
            dense = [t.cpu().numpy() for t in e.forward(frames)]
            det = e.detect(frames)
            guards = e.check_guards() if "guard_zones" in flags else 0
            out[flags] = (dense, det, set(e.kernel_names(frames)), e.plan_hash(), guards)
        finally:
            e.close()
    want = out[("tiles_round5",)]
    assert STACKED not in want[2] and STACKED in out[()][2], sorted(out[()][2])
    for flags in ((), ("guard_zones",)):
        dense, det, _, ph, guards = out[flags]
        assert ph == want[3] and guards == 0
        for a, b in zip(dense, want[0]):
            assert np.array_equal(bits(a), bits(b)), flags
        for f, (a, b) in enumerate(zip(det, want[1])):
            assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2])), (flags, f)
