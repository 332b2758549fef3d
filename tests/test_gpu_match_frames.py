"""Batched descriptor matching on the GPU (fpc_match_frames / fpc_first_within_frames): a whole detect batch matched in
one asynchronous call, frame by frame the same as fpc_match / fpc_first_within on the same pair (indices identical,
distances bit-equal), plus Lowe's ratio test against the float64 restatement of tests/test_match_frames.py.
Synthetic weights at QVGA, 8 frames per batch, every context under the canary zones.  Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_match_frames import frames_rule

pytestmark = pytest.mark.gpu

H, W, N = 240, 320, 8
FPC_E_INVALID = -1


def engine(h=H, w=W, b=N, **kw):
    from fpc_amd.engine import Engine
    kw.setdefault("plan_flags", ["guard_zones"])
    return Engine(h, w, max_batch=b, **kw)


def _unit(a):
    a = np.asarray(a, np.float32)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def qvga():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(conf_thresh=0.001)
    e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(300, N, H, W))
    desc = [r[2] for r in res]
    assert min(len(d) for d in desc) > 1000, [len(d) for d in desc]
    assert any(len(d) % 128 for d in desc)
    rng = np.random.Generator(np.random.PCG64(3))
    src = desc[2]
    planted = _unit(src[rng.permutation(len(src))[:400]] + rng.normal(0, 0.02, (400, 128)))
    keys = {"real": desc[5].copy(), "planted": planted}
    yield e, desc, keys
    assert e.check_guards() == 0
    e.close()


def _assert_frame_equals_pair(e, m, d, q, t, cross, md):
    om, od = e.match(q, t, cross, md) if len(t) else (np.full(len(q), -1, np.int32), np.full(len(q), np.inf, np.float32))
    np.testing.assert_array_equal(m, om)
    if len(q) and len(t):
        np.testing.assert_allclose(d, od, rtol=0, atol=1e-6)
    with np.errstate(invalid="ignore"):
        assert ((d == od) | (np.abs(d - od) <= 1e-6)).all()


def test_key_pairing_equals_pairwise_match(qvga):
    e, desc, keys = qvga
    for name, key in keys.items():
        for cross, md in ((True, 0.0), (False, 0.0), (True, 0.7), (False, 0.7)):
            got = e.match_frames(N, key=key, pairing="key", cross_check=cross, max_dist=md)
            for f in range(N):
                m, d = got[f]
                assert len(m) == len(desc[f])
                _assert_frame_equals_pair(e, m, d, desc[f], key, cross, md)
        m, _ = e.match_frames(N, key=key, cross_check=True)[2]
        if name == "planted":
            assert (m >= 0).sum() >= 100                                             # planted pairs survive the cross check
    m, d = e.match_frames_async(N, key=keys["real"])
    e.sync()
    cnt = e.counts(N)[0]
    m, d = m.cpu().numpy(), d.cpu().numpy()
    for f in range(N):
        assert (m[f, cnt[f]:] == -1).all() and np.isinf(d[f, cnt[f]:]).all()        # rows past count[f]


def test_previous_pairing_and_chaining_through_keep_frame(qvga):
    import torch
    e, desc, keys = qvga
    key = keys["planted"]
    got = e.match_frames(N, key=key, pairing="previous", cross_check=True)
    for f in range(N):
        _assert_frame_equals_pair(e, got[f][0], got[f][1], desc[f], desc[f - 1] if f else key, True, 0.0)
    got = e.match_frames(N, key=None, pairing="previous", cross_check=False, max_dist=0.7)
    assert (got[0][0] == -1).all() and np.isinf(got[0][1]).all()
    for f in range(1, N):
        _assert_frame_equals_pair(e, got[f][0], got[f][1], desc[f], desc[f - 1], False, 0.7)
    # two batches chained on the device: keep the last frame of batch 1, detect batch 2, match it against that frame --
    # no host synchronisation between the first match call and the second
    frames2 = torch.from_numpy(synth.make_batch(400, N, H, W)).to(e.torch_device).contiguous()
    frames1 = torch.from_numpy(synth.make_batch(300, N, H, W)).to(e.torch_device).contiguous()
    torch.cuda.synchronize()
    e.detect_async(frames1, N)
    m1, d1 = e.match_frames_async(N, key=key, pairing="previous")
    kept = e.keep_frame(N - 1)
    e.detect_async(frames2, N)
    m2, d2 = e.match_frames_async(N, key=kept, pairing="previous", ratio=0.9)
    e.sync()
    res2 = e.fetch(N)
    desc2 = [r[2] for r in res2]
    cnt1 = np.array([len(d) for d in desc])
    m1, m2, d2 = m1.cpu().numpy(), m2.cpu().numpy(), d2.cpu().numpy()
    for f in range(N):
        _assert_frame_equals_pair(e, m1[f, :cnt1[f]], d1.cpu().numpy()[f, :cnt1[f]], desc[f], desc[f - 1] if f else key,
                                  True, 0.0)
    assert int(kept[1].cpu()[0]) == len(desc[N - 1])
    np.testing.assert_array_equal(kept[0][:len(desc[N - 1])].cpu().numpy(), desc[N - 1])
    for f in range(N):
        t = desc2[f - 1] if f else desc[N - 1]
        om, od = e.match(desc2[f], t, True)
        k = len(desc2[f])
        np.testing.assert_array_equal(d2[f, :k], od)
        assert ((m2[f, :k] == om) | (m2[f, :k] == -1)).all() and (m2[f, k:] == -1).all()
    e.detect(synth.make_batch(300, N, H, W))         # (the module's later tests see batch 1 again)


def _ratio_exclusions(d1, d2, ratio):
    return (np.abs(d1 - ratio * d2) < 1e-5) | (np.abs(d2 - d1) < 2e-5)


def test_ratio_test_against_the_float64_rule(qvga):
    e, desc, keys = qvga
    counts = np.array([len(d) for d in desc])
    cap = e.capacity
    stack = np.zeros((N, cap, 128), np.float32)
    for f in range(N):
        stack[f, :counts[f]] = desc[f]
    for name, key in keys.items():
        for pairing, pcode in (("key", 0), ("previous", 1)):
            for cross, ratio in ((False, 0.8), (True, 0.8), (False, 0.95)):
                m, d = e.match_frames_async(N, key=key, pairing=pairing, cross_check=cross, ratio=ratio)
                e.sync()
                m, d = m.cpu().numpy(), d.cpu().numpy()
                rm, rd1, rd2 = frames_rule(stack, counts, key, pcode, cross, 0.0, ratio)
                for f in range(N):
                    k = counts[f]
                    ok = ~_ratio_exclusions(rd1[f, :k], rd2[f, :k], ratio)
                    np.testing.assert_array_equal(m[f, :k][ok], rm[f, :k][ok])
                    # (fp32 |q|^2 + |t|^2 - 2 q.t carries ~1e-7 absolute on d^2: compared as squares, as near 0 the
                    # square root magnifies it)
                    np.testing.assert_allclose(d[f, :k].astype(np.float64) ** 2, rd1[f, :k] ** 2, rtol=0, atol=2e-6)
                    assert (m[f, k:] == -1).all()
                assert (m >= 0).sum() > 0
    # ties on planted duplicates: frame 4's own rows as the key, row 5 repeated behind it
    q = desc[4]
    dup = np.concatenate([q[:200], q[5:6]])
    got = e.match_frames(N, key=dup, cross_check=False)[4][0]
    assert got[5] == 5                                                               # the lower index wins
    got = e.match_frames(N, key=dup, cross_check=False, ratio=0.99)[4][0]
    assert got[5] == -1                                                              # best and second best tie
    one = np.ascontiguousarray(q[5:6])
    got = e.match_frames(N, key=one, cross_check=False, ratio=0.8)
    assert all((m == -1).all() for m, _ in got)                                      # one train row: no second best
    got = e.match_frames(N, key=one, cross_check=False)
    assert all((m == 0).all() for m, _ in got)


def test_first_within_frames_equals_pairwise(qvga):
    e, desc, keys = qvga
    for key in (keys["real"], keys["planted"], keys["planted"][:130]):
        for tol in (0.8, 0.3):
            got = e.first_within_frames(N, key, tol)
            for f in range(N):
                np.testing.assert_array_equal(got[f], e.first_within(key, desc[f], tol))
        out, _ = e.first_within_frames_async(N, key, 0.8)
        e.sync()
        assert (out.cpu().numpy()[:, len(key):] == -1).all()


def test_key_count_is_read_on_the_device(qvga):
    import torch
    e, desc, keys = qvga
    kd = torch.from_numpy(keys["real"]).to(e.torch_device)
    kc = torch.tensor([len(keys["real"])], dtype=torch.int32, device=e.torch_device)
    torch.cuda.synchronize()
    m1, _ = e.match_frames_async(N, key=(kd, kc), cross_check=True)
    with torch.cuda.stream(e.torch_stream()):
        kc.fill_(50)                                     # on the ctx stream, between the two calls
    m2, _ = e.match_frames_async(N, key=(kd, kc), cross_check=True)
    f1, _ = e.first_within_frames_async(N, (kd, kc), 0.8)
    with torch.cuda.stream(e.torch_stream()):
        kc.fill_(0)
    m3, d3 = e.match_frames_async(N, key=(kd, kc))
    e.sync()
    m1, m2, f1, m3 = m1.cpu().numpy(), m2.cpu().numpy(), f1.cpu().numpy(), m3.cpu().numpy()
    for f in range(N):
        k = len(desc[f])
        np.testing.assert_array_equal(m1[f, :k], e.match(desc[f], keys["real"], True)[0])
        np.testing.assert_array_equal(m2[f, :k], e.match(desc[f], keys["real"][:50], True)[0])
        np.testing.assert_array_equal(f1[f, :50], e.first_within(keys["real"][:50], desc[f], 0.8))
        assert (f1[f, 50:] == -1).all()
    assert (m3 == -1).all() and np.isinf(d3.cpu().numpy()).all()                    # nkey = 0


def test_outputs_are_deterministic(qvga):
    e, desc, keys = qvga
    outs = []
    for _ in range(2):
        m, d = e.match_frames_async(N, key=keys["planted"], pairing="previous", cross_check=True, max_dist=0.9, ratio=0.9)
        f, _ = e.first_within_frames_async(N, keys["planted"], 0.8)
        e.sync()
        outs.append((m.cpu().numpy(), d.cpu().numpy().view(np.uint32), f.cpu().numpy()))
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, b)


def test_bad_arguments_are_refused(qvga):
    import torch
    e, desc, keys = qvga
    lib = _lib.load()
    kd = torch.from_numpy(keys["real"]).to(e.torch_device)
    kc = torch.tensor([len(keys["real"])], dtype=torch.int32, device=e.torch_device)
    out = torch.empty((N, e.capacity), dtype=torch.int32, device=e.torch_device)
    torch.cuda.synchronize()
    ctx, kp, cp, op = e._ctx, kd.data_ptr(), kc.data_ptr(), out.data_ptr()
    mf = lambda *a: lib.fpc_match_frames(ctx, *a)                           # noqa: E731
    assert mf(N, 0, kp, cp, 1, 0.0, 0.0, op, None) == 0
    assert mf(N + 1, 0, kp, cp, 1, 0.0, 0.0, op, None) == FPC_E_INVALID      # more frames than the last call
    assert mf(0, 0, kp, cp, 1, 0.0, 0.0, op, None) == FPC_E_INVALID
    assert mf(N, 2, kp, cp, 1, 0.0, 0.0, op, None) == FPC_E_INVALID          # pairing
    assert mf(N, 0, kp, cp, 1, 0.0, 1.5, op, None) == FPC_E_INVALID          # ratio outside [0, 1]
    assert mf(N, 0, kp, cp, 1, 0.0, -0.1, op, None) == FPC_E_INVALID
    assert mf(N, 0, kp, cp, 1, -1.0, 0.0, op, None) == FPC_E_INVALID         # max_dist < 0
    assert mf(N, 0, None, None, 1, 0.0, 0.0, op, None) == FPC_E_INVALID      # no key in KEY mode
    assert mf(N, 0, kp, None, 1, 0.0, 0.0, op, None) == FPC_E_INVALID        # a key without its count
    assert mf(N, 0, kp, cp, 1, 0.0, 0.0, None, None) == FPC_E_INVALID        # no output
    assert mf(N, 1, None, None, 1, 0.0, 0.0, op, None) == 0                  # PREVIOUS needs no key
    fw = lambda *a: lib.fpc_first_within_frames(ctx, *a)                    # noqa: E731
    assert fw(N, kp, cp, ctypes.c_float(0.8), op) == 0
    assert fw(N, kp, cp, ctypes.c_float(-0.1), op) == FPC_E_INVALID
    assert fw(N, None, None, ctypes.c_float(0.8), op) == FPC_E_INVALID
    assert fw(N, kp, cp, ctypes.c_float(0.8), None) == FPC_E_INVALID
    assert fw(N + 1, kp, cp, ctypes.c_float(0.8), op) == FPC_E_INVALID
    e.sync()
    # a detect of fewer frames bounds n
    e.detect(synth.make_batch(300, 2, H, W))
    assert mf(3, 0, kp, cp, 1, 0.0, 0.0, op, None) == FPC_E_INVALID
    assert mf(2, 0, kp, cp, 1, 0.0, 0.0, op, None) == 0
    # fpc_get_points without a descriptor map produced no descriptors
    prob = torch.zeros((2, H, W), device=e.torch_device)
    e.get_points(prob)
    assert mf(2, 0, kp, cp, 1, 0.0, 0.0, op, None) == FPC_E_INVALID
    assert fw(2, kp, cp, ctypes.c_float(0.8), op) == FPC_E_INVALID
    e.sync()
    e.detect(synth.make_batch(300, N, H, W))         # (the module's later tests see batch 1 again)
    # a context without the descriptor head
    d = engine(descriptor_enabled=False, b=2)
    d.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
    d.detect(synth.make_batch(300, 2, H, W))
    assert lib.fpc_match_frames(d._ctx, 2, 1, None, None, 1, 0.0, 0.0, op, None) == FPC_E_INVALID
    assert lib.fpc_first_within_frames(d._ctx, 2, kp, cp, ctypes.c_float(0.8), op) == FPC_E_INVALID
    assert d.check_guards() == 0
    d.close()
    with pytest.raises(_lib.FpcError):
        e.match_frames(N, key=None, pairing="key")


def test_empty_frame_from_get_points(qvga):
    """A frame with no keypoints inside the batch: fpc_get_points with an all-zero probability map for that frame."""
    import torch
    e, desc, keys = qvga
    frames = synth.make_batch(300, N, H, W)
    prob, dmap, _ = e.forward(frames)
    prob[3].zero_()
    res = e.get_points(prob, dmap)
    d = [r[2] for r in res]
    assert len(d[3]) == 0 and len(d[2]) > 0 and len(d[4]) > 0
    key = keys["planted"]
    for pairing in ("key", "previous"):
        got = e.match_frames(N, key=key, pairing=pairing, cross_check=True)
        for f in range(N):
            t = d[f - 1] if pairing == "previous" and f else key
            _assert_frame_equals_pair(e, got[f][0], got[f][1], d[f], t, True, 0.0)
    m, dd = e.match_frames_async(N, key=key, pairing="previous")
    e.sync()
    assert (m[3].cpu() == -1).all() and (m[4].cpu() == -1).all() and torch.isinf(dd[4, :len(d[4])].cpu()).all()
    fw = e.first_within_frames(N, key, 0.8)
    assert (fw[3] == -1).all()
    for f in (2, 4):
        np.testing.assert_array_equal(fw[f], e.first_within(key, d[f], 0.8))
    e.detect(synth.make_batch(300, N, H, W))


@pytest.mark.parametrize("variant", ["full_capacity", "vgg", "bf16"])
def test_other_contexts(variant):
    """count == cap (a small max_keypoints), FPC_ARCH_VGG (D = 256), an FPC_BF16 context."""
    if variant == "vgg":
        e = engine(in_channels=1, arch="vgg")
        e.load_state_dict(synth.make_vgg_state_dict(4, 3.0))
        frames = synth.make_batch(300, N, H, W, gray=True)[:, :1]
    else:
        kw = {"max_keypoints": 200} if variant == "full_capacity" else {"dtype": "bf16"}
        e = engine(conf_thresh=0.001, **kw)
        e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
        frames = synth.make_batch(300, N, H, W)
    desc = [r[2] for r in e.detect(np.ascontiguousarray(frames))]
    dim = 256 if variant == "vgg" else 128
    assert all(x.shape[1] == dim for x in desc) and sum(len(x) for x in desc) > 100
    if variant == "full_capacity":
        assert e.capacity == 200 and all(len(x) == 200 for x in desc)
    key = desc[1][: len(desc[1]) - 3]
    for pairing in ("key", "previous"):
        for cross in (True, False):
            got = e.match_frames(N, key=key, pairing=pairing, cross_check=cross)
            for f in range(N):
                t = desc[f - 1] if pairing == "previous" and f else key
                _assert_frame_equals_pair(e, got[f][0], got[f][1], desc[f], t, cross, 0.0)
    got = e.first_within_frames(N, key, 0.8)
    for f in range(N):
        np.testing.assert_array_equal(got[f], e.first_within(key, desc[f], 0.8))
    assert e.check_guards() == 0
    e.close()


def test_batch_correspondences_equal_per_frame(qvga):
    from fpc_amd.inference import get_best_correspondences, get_best_correspondences_batch
    e, desc, keys = qvga
    res = e.fetch(N)
    stop = np.hstack((np.zeros((len(keys["planted"]), 3)), keys["planted"]))
    batch = get_best_correspondences_batch(stop, e, N)
    for f in range(N):
        xy, conf, d, _ = res[f]
        feats = np.hstack((xy.astype(np.float64), conf[:, None].astype(np.float64), d))
        rows, idx = get_best_correspondences(stop, feats, e)
        np.testing.assert_array_equal(batch[f][1], idx)
        np.testing.assert_array_equal(batch[f][0], rows)
