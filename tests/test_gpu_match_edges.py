"""The five 64 x 64 distance tiles on the GPU, held to the float64 rule of tests/test_match_edges.py at tile edges, on exact
ties and on non-finite rows: fpc_match / fpc_first_within on explicit pairs, fpc_match_frames / fpc_first_within_frames,
fpc_match_bank and fpc_match_bank_topk on an fp32 bank, the bf16 bank, the guided entry points (bit-equal to
fpc_match_frames where every pair is a candidate, on non-finite rows too) and a D = 256 context.

The scenes ("edges", "ties", "nonfinite": counts of 0, 1, 2, 63 .. 65, 127 .. 129, 191 .. 193, 255 .. 257 and 384 rows, the last
row and the first row of the last tile winners, bit-equal rows across waves, rounds and workgroups, NaN / Inf rows at 0, 63,
64 and n - 1) are written straight into the library's device results as tests/test_gpu_match_guided.py's plant does: no
network forward.  Contexts: eight frames, capacity 384, under the canary zones; 120 x 160 at D = 256 and 128 x 160 at D = 128,
whose descriptor head takes multiples of 16 only (the scenes' pixels lie inside 120 x 160).

Bars: indices exact outside the rows the rule leaves out; dist^2 within 2e-6 of float64 at D = 128; rows past the count and
rows without a finite distance exactly -1 / +inf.  At D = 256: twice the largest error of the same expression in plain
fp32 on the CPU, never more than 8 D 2^-24 (DESIGN.md section 7 has the measured figures).  The bf16 bank: the derived
8 D 2^-24 of tests/test_gpu_match_bank_bf16.py on the rounded rows.  Every case prints the device's largest d^2 error beside
the CPU's fp32 one; nothing is asserted from their ratio.  Need a real MI355X: pytest -m gpu"""
import functools

import numpy as np
import pytest

import fpc_amd  # noqa: F401

from tests.test_gpu_match_bank import _expect_best
from tests.test_gpu_match_guided import BIG, plant
from tests.test_match_edges import (BAR_D128, CAP, EXPLICIT, FRAME_H, FRAME_W, OPTIONS, PAIR_KEY, PAIR_PREVIOUS, TIE_OPTIONS,
                                    TOLERANCES, all_pairs, analytic_bar, compare, compare_first, explicit_pair, fp32_error,
                                    reference, rows_of, scene_of, train_of)
from tests.test_match_epipolar import ALL_PASS, epipolar_gate
from tests.test_match_guided import gate
from tests.test_match_pose import all_pass_radius, pose_gate

pytestmark = pytest.mark.gpu

N = 8
KVEC = (100.0, 100.0, 80.0, 60.0)
BF16_OPTIONS = ((True, 0.7, 0.0), (False, 0.7, 0.0), (True, 0.0, 0.8), (False, 0.0, 0.8))
TIES_EXPLICIT = ((("frame", 0, 0), ("key", 2)), (("frame", 0, 1), ("key", 0)), (("frame", 0, 3), ("key", 1)),
                 (("frame", 0, 4), ("key", 3)))
SCENES = ("edges", "ties", "nonfinite")


def _engine(h=FRAME_H, **kw):
    from fpc_amd.engine import Engine
    e = Engine(h, FRAME_W, max_batch=N, plan_flags=["guard_zones"], max_keypoints=CAP, **kw)
    assert e.capacity == CAP
    return e


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = _engine(128)                                                 # (fpc_create refuses 120 rows with the descriptor head)
    assert e.desc_dim == 128
    e.pnp_reserve()                                                  # (the pose-guided call's workspace)
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _options(name):
    return TIE_OPTIONS if name == "ties" else OPTIONS


@functools.lru_cache(maxsize=None)
def _cpu_fp32(name, dim):
    """The plain fp32 evaluation's largest d^2 error on the scene's explicit pairs and PREVIOUS pairs (computed once)."""
    scene = scene_of(name, dim)
    pairs = list(TIES_EXPLICIT) if name == "ties" else [explicit_pair(scene, nq, nt) for nq, nt in EXPLICIT]
    return fp32_error(scene, pairs + all_pairs(scene, ("previous",)))


def _report(label, worst, name, dim, bar):
    print("%-60s d^2 error: device %.3e, CPU fp32 %.3e (bar %.3e)" % (label, worst, _cpu_fp32(name, dim), bar))


def _explicit(e, name, dim, bar):
    scene = scene_of(name, dim)
    pairs = TIES_EXPLICIT if name == "ties" else [explicit_pair(scene, nq, nt) for nq, nt in EXPLICIT]
    worst = 0.0
    for q, t in pairs:
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        for cross in (True, False):
            for md in (0.0, 0.7):
                m, d = e.match(qr, tr, cross_check=cross, max_dist=md)
                label = "%s fpc_match %s %s %s" % (name, q, t, (cross, md))
                worst = max(worst, compare(m, d, reference(name, dim, q, t, (cross, md, 0.0)), bar, label)[0])
        for tol in TOLERANCES:                                       # key = the train set, cur = the query set
            compare_first(e.first_within(tr, qr, tol), tr, qr, tol, "%s fpc_first_within %s %s %s" % (name, t, q, tol))
    _report("%s D=%d fpc_match, explicit pairs" % (name, dim), worst, name, dim, bar)


@pytest.mark.parametrize("name", SCENES)
def test_explicit_pairs(ctx, name):
    _explicit(ctx, name, 128, BAR_D128)


def test_match_without_train_rows_is_minus_one_and_infinity(ctx):
    import torch
    from fpc_amd import _lib
    e = ctx
    q = torch.from_numpy(rows_of(scene_of("edges"), ("frame", 0, 7)).copy()).to(e.torch_device)
    m = torch.full((len(q),), 7, dtype=torch.int32, device=e.torch_device)
    d = torch.full((len(q),), 7.0, dtype=torch.float32, device=e.torch_device)
    torch.cuda.synchronize()
    for cross in (1, 0):
        _lib.check(e._l.fpc_match(e._ctx, q.data_ptr(), len(q), q.data_ptr(), 0, cross, 0.0, m.data_ptr(), d.data_ptr()),
                   "fpc_match")
        e.sync()
        assert (m.cpu().numpy() == -1).all() and (d.cpu().numpy() == np.inf).all()


def _frames(e, name, dim, bar, b, batch):
    scene = scene_of(name, dim)
    counts = batch["counts"]
    plant(e, batch)
    worst = 0.0
    cases = [("key", PAIR_KEY, k) for k in range(len(scene["keys"]))] + [("previous", PAIR_PREVIOUS, len(scene["keys"]) - 1),
                                                                        ("previous", PAIR_PREVIOUS, None)]
    for pairing, pcode, k in cases:
        key = None if k is None else scene["keys"][k][0]
        for opt in _options(name):
            m, d = e.match_frames_async(N, key=key, pairing=pairing, cross_check=opt[0], max_dist=opt[1], ratio=opt[2])
            e.sync()
            m, d = m.cpu().numpy(), d.cpu().numpy()
            for f, n in enumerate(counts):
                q, t = ("frame", b, f), train_of(scene, b, f, pcode, k)
                label = "%s batch %d %s key=%s %s frame %d" % (name, b, pairing, k, opt, f)
                worst = max(worst, compare(m[f, :n], d[f, :n], reference(name, dim, q, t, opt), bar, label)[0])
                assert (m[f, n:] == -1).all() and (d[f, n:] == np.inf).all(), label
        if key is not None and pcode == PAIR_KEY:
            for tol in TOLERANCES:
                out, _ = e.first_within_frames_async(N, key, tol)
                e.sync()
                out = out.cpu().numpy()
                for f, n in enumerate(counts):
                    compare_first(out[f, :len(key)], key, batch["desc"][f, :n], tol,
                                  "%s batch %d first_within_frames key=%s tol=%s frame %d" % (name, b, k, tol, f))
                    assert (out[f, len(key):] == -1).all()
    _report("%s D=%d batch %d fpc_match_frames" % (name, dim, b), worst, name, dim, bar)


@pytest.mark.parametrize("name,b", [("edges", 0), ("edges", 1), ("ties", 0), ("nonfinite", 0), ("nonfinite", 1)])
def test_match_frames_and_first_within_frames(ctx, name, b):
    _frames(ctx, name, 128, BAR_D128, b, scene_of(name)["batches"][b])


def _store(e, scene):
    for s, (d, p) in enumerate(scene["slots"]):
        e.bank_store_rows(s, d, p)
    e.sync()


def _bank_scores(name, b, opt, score, bf16=False):
    """score [N][slots] against the rule's survivors: equal on (frame, slot) pairs without left-out rows, else within their
    number -> the left-out rows in all."""
    scene = scene_of(name)
    left = 0
    for f in range(N):
        for s in range(len(scene["slots"])):
            rm, _, _, out = reference(name, 128, ("frame", b, f), ("slot", s), opt, bf16)
            want = int((rm >= 0).sum())
            assert abs(int(score[f, s]) - want) <= out.sum(), (name, b, f, s, opt, int(score[f, s]), want, int(out.sum()))
            left += int(out.sum())
    return left


@pytest.mark.parametrize("name,b", [("edges", 0), ("edges", 1), ("ties", 0), ("nonfinite", 0), ("nonfinite", 1)])
def test_bank_and_topk(ctx, name, b):
    e, scene = ctx, scene_of(name)
    batch = scene["batches"][b]
    counts = batch["counts"]
    plant(e, batch)
    e.bank_create(len(scene["slots"]), CAP)
    try:
        assert e.bank_topk_reserve(2) > 0
        _store(e, scene)
        worst = 0.0
        for opt in _options(name):
            score, best, m, d = e.match_bank_async(N, cross_check=opt[0], max_dist=opt[1], ratio=opt[2])
            tscore, cs, csc, tm, td = e.match_bank_topk_async(N, 2, cross_check=opt[0], max_dist=opt[1], ratio=opt[2])
            e.sync()
            score, best, m, d, tscore, cs, csc, tm, td = (x.cpu().numpy() for x in (score, best, m, d, tscore, cs, csc, tm, td))
            _bank_scores(name, b, opt, score)
            np.testing.assert_array_equal(tscore, score)
            np.testing.assert_array_equal(best, _expect_best(score))
            order = np.argsort(-score, axis=1, kind="stable")[:, :2]               # descending score, the lower slot first
            top = np.take_along_axis(score, order, 1)
            np.testing.assert_array_equal(cs, np.where(top >= 1, order, -1))
            np.testing.assert_array_equal(csc, np.where(top >= 1, top, 0))
            for f, n in enumerate(counts):
                for slot, tab in ((best[f], (m[f], d[f])), (cs[f, 0], (tm[f, 0], td[f, 0])), (cs[f, 1], (tm[f, 1], td[f, 1]))):
                    label = "%s batch %d bank %s frame %d slot %d" % (name, b, opt, f, slot)
                    t = ("slot", int(slot)) if slot >= 0 else None
                    ref = reference(name, 128, ("frame", b, f), t, opt)
                    worst = max(worst, compare(tab[0][:n], tab[1][:n], ref, BAR_D128, label)[0])
                    assert (tab[0][n:] == -1).all() and (tab[1][n:] == np.inf).all(), label
        _report("%s batch %d fpc_match_bank / _topk" % (name, b), worst, name, 128, BAR_D128)
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()


@pytest.mark.parametrize("name,b", [("edges", 0), ("edges", 1), ("ties", 0), ("nonfinite", 0), ("nonfinite", 1)])
def test_bf16_bank(ctx, name, b):
    """Against bank_rule_bf16's construction -- the pair rule, masked, on rows rounded as the store rounds them -- with its
    derived tolerance: d^2 within 8 D 2^-24, rows within twice that of flipping left out (at most 2 % of all)."""
    import torch
    from tests.test_match_bank_bf16 import bf16_bits
    e, scene = ctx, scene_of(name)
    batch = scene["batches"][b]
    counts = batch["counts"]
    plant(e, batch)
    e.bank_create(len(scene["slots"]), CAP, format="bf16")
    try:
        _store(e, scene)
        bd, _, bc = e.bank_view()
        bits = bd.view(torch.int16).cpu().numpy().view(np.uint16)
        for s, (rows, _) in enumerate(scene["slots"]):
            assert int(bc[s]) == len(rows)
            np.testing.assert_array_equal(bits[s, :len(rows)], bf16_bits(rows))       # (a NaN is stored as 0x7FC0)
        bar, worst, left, total = analytic_bar(128), 0.0, 0, 0
        eye = np.tile(np.eye(3, dtype=np.float32), (N, 1, 1))
        for opt in BF16_OPTIONS:
            score, best, m, d = e.match_bank_async(N, cross_check=opt[0], max_dist=opt[1], ratio=opt[2])
            e.sync()
            score, best, m, d = (x.cpu().numpy() for x in (score, best, m, d))
            left += _bank_scores(name, b, opt, score, bf16=True)
            np.testing.assert_array_equal(best, _expect_best(score))
            for s in range(len(scene["slots"])):                  # every frame against slot s: the guided call, every pair a candidate
                slot = torch.full((N,), s, dtype=torch.int32, device=e.torch_device)
                gm, gd = e.match_bank_guided_async(N, slot, eye, BIG, cross_check=opt[0], max_dist=opt[1], ratio=opt[2])
                e.sync()
                gm, gd = gm.cpu().numpy(), gd.cpu().numpy()
                for f, n in enumerate(counts):
                    label = "%s batch %d bf16 bank %s frame %d slot %d" % (name, b, opt, f, s)
                    ref = reference(name, 128, ("frame", b, f), ("slot", s), opt, True)
                    worst = max(worst, compare(gm[f, :n], gd[f, :n], ref, bar, label, share=1.0)[0])
                    assert (gm[f, n:] == -1).all() and (gd[f, n:] == np.inf).all(), label
                    total += int(n)
                    if best[f] == s:
                        np.testing.assert_array_equal(m[f], gm[f])
                        np.testing.assert_array_equal(d[f].view(np.uint32), gd[f].view(np.uint32))
        print("%s batch %d bf16 bank: d^2 error %.3e (bar %.3e), %d of %d rows left out" % (name, b, worst, bar, left, total))
        assert left <= 0.02 * total
        assert e.check_guards() == 0
    finally:
        e.bank_destroy()


def _landmarks(xy):
    """Points in front of the identity camera KVEC that project onto the pixels xy."""
    z = 2.0 + (np.arange(len(xy)) % 7).astype(np.float64)
    return np.stack([(xy[:, 0] - KVEC[2]) / KVEC[0] * z, (xy[:, 1] - KVEC[3]) / KVEC[1] * z, z], 1).astype(np.float32)


@pytest.mark.parametrize("b", [0, 1])
def test_guided_entry_points_equal_match_frames_on_nonfinite_rows(ctx, b):
    """Every pair a candidate (asserted from the gates' restatements): each guided call's table is fpc_match_frames', bit for
    bit -- on rows that hold NaN and Inf too, through the two tiles fpc_match_frames does not share."""
    e, scene = ctx, scene_of("nonfinite")
    batch = scene["batches"][b]
    xy, counts = batch["xy"], batch["counts"]
    plant(e, batch)
    eye = np.tile(np.eye(3, dtype=np.float32).reshape(9), (N, 1))
    fund = np.tile(np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32), (N, 1))   # a pure sideways translation
    rs, ts = eye.copy(), np.zeros((N, 3), np.float32)
    for k in (4, 3, 1):                                             # 384 and 257 rows, and the all-NaN key
        key, key_xy = scene["keys"][k]
        xyz = _landmarks(key_xy)
        big = all_pass_radius(rs, ts, KVEC, xy, counts, [(key, xyz, None)] * N)
        assert big is not None
        for pairing, pcode in (("key", PAIR_KEY), ("previous", PAIR_PREVIOUS)):
            for f, n in enumerate(counts):                           # the premise, by the restatements
                txy = xy[f - 1, :counts[f - 1]] if pcode == PAIR_PREVIOUS and f > 0 else key_xy
                assert gate(eye[f], xy[f, :n], txy, BIG)[0].all() and epipolar_gate(fund[f], xy[f, :n], txy, ALL_PASS)[0].all()
                assert pose_gate(rs[f], ts[f], KVEC, xy[f, :n], xyz, None, big)[0].all()
            for cross, md, ratio in ((True, 0.0, 0.0), (False, 0.0, 0.0), (True, 0.7, 0.8)):
                opt = dict(cross_check=cross, max_dist=md, ratio=ratio)
                um, ud = e.match_frames_async(N, key=key, pairing=pairing, **opt)
                calls = {"guided": e.match_frames_guided_async(N, eye, BIG, key=key, key_xy=key_xy, pairing=pairing, **opt),
                         "guided_cells": e.match_frames_guided_cells_async(N, eye, BIG, key=key, key_xy=key_xy,
                                                                           pairing=pairing, **opt),
                         "guided_epipolar": e.match_frames_guided_epipolar_async(N, fund, ALL_PASS, key=key, key_xy=key_xy,
                                                                                 pairing=pairing, **opt),
                         "guided_epipolar_cells": e.match_frames_guided_epipolar_cells_async(N, fund, ALL_PASS, key=key,
                                                                                             key_xy=key_xy, pairing=pairing,
                                                                                             **opt)}
                if pcode == PAIR_KEY:
                    calls["guided_pose"] = e.match_frames_guided_pose_async(N, rs, ts, big, key, xyz, K=KVEC, **opt)
                e.sync()
                um, ud = um.cpu().numpy(), ud.cpu().numpy()
                for f, n in enumerate(counts):                       # ... and fpc_match_frames' table is the rule's
                    ref = reference("nonfinite", 128, ("frame", b, f), train_of(scene, b, f, pcode, k), (cross, md, ratio))
                    compare(um[f, :n], ud[f, :n], ref, BAR_D128, "match_frames %s key %d frame %d" % (pairing, k, f))
                for what, (m, d) in calls.items():
                    label = "%s %s key %d %s" % (what, pairing, k, (cross, md, ratio))
                    np.testing.assert_array_equal(m.cpu().numpy(), um, err_msg=label)
                    np.testing.assert_array_equal(d.cpu().numpy().view(np.uint32), ud.view(np.uint32), err_msg=label)


@pytest.fixture(scope="module")
def ctx256():
    """FPC_ARCH_VGG: D = 256."""
    e = _engine(in_channels=1, arch="vgg")
    assert e.desc_dim == 256
    yield e
    try:
        assert e.check_guards() == 0
    finally:
        e.close()


def _bar256(name):
    """Twice the plain fp32 evaluation's largest error on the scene, at most 8 D 2^-24."""
    bar = min(2 * _cpu_fp32(name, 256), analytic_bar(256))
    assert 0 < bar <= analytic_bar(256)
    return bar


@pytest.mark.parametrize("name", ["edges", "nonfinite"])
def test_256_components_explicit_pairs(ctx256, name):
    _explicit(ctx256, name, 256, _bar256(name))


@pytest.mark.parametrize("name,b", [("edges", 0), ("edges", 1), ("nonfinite", 0), ("nonfinite", 1)])
def test_256_components_frames(ctx256, name, b):
    _frames(ctx256, name, 256, _bar256(name), b, scene_of(name, 256)["batches"][b])
