"""Top-K relocalisation by pose on the GPU (fpc_pnp_topk_reserve / fpc_pnp_bank_topk / fpc_p3p_bank_topk /
fpc_fundamental_bank_topk / fpc_essential_bank_topk) held to the single-slot calls, bit for bit: problem (f, j) of every
model is fpc_pnp_bank / fpc_p3p_bank / fpc_fundamental_bank / fpc_essential_bank called with column j -- for k below and at
kmax, with candidates of -1, slots outside the bank, a slot without landmarks, frames without rows and n < max_batch --
the pick and the picked model are the integer rule of tests/test_match_bank_topk.py, the true column's pose is the float64
restatement's (tests/test_pnp_ransac.py, tests/test_p3p_ransac.py), and the decoy scene of tests/test_pose_bank_topk.py
comes out as it does there: appearance takes the decoy, every model the true slot, at the planted pose.

8 VGA frames of tests/test_match_pose.py's GPU_SCENE, written into the library's device results as in
tests/test_gpu_match_guided.py; a bank of 6 slots x 1024 rows (fp32 and bf16): the key with its landmarks, its decoy (29
look-alike rows per frame: 1024 rows in all) with landmarks scrambled over the scene's box, an empty slot, a slot stored
without landmarks, two equal slots; kmax 4, 256 iterations; every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_gpu_match_guided import engine, plant
from tests.test_match_bank_topk import pick_rule
from tests.test_match_pose import GPU_SCENE, KVEC, RADIUS, scene_of
from tests.test_pnp_ransac import ROT_BAR, TRANS_BAR, pose_errors
from tests.test_pose_bank_topk import CHANCE, POSE_RULES, box_landmarks, decoy_slot_of, landmark_pairs

pytestmark = pytest.mark.gpu

N = 8
FPC_E_INVALID = -1
SLOTS, KMAX = 6, 4
A, B, EMPTY, NOLM, TIE = 3, 1, 0, 2, (4, 5)   # the key, its decoy, nothing, rows without landmarks, two equal slots
TIE_ROWS = 400
OPTIONS = (True, 0.7, 0.0)                     # cross check, max_dist, ratio
PARAMS = dict(iterations=256, seed=3)          # the other fields: each model's defaults
MODELS = ("pnp", "p3p", "fundamental", "essential")
SINGLE = {"pnp": "pnp_bank_async", "p3p": "p3p_bank_async", "fundamental": "fundamental_bank_async",
          "essential": "essential_bank_async"}
NMODEL = {"pnp": 2, "p3p": 2, "fundamental": 1, "essential": 2}      # model tensors in front of ninliers: (R, t), (F), (F, E)


def _host(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _pad(a, rows):
    out = np.zeros((rows,) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


def _bank_bytes(e):
    v = _lib.FpcBankView()
    assert _lib.load().fpc_bank_get(e._ctx, ctypes.byref(v)) == 0
    return v.bytes, v.chunk


def fill_bank(e, scene, fmt):
    """The six slots and their landmarks; then the reservations, which must leave the bank's own figures alone."""
    e.bank_create(SLOTS, format=fmt)
    rows = e.bank_info()["rows"]
    assert rows == e.capacity == 1024
    decoy = decoy_slot_of(scene, 29)
    assert len(decoy[0]) == rows
    tie = (scene["key"][:TIE_ROWS], scene["key_xy"][:TIE_ROWS], scene["key_xyz"][:TIE_ROWS], scene["key_valid"][:TIE_ROWS])
    slots = {A: (scene["key"], scene["key_xy"], scene["key_xyz"], scene["key_valid"]),
             B: (*decoy, box_landmarks(rows, 40 + B), np.ones(rows, bool)),
             NOLM: (scene["key"][:TIE_ROWS], scene["key_xy"][:TIE_ROWS], None, None), TIE[0]: tie, TIE[1]: tie}
    assert e.bank_landmarks_reserve() >= SLOTS * rows * 16
    for sl, (d, p, xyz, valid) in slots.items():
        e.bank_store_rows(sl, d, p)
        if xyz is not None:
            e.bank_store_landmarks(sl, _pad(xyz, rows), _pad(valid, rows))
    e.sync()
    before = _bank_bytes(e)
    assert e.bank_topk_reserve(KMAX) > 0 and e.pnp_reserve() > 0
    nbytes = e.pnp_topk_reserve()
    assert nbytes >= N * KMAX * e.capacity * 32                              # two float4 per record
    assert _bank_bytes(e) == before and e.bank_info()["bytes"] == before[0]  # bytes and chunk: unchanged
    return slots


@pytest.fixture(scope="module", params=["f32", "bf16"])
def rig(request):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine()
    scene = scene_of(GPU_SCENE)
    assert e.capacity == GPU_SCENE["cap"] and (scene["counts"] == 820).all() and len(scene["key"]) == 792
    plant(e, scene)
    slots = fill_bank(e, scene, request.param)
    yield e, scene, slots, request.param
    try:
        assert e.check_guards() == 0
        e.bank_destroy()
        assert _lib.load().fpc_pnp_topk_reserve(e._ctx, None) == FPC_E_INVALID      # no bank, no top-K reservation
    finally:
        e.close()


def topk_call(e, model, n, cs, m, **params):
    """The model's top-K call on device tensors -> host (models [n][k][..] ..., ninliers, mask, pick, best, best models ...)."""
    call = getattr(e, {"pnp": "pnp_bank_topk_async", "p3p": "p3p_bank_topk_async", "fundamental": "fundamental_bank_topk_async",
                       "essential": "essential_bank_topk_async"}[model])
    out = call(n, cs, m, **dict(PARAMS, **params))
    e.sync()
    return _host(*out)


def single_call(e, model, n, slot, m, **params):
    out = getattr(e, SINGLE[model])(n, slot, m, **dict(PARAMS, **params))
    e.sync()
    return _host(*out)


def assert_columns_equal_the_single_slot_call(e, model, n, cs, m, label, **params):
    """Problem (f, j) against the single-slot call with column j, as uint32 / uint8 views; then the derived outputs."""
    k = cs.shape[1]
    out = topk_call(e, model, n, cs, m, **params)
    nm = NMODEL[model]
    models, ni, mask, pick, best, picked = out[:nm], out[nm], out[nm + 1], out[nm + 2], out[nm + 3], out[nm + 4:]
    assert ni.shape == (n, k) and mask.shape == (n, k, e.capacity)
    for j in range(k):
        ref = single_call(e, model, n, cs[:, j].contiguous(), m[:, j].contiguous(), **params)
        for a, b in zip(models, ref[:nm]):
            np.testing.assert_array_equal(a[:, j].reshape(n, -1).view(np.uint32), b.reshape(n, -1).view(np.uint32),
                                          err_msg="%s %s column %d" % (model, label, j))
        np.testing.assert_array_equal(ni[:, j], ref[nm], err_msg="%s %s column %d" % (model, label, j))
        np.testing.assert_array_equal(mask[:, j].view(np.uint8), ref[nm + 1].view(np.uint8),
                                      err_msg="%s %s column %d" % (model, label, j))
    csh = cs.cpu().numpy()
    want_pick, want_best = pick_rule(ni, csh)
    np.testing.assert_array_equal(pick, want_pick)
    np.testing.assert_array_equal(best, want_best)
    np.testing.assert_array_equal(mask.sum(2), ni)
    # the picked model: the picked column's bits, or zeros (R and t of the pose calls, F of the epipolar ones)
    for got, full in zip(picked, models):
        want = np.where((pick >= 0).reshape(n, *[1] * (full.ndim - 2)), full[np.arange(n), np.maximum(pick, 0)], 0)
        np.testing.assert_array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    assert len(picked) == (2 if model in POSE_RULES else 1)
    failed = ni == 0                                                    # a failed problem: zeros, 0, an all-zero mask
    for a in models:
        flat = a.reshape(n * k, -1)
        assert not flat[failed.ravel()].any() and flat[~failed.ravel()].any(1).all()
    assert not mask[failed].any()
    return csh, ni, pick, best, models


@pytest.mark.parametrize("model", MODELS)
def test_every_column_is_bit_identical_to_the_single_slot_call(rig, model):
    e, s, _, _ = rig
    score, cs, csc, m, _ = e.match_bank_topk_async(N, KMAX, *OPTIONS, 0)
    e.sync()
    sc = score.cpu().numpy()
    few = int(sc[:, TIE[0]].max()) + 1                                   # only A and B reach it: candidates of -1 behind them
    for k in (1, 3, KMAX):                                               # k < kmax: a kmax-for-k stride would show
        for min_score in (0, few):
            _, cs, _, m, _ = e.match_bank_topk_async(N, k, *OPTIONS, min_score)
            csh, ni, pick, best, _ = assert_columns_equal_the_single_slot_call(e, model, N, cs, m, (k, min_score))
            if min_score == 0:
                np.testing.assert_array_equal(csh, np.tile(np.array([B, A, NOLM, TIE[0]], np.int32)[:k], (N, 1)))
                if k > 1:
                    assert (ni[:, 1] >= 100).all() and (best == A).all() and (pick == 1).all()
                if k > 2 and model in POSE_RULES:
                    assert (ni[:, 2] == 0).all()                         # stored without landmarks: no pairs
                if k > 3:
                    assert (ni[:, 3] >= 100).all()                       # part of the key, with its landmarks
            elif k > 2:
                assert (csh[:, 2:] == -1).all() and (ni[:, 2:] == 0).all()
    # the two equal slots side by side on one table: equal counts, and the pick goes to the LOWER j (here the higher slot)
    _, cs, _, m, _ = e.match_bank_topk_async(N, KMAX, *OPTIONS, 0)
    assert (cs.cpu().numpy()[:, 3] == TIE[0]).all()
    tied = cs.clone()
    tied[:, 1], tied[:, 2], tied[:, 3] = TIE[1], TIE[0], TIE[1]
    tm = m[:, [0, 3, 3, 3]].contiguous()
    _, ni, pick, best, _ = assert_columns_equal_the_single_slot_call(e, model, N, tied[:, :3].contiguous(),
                                                                     tm[:, :3].contiguous(), "tie")
    assert (ni[:, 1] == ni[:, 2]).all() and (ni[:, 1] >= 100).all() and (ni[:, 1] > ni[:, 0]).all()
    assert (pick == 1).all() and (best == TIE[1]).all()
    _, ni, pick, best, _ = assert_columns_equal_the_single_slot_call(e, model, N, tied[:, 1:].contiguous(),
                                                                     tm[:, 1:].contiguous(), "tie of three")
    assert (ni[:, 0] == ni[:, 1]).all() and (ni[:, 1] == ni[:, 2]).all() and (pick == 0).all() and (best == TIE[1]).all()
    # slots outside the bank in the shortlist; n < max_batch
    _, cs, _, m, _ = e.match_bank_topk_async(N, 3, *OPTIONS, 0)
    cs = cs.clone()
    cs[2, 1], cs[4, 0], cs[6, 2] = SLOTS, -5, EMPTY
    csh, ni, pick, best, _ = assert_columns_equal_the_single_slot_call(e, model, 5, cs[:5].contiguous(), m[:5].contiguous(),
                                                                       "bad slots")
    assert ni[2, 1] == 0 and ni[4, 0] == 0 and best[4] == A
    # other parameters reach every problem: no refits, another seed and threshold
    assert_columns_equal_the_single_slot_call(e, model, N, cs, m, "params", refits=0, seed=9, reproj_threshold=1.5,
                                              iterations=100)


@pytest.mark.parametrize("model", MODELS)
def test_frames_without_rows_and_short_pair_lists(rig, model):
    e, s, _, _ = rig
    r = dict(s)
    r["counts"] = np.array([0, 3, 5, 9, 64, 65, 257, s["counts"][7]])
    plant(e, r)
    try:
        _, cs, _, m, _ = e.match_bank_topk_async(N, KMAX, *OPTIONS, 0)
        csh, ni, pick, best, _ = assert_columns_equal_the_single_slot_call(e, model, N, cs, m, "ragged")
        assert (csh[0] == -1).all() and (ni[:2] == 0).all() and (pick[:2] == -1).all() and (best[:2] == -1).all()
        assert ni[7].max() >= 100
    finally:
        plant(e, s)


def test_decoy_scene_appearance_takes_the_decoy_and_every_model_the_true_slot(rig):
    e, s, _, _ = rig
    _, best0, _, _ = e.match_bank_async(N, *OPTIONS, table=False)
    _, cs, csc, m, _ = e.match_bank_topk_async(N, 2, *OPTIONS, 0)
    e.sync()
    np.testing.assert_array_equal(best0.cpu().numpy(), np.full(N, B))                # fpc_match_bank's best: the decoy
    np.testing.assert_array_equal(cs.cpu().numpy(), np.tile(np.array([B, A], np.int32), (N, 1)))
    for model in MODELS:
        out = topk_call(e, model, N, cs, m)
        nm = NMODEL[model]
        ni, pick, best = out[nm], out[nm + 2], out[nm + 3]
        print(model, "scores", csc.cpu().numpy().tolist(), "inliers", ni.tolist())
        np.testing.assert_array_equal(pick, np.full(N, 1))
        np.testing.assert_array_equal(best, np.full(N, A))                           # all 8 frames
        if model in POSE_RULES:
            np.testing.assert_array_equal(ni[:, 0], 0)
            assert not out[0][:, 0].any() and not out[1][:, 0].any()
            for f in range(N):
                cam = s["cams"][1 + f]
                for rm, tv in ((out[0][f, 1], out[1][f, 1]), (out[nm + 4][f], out[nm + 5][f])):
                    rot, tr = pose_errors(rm, tv, (None, None, None, cam[0], cam[1]))
                    assert rot <= ROT_BAR and tr <= TRANS_BAR, (model, f, rot, tr)
                print("  %s frame %d: %d inliers, rotation %.4f deg, translation %.3e" % (model, f, ni[f, 1], rot, tr))
        else:
            assert (ni[:, 0] < CHANCE).all() and (ni[:, 1] >= 400).all()


@pytest.mark.parametrize("model", sorted(POSE_RULES))
def test_true_column_equals_the_float64_restatement(rig, model):
    """R, t, the count and the mask of the true column against pnp_rule / p3p_rule on the device's own table (a bf16 bank
    yields other tables than an fp32 one): the restatement's fp32 outputs, entry for entry."""
    e, s, slots, fmt = rig
    _, cs, _, m, _ = e.match_bank_topk_async(N, 2, *OPTIONS, 0)
    rm, tv, ni, mask = topk_call(e, model, N, cs, m)[:4]
    mh = m.cpu().numpy()
    assert (cs.cpu().numpy()[:, 1] == A).all()
    for f in range(N):
        rows, pxy, pxyz = landmark_pairs(s["xy"][f], mh[f, 1, :s["counts"][f]], slots[A][2], slots[A][3])
        want = POSE_RULES[model](pxy, pxyz, PARAMS, f, KVEC)
        dr = np.abs(rm[f, 1].astype(np.float64) - want.R).max()
        dt = np.abs(tv[f, 1].astype(np.float64) - want.t).max()
        print("%s %s frame %d: %d pairs, %d inliers (restatement %d), |dR| %.3e, |dt| %.3e, masks differ in %d rows"
              % (fmt, model, f, len(rows), ni[f, 1], want.ninliers, dr, dt, (mask[f, 1][rows] != want.mask).sum()))
        assert not want.failed
        assert ni[f, 1] == want.ninliers
        np.testing.assert_array_equal(mask[f, 1][rows], want.mask)
        assert not np.delete(mask[f, 1], rows).any()
        np.testing.assert_array_equal(rm[f, 1], want.R.astype(np.float32))
        np.testing.assert_array_equal(tv[f, 1], want.t.astype(np.float32))


@pytest.mark.parametrize("model", sorted(POSE_RULES))
def test_relocalise_pose_chain_and_determinism(rig, model):
    e, s, _, fmt = rig
    if fmt == "bf16":                       # the chain's second pass, fpc_match_bank_guided_pose, is an "f32" bank's:
        with pytest.raises(ValueError):     # refused up front, before anything is launched
            e.relocalise_pose(N, 3, model=model, radius=RADIUS, **PARAMS)
        return
    first = e.relocalise_pose(N, 3, model=model, radius=RADIUS, **PARAMS)
    again = e.relocalise_pose(N, 3, model=model, radius=RADIUS, **PARAMS)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    best, rm, tv, ni, mask, rk, tk, nk, pick, cs, csc = first
    print(model, "best", best, "picked candidate's inliers", nk[np.arange(N), pick], "-> second pose", ni)
    np.testing.assert_array_equal(best, np.full(N, A))
    np.testing.assert_array_equal(pick, np.full(N, 1))
    assert (ni >= nk[np.arange(N), pick]).all() and (ni >= 400).all()
    np.testing.assert_array_equal(mask.sum(1), ni)
    for f in range(N):
        cam = s["cams"][1 + f]
        rot, tr = pose_errors(rm[f], tv[f], (None, None, None, cam[0], cam[1]))
        assert rot <= ROT_BAR and tr <= TRANS_BAR, (model, f, rot, tr)
    with pytest.raises(ValueError):
        e.relocalise_pose(N, 3, model="essential")
    assert e.check_guards() == 0


def test_reservations_leave_the_others_alone_and_go_with_the_bank(rig):
    e0, s, _, _ = rig
    lib = _lib.load()
    nb = ctypes.c_size_t(0)
    assert lib.fpc_pnp_topk_reserve(e0._ctx, ctypes.byref(nb)) == FPC_E_INVALID and nb.value == 0      # it exists already
    e = engine(b=2)
    try:
        assert lib.fpc_pnp_topk_reserve(e._ctx, ctypes.byref(nb)) == FPC_E_INVALID                     # no bank
        e.bank_create(3)
        assert lib.fpc_pnp_topk_reserve(e._ctx, ctypes.byref(nb)) == FPC_E_INVALID and nb.value == 0   # no top-K reservation
        bank = _bank_bytes(e)
        topk = e.bank_topk_reserve(2)
        mine = e.pnp_topk_reserve()
        assert mine >= 2 * 2 * e.capacity * 32 and _bank_bytes(e) == bank
        assert lib.fpc_pnp_topk_reserve(e._ctx, ctypes.byref(nb)) == FPC_E_INVALID and nb.value == 0   # twice
        pnp = e.pnp_reserve()                                       # (behind it: the PnP reservation is what it is without)
        assert e.check_guards() == 0
        e.bank_destroy()
        assert lib.fpc_pnp_topk_reserve(e._ctx, ctypes.byref(nb)) == FPC_E_INVALID                     # it went with the bank
        e.bank_create(3)
        assert _bank_bytes(e) == bank
        assert e.bank_topk_reserve(2) == topk                       # the top-K reservation: the same bytes behind a pose one
        assert e.pnp_topk_reserve() == mine                         # ... and it can be made again
        # a bank without landmark storage: every problem fails, nothing faults
        import torch
        plant2 = dict(s, desc=s["desc"][:2], xy=s["xy"][:2], counts=s["counts"][:2])
        plant(e, plant2)
        e.bank_store_rows(1, s["key"], s["key_xy"])
        _, cs, _, m, _ = e.match_bank_topk_async(2, 2, *OPTIONS, 0)
        for model in sorted(POSE_RULES):
            rm, tv, ni, mask, pick, best, br, bt = topk_call(e, model, 2, cs, m)
            assert (cs.cpu().numpy()[:, 0] == 1).all()
            assert not rm.any() and not tv.any() and not ni.any() and not mask.any() and not br.any() and not bt.any()
            assert (pick == -1).all() and (best == -1).all()
        fm, ni, mask, pick, best, bf = topk_call(e, "fundamental", 2, cs, m)     # the epipolar calls need keypoints only
        assert (ni[:, 0] >= 400).all() and (best == 1).all() and bf.any(axis=(1, 2)).all()
        assert e.check_guards() == 0
        torch.cuda.synchronize()
    finally:
        e.close()
    e = engine(b=2)
    try:
        assert e.pnp_reserve() == pnp                                # the PnP reservation of a context without any of this
    finally:
        e.close()


def test_bad_arguments_are_refused_and_write_nothing(rig):
    import torch
    e, s, _, _ = rig
    lib, dev, ctx = _lib.load(), e.torch_device, e._ctx
    _, cs, _, m, _ = e.match_bank_topk_async(N, KMAX, *OPTIONS, 0)
    e.sync()

    def filled(*shape, dtype=torch.float32):
        return torch.full(shape, -7, dtype=dtype, device=dev)
    outs = dict(R=filled(N, KMAX, 9), t=filled(N, KMAX, 3), E=filled(N, KMAX, 9), ni=filled(N, KMAX, dtype=torch.int32),
                mask=filled(N, KMAX, e.capacity, dtype=torch.uint8), pick=filled(N, dtype=torch.int32),
                best=filled(N, dtype=torch.int32), bR=filled(N, 9), bt=filled(N, 3))
    accepted = {k: filled(*v.shape, dtype=v.dtype) for k, v in outs.items()}      # the outputs of the calls that are NOT refused
    torch.cuda.synchronize()
    ptr = {k: v.data_ptr() for k, v in outs.items()}

    def untouched(v):
        h = v.cpu().numpy()
        return bool((h == np.array(-7, np.int64).astype(h.dtype)).all())                    # (uint8: 249)
    pp, rp, ep = _lib.FpcPnpParams(), _lib.FpcRansacParams(), _lib.FpcEssentialParams()
    assert lib.fpc_default_pnp_params(ctypes.byref(pp)) == 0 and lib.fpc_default_ransac_params(ctypes.byref(rp)) == 0
    assert lib.fpc_default_essential_params(ctypes.byref(ep)) == 0

    def call(model, c=ctx, n=N, k=KMAX, cand=cs.data_ptr(), match=m.data_ptr(), params=True, **kw):
        q = dict(ptr, **kw)
        if model in POSE_RULES:
            fn = lib.fpc_pnp_bank_topk if model == "pnp" else lib.fpc_p3p_bank_topk
            return fn(c, n, k, cand, match, ctypes.byref(pp) if params else None, q["R"], q["t"], q["ni"], q["mask"], q["pick"],
                      q["best"], q["bR"], q["bt"])
        if model == "fundamental":
            return lib.fpc_fundamental_bank_topk(c, n, k, cand, match, ctypes.byref(rp) if params else None, q["R"], q["ni"],
                                                 q["mask"], q["pick"], q["best"], q["bR"])
        return lib.fpc_essential_bank_topk(c, n, k, cand, match, ctypes.byref(ep) if params else None, q["R"], q["E"], q["ni"],
                                           q["mask"], q["pick"], q["best"], q["bR"])
    sample = {"pnp": 6, "p3p": 4, "fundamental": 8, "essential": 6}
    nan = float("nan")
    other = engine(b=2)                       # a context with a bank and keypoints, but without the reservations
    try:
        plant(other, dict(s, desc=s["desc"][:2], xy=s["xy"][:2], counts=s["counts"][:2]))
        for model in MODELS:
            par = pp if model in POSE_RULES else rp if model == "fundamental" else ep
            assert call(model, c=None) == FPC_E_INVALID
            for bad in (dict(n=0), dict(n=N + 1), dict(k=0), dict(k=KMAX + 1), dict(k=-1), dict(cand=None), dict(match=None),
                        dict(R=None), dict(ni=None), dict(params=False)):
                assert call(model, **bad) == FPC_E_INVALID, (model, bad)
            if model in POSE_RULES:
                assert call(model, t=None) == FPC_E_INVALID
            fields = [("iterations", 0), ("iterations", 4097), ("reproj_threshold", 0.0), ("reproj_threshold", nan),
                      ("refits", -1), ("refits", 5), ("min_inliers", sample[model] - 1)]
            if model in POSE_RULES:
                fields += [("fx", 0.0), ("fy", -1.0), ("cx", nan)]
            if model == "essential":
                fields += [("q_fx", 0.0), ("t_fy", nan)]
            for name, value in fields:
                keep = getattr(par, name)
                setattr(par, name, value)
                assert call(model) == FPC_E_INVALID, (model, name, value)
                setattr(par, name, keep)
            # no bank; a bank without a top-K reservation; a top-K reservation without the pose one
            assert call(model, c=other._ctx, n=2, k=1) == FPC_E_INVALID
            other.bank_create(2)
            assert call(model, c=other._ctx, n=2, k=1) == FPC_E_INVALID
            other.bank_topk_reserve(2)
            if model in POSE_RULES:
                assert call(model, c=other._ctx, n=2, k=1) == FPC_E_INVALID
            else:                             # (the epipolar calls need no more: accepted, into tensors of its own)
                assert call(model, c=other._ctx, n=2, k=1, **{k_: v.data_ptr() for k_, v in accepted.items()}) == 0
            other.sync()
            other.bank_destroy()
            # nothing stands between this model's refusals and the check: no refused call wrote anything
            e.sync()
            for name, v in outs.items():
                assert untouched(v), (model, name)
        assert all(not untouched(accepted[name]) for name in ("R", "ni", "mask", "pick", "best", "bR"))
        # the outputs that may be NULL, and a valid form of every call
        for model in MODELS:
            assert call(model, mask=None, pick=None, best=None, bR=None, bt=None, E=None) == 0, model
            assert call(model) == 0, model
        e.sync()
        assert (outs["ni"].cpu().numpy() != -7).all() and (outs["best"].cpu().numpy() == A).all()
        assert other.check_guards() == 0
    finally:
        other.close()
