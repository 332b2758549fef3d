"""CPU checks of the key-frame bank (fpc_bank_* / fpc_match_bank / fpc_homography_bank): the entry points exist and
refuse a NULL context, the binding declares them, and a float64 restatement of the bank rule (`bank_rule`, built on
tests/test_match_frames.py's pair_rule) -- which the GPU tests (test_gpu_match_bank.py) hold the kernels to through
fpc_match_frames -- behaves as include/fpc.h states on planted data: the planted slot is recovered with max_dist or a
ratio, and NOT reliably with a bare cross check (the header's warning)."""
import ctypes

import numpy as np

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_match_frames import pair_rule

FPC_E_INVALID = -1


def bank_rule(desc, counts, slots, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0):
    """desc [n][cap][D], counts [n], slots: list of [k_s][D] arrays (k_s = 0: empty) -> (score int64 [n][S], best int64
    [n], match int32 [n][cap], d1 float64 [n][cap]): score = surviving rows per (frame, slot); best = the largest score,
    ties to the lower slot, -1 below max(min_score, 1); the table is the pair rule against slot best[f]."""
    n, cap = len(counts), desc.shape[1]
    score = np.zeros((n, len(slots)), np.int64)
    best = np.full(n, -1, np.int64)
    match = np.full((n, cap), -1, np.int32)
    d1 = np.full((n, cap), np.inf)
    for f in range(n):
        q = desc[f, :counts[f]]
        tables = [pair_rule(q, t, cross_check, max_dist, ratio) for t in slots]
        score[f] = [(m >= 0).sum() for m, _, _ in tables]
        s = int(np.argmax(score[f]))                              # argmax: the first (lowest) slot on ties
        if score[f, s] >= max(min_score, 1):
            best[f] = s
            match[f, :counts[f]], d1[f, :counts[f]] = tables[s][0], tables[s][1]
    return score, best, match, d1


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def planted(seed=7, n_slots=12, empty=5, dim=128):
    """12 slots of 120-300 random unit rows (one empty); per non-empty slot one query frame: half of the slot's rows
    + N(0, 0.02) noise, then 150 unrelated rows.  -> (desc [n][cap][D], counts [n], slots, the slot each query was
    planted from)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    slots = []
    for s in range(n_slots):
        k = 0 if s == empty else int(rng.integers(120, 301))
        slots.append(_unit(rng.normal(size=(k, dim))) if k else np.zeros((0, dim), np.float32))
    frames, origin = [], []
    for s, t in enumerate(slots):
        if not len(t):
            continue
        pick = rng.permutation(len(t))[:len(t) // 2]
        q = np.concatenate([_unit(t[pick] + rng.normal(0, 0.02, (len(pick), dim))), _unit(rng.normal(size=(150, dim)))])
        frames.append(q)
        origin.append(s)
    cap = max(len(q) for q in frames)
    desc = np.zeros((len(frames), cap, dim), np.float32)
    for f, q in enumerate(frames):
        desc[f, :len(q)] = q
    return desc, np.array([len(q) for q in frames]), slots, np.array(origin)


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    view = _lib.FpcBankView()
    rp = _lib.FpcRansacParams()
    assert lib.fpc_default_ransac_params(ctypes.byref(rp)) == 0
    assert lib.fpc_bank_create(None, 4, 16) == FPC_E_INVALID
    assert lib.fpc_bank_destroy(None) == FPC_E_INVALID
    assert lib.fpc_bank_get(None, ctypes.byref(view)) == FPC_E_INVALID
    assert lib.fpc_bank_store(None, 0, 0) == FPC_E_INVALID
    assert lib.fpc_bank_store_rows(None, 0, p, p, p) == FPC_E_INVALID
    assert lib.fpc_bank_clear(None, -1) == FPC_E_INVALID
    assert lib.fpc_match_bank(None, 1, 1, 0.7, 0.0, 0, p, p, None, None) == FPC_E_INVALID
    assert lib.fpc_homography_bank(None, 1, p, p, ctypes.byref(rp), p, p, None) == FPC_E_INVALID
    assert (buf == 0).all() and view.bytes == 0


def test_binding_declares_the_bank():
    lib = _lib.load()
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.fpc_bank_create.argtypes == [vp, ci, ci]
    assert lib.fpc_bank_store.argtypes == [vp, ci, ci]
    assert lib.fpc_bank_store_rows.argtypes == [vp, ci, vp, vp, vp]
    assert lib.fpc_bank_clear.argtypes == [vp, ci]
    assert lib.fpc_match_bank.argtypes == [vp, ci, ci, cf, cf, ci, vp, vp, vp, vp]
    assert lib.fpc_homography_bank.argtypes[:4] == [vp, ci, vp, vp] and len(lib.fpc_homography_bank.argtypes) == 8
    # fpc_bank_view: three pointers, four ints, a size_t
    assert ctypes.sizeof(_lib.FpcBankView) == 3 * 8 + 4 * 4 + 8
    assert _lib.FpcBankView.bytes.offset == 40
    assert _lib.BANK_MAX_SLOTS == 1024
    assert lib.fpc_abi_version() == 4                              # symbols were only added
    for name in ("bank_create", "bank_store", "bank_store_rows", "bank_clear", "bank_view", "match_bank_async",
                 "match_bank", "homography_bank_async", "homography_bank"):
        from fpc_amd.engine import Engine
        assert callable(getattr(Engine, name)), name
    from fpc_amd import inference
    assert callable(inference.relocalise_batch)


def test_planted_slot_is_recovered_with_a_distance_or_ratio_bound():
    desc, counts, slots, origin = planted()
    assert len(slots) == 12 and sum(len(t) == 0 for t in slots) == 1 and len(origin) == 11
    for cross, md, ratio in ((True, 0.7, 0.0), (True, 0.0, 0.8), (False, 0.7, 0.0)):
        score, best, match, d1 = bank_rule(desc, counts, slots, cross, md, ratio)
        np.testing.assert_array_equal(best, origin)                # every query finds the slot it was planted from
        for f, s in enumerate(origin):
            assert score[f, s] == len(slots[s]) // 2, (cross, md, ratio, f, score[f])   # every planted row (0.23 away), no other
            others = np.delete(score[f], s)
            assert others.max() == 0, (cross, md, ratio, f, score[f])
            # the table is the pair rule against the winning slot
            m, a, _ = pair_rule(desc[f, :counts[f]], slots[s], cross, md, ratio)
            np.testing.assert_array_equal(match[f, :counts[f]], m)
            np.testing.assert_array_equal(d1[f, :counts[f]], a)
            assert (match[f, counts[f]:] == -1).all() and np.isinf(d1[f, counts[f]:]).all()
            assert (match[f, :counts[f]] >= 0).sum() == score[f, s]
        assert (score[:, 5] == 0).all()                            # the empty slot


def test_a_bare_cross_check_does_not_discriminate():
    """What include/fpc.h warns of: unrelated sets have many mutual nearest neighbours."""
    desc, counts, slots, origin = planted()
    score, best, _, _ = bank_rule(desc, counts, slots, True, 0.0, 0.0)
    wrong = [np.delete(score[f], [s]).max() for f, s in enumerate(origin)]
    assert max(wrong) > 60, wrong                                  # other slots score as high as a planted one can
    assert (score[:, 5] == 0).all()


def test_ties_min_score_empty_bank_and_truncation():
    desc, counts, slots, origin = planted()
    # two identical slots tie: the lower index wins
    twin = list(slots)
    twin[9] = slots[2].copy()
    score, best, _, _ = bank_rule(desc, counts, twin, True, 0.7)
    f2 = int(np.flatnonzero(origin == 2)[0])
    assert score[f2, 2] == score[f2, 9] > 0 and best[f2] == 2
    twin[2], twin[9] = slots[9], slots[9].copy()
    f9 = int(np.flatnonzero(origin == 9)[0])
    score, best, _, _ = bank_rule(desc, counts, twin, True, 0.7)
    assert score[f9, 2] == score[f9, 9] > 0 and best[f9] == 2
    # min_score above the best score: no slot
    score, best, match, d1 = bank_rule(desc, counts, slots, True, 0.7, min_score=int(score.max()) + 1)
    assert (best == -1).all() and (match == -1).all() and np.isinf(d1).all()
    score0, best0, _, _ = bank_rule(desc, counts, slots, True, 0.7, min_score=int(score.max()))
    assert (best0 >= 0).sum() >= 1 and ((best0 == -1) | (best0 == origin)).all()
    # a bank of empty slots
    none = [np.zeros((0, 128), np.float32)] * 4
    score, best, match, d1 = bank_rule(desc, counts, none, True, 0.7)
    assert (score == 0).all() and (best == -1).all() and (match == -1).all() and np.isinf(d1).all()
    # rows truncation keeps the FIRST rows: a slot cut to 40 rows scores what its first 40 rows score, and every match
    # index is below 40
    rows = 40
    cut = [t[:rows] for t in slots]
    score, best, match, _ = bank_rule(desc, counts, cut, False, 0.7)
    assert match.max() < rows
    for f, s in enumerate(origin):
        m, _, _ = pair_rule(desc[f, :counts[f]], slots[s][:rows], False, 0.7)
        assert score[f, s] == (m >= 0).sum()
        full, _, _ = pair_rule(desc[f, :counts[f]], slots[s], False, 0.7)
        keep = (full >= 0) & (full < rows)
        np.testing.assert_array_equal(m[keep], full[keep])         # rows that matched a kept row still match it
