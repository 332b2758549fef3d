"""CPU checks of verified relocalisation (fpc_bank_topk_reserve / fpc_match_bank_topk / fpc_homography_bank_topk): the
entry points exist, are bound with the prototypes of include/fpc.h and refuse a NULL context; the header carries the
contract; and a numpy restatement of the top-K order (`topk_rule`) and of the pick rule (`pick_rule`), chained with the
restatements of tests/test_match_bank.py, tests/test_match_guided.py and tests/test_homography_ransac.py
(`relocalise_rule`), shows on a planted DECOY scene what the feature is for: a slot with the true key's descriptors plus
look-alike rows, at scrambled coordinates, outscores the true slot by appearance, and the geometric check picks the true
one.  tests/test_gpu_match_bank_topk.py holds the kernels to these rules."""
import ctypes
import re
import subprocess

import numpy as np

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_homography_ransac import CORNER_BAR, FRAME_H, FRAME_W, corner_error, header_text, ransac_rule
from tests.test_match_bank import bank_rule
from tests.test_match_guided import f10, guided_frames_rule, planted_h, planted_scene, PAIR_KEY

FPC_E_INVALID = -1
BIG = 1e4                      # a radius beyond the frame diagonal (800 px)
IDENTITY = np.eye(3, dtype=np.float32).reshape(9)
NAMES = ("fpc_bank_topk_reserve", "fpc_match_bank_topk", "fpc_homography_bank_topk")
LOOKALIKES, LOOKALIKE_NOISE = 30, 0.02   # per frame: decoy rows planted from the frame's rows that the true key lacks


# ---- the rules, restated --------------------------------------------------------------------------------------------------
def topk_rule(score, k, min_score=0):
    """score int [n][S] -> (cand_slot int32 [n][k], cand_score int32 [n][k]): the slots with score >= max(min_score, 1) in
    descending (score, then lower slot first) order, the first k of them; -1 / 0 behind the last."""
    score = np.asarray(score)
    n, floor = len(score), max(int(min_score), 1)
    slot = np.full((n, k), -1, np.int32)
    sc = np.zeros((n, k), np.int32)
    for f in range(n):
        order = sorted(range(score.shape[1]), key=lambda s: (-int(score[f, s]), s))
        order = [s for s in order if score[f, s] >= floor][:k]
        slot[f, :len(order)] = order
        sc[f, :len(order)] = score[f, order]
    return slot, sc


def pick_rule(ninliers, cand_slot):
    """ninliers int [n][k], cand_slot int [n][k] -> (pick int32 [n], best int32 [n]): the j with the most inliers, ties
    to the lower j, -1 when there are none; best = cand_slot[f][pick[f]] or -1."""
    ninliers, cand_slot = np.asarray(ninliers), np.asarray(cand_slot)
    pick = np.argmax(ninliers, axis=1).astype(np.int32)               # argmax: the first (lowest) j on ties
    pick[ninliers.max(axis=1) <= 0] = -1
    best = np.where(pick >= 0, cand_slot[np.arange(len(pick)), np.maximum(pick, 0)], -1).astype(np.int32)
    return pick, best


def candidate_tables(desc, xy, counts, slots, cand_slot, cross_check=True, max_dist=0.0, ratio=0.0):
    """slots: list of (desc [k_s][D], xy [k_s][2]); cand_slot [n][k] -> match int32 [n][k][cap]: column j is the guided
    rule with slot cand_slot[:, j], an identity H and a radius beyond the frame (the header's statement of the table); a
    candidate of -1 has no train rows."""
    n, k = cand_slot.shape
    empty = (desc[0, :0], xy[0, :0])
    hs = np.tile(IDENTITY, (n, 1))
    out = np.full((n, k, desc.shape[1]), -1, np.int32)
    for j in range(k):
        trains = [slots[s] if s >= 0 else empty for s in cand_slot[:, j]]
        out[:, j] = guided_frames_rule(desc, xy, counts, trains, hs, BIG, cross_check, max_dist, ratio)[0]
    return out


def relocalise_rule(desc, xy, counts, slots, k, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0, **params):
    """The two calls chained -> dict(score, cand_slot, cand_score, match [n][k][cap], H float64 [n][k][3][3], ninliers
    [n][k], pick [n], best [n]).  Problem (f, j) is ransac_rule at frame index f: the sampler hashes f."""
    n = len(counts)
    score = bank_rule(desc, counts, [d for d, _ in slots], cross_check, max_dist, ratio, min_score)[0]
    cand_slot, cand_score = topk_rule(score, k, min_score)
    match = candidate_tables(desc, xy, counts, slots, cand_slot, cross_check, max_dist, ratio)
    hm, ninl = np.zeros((n, k, 3, 3)), np.zeros((n, k), np.int32)
    for f in range(n):
        for j in range(k):
            s = cand_slot[f, j]
            if s < 0:
                continue
            m = match[f, j, :counts[f]]
            rows = np.flatnonzero((m >= 0) & (m < len(slots[s][1])))
            hm[f, j], inl = ransac_rule(xy[f, rows], slots[s][1][m[rows]], params, f)
            ninl[f, j] = inl.sum()
    pick, best = pick_rule(ninl, cand_slot)
    return dict(score=score, cand_slot=cand_slot, cand_score=cand_score, match=match, H=hm, ninliers=ninl, pick=pick,
                best=best)


# ---- the decoy scene ------------------------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def decoy_slot(scene, seed=3):
    """The decoy of scene["key"]: its descriptors, then per frame LOOKALIKES rows planted from the frame's rows that have
    no counterpart in the key (so that the decoy matches everything the key matches, and more), every row at a random
    pixel: appearance says "this place", geometry says no.  -> (desc [K'][D], xy int32 [K'][2])."""
    rng = np.random.Generator(np.random.PCG64([seed, len(scene["key"])]))
    extra = []
    for f, cnt in enumerate(scene["counts"]):
        rows = np.flatnonzero(scene["ids"][f, :cnt] < 0)[:LOOKALIKES]
        assert len(rows) == LOOKALIKES
        extra.append(_unit(scene["desc"][f, rows] + rng.normal(0, LOOKALIKE_NOISE, (len(rows), scene["desc"].shape[2]))))
    d = np.concatenate([scene["key"]] + extra)
    p = np.stack([rng.integers(0, FRAME_W, len(d)), rng.integers(0, FRAME_H, len(d))], 1).astype(np.int32)
    return d, p


HOMS = [("defaults", 1), ("preprocess", 3), ("defaults", 8), ("preprocess", 10)]
A, B = 2, 1


def decoy_bank(scene):
    """Slot A = the true key, slot B = its decoy, slot 0 empty, slot 3 unrelated rows."""
    rng = np.random.Generator(np.random.PCG64(17))
    other = _unit(rng.normal(size=(150, scene["desc"].shape[2])))
    other_xy = np.stack([rng.integers(0, FRAME_W, 150), rng.integers(0, FRAME_H, 150)], 1).astype(np.int32)
    slots = [(scene["key"][:0], scene["key_xy"][:0]), None, None, (other, other_xy)]
    slots[A] = (scene["key"], scene["key_xy"])
    slots[B] = decoy_slot(scene)
    return slots


# ---- tests ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_with_the_stated_prototypes():
    lib = _lib.load()
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name in exported, name
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert lib.fpc_bank_topk_reserve.argtypes == [vp, ci, ctypes.POINTER(ctypes.c_size_t)]
    assert lib.fpc_match_bank_topk.argtypes == [vp, ci, ci, ci, cf, cf, ci, vp, vp, vp, vp, vp]
    assert lib.fpc_homography_bank_topk.argtypes == [vp, ci, ci, vp, vp, ctypes.POINTER(_lib.FpcRansacParams), vp, vp, vp,
                                                     vp, vp]
    # the header's parameter lists, counted: 3, 12 and 11 parameters
    for name, nargs in zip(NAMES, (3, 12, 11)):
        args = re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == nargs, (name, args)
    assert int(re.search(r"#define FPC_BANK_TOPK_MAX (\d+)", hdr).group(1)) == _lib.BANK_TOPK_MAX == 16
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 == lib.fpc_abi_version()   # symbols were only added
    from fpc_amd.engine import Engine
    for name in ("bank_topk_reserve", "match_bank_topk_async", "match_bank_topk", "homography_bank_topk_async",
                 "homography_bank_topk", "relocalise"):
        assert callable(getattr(Engine, name)), name


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    rp = _lib.FpcRansacParams()
    nbytes = ctypes.c_size_t(0)
    assert lib.fpc_default_ransac_params(ctypes.byref(rp)) == 0
    assert lib.fpc_bank_topk_reserve(None, 4, ctypes.byref(nbytes)) == FPC_E_INVALID
    assert lib.fpc_match_bank_topk(None, 1, 1, 1, 0.7, 0.0, 0, p, p, p, p, p) == FPC_E_INVALID
    assert lib.fpc_homography_bank_topk(None, 1, 1, p, p, ctypes.byref(rp), p, p, p, p, p) == FPC_E_INVALID
    assert (buf == 0).all() and nbytes.value == 0


def test_header_carries_the_contract():
    hdr = " ".join(re.sub(r"\n \* ?", " ", header_text()).split())       # comment blocks as running text
    for phrase in ("fpc_bank_topk_reserve: 1 <= kmax <= min(FPC_BANK_TOPK_MAX, slots)",
                   "descending (score, then LOWER slot first)",
                   "cand_slot[f][0] is fpc_match_bank's best[f]",
                   "an identity H and a radius beyond the frame diagonal",
                   "equals cand_score[f][j]",
                   "the sampler hashes f, not f k + j",
                   "ties to the LOWER j",
                   "(ninliers << 32) | ~j",
                   "fpc_bank_get().bytes and chunk",
                   "does not depend on n or k",
                   "fpc_match_bank_topk, fpc_homography_bank_topk, fpc_match_bank_guided(best), fpc_homography_bank(best)",
                   "no reservation; k outside [1, kmax]; a NULL cand_slot_dev"):
        assert phrase in hdr, phrase


def test_topk_order_ties_and_fewer_slots_than_k():
    score = np.array([[5, 9, 0, 9, 2, 5],
                      [0, 0, 0, 0, 0, 0],
                      [1, 2, 3, 4, 5, 6],
                      [7, 7, 7, 7, 7, 7]])
    slot, sc = topk_rule(score, 4)
    np.testing.assert_array_equal(slot, [[1, 3, 0, 5], [-1, -1, -1, -1], [5, 4, 3, 2], [0, 1, 2, 3]])
    np.testing.assert_array_equal(sc, [[9, 9, 5, 5], [0, 0, 0, 0], [6, 5, 4, 3], [7, 7, 7, 7]])
    slot, sc = topk_rule(score, 4, min_score=6)                       # fewer qualifying slots than k
    np.testing.assert_array_equal(slot, [[1, 3, -1, -1], [-1, -1, -1, -1], [5, -1, -1, -1], [0, 1, 2, 3]])
    np.testing.assert_array_equal(sc, [[9, 9, 0, 0], [0, 0, 0, 0], [6, 0, 0, 0], [7, 7, 7, 7]])
    for k in (1, 2, 6):
        s1, c1 = topk_rule(score, k)
        np.testing.assert_array_equal(s1, topk_rule(score, 6)[0][:, :k])       # a prefix of the full order
        # column 0 is fpc_match_bank's best: the largest score, ties to the lower slot, -1 below 1
        best = np.where(score.max(1) >= 1, np.argmax(score, 1), -1)
        np.testing.assert_array_equal(s1[:, 0], best)
    # the device's key, restated: (score << 32) | ~slot as uint64, descending
    key = (score[0].astype(np.uint64) << np.uint64(32)) | (~np.arange(6, dtype=np.uint32)).astype(np.uint64)
    np.testing.assert_array_equal(np.argsort(key)[::-1][:4], topk_rule(score, 4)[0][0])


def test_pick_rule():
    cand = np.array([[4, 2, 7], [4, 2, -1], [1, 0, 3], [5, 6, 2]], np.int32)
    ninl = np.array([[0, 31, 31], [12, 0, 0], [0, 0, 0], [9, 9, 10]], np.int32)
    pick, best = pick_rule(ninl, cand)
    np.testing.assert_array_equal(pick, [1, 0, -1, 2])
    np.testing.assert_array_equal(best, [2, 4, -1, 2])
    key = (ninl.astype(np.uint64) << np.uint64(32)) | (~np.arange(3, dtype=np.uint32)).astype(np.uint64)[None]
    np.testing.assert_array_equal(np.where(ninl.max(1) > 0, np.argmax(key, 1), -1), pick)


def test_decoy_scene_appearance_picks_the_decoy_and_geometry_the_true_slot():
    scene = planted_scene(21, [f10(name, i) for name, i in HOMS])
    desc, xy, counts = scene["desc"], scene["xy"], scene["counts"]
    slots = decoy_bank(scene)
    params = dict(iterations=256, seed=3)
    r = relocalise_rule(desc, xy, counts, slots, 3, True, 0.7, 0.0, 0, **params)
    print("scores", r["score"].tolist(), "inliers", r["ninliers"].tolist())
    assert (r["score"][:, B] >= r["score"][:, A]).all() and (r["score"][:, A] > 100).all()
    assert (r["score"][:, B] >= r["score"][:, A] + LOOKALIKES // 2).all()       # the look-alikes do score
    # appearance alone (fpc_match_bank's best) takes the decoy
    np.testing.assert_array_equal(bank_rule(desc, counts, [d for d, _ in slots], True, 0.7)[1], np.full(len(counts), B))
    np.testing.assert_array_equal(r["cand_slot"][:, 0], np.full(len(counts), B))
    np.testing.assert_array_equal(r["cand_slot"][:, 1], np.full(len(counts), A))
    np.testing.assert_array_equal(r["cand_slot"][:, 2], np.full(len(counts), -1))   # the empty and the unrelated slot score 0
    np.testing.assert_array_equal((r["match"] >= 0).sum(2), r["cand_score"])
    assert (r["match"][:, 2] == -1).all()
    # geometry: the decoy's scrambled pixels support no homography, the true key's do
    np.testing.assert_array_equal(r["ninliers"][:, 0], 0)
    assert (r["ninliers"][:, 1] >= 100).all()
    np.testing.assert_array_equal(r["pick"], np.full(len(counts), 1))
    np.testing.assert_array_equal(r["best"], np.full(len(counts), A))
    truth = planted_h(scene, PAIR_KEY)
    for f in range(len(counts)):
        err = corner_error(r["H"][f, 1], truth[f].astype(np.float64).reshape(3, 3))
        print("frame %d: planted-H corner error %.3f px" % (f, err))
        assert err <= CORNER_BAR, (f, err)
        assert not r["H"][f, 0].any() and not r["H"][f, 2].any()


def test_identical_slots_tie_lower_first_and_min_score_leaves_fewer_than_k():
    scene = planted_scene(21, [f10(name, i) for name, i in HOMS])
    desc, xy, counts = scene["desc"], scene["xy"], scene["counts"]
    slots = decoy_bank(scene)
    slots[0] = (scene["key"].copy(), scene["key_xy"].copy())          # slots 0 and A: identical contents
    r = relocalise_rule(desc, xy, counts, slots, 3, True, 0.7, 0.0, 0, iterations=256, seed=3)
    np.testing.assert_array_equal(r["score"][:, 0], r["score"][:, A])
    np.testing.assert_array_equal(r["cand_slot"], np.tile(np.array([B, 0, A], np.int32), (len(counts), 1)))
    np.testing.assert_array_equal(r["match"][:, 1], r["match"][:, 2])
    # equal inlier counts too: the pick goes to the lower j, i.e. the lower slot
    np.testing.assert_array_equal(r["ninliers"][:, 1], r["ninliers"][:, 2])
    np.testing.assert_array_equal(r["pick"], 1)
    np.testing.assert_array_equal(r["best"], 0)
    # a min_score between the true key's and the decoy's score leaves one candidate, above both none
    floor = int(r["score"][:, A].max()) + 1
    assert floor <= r["score"][:, B].min()
    slot, sc = topk_rule(r["score"], 3, floor)
    np.testing.assert_array_equal(slot, np.tile(np.array([B, -1, -1], np.int32), (len(counts), 1)))
    assert (sc[:, 1:] == 0).all()
    slot, _ = topk_rule(r["score"], 3, int(r["score"].max()) + 1)
    assert (slot == -1).all()
    pick, best = pick_rule(np.zeros((len(counts), 3), np.int32), slot)
    assert (pick == -1).all() and (best == -1).all()
