"""CPU checks of top-K relocalisation by pose (fpc_pnp_topk_reserve / fpc_pnp_bank_topk / fpc_p3p_bank_topk /
fpc_fundamental_bank_topk / fpc_essential_bank_topk): the entry points exist, are bound with the prototypes of
include/fpc.h and refuse a NULL context; the header carries the contract; and the float64 restatements the suite already
has, chained (`relocalise_pose_rule`: topk_rule -> candidate_tables -> pnp_rule / p3p_rule / the fundamental ransac_rule /
essential_rule keyed by the FRAME -> pick_rule), show on a 3-D decoy scene what the calls are for.

The scene is tests/test_match_pose.py's GPU_SCENE (seed 11, eight cameras, 792 key rows with landmarks, 820 rows per frame);
the bank is tests/test_match_bank_topk.py's decoy bank: slot A holds the key, slot B decoy_slot(scene) -- the key's
descriptors plus look-alike rows, every row at a random pixel -- with landmarks drawn uniformly in the scene's box
[-4, 4] x [-3, 3] x [2, 8], all valid.  Appearance takes the decoy in every frame; behind the two tables, at 256 iterations
and seed 3, the absolute-pose models keep NO inlier on the decoy, the epipolar models a chance handful (a pair is held to a
line, not to a point), and all four pick the true slot, whose PnP / P3P pose meets the planted-truth bars of
tests/test_pnp_ransac.py.  tests/test_gpu_pose_bank_topk.py holds the kernels to these rules."""
import ctypes
import functools
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_essential_ransac import essential_rule
from tests.test_fundamental_ransac import ransac_rule as fundamental_rule
from tests.test_homography_ransac import header_text
from tests.test_match_bank import bank_rule
from tests.test_match_bank_topk import LOOKALIKE_NOISE, LOOKALIKES, A, B, _unit, candidate_tables, decoy_bank, pick_rule, topk_rule
from tests.test_match_pose import FRAME_H, FRAME_W, GPU_SCENE, KVEC, scene_of
from tests.test_p3p_ransac import p3p_rule
from tests.test_pnp_ransac import ROT_BAR, TRANS_BAR, pnp_rule, pose_errors

FPC_E_INVALID = -1
NAMES = ("fpc_pnp_topk_reserve", "fpc_pnp_bank_topk", "fpc_p3p_bank_topk", "fpc_fundamental_bank_topk",
         "fpc_essential_bank_topk")
MODELS = ("pnp", "p3p", "fundamental", "essential")
POSE_RULES = {"pnp": pnp_rule, "p3p": p3p_rule}
OPTIONS = (True, 0.7, 0.0)                     # cross check, max_dist, ratio
PARAMS = dict(iterations=256, seed=3)          # the other fields: each model's defaults
CHANCE = 64                                    # an epipolar model's inliers on a scrambled candidate stay below this (of > 600)


# ---- the chain, restated -----------------------------------------------------------------------------------------------------
def landmark_pairs(xy, m, xyz, valid):
    """A frame's rows against one slot's landmarks -> (rows, pixels float32 [M][2], points float32 [M][3]): the rows whose
    match is a row of the slot with a valid, finite landmark, in ascending order (pnp_gather_kernel's list)."""
    ok = np.isfinite(xyz).all(1) & (np.ones(len(xyz), bool) if valid is None else np.asarray(valid, bool))
    rows = np.flatnonzero((m >= 0) & (m < len(xyz)))
    rows = rows[ok[m[rows]]]
    return rows, xy[rows].astype(np.float32), xyz[m[rows]]


def pixel_pairs(xy, m, txy):
    """... against one slot's pixels -> (rows, src float32 [M][2], dst float32 [M][2]) (hf_gather_kernel's list)."""
    rows = np.flatnonzero((m >= 0) & (m < len(txy)))
    return rows, xy[rows].astype(np.float32), txy[m[rows]].astype(np.float32)


def candidate_rule(model, xy, count, m, slot, params, f, kvec=KVEC):
    """Problem (f, j): one frame's table `m` against `slot` = (desc, xy, xyz, valid) under `model`, its sampler keyed by the
    frame f -> dict(model: R [3][3] and t [3], or F [3][3]; ninliers; mask bool [cap] by query row)."""
    mask = np.zeros(len(m), bool)
    m = m[:count]
    if model in POSE_RULES:
        rows, pxy, pxyz = landmark_pairs(xy, m, slot[2], slot[3])
        res = POSE_RULES[model](pxy, pxyz, params, f, kvec)
        mask[rows] = res.mask
        return dict(R=res.R, t=res.t, ninliers=res.ninliers, mask=mask, rows=rows, res=res)
    rows, src, dst = pixel_pairs(xy, m, slot[1])
    if model == "fundamental":
        fm, inl = fundamental_rule(src, dst, params, f)
    else:
        res = essential_rule(src, dst, params, f, kvec, kvec)
        fm, inl = res.F.reshape(3, 3), res.mask
    mask[rows] = inl
    return dict(F=fm, ninliers=int(inl.sum()), mask=mask, rows=rows)


def relocalise_pose_rule(desc, xy, counts, slots, k, model, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0,
                         kvec=KVEC, **params):
    """The shortlist and one problem per (frame, candidate) -> dict(score, cand_slot, cand_score, match [n][k][cap], cand
    [n][k] of candidate_rule's dicts (None: a candidate of -1), ninliers [n][k], pick [n], best [n]).  slots: list of (desc,
    xy, xyz, valid)."""
    n = len(counts)
    score = bank_rule(desc, counts, [s[0] for s in slots], cross_check, max_dist, ratio, min_score)[0]
    cand_slot, cand_score = topk_rule(score, k, min_score)
    match = candidate_tables(desc, xy, counts, [(s[0], s[1]) for s in slots], cand_slot, cross_check, max_dist, ratio)
    cand = [[None] * k for _ in range(n)]
    ninl = np.zeros((n, k), np.int32)
    for f in range(n):
        for j in range(k):
            if cand_slot[f, j] >= 0:
                cand[f][j] = candidate_rule(model, xy[f], counts[f], match[f, j], slots[cand_slot[f, j]], params, f, kvec)
                ninl[f, j] = cand[f][j]["ninliers"]
    pick, best = pick_rule(ninl, cand_slot)
    return dict(score=score, cand_slot=cand_slot, cand_score=cand_score, match=match, cand=cand, ninliers=ninl, pick=pick,
                best=best)


# ---- the decoy scene ----------------------------------------------------------------------------------------------------------
def box_landmarks(rows, seed):
    """`rows` landmarks drawn uniformly in the scenes' box, all valid: the decoy's scrambled map."""
    rng = np.random.Generator(np.random.PCG64([seed, rows]))
    return np.stack([rng.uniform(-4, 4, rows), rng.uniform(-3, 3, rows), rng.uniform(2, 8, rows)], 1).astype(np.float32)


def decoy_slot_of(scene, lookalikes=LOOKALIKES, seed=3):
    """tests/test_match_bank_topk.py's decoy_slot with the number of look-alike rows per frame as an argument (a bank of
    1024 rows holds the 792 key rows and 29 look-alikes per frame; LOOKALIKES: decoy_slot itself, draw for draw)."""
    rng = np.random.Generator(np.random.PCG64([seed, len(scene["key"])]))
    extra = []
    for f, cnt in enumerate(scene["counts"]):
        rows = np.flatnonzero(scene["ids"][f, :cnt] < 0)[:lookalikes]
        assert len(rows) == lookalikes
        extra.append(_unit(scene["desc"][f, rows] + rng.normal(0, LOOKALIKE_NOISE, (len(rows), scene["desc"].shape[2]))))
    d = np.concatenate([scene["key"]] + extra)
    p = np.stack([rng.integers(0, FRAME_W, len(d)), rng.integers(0, FRAME_H, len(d))], 1).astype(np.int32)
    return d, p


def with_landmarks(scene, slots):
    """decoy_bank's (desc, xy) slots as (desc, xy, xyz, valid): the key's own landmarks and flags in slot A, box landmarks,
    all valid, everywhere else."""
    out = []
    for sl, (d, p) in enumerate(slots):
        if sl == A:
            out.append((d, p, scene["key_xyz"], scene["key_valid"]))
        else:
            out.append((d, p, box_landmarks(len(d), 40 + sl), np.ones(len(d), bool)))
    return out


@functools.lru_cache(maxsize=None)
def decoy_chain(model):
    """relocalise_pose_rule on the decoy scene, k = 3, computed once per model."""
    scene = scene_of(GPU_SCENE)
    slots = with_landmarks(scene, decoy_bank(scene))
    return scene, slots, relocalise_pose_rule(scene["desc"], scene["xy"], scene["counts"], slots, 3, model, *OPTIONS, 0,
                                              **PARAMS)


# ---- tests --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound_with_the_stated_prototypes():
    lib = _lib.load()
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name) and name in exported, name
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.fpc_pnp_topk_reserve.argtypes == [vp, ctypes.POINTER(ctypes.c_size_t)]
    assert lib.fpc_pnp_bank_topk.argtypes == [vp, ci, ci, vp, vp, ctypes.POINTER(_lib.FpcPnpParams)] + [vp] * 8
    assert lib.fpc_p3p_bank_topk.argtypes == lib.fpc_pnp_bank_topk.argtypes
    assert lib.fpc_fundamental_bank_topk.argtypes == [vp, ci, ci, vp, vp, ctypes.POINTER(_lib.FpcRansacParams)] + [vp] * 6
    assert lib.fpc_essential_bank_topk.argtypes == [vp, ci, ci, vp, vp, ctypes.POINTER(_lib.FpcEssentialParams)] + [vp] * 7
    # the header's parameter lists, counted
    for name, nargs in zip(NAMES, (2, 14, 14, 12, 13)):
        args = re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == nargs == len(getattr(lib, name).argtypes), (name, args)
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 == lib.fpc_abi_version()   # symbols were only added
    from fpc_amd.engine import Engine
    for name in ("pnp_topk_reserve", "pnp_bank_topk", "p3p_bank_topk", "fundamental_bank_topk", "essential_bank_topk"):
        assert callable(getattr(Engine, name)), name
        assert name == "pnp_topk_reserve" or callable(getattr(Engine, name + "_async")), name
    assert callable(Engine.relocalise_pose)


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)
    p = buf.ctypes.data
    rp, pp, ep = _lib.FpcRansacParams(), _lib.FpcPnpParams(), _lib.FpcEssentialParams()
    nbytes = ctypes.c_size_t(0)
    assert lib.fpc_default_ransac_params(ctypes.byref(rp)) == 0 and lib.fpc_default_pnp_params(ctypes.byref(pp)) == 0
    assert lib.fpc_default_essential_params(ctypes.byref(ep)) == 0
    assert lib.fpc_pnp_topk_reserve(None, ctypes.byref(nbytes)) == FPC_E_INVALID
    assert lib.fpc_pnp_bank_topk(None, 1, 1, p, p, ctypes.byref(pp), p, p, p, p, p, p, p, p) == FPC_E_INVALID
    assert lib.fpc_p3p_bank_topk(None, 1, 1, p, p, ctypes.byref(pp), p, p, p, p, p, p, p, p) == FPC_E_INVALID
    assert lib.fpc_fundamental_bank_topk(None, 1, 1, p, p, ctypes.byref(rp), p, p, p, p, p, p) == FPC_E_INVALID
    assert lib.fpc_essential_bank_topk(None, 1, 1, p, p, ctypes.byref(ep), p, p, p, p, p, p, p) == FPC_E_INVALID
    assert (buf == 0).all() and nbytes.value == 0


def test_header_carries_the_contract():
    hdr = " ".join(re.sub(r"\n \* ?", " ", header_text()).split())       # comment blocks as running text
    for phrase in ("fpc_pnp_topk_reserve: needs a bank and a fpc_bank_topk_reserve reservation, whose kmax it takes",
                   "No fpc_pnp_reserve is needed",
                   "bit-identical to fpc_pnp_bank / fpc_p3p_bank(n, slot = cand_slot[.][j], match = match[.][j], params)",
                   "The sampler and the refit's re-derivation hash f, not f k + j",
                   "zeros where pick[f] is -1",
                   "fpc_match_bank_guided_pose(best, best_R, best_t)",
                   "fpc_match_bank_guided_epipolar(best, best_F) and fpc_pose_bank",
                   "bit-identical to fpc_fundamental_bank / fpc_essential_bank with column j",
                   "still collects CHANCE inliers: 15 - 36",
                   "min_inliers is therefore the CALLER's floor against chance, and pick is by maximum",
                   "(gather, score, refit, pick) does not depend on n or k",
                   "no fpc_pnp_topk_reserve (absolute-pose calls); k outside [1, kmax]"):
        assert phrase in hdr, phrase


def test_decoy_slot_of_is_decoy_slot_draw_for_draw():
    from tests.test_match_bank_topk import decoy_slot
    scene = scene_of(GPU_SCENE)
    d, p = decoy_slot(scene)
    d2, p2 = decoy_slot_of(scene)
    np.testing.assert_array_equal(d, d2)
    np.testing.assert_array_equal(p, p2)
    d3, _ = decoy_slot_of(scene, 29)
    assert len(d3) == 1024 == GPU_SCENE["cap"] and len(d) == 1032                 # 29 per frame: the decoy that a bank holds


@pytest.mark.parametrize("model", MODELS)
def test_decoy_scene_appearance_picks_the_decoy_and_every_model_the_true_slot(model):
    scene, slots, r = decoy_chain(model)
    n = len(scene["counts"])
    assert n == 8 and len(scene["key"]) == 792 and (scene["counts"] == 820).all()
    # the premise: appearance takes the decoy in EVERY frame
    print(model, "scores B", r["score"][:, B].tolist(), "A", r["score"][:, A].tolist(), "inliers", r["ninliers"].tolist())
    assert (r["score"][:, B] > r["score"][:, A]).all() and (r["score"][:, A] > 500).all()
    np.testing.assert_array_equal(bank_rule(scene["desc"], scene["counts"], [s[0] for s in slots], *OPTIONS)[1], np.full(n, B))
    np.testing.assert_array_equal(r["cand_slot"], np.tile(np.array([B, A, -1], np.int32), (n, 1)))
    np.testing.assert_array_equal((r["match"] >= 0).sum(2), r["cand_score"])
    # geometry: nothing (pose) or chance (epipolar) on the decoy, the true slot in every frame
    if model in POSE_RULES:
        np.testing.assert_array_equal(r["ninliers"][:, 0], 0)
        assert all(not c[0]["R"].any() and not c[0]["t"].any() and not c[0]["mask"].any() for c in r["cand"])
        assert all(len(c[0]["rows"]) == sc for c, sc in zip(r["cand"], r["cand_score"][:, 0]))   # every decoy landmark is valid
    else:
        assert (r["ninliers"][:, 0] < CHANCE).all()
    assert (r["ninliers"][:, 1] >= 400).all()
    np.testing.assert_array_equal(r["pick"], np.full(n, 1))
    np.testing.assert_array_equal(r["best"], np.full(n, A))                  # every frame is included
    assert all(c[2] is None for c in r["cand"])
    if model in POSE_RULES:
        for f in range(n):
            cam = scene["cams"][1 + f]
            rot, tr = pose_errors(r["cand"][f][1]["R"], r["cand"][f][1]["t"], (None, None, None, cam[0], cam[1]))
            print("  %s frame %d: %d of %d pairs, rotation %.4f deg, translation %.3e"
                  % (model, f, r["ninliers"][f, 1], len(r["cand"][f][1]["rows"]), rot, tr))
            assert rot <= ROT_BAR and tr <= TRANS_BAR, (model, f, rot, tr)
    else:
        # the epipolar models keep every pair of the true table but the few whose rounded pixels leave the 3 px band
        assert all(c[1]["ninliers"] >= 0.95 * len(c[1]["rows"]) for c in r["cand"])


def test_the_sampler_is_keyed_by_the_frame_not_by_the_problem():
    """Problem (f, j) is the single-slot rule at frame index f: with another key (f k + j, a batch index) the best sample
    differs, which is what a kmax-for-k stride or a hashed problem index would show on the device."""
    scene, slots, r = decoy_chain("p3p")
    f, j, k = 5, 1, 3
    c = r["cand"][f][j]
    pxy, pxyz = scene["xy"][f, c["rows"]].astype(np.float32), slots[A][2][r["match"][f, j, c["rows"]]]
    assert p3p_rule(pxy, pxyz, PARAMS, f).best_t == c["res"].best_t
    assert p3p_rule(pxy, pxyz, PARAMS, f * k + j).best_t != c["res"].best_t
