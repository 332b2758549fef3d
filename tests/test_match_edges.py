"""The matchers' float64 rule at tile edges and on non-finite rows, and the planted scenes that
tests/test_gpu_match_edges.py holds the five 64 x 64 distance tiles to (csrc/match.h, match_frames.h, match_guided.h,
match_guided_epipolar.h, match_bank_bf16.h).  CPU only.

The rule is tests/test_match_frames.py's `pair_rule` (and `first_rule` here) with include/fpc.h's rule for non-finite
descriptor rows: a pair whose distance is NaN or +inf is no row minimum, no column minimum, no second best and within no
tolerance; a row without a finite distance is -1 / +inf.

Scenes (numpy only, fixed seeds; a scene is a dict: "batches" of eight frames each -- desc [8][384][D], xy, counts -- "keys"
and "slots" as (desc, xy) pairs, "protected": the rows per set that no comparison may leave out):
  "edges"      every count of E = {0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 384} occurs as a query
               count and as a train count.  Every set of n rows holds noisy copies (sigma = 0.02, renormalised) of rows
               0 .. n - 1 of one pool of unit rows: pool row 0 in its LAST row, pool row 1 in the first row of its last
               64-row tile, the others shuffled.  So in every pair of non-empty sets the last query row and the last train
               row are mutual nearest neighbours, and min(nq, nt) rows have a copy on the other side.
  "ties"       the same construction at 384 / 257 rows with exact duplicates (bit-equal rows, hence bit-equal d^2): train
               rows 63 / 64 (two waves), 0 / 256 (one wave, two rounds), 255 / 256, query rows 63 / 64 (two strips: a tie
               of the column minimum) and 127 / 128 (two workgroups of match_gemm_kernel).  The lower index wins.
  "nonfinite"  the "edges" data with NaN rows, rows with one NaN, one +Inf, +Inf and -Inf planted at rows 0, 63, 64, n - 1
               and a few more, among queries and train rows alike, an all-NaN frame, key set and bank slot.

Left out of an index comparison (the bars of test_gpu_match_frames.py's `_ratio_exclusions` and test_match_guided.py's
`left_out`): a row whose nearest and second nearest, or whose column's two lowest, differ by less than 2e-5 in distance
without being equal, or whose distance lies within 1e-5 of a threshold.  At most 1 % of a frame's rows, none of them
protected: asserted below from the rule alone.

The comparison (`compare`, `compare_first`: what the GPU module applies to the device's tables) is itself checked here in
the manner of tests/test_layer_oracle.py: numpy emulations of a kernel with one mistake each must fail it."""
import functools

import numpy as np
import pytest

from tests.test_match_frames import PAIR_KEY, PAIR_PREVIOUS  # noqa: F401  (the GPU module takes them from here)
from tests.test_match_frames import pair_rule as _pair_rule

CAP = 384
E = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, CAP)
FRAME_H, FRAME_W = 120, 160
NOISE = 0.02
TIE = 2e-5                     # distance: a smaller gap between the two lowest of a row or a column leaves the row out
EDGE = 1e-5                    # distance: closer to max_dist, ratio * d2 or the tolerance leaves the row out
BAR_D128 = 2e-6                # d^2 against float64 at D = 128: the bar of test_gpu_match_frames.py and _compare
OPTIONS = ((True, 0.0, 0.0), (False, 0.0, 0.0), (True, 0.7, 0.0), (False, 0.0, 0.8), (True, 0.7, 0.8))
TIE_OPTIONS = OPTIONS + ((False, 0.0, 0.99),)
TOLERANCES = (0.8, 0.3)
COUNTS = ((0, 129, 2, 63, 127, 128, 191, 64), (192, 193, 255, 256, 65, 1, 257, CAP))
KEY_ROWS = (1, 64, 65, 257, CAP)
SLOT_ROWS = (CAP, 256, 129, 64)
EXPLICIT = ((1, 1), (64, 65), (65, 64), (129, 257), (CAP, CAP))          # fpc_match / fpc_first_within pair shapes
SEEDS = {("edges", 128): 3, ("edges", 256): 5, ("ties", 128): 7}
BUGS = ("nan_to_zero", "drop_last_column", "drop_last_query_row", "tie_to_higher_index", "skip_second_round")


def analytic_bar(dim):
    """DESIGN.md's bound on the fp32 d^2 of unit rows: 8 D 2^-24."""
    return 8.0 * dim * 2.0 ** -24


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def _gram(a, b):
    """a b^T with every dot product through the same loop: bit-equal rows give bit-equal products, at any position."""
    return np.einsum("ik,jk->ij", a, b)


def pair_rule(q, t, cross_check=True, max_dist=0.0, ratio=0.0):
    """tests/test_match_frames.py's rule, with exact ties where rows are bit-equal (`_gram`)."""
    return _pair_rule(q, t, cross_check, max_dist, ratio, gram=_gram)


def distances(q, t):
    """pair_rule's float64 distance matrix [nq][nt], non-finite entries masked to +inf."""
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * _gram(q64, t64)
        dd = np.sqrt(np.maximum(dd, 0.0))
    dd[~np.isfinite(dd)] = np.inf
    return dd


def first_rule(key, cur, tolerance):
    """SearchKeyFrameCorrespondence in float64 -> (first int32 [nk]: the lowest row of `cur` closer than `tolerance` or -1,
    borderline bool [nk]: some distance within EDGE of the tolerance).  A non-finite distance is within no tolerance."""
    nk = len(key)
    first, border = np.full(nk, -1, np.int32), np.zeros(nk, bool)
    if nk == 0 or len(cur) == 0:
        return first, border
    dd = distances(key, cur)
    tol = float(np.float32(tolerance))
    hit = dd < tol
    first[hit.any(1)] = np.argmax(hit, axis=1)[hit.any(1)]
    border = (np.abs(dd - tol) < EDGE).any(1)
    return first, border


def exclusions(dd, rule, cross_check, max_dist, ratio, tie=TIE, edge=EDGE, squared=False):
    """The rows of one pair that an index comparison leaves out (module docstring).  An exact tie is decided by the index
    and is NOT left out.  squared: `tie` and `edge` bound differences of d^2 instead of differences of the distance (the bf16
    bank, whose tolerance is derived for d^2)."""
    _, d1, d2 = rule
    nq, nt = dd.shape
    out = np.zeros(nq, bool)
    if nq == 0 or nt == 0:
        return out
    p = 2 if squared else 1
    fin1, fin2 = np.isfinite(d1), np.isfinite(d2)
    with np.errstate(invalid="ignore"):
        out |= fin2 & (d2 ** p - d1 ** p < tie) & (d2 != d1)
        if cross_check and nq >= 2:
            low = np.sort(dd, axis=0)[:2]
            near = np.isfinite(low[1]) & (low[1] ** p - low[0] ** p < tie) & (low[1] != low[0])
            out |= fin1 & near[np.argmin(dd, axis=1)]
        if max_dist > 0:
            out |= fin1 & (np.abs(d1 ** p - max_dist ** p) < edge)
        if ratio > 0:
            out |= fin2 & (np.abs(d1 ** p - (ratio * d2) ** p) < edge)
    return out


def reference_rows(q, t, options, tie=TIE, edge=EDGE, squared=False, dd=None):
    """The rule on one pair of row sets -> (match, d1, d2, left out).  dd: distances(q, t), where the caller has it."""
    rule = pair_rule(q, t, *options)
    return rule + (exclusions(distances(q, t) if dd is None else dd, rule, *options, tie, edge, squared),)


@functools.lru_cache(maxsize=None)
def _scene_rows(name, dim, q, t, bf16):
    """(query rows, train rows, their distances) of the sets q and t of a scene, once per pair."""
    scene = scene_of(name, dim)
    qr = rows_of(scene, q)
    tr = rows_of(scene, t) if t is not None else qr[:0]
    if bf16:
        from tests.test_match_bank_bf16 import bf16_round
        qr, tr = bf16_round(qr), bf16_round(tr)
    return qr, tr, distances(qr, tr)


@functools.lru_cache(maxsize=None)
def reference(name, dim, q, t, options, bf16=False):
    """reference_rows on the sets q and t (ids; t None: no train rows) of scene `name`, computed once and shared.  bf16: on
    the rows rounded as the bf16 bank stores them (a NaN to 0x7FC0), left out within twice the derived d^2 tolerance
    8 D 2^-24 of tests/test_gpu_match_bank_bf16.py."""
    qr, tr, dd = _scene_rows(name, dim, q, t, bf16)
    if bf16:
        ref = reference_rows(qr, tr, options, 2 * analytic_bar(dim), 2 * analytic_bar(dim), True, dd)
    else:
        ref = reference_rows(qr, tr, options, dd=dd)
    for a in ref:
        a.setflags(write=False)
    return ref


def compare(m, d, ref, bar, label="", share=0.01):
    """One pair's table (match int32 [nq], dist float32 [nq]: the device's, or an emulation's) against the rule `ref`
    (reference / reference_rows): indices exact outside the rows left out, which are at most `share` of the rows; a row
    without a finite distance exactly -1 / +inf; dist^2 within `bar` of float64 (of the second best where the row is left
    out and the device took that one).  -> (largest d^2 error, rows left out)."""
    rm, rd1, rd2, out = ref
    m, d = np.asarray(m), np.asarray(d, np.float64)
    assert m.shape == rm.shape and d.shape == rd1.shape, label
    assert out.sum() <= share * len(rm), "%s: %d of %d rows left out" % (label, out.sum(), len(rm))
    np.testing.assert_array_equal(m[~out], rm[~out], err_msg=label)
    fin = np.isfinite(rd1)
    np.testing.assert_array_equal(np.isfinite(d), fin, err_msg=label)
    assert (d[~fin] == np.inf).all() and (m[~fin] == -1).all(), label
    worst = 0.0
    if fin.any():
        err = np.abs(d[fin] ** 2 - rd1[fin] ** 2)
        with np.errstate(invalid="ignore"):
            other = np.abs(d[fin] ** 2 - rd2[fin] ** 2)
        err = np.where(out[fin] & (other < err), other, err)
        worst = float(err.max())
    assert worst <= bar, "%s: d^2 off by %.3e (bar %.3e)" % (label, worst, bar)
    return worst, int(out.sum())


def compare_first(first, key, cur, tolerance, label=""):
    """fpc_first_within's output for one pair against first_rule, exact outside the borderline rows (<= 1 %)."""
    want, border = first_rule(key, cur, tolerance)
    assert border.sum() <= 0.01 * len(want), "%s: %d of %d rows left out" % (label, border.sum(), len(want))
    np.testing.assert_array_equal(np.asarray(first)[~border], want[~border], err_msg=label)
    return int(border.sum())


# ---- the same expression in fp32, with or without a mistake ---------------------------------------------------------------------
def d2_fp32(q, t):
    """d^2 = |q|^2 + |t|^2 - 2 q.t in plain fp32 (numpy float32), every sum accumulated term by term over the D components
    as a C loop over float would; negatives and -0 to +0, a NaN stays."""
    q32, t32 = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)
    qn, tn = np.zeros(len(q32), np.float32), np.zeros(len(t32), np.float32)
    acc = np.zeros((len(q32), len(t32)), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(q32.shape[1]):
            qn += q32[:, k] * q32[:, k]
            tn += t32[:, k] * t32[:, k]
            acc += q32[:, k, None] * t32[None, :, k]
        d2 = qn[:, None] + tn[None, :] - np.float32(2) * acc
        return np.where(d2 <= 0, np.float32(0), d2)


def emulate(q, t, options, bug=None, fp32=False):
    """What a matcher returns for one pair -> (match int32 [nq], dist float32 [nq]): d^2 in float64 (fp32: d2_fp32), the
    scans with a strict < against +inf, the keys' tie order, dist = sqrtf(d^2).  bug: one of BUGS, the mistake of a
    wrong kernel."""
    cross, md, ratio = options
    nq, nt = len(q), len(t)
    m, d = np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    if nq == 0 or nt == 0:
        return m, d
    if fp32:
        d2 = d2_fp32(q, t).astype(np.float64)
    else:
        q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = (q64 * q64).sum(1)[:, None] + (t64 * t64).sum(1)[None, :] - 2.0 * q64 @ t64.T
            d2 = np.where(d2 <= 0, 0.0, d2)
    with np.errstate(invalid="ignore"):
        if bug == "nan_to_zero":
            d2 = np.where(d2 > 0, d2, 0.0)                              # d2 > 0 ? d2 : 0 -- a NaN becomes an exact hit
        d2 = np.where(d2 < np.inf, d2, np.inf)                          # e < best with best = +inf: NaN and +inf never win
    rowscan, colscan = d2.copy(), d2.copy()
    if bug == "drop_last_column" and nt % 64:
        rowscan[:, nt - 1] = colscan[:, nt - 1] = np.inf
    if bug == "skip_second_round":
        rowscan[:, 256:] = colscan[:, 256:] = np.inf
    if bug == "drop_last_query_row" and nq % 64:
        colscan[nq - 1] = np.inf
    rows = np.arange(nq)
    if bug == "tie_to_higher_index":
        order = nt - 1 - np.argsort(rowscan[:, ::-1], axis=1, kind="stable")
        colmin = nq - 1 - np.argmin(colscan[::-1], axis=0)
    else:
        order = np.argsort(rowscan, axis=1, kind="stable")
        colmin = np.argmin(colscan, axis=0)
    best = order[:, 0]
    b1 = rowscan[rows, best]
    b2 = rowscan[rows, order[:, 1]] if nt >= 2 else np.full(nq, np.inf)
    d1 = np.sqrt(b1.astype(np.float32))
    ok = b1 < np.inf
    if cross:
        ok &= colmin[best] == rows
    if md > 0:
        ok &= d1 < np.float32(md)
    if ratio > 0:
        with np.errstate(invalid="ignore"):
            ok &= (b2 < np.inf) & (d1 < np.float32(ratio) * np.sqrt(b2.astype(np.float32)))
    m[ok] = best[ok]
    d[b1 < np.inf] = d1[b1 < np.inf]
    return m, d


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _pixels(rng, n):
    return np.stack([rng.integers(0, FRAME_W, n), rng.integers(0, FRAME_H, n)], 1).astype(np.int32)


def _bases(rng, n):
    """Which pool row each of a set's n rows copies: pool row 0 in the last row, pool row 1 in the first row of the last
    64-row tile (where that is another row), the others shuffled."""
    b = np.full(n, -1, np.int64)
    if n == 0:
        return b
    b[n - 1] = 0
    r = 64 * ((n - 1) // 64)
    if r != n - 1:
        b[r] = 1
    rest = np.setdiff1d(np.arange(n), b[b >= 0])
    b[b < 0] = rng.permutation(rest)
    return b


def _copies(rng, pool, n):
    b = _bases(rng, n)
    rows = _unit(pool[b].astype(np.float64) + rng.normal(0, NOISE, (n, pool.shape[1])))
    return rows.reshape(n, pool.shape[1]), b


def _planted_rows(n):
    return set() if n == 0 else {n - 1, 64 * ((n - 1) // 64)}


def _assemble(name, dim, counts, sets, keys, slots, rng):
    """sets: per batch a list of eight row arrays -> the scene dict, xy drawn for every set."""
    scene = {"name": name, "dim": dim, "batches": [], "keys": [], "slots": [], "protected": {}}
    for b, frames in enumerate(sets):
        desc = np.zeros((len(frames), CAP, dim), np.float32)
        xy = np.zeros((len(frames), CAP, 2), np.int32)
        for f, rows in enumerate(frames):
            desc[f, :len(rows)] = rows
            xy[f, :len(rows)] = _pixels(rng, len(rows))
            scene["protected"]["frame", b, f] = _planted_rows(len(rows))
        scene["batches"].append({"desc": desc, "xy": xy, "counts": np.array(counts[b], np.int32)})
    for kind, group in (("key", keys), ("slot", slots)):
        for i, rows in enumerate(group):
            scene[kind + "s"].append((np.ascontiguousarray(rows, np.float32), _pixels(rng, len(rows))))
            scene["protected"][kind, i] = _planted_rows(len(rows))
    return scene


def _freeze(scene):
    for batch in scene["batches"]:
        for a in batch.values():
            a.setflags(write=False)
    for group in (scene["keys"], scene["slots"]):
        for d, p in group:
            d.setflags(write=False)
            p.setflags(write=False)
    return scene


def _edges_sets(dim):
    rng = np.random.Generator(np.random.PCG64(SEEDS["edges", dim]))
    pool = _unit(rng.normal(size=(CAP, dim)))
    sets = [[_copies(rng, pool, n)[0] for n in batch] for batch in COUNTS]
    keys = [_copies(rng, pool, n)[0] for n in KEY_ROWS]
    slots = [_copies(rng, pool, n)[0] for n in SLOT_ROWS]
    return rng, sets, keys, slots


def _poison(rows, s, train_only):
    """Non-finite rows into a copy of `rows` (set number s) -> (rows, the poisoned indices)."""
    rows = rows.copy()
    n = len(rows)
    kinds = ("nan_row", "nan_one", "inf_one", "inf_pm")
    spots = {}
    if n >= 3:
        spots[0] = kinds[s % 4] if train_only else "nan_row"
    if n > 64:
        spots[63] = "nan_row" if not train_only else kinds[(s + 3) % 4]
        spots[64] = kinds[(s + 2) % 4] if train_only else "nan_row"
    if n >= 2 and n - 1 not in spots:
        spots[n - 1] = kinds[(s + 1) % 4]                             # the target of a planted copy
    for pos, kind in ((5, "nan_one"), (17, "inf_one"), (40, "inf_pm")):
        if pos < n - 1 and pos not in spots:
            spots[pos] = kind
    for i, kind in spots.items():
        if kind == "nan_row":
            rows[i] = np.nan
        elif kind == "nan_one":
            rows[i, 11] = np.nan
        elif kind == "inf_one":
            rows[i, 7] = np.inf
        else:
            rows[i, 3], rows[i, 90] = np.inf, -np.inf
    return rows, set(spots)


NAN_FRAME, NAN_KEY, NAN_SLOT = (0, 3), 1, 3          # the all-NaN sets of "nonfinite": 63, 64 and 64 rows


@functools.lru_cache(maxsize=None)
def scene_of(name, dim=128):
    """The scene `name` at descriptor length `dim`, built once and read-only."""
    if name in ("edges", "nonfinite"):
        rng, sets, keys, slots = _edges_sets(dim)
        bad = {}
        if name == "nonfinite":
            s = 0
            for b, frames in enumerate(sets):
                for f in range(len(frames)):
                    frames[f], bad["frame", b, f] = _poison(frames[f], s, False)
                    s += 1
            for kind, group in (("key", keys), ("slot", slots)):
                for i in range(len(group)):
                    group[i], bad[kind, i] = _poison(group[i], s, True)
                    s += 1
            for sid, group, i in ((("frame",) + NAN_FRAME, sets[NAN_FRAME[0]], NAN_FRAME[1]), (("key", NAN_KEY), keys, NAN_KEY),
                                  (("slot", NAN_SLOT), slots, NAN_SLOT)):
                group[i] = np.full_like(group[i], np.nan)
                bad[sid] = set(range(len(group[i])))
        scene = _assemble(name, dim, COUNTS, sets, keys, slots, rng)
        for sid, rows in bad.items():
            scene["protected"][sid] |= rows
        scene["nonfinite"] = bad
        return _freeze(scene)
    assert name == "ties"
    rng = np.random.Generator(np.random.PCG64(SEEDS["ties", dim]))
    pool = _unit(rng.normal(size=(CAP, dim)))
    counts = ((CAP, CAP, CAP, 257, CAP, 129, CAP, 65),)
    frames = [_copies(rng, pool, n)[0] for n in counts[0]]
    keys = [_copies(rng, pool, n)[0] for n in (CAP, CAP, CAP, 257)]
    slots = [_copies(rng, pool, n)[0] for n in (CAP, CAP, CAP, 257)]
    # (set, rows made bit-equal): the second row becomes a copy of the first
    dups = {("frame", 0, 0): ((63, 64), (0, 256)), ("frame", 0, 1): ((63, 64), (127, 128)), ("frame", 0, 2): ((255, 256),),
            ("key", 0): ((63, 64), (0, 256)), ("key", 1): ((255, 256),), ("key", 3): ((127, 128),),
            ("slot", 0): ((63, 64), (0, 256)), ("slot", 1): ((255, 256),), ("slot", 3): ((127, 128),)}
    groups = {"frame": frames, "key": keys, "slot": slots}
    for sid, pairs in dups.items():
        for a, b in pairs:
            groups[sid[0]][sid[-1]][b] = groups[sid[0]][sid[-1]][a]
    scene = _assemble("ties", dim, counts, [frames], keys, slots, rng)
    for sid, pairs in dups.items():
        scene["protected"][sid] |= {i for p in pairs for i in p}
    scene["dups"] = dups
    return _freeze(scene)


def rows_of(scene, sid):
    """The descriptor rows of the set `sid`: ("frame", batch, f), ("key", i) or ("slot", i)."""
    if sid[0] == "frame":
        batch = scene["batches"][sid[1]]
        return batch["desc"][sid[2], :batch["counts"][sid[2]]]
    return scene[sid[0] + "s"][sid[1]][0]


def pairs_of(scene, batch, kinds=("key", "previous", "slot")):
    """(query set, train set or None) of every pair that a call on `batch` matches: each frame against each key, against
    its predecessor (frame 0: nothing) and against each bank slot."""
    out = []
    for f in range(len(scene["batches"][batch]["counts"])):
        q = ("frame", batch, f)
        if "key" in kinds:
            out += [(q, ("key", i)) for i in range(len(scene["keys"]))]
        if "previous" in kinds:
            out.append((q, ("frame", batch, f - 1) if f else None))
        if "slot" in kinds:
            out += [(q, ("slot", i)) for i in range(len(scene["slots"]))]
    return out


def all_pairs(scene, kinds=("key", "previous", "slot")):
    return [p for b in range(len(scene["batches"])) for p in pairs_of(scene, b, kinds) if p[1] is not None]


def explicit_pair(scene, nq, nt):
    """A (query set, train set) of the "edges" layout with these row counts: a frame against a key set."""
    for b, batch in enumerate(COUNTS):
        if nq in batch:
            return ("frame", b, batch.index(nq)), ("key", KEY_ROWS.index(nt))
    raise KeyError((nq, nt))


def train_of(scene, batch, f, pairing, key):
    """The train set id of frame f under fpc_match_frames' pairing (key: a key index or None)."""
    if pairing == PAIR_PREVIOUS and f > 0:
        return ("frame", batch, f - 1)
    return None if key is None else ("key", key)


def fp32_error(scene, pairs, options=(False, 0.0, 0.0)):
    """The largest d^2 error of the plain fp32 evaluation (emulate(fp32=True)) over `pairs`, by compare's own measure."""
    worst = 0.0
    for q, t in pairs:
        if t is None:
            continue
        m, d = emulate(rows_of(scene, q), rows_of(scene, t), options, fp32=True)
        ref = reference(scene["name"], scene["dim"], q, t, options)
        worst = max(worst, compare(m, d, ref, analytic_bar(scene["dim"]), "fp32 %s %s" % (q, t))[0])
    return worst


# ---- tests ------------------------------------------------------------------------------------------------------------------
def _masked_like_the_oracle(scene, pairs):
    from oracle import oracle
    for q, t in pairs:
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        if len(qr) == 0:
            continue
        dd = distances(qr, tr)
        for cross, md in ((True, 0.0), (False, 0.0), (True, 0.7)):
            rule = pair_rule(qr, tr, cross, md, 0.0)
            keep = ~exclusions(dd, rule, cross, md, 0.0)
            om, od = oracle.match(qr, tr, cross, md)
            np.testing.assert_array_equal(rule[0][keep], om[keep], err_msg=str((q, t, cross, md)))
            fin = np.isfinite(rule[1])
            np.testing.assert_allclose(od[fin], rule[1][fin], rtol=1e-5, atol=1e-6)
            assert np.isinf(rule[1][~fin]).all() and (rule[0][~fin] == -1).all() and (om[~fin] == -1).all()
        for tol in TOLERANCES:
            first, border = first_rule(tr, qr, tol)                # key = the train set, cur = the query set
            np.testing.assert_array_equal(first[~border], oracle.first_within(tr, qr, tol)[~border])


def test_rule_equals_the_oracle_on_the_scenes():
    for name in ("edges", "ties", "nonfinite"):
        scene = scene_of(name)
        pairs = [explicit_pair(scene, nq, nt) for nq, nt in EXPLICIT] if name != "ties" else []
        pairs += [p for p in all_pairs(scene, ("previous",))] + all_pairs(scene, ("slot",))[:8]
        _masked_like_the_oracle(scene, pairs)


def test_edges_scene_covers_the_edge_set_and_plants_what_it_claims():
    scene = scene_of("edges")
    nq = {int(c) for batch in scene["batches"] for c in batch["counts"]}
    nt = {len(rows_of(scene, t)) for _, t in all_pairs(scene)}
    assert nq == set(E) and nt == set(E), (sorted(nq), sorted(nt))
    assert scene["batches"][0]["desc"].shape == (8, CAP, 128) and len(scene["batches"]) == 2
    assert {len(d) for d, _ in scene["keys"]} == {1, 64, 65, 257, CAP} and len(scene["slots"]) == 4
    for d, _ in scene["keys"] + scene["slots"]:
        np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    seen = {}
    for q, t in all_pairs(scene):
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        if len(qr) == 0 or len(tr) == 0:
            continue
        last, tile = len(tr) - 1, 64 * ((len(tr) - 1) // 64)
        m0 = pair_rule(qr, tr, False)[0]
        mx = pair_rule(qr, tr, True)[0]
        mr = pair_rule(qr, tr, False, 0.0, 0.8)[0]
        assert m0[-1] == last and mx[-1] == last, (q, t)          # the last query row and the last train row, mutually
        flags = seen.setdefault(t, [False, False])
        flags[0] = True
        if len(qr) >= 2:
            assert (m0 == tile).any(), (q, t)
        flags[1] |= bool((m0 == tile).any())
        quarter = 0.25 * min(len(qr), len(tr))
        assert (mx >= 0).sum() >= quarter, (q, t)
        if len(tr) >= 2:
            assert (mr >= 0).sum() >= quarter, (q, t)
    assert all(all(v) for v in seen.values()) and len(seen) == 14 + 5 + 4 - 1        # (the empty frame is no train set)


def _within_the_condition(scene, options_sets):
    """The rule alone keeps the scene inside the exclusions' condition -> the rows left out in all."""
    total = 0
    for q, t in all_pairs(scene):
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        if len(qr) == 0:
            continue
        dd = distances(qr, tr)
        keep = np.array(sorted(scene["protected"][q]), np.int64)
        for opt in options_sets:
            out = exclusions(dd, pair_rule(qr, tr, *opt), *opt)
            assert out.sum() <= 0.01 * len(qr), (scene["name"], q, t, opt, int(out.sum()))
            assert not out[keep].any(), (scene["name"], q, t, opt)
            total += int(out.sum())
        for tol in TOLERANCES:
            _, border = first_rule(tr, qr, tol)
            assert border.sum() <= 0.01 * len(tr), (scene["name"], q, t, tol)
            total += int(border.sum())
    return total


@pytest.mark.parametrize("name,dim", [("edges", 128), ("ties", 128), ("nonfinite", 128), ("edges", 256), ("nonfinite", 256)])
def test_scenes_stay_within_the_exclusions_condition(name, dim):
    scene = scene_of(name, dim)
    if dim == 256:                                                   # the D = 256 context has no bank
        scene = dict(scene, slots=[])
    total = _within_the_condition(scene, TIE_OPTIONS if name == "ties" else OPTIONS)
    print(name, dim, "rows left out over all pairs, option sets and tolerances:", total)


def test_ties_go_to_the_lower_index():
    scene = scene_of("ties")
    checked = 0
    for q, t in all_pairs(scene):
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        dd = distances(qr, tr)
        m0, d1, d2 = pair_rule(qr, tr, False)
        mx = pair_rule(qr, tr, True)[0]
        m99 = pair_rule(qr, tr, False, 0.0, 0.99)[0]
        for a, b in scene["dups"].get(t, ()):                        # train rows a < b bit-equal
            if b >= len(tr):
                continue
            assert (dd[:, a] == dd[:, b]).all()                      # bit-equal rows give bit-equal float64 distances too
            rows = np.flatnonzero(m0 == a)                           # (the copy of that row, where the query set has it)
            assert not (m0 == b).any() and not (mx == b).any(), (q, t, a, b)
            assert (d1[rows] == d2[rows]).all() and (m99[rows] == -1).all()
            checked += len(rows) > 0
        for a, b in scene["dups"].get(q, ()):                        # query rows a < b bit-equal
            if b >= len(qr):
                continue
            assert (dd[a] == dd[b]).all() and m0[a] == m0[b] >= 0 and mx[b] == -1
            checked += mx[a] >= 0                                    # the column's minimum is tied: the lower row keeps it
    assert checked > 60


def test_nonfinite_rows_match_nothing_and_leave_the_others_alone():
    scene, plain = scene_of("nonfinite"), scene_of("edges")
    kinds = set()
    for sid, rows in scene["nonfinite"].items():
        r = rows_of(scene, sid)
        assert all(not np.isfinite(r[i]).all() for i in rows) and np.isfinite(np.delete(r, sorted(rows), axis=0)).all()
        if sid[0] == "frame" and len(r) > 64:
            assert np.isnan(r[[0, 63, 64]]).all()
        kinds |= {(bool(np.isnan(r[i]).all()), bool(np.isnan(r[i]).any()), bool(np.isposinf(r[i]).any()),
                   bool(np.isneginf(r[i]).any())) for i in rows}
    assert kinds == {(True, True, False, False), (False, True, False, False), (False, False, True, False),
                     (False, False, True, True)}
    for q, t in all_pairs(scene):
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        qbad, tbad = sorted(scene["nonfinite"][q]), sorted(scene["nonfinite"][t])
        qkeep = np.setdiff1d(np.arange(len(qr)), qbad)
        tkeep = np.setdiff1d(np.arange(len(tr)), tbad)
        for opt in OPTIONS:
            m, d1, d2 = pair_rule(qr, tr, *opt)
            assert (m[qbad] == -1).all() and np.isinf(d1[qbad]).all() and not np.isin(m, tbad).any()
            # ... and every other row as if the non-finite rows were absent: delete them, match, re-index
            sm, sd1, sd2 = pair_rule(qr[qkeep], tr[tkeep], *opt)
            back = np.where(sm >= 0, tkeep[np.maximum(sm, 0)] if len(tkeep) else -1, -1)
            np.testing.assert_array_equal(m[qkeep], back)
            np.testing.assert_allclose(d1[qkeep], sd1, rtol=0, atol=1e-12)
        for tol in TOLERANCES:
            first, _ = first_rule(tr, qr, tol)                        # key = tr, cur = qr
            assert (first[tbad] == -1).all() and not np.isin(first, qbad).any()
            sub, _ = first_rule(tr[tkeep], qr[qkeep], tol)
            np.testing.assert_array_equal(first[tkeep], np.where(sub >= 0, qkeep[np.maximum(sub, 0)] if len(qkeep) else -1, -1))
    # the all-NaN sets, and the finite rows are those of "edges"
    assert np.isnan(rows_of(scene, ("frame",) + NAN_FRAME)).all() and np.isnan(scene["keys"][NAN_KEY][0]).all()
    assert np.isnan(scene["slots"][NAN_SLOT][0]).all()
    a, b = scene["batches"][1]["desc"], plain["batches"][1]["desc"]
    assert (np.isfinite(a) <= (a == b)).all() and (a != b).any()


def _emulation_cases(name):
    scene = scene_of(name)
    pairs = all_pairs(scene, ("key", "previous"))
    return scene, [(q, t) for q, t in pairs if len(rows_of(scene, q))]


def _fails(scene, pairs, options_sets, bug):
    """The (pair, options) on which the emulation with `bug` fails the comparison."""
    failed = []
    for q, t in pairs:
        qr, tr = rows_of(scene, q), rows_of(scene, t)
        for opt in options_sets:
            m, d = emulate(qr, tr, opt, bug)
            try:
                compare(m, d, reference(scene["name"], scene["dim"], q, t, opt), BAR_D128, "%s %s %s" % (q, t, opt))
            except AssertionError:
                failed.append((q, t, opt))
    return failed


def test_the_comparison_passes_a_correct_matcher():
    for name in ("edges", "ties", "nonfinite"):
        scene, pairs = _emulation_cases(name)
        assert _fails(scene, pairs, OPTIONS[:2] + OPTIONS[4:], None) == []
    # ... and one that evaluates d^2 in plain fp32 (the explicit pair shapes)
    scene = scene_of("nonfinite")
    for nq, nt in EXPLICIT:
        q, t = explicit_pair(scene, nq, nt)
        for opt in OPTIONS:
            m, d = emulate(rows_of(scene, q), rows_of(scene, t), opt, fp32=True)
            compare(m, d, reference("nonfinite", 128, q, t, opt), BAR_D128, "fp32 %s %s %s" % (q, t, opt))


@pytest.mark.parametrize("bug,name", [("nan_to_zero", "nonfinite"), ("drop_last_column", "edges"),
                                      ("drop_last_query_row", "edges"), ("tie_to_higher_index", "ties"),
                                      ("skip_second_round", "edges")])
def test_the_comparison_catches_a_wrong_matcher(bug, name):
    scene, pairs = _emulation_cases(name)
    failed = _fails(scene, pairs, OPTIONS[:2], bug)
    print(bug, "fails", len(failed), "of", 2 * len(pairs), "comparisons on", name)
    assert len(failed) >= 8
    if bug == "drop_last_query_row":                                 # only the cross check reads the column scan
        assert all(opt[0] for _, _, opt in failed)


def test_the_clamp_that_turned_a_nan_into_a_hit():
    """What the library did before include/fpc.h's rule: `d2 > 0 ? d2 : 0` makes a NaN distance 0.  On "nonfinite" a NaN
    query row then reports train row 0 at distance 0, and -- holding every column's minimum -- strips the cross-checked
    matches of valid rows.  The comparison fails on exactly that."""
    scene = scene_of("nonfinite")
    q, t = ("frame", 1, 7), ("key", 4)                               # 384 x 384, NaN rows at 0, 63, 64 of the queries
    qr, tr = rows_of(scene, q), rows_of(scene, t)
    m, d = emulate(qr, tr, (False, 0.0, 0.0), "nan_to_zero")
    assert m[0] == 0 and d[0] == 0 and m[63] == 0 and d[64] == 0
    mx, _ = emulate(qr, tr, (True, 0.0, 0.0), "nan_to_zero")
    rule = pair_rule(qr, tr, True)[0]
    lost = (rule >= 0) & (mx == -1)
    print("cross-checked matches of valid rows lost to the NaN rows:", int(lost.sum()), "of", int((rule >= 0).sum()))
    assert lost.sum() == (rule >= 0).sum() > 300
    for opt in ((False, 0.0, 0.0), (True, 0.0, 0.0)):
        with pytest.raises(AssertionError):
            compare(*emulate(qr, tr, opt, "nan_to_zero"), reference("nonfinite", 128, q, t, opt), BAR_D128)
    # first-within: the NaN row is "within" every tolerance under that clamp; by the rule it is within none
    first, _ = first_rule(tr, qr, 0.3)
    assert not np.isin(first, sorted(scene["nonfinite"][q])).any()


def test_fp32_bar_at_256_components():
    """The D = 256 bar of tests/test_gpu_match_edges.py: twice the largest d^2 error of the plain fp32 evaluation on the
    scene, never more than 8 D 2^-24."""
    for name in ("edges", "nonfinite"):
        scene = scene_of(name, 256)
        worst = fp32_error(scene, [explicit_pair(scene, nq, nt) for nq, nt in EXPLICIT])
        print(name, "D = 256: plain fp32 d^2 error %.3e, analytic %.3e" % (worst, analytic_bar(256)))
        assert 0 < 2 * worst <= analytic_bar(256)
