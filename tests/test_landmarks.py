"""CPU checks of map growth (fpc_landmarks_pairs / fpc_landmarks_frames / fpc_landmarks_bank): the header declares it, the
binding binds it, the built library exports it -- and this file's float64 restatement of the rule of include/fpc.h (carry a
valid landmark over under the PnP pose or drop the row, triangulate the others by the midpoint of the two rays, the parallax
gate, the two ray parameters and the two reprojection tests), which the GPU tests (test_gpu_landmarks.py) hold the kernel to,
does what it is for on planted VGA scenes: points at depths 4 .. 12 seen by two cameras, pixels rounded to integers.

Planted truth, measured with this restatement (SCENES, 900 pairs each, 3 px, 1 degree): the wide baselines (|t| = 3.3 and
1.5) keep all 900 right pairs as kind 2; the short sideways baseline (|t| = 0.20) keeps 675 and the forward one (|t| = 0.59)
keeps 682, every row the parallax gate cuts having a ray angle below 1 degree; no row of any planted batch lies within 1e-9
relative of a threshold (0 `near` rows in every frame; the cap the GPU comparison may leave out is 1 % of a frame's rows).

Chain, restated (chain_scene: key frame B with exact landmarks on about half of its rows, C localised by pnp_rule against them,
C's landmarks by landmarks_rule, D localised by pnp_rule against C's landmarks; D against the planted composition
X_D = R_DB R_CB^T (X_C - t_CB) + t_DB): with every kind, rotation 0.0178 degrees and relative translation 3.070e-04; with
kind 2 only, 0.0224 degrees and 1.051e-03.  The bars of the device's end-to-end test are twice the worst of the two, by
the rule that set test_pnp_ransac.py's ROT_BAR and TRANS_BAR (a different, equally good best sample is allowed):
CHAIN_ROT_BAR and CHAIN_TRANS_BAR."""
import collections
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_pnp_ransac import FRAME_H, FRAME_W, KVEC, _rotation, camera_points, pnp_rule, pose_errors
from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
PARALLEL = 1e-12             # det / ((a.a)(b.b)) floor at min_parallax_deg = 0: the pose calls' (include/fpc.h)
NEAR = 1e-9                  # relative distance to a threshold inside which a row is left out of the device comparison
NEAR_CAP = 0.01              # ... and the share of a frame's rows that may be
DEFAULTS = dict(reproj_threshold=3.0, min_parallax_deg=1.0)
NAMES = ("fpc_default_landmark_params", "fpc_landmarks_pairs", "fpc_landmarks_frames", "fpc_landmarks_bank")
KQVGA = (250.0, 250.0, 160.0, 120.0)
CHAIN_ROT_BAR = 2 * 0.0224       # degrees: twice the worst of the restated chain (module docstring)
CHAIN_TRANS_BAR = 2 * 1.051e-03  # |t - t_planted| / |t_planted|, likewise
CHAIN_PNP = dict(iterations=1024, seed=3, reproj_threshold=3.0, refits=4, min_inliers=12)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
Landmarks = collections.namedtuple("Landmarks", "xyz kind counts near")


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _reprojects(kvec, px, py, a, b, c, thr):
    """The PnP inlier test of the header, float64, without the division -> (passes, near its threshold)."""
    fx, fy, cx, cy = (float(np.float32(v)) for v in kvec)
    ex = fx * a - (px - cx) * c
    ey = fy * b - (py - cy) * c
    e2, lim = ex * ex + ey * ey, thr * thr * (c * c)
    scale = np.abs(np.where(np.isfinite(c), c, 0.0)).max(initial=0.0)
    return (c > 0) & (e2 < lim), (np.abs(e2 - lim) <= NEAR * lim) | (np.abs(c) <= NEAR * scale)


def landmarks_rule(q_xy, t_xy, t_xyz, t_valid, r, t, k_query=KVEC, k_train=KVEC, reproj_threshold=3.0, min_parallax_deg=1.0):
    """include/fpc.h's rule for one frame in float64: q_xy, t_xy [M,2] pixels, t_xyz [M,3] or None, t_valid [M] or None, the
    pose r [3,3], t [3] with X_query = r X_train + t (fp32 values) -> Landmarks(xyz float64 [M,3] holding fp32 values, kind
    uint8 [M], counts (kind 1, kind 2), near bool [M]: a quantity the row was tested on lies within NEAR of its threshold)."""
    q, p = _f32(q_xy).reshape(-1, 2), _f32(t_xy).reshape(-1, 2)
    m = len(q)
    r, t = _f32(r).reshape(3, 3), _f32(t).reshape(3)
    thr = float(np.float32(reproj_threshold))
    deg = float(np.float32(min_parallax_deg))
    par = np.sin(np.deg2rad(deg)) ** 2 if deg > 0 else PARALLEL
    xyz, kind, near = np.zeros((m, 3)), np.zeros(m, np.uint8), np.zeros(m, bool)
    if not r.any() or not np.isfinite(r).all() or not np.isfinite(t).all() or m == 0:
        return Landmarks(xyz, kind, (0, 0), near)
    has = np.zeros(m, bool)
    lm = np.zeros((m, 3))
    if t_xyz is not None:
        lm32 = np.asarray(t_xyz, np.float32).reshape(-1, 3)
        has = np.isfinite(lm32).all(1) & (np.ones(m, bool) if t_valid is None else np.asarray(t_valid).reshape(-1) != 0)
        lm = np.where(has[:, None], lm32.astype(np.float64), 0.0)
    x, y, u, v = q[:, 0], q[:, 1], p[:, 0], p[:, 1]
    qfx, qfy, qcx, qcy = (float(np.float32(k)) for k in k_query)
    tfx, tfy, tcx, tcy = (float(np.float32(k)) for k in k_train)
    with np.errstate(all="ignore"):
        # transfer
        a = r[0, 0] * lm[:, 0] + r[0, 1] * lm[:, 1] + r[0, 2] * lm[:, 2] + t[0]
        b = r[1, 0] * lm[:, 0] + r[1, 1] * lm[:, 1] + r[1, 2] * lm[:, 2] + t[1]
        c = r[2, 0] * lm[:, 0] + r[2, 1] * lm[:, 1] + r[2, 2] * lm[:, 2] + t[2]
        keep1, near1 = _reprojects(k_query, x, y, a, b, c, thr)
        # triangulation: the rays lam a (query) and t + mu b (train), b = R q^
        a0, a1, a2 = (x - qcx) / qfx, (y - qcy) / qfy, np.ones(m)
        q0, q1 = (u - tcx) / tfx, (v - tcy) / tfy
        b0 = r[0, 0] * q0 + r[0, 1] * q1 + r[0, 2]
        b1 = r[1, 0] * q0 + r[1, 1] * q1 + r[1, 2]
        b2 = r[2, 0] * q0 + r[2, 1] * q1 + r[2, 2]
        aa, bb, ab = a0 * a0 + a1 * a1 + a2 * a2, b0 * b0 + b1 * b1 + b2 * b2, a0 * b0 + a1 * b1 + a2 * b2
        at, bt = a0 * t[0] + a1 * t[1] + a2 * t[2], b0 * t[0] + b1 * t[1] + b2 * t[2]
        det = aa * bb - ab * ab
        lam, mu = (at * bb - ab * bt) / det, (ab * at - aa * bt) / det
        x0, x1, x2 = (lam * a0 + t[0] + mu * b0) / 2.0, (lam * a1 + t[1] + mu * b1) / 2.0, (lam * a2 + t[2] + mu * b2) / 2.0
        d0, d1, d2 = x0 - t[0], x1 - t[1], x2 - t[2]
        y0 = r[0, 0] * d0 + r[1, 0] * d1 + r[2, 0] * d2
        y1 = r[0, 1] * d0 + r[1, 1] * d1 + r[2, 1] * d2
        y2 = r[0, 2] * d0 + r[1, 2] * d1 + r[2, 2] * d2
        floor = par * (aa * bb)
        keep_q, near_q = _reprojects(k_query, x, y, x0, x1, x2, thr)
        keep_t, near_t = _reprojects(k_train, u, v, y0, y1, y2, thr)
        keep2 = (det > floor) & (lam > 0) & (mu > 0) & keep_q & keep_t
        fin = np.isfinite(lam) & np.isfinite(mu)
        scale = max(np.abs(lam[~has & fin]).max(initial=0.0), np.abs(mu[~has & fin]).max(initial=0.0))
        near2 = (np.abs(det - floor) <= NEAR * floor) | (np.abs(lam) <= NEAR * scale) | (np.abs(mu) <= NEAR * scale) | \
            near_q | near_t
    kind[has & keep1] = 1
    kind[~has & keep2] = 2
    xyz[kind == 1] = _f32(np.stack([a, b, c], 1))[kind == 1]
    xyz[kind == 2] = _f32(np.stack([x0, x1, x2], 1))[kind == 2]
    near = np.where(has, near1, near2)
    return Landmarks(xyz, kind, (int((kind == 1).sum()), int((kind == 2).sum())), near)


def ray_angle_deg(q_xy, t_xy, r, k_query=KVEC, k_train=KVEC):
    """The angle between the two rays of every pair, by the arc cosine (the rule tests its sine, without a division)."""
    q, p = np.asarray(q_xy, np.float64), np.asarray(t_xy, np.float64)
    a = np.stack([(q[:, 0] - k_query[2]) / k_query[0], (q[:, 1] - k_query[3]) / k_query[1], np.ones(len(q))], 1)
    b = np.stack([(p[:, 0] - k_train[2]) / k_train[0], (p[:, 1] - k_train[3]) / k_train[1], np.ones(len(p))], 1) @ _f32(r).T
    cosang = (a * b).sum(1) / np.sqrt((a * a).sum(1) * (b * b).sum(1))
    return np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))


# ---- planted scenes -------------------------------------------------------------------------------------------------------
# (axis, degrees, t) of X_query = R X_train + t: two wide baselines, a short sideways one and a forward one
SCENES = [([0.2, 1.0, 0.1], 8.0, [3.2, 0.5, 0.6]), ([1.0, -0.4, 0.3], 6.0, [-1.3, 0.6, 0.4]),
          ([0.3, 1.0, -0.2], 3.0, [0.19, 0.06, 0.02]),([0.1, 0.2, 1.0], 2.0, [0.05, -0.03, 0.59])]
WIDE, SHORT = (0, 1), (2, 3)
Scene = collections.namedtuple("Scene", "q_xy t_xy xyz R t")


def _project(xc, kvec):
    return np.round(np.stack([kvec[0] * xc[:, 0] / xc[:, 2] + kvec[2], kvec[1] * xc[:, 1] / xc[:, 2] + kvec[3]], 1))


@functools.lru_cache(maxsize=None)
def planted_scene(i, npts=900, kvec=KVEC, h=FRAME_H, w=FRAME_W):
    """npts points at depths 4 .. 12 in the train camera's frame that both cameras see -> Scene(query pixels, train pixels
    (rounded, float32), the points float32 [npts,3] in the train camera's frame, R and t as fp32 values)."""
    axis, deg, t = SCENES[i]
    rng = np.random.default_rng(100 + i)
    r, t = _f32(_rotation(axis, np.deg2rad(deg))), _f32(t)
    px = np.stack([rng.uniform(8, w - 8, 4 * npts), rng.uniform(8, h - 8, 4 * npts)], 1)
    z = rng.uniform(4.0, 12.0, 4 * npts)
    xt = np.stack([(px[:, 0] - kvec[2]) / kvec[0] * z, (px[:, 1] - kvec[3]) / kvec[1] * z, z], 1).astype(np.float32)
    xq = camera_points(r, t, xt)
    pq, pt = _project(xq, kvec), _project(xt.astype(np.float64), kvec)
    seen = np.flatnonzero((xq[:, 2] > 0.5) & (pq[:, 0] >= 0) & (pq[:, 0] < w) & (pq[:, 1] >= 0) & (pq[:, 1] < h))[:npts]
    assert len(seen) == npts
    return Scene(pq[seen].astype(np.float32), pt[seen].astype(np.float32), xt[seen], r, t)


Frame = collections.namedtuple("Frame", "q_xy t_xy t_xyz t_valid R t npairs right")
STRIDE = 900


def _mixed_frame(i, npairs, seed, r=None, t=None):
    """Scene i as one frame of the explicit call: about half of the rows carry their exact landmark, a tenth of the pairs is
    wrong (a random query pixel), a few landmarks are wrong (they contradict the match), a few are not finite under a set
    flag (no landmark: triangulated) and a few flags are clear over a good point."""
    s = planted_scene(i)
    rng = np.random.default_rng(seed)
    m = len(s.q_xy)
    q_xy, lm = s.q_xy.copy(), s.xyz.copy()
    valid = rng.uniform(size=m) < 0.5
    right = np.ones(m, bool)
    wrong = rng.choice(m, m // 10, replace=False)
    q_xy[wrong] = np.stack([rng.integers(0, FRAME_W, len(wrong)), rng.integers(0, FRAME_H, len(wrong))], 1)
    right[wrong] = False
    moved = rng.choice(m, 30, replace=False)                       # a landmark that is not where the match says
    lm[moved] += rng.uniform(0.5, 1.5, (30, 3)).astype(np.float32)
    right[moved[valid[moved]]] = False
    odd = rng.choice(m, 12, replace=False)
    lm[odd[:4], 0], lm[odd[4:8], 2], lm[odd[8:], 1] = np.nan, np.inf, -np.inf
    return Frame(q_xy, s.t_xy, lm, valid.astype(np.uint8), s.R if r is None else r, s.t if t is None else t, npairs, right)


@functools.lru_cache(maxsize=None)
def explicit_batch():
    """The eight frames of the GPU test's explicit call: pair counts around the 256-lane walk, wide and short baselines, a
    failed (all-zero) pose and a pose with a NaN."""
    zero_r, nan_t = np.zeros((3, 3)), np.array([0.1, np.nan, 0.2])
    return [_mixed_frame(0, 0, 1), _mixed_frame(2, 1, 2), _mixed_frame(1, 255, 3), _mixed_frame(3, 256, 4),
            _mixed_frame(0, 257, 5), _mixed_frame(2, STRIDE, 6), _mixed_frame(1, STRIDE, 7, r=zero_r, t=np.zeros(3)),
            _mixed_frame(3, STRIDE, 8, t=nan_t)]


def rule_of(frame, **params):
    m = frame.npairs
    return landmarks_rule(frame.q_xy[:m], frame.t_xy[:m], frame.t_xyz[:m], frame.t_valid[:m], frame.R, frame.t, **params)


World = collections.namedtuple("World", "key_xy key_xyz key_valid views")
WORLD_N, WORLD_H, WORLD_W = 8, 240, 320


@functools.lru_cache(maxsize=None)
def frames_world(nkey=700, seed=3):
    """A QVGA key frame and WORLD_N views of it for the frames and bank calls (test_gpu_pnp_ransac.py's _world, with the key's
    pixels): key_xy int32 [nkey,2], key_xyz float32 [nkey,3] with three rows that are not finite, key_valid bool [nkey]
    (about half set), and per view (xy int32 [k,2], match int32 [k], R, t as fp32 values).  A fifth of a view's matches is
    wrong, some rows have no match, some a match beyond the key's rows; the baselines alternate between wide and short."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KQVGA
    px = np.stack([rng.uniform(20, WORLD_W - 20, nkey), rng.uniform(20, WORLD_H - 20, nkey)], 1)
    z = rng.uniform(4.0, 12.0, nkey)
    key_xyz = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    key_xy = _project(key_xyz.astype(np.float64), KQVGA).astype(np.int32)
    valid = rng.uniform(size=nkey) < 0.5
    views = []
    for f in range(WORLD_N):
        r = _f32(_rotation(rng.normal(size=3), np.deg2rad(rng.uniform(1.0, 6.0))))
        t = _f32(rng.normal(size=3) * (1.2 if f % 2 == 0 else 0.2))
        xc = camera_points(r, t, key_xyz)
        pix = _project(xc, KQVGA).astype(np.int32)
        seen = np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < WORLD_W) & (pix[:, 1] >= 0) & (pix[:, 1] < WORLD_H))
        rows = rng.permutation(seen)[:600 - 40 * f]
        match = rows.astype(np.int32)
        wrong = rng.choice(len(rows), len(rows) // 5, replace=False)
        match[wrong] = rng.integers(0, nkey, len(wrong))
        match[rng.choice(len(rows), 20, replace=False)] = -1
        match[rng.choice(len(rows), 5, replace=False)] = nkey + 3
        views.append((pix[rows], match, r, t))
    bad = key_xyz.copy()
    bad[5, 1], bad[17, 0], bad[40, 2] = np.nan, np.inf, -np.inf
    valid[[5, 17]] = True
    return World(key_xy, bad, valid, views)


def world_lists(world, nkey, cap, with_landmarks=True, key_valid="world"):
    """The frames call's rows gathered on the host, ascending: the explicit call's inputs (q_xy, t_xy float32 [N,cap,2],
    t_xyz float32 [N,cap,3], t_valid uint8 [N,cap], npairs [N]) and, per view, the query rows the pairs came from: rows i with
    0 <= match < nkey.  key_valid: "world" (the world's flags), None (every row) or an array."""
    n = len(world.views)
    q_xy, t_xy = np.zeros((n, cap, 2), np.float32), np.zeros((n, cap, 2), np.float32)
    t_xyz, t_valid = np.zeros((n, cap, 3), np.float32), np.zeros((n, cap), np.uint8)
    npairs, rows = np.zeros(n, np.int32), []
    valid = world.key_valid if isinstance(key_valid, str) else key_valid
    for f, (pix, match, _, _) in enumerate(world.views):
        i = np.flatnonzero((match >= 0) & (match < nkey))
        j = match[i]
        q_xy[f, :len(i)], t_xy[f, :len(i)] = pix[i], world.key_xy[j]
        if with_landmarks:
            t_xyz[f, :len(i)] = world.key_xyz[j]
            t_valid[f, :len(i)] = 1 if valid is None else valid[j]
        npairs[f] = len(i)
        rows.append(i)
    return q_xy, t_xy, t_xyz, t_valid, npairs, rows


Chain = collections.namedtuple("Chain", "pb pc pd rows_b rows_c rows_d lm_b has_b m_cb m_dc r_cb t_cb r_dc t_dc wrong_c")


@functools.lru_cache(maxsize=None)
def chain_scene(npts=900, seed=33):
    """One 3-D scene in key frame B's camera frame seen by B, C and D at VGA: the rows of each frame (a permutation of the
    points it sees), B's exact landmarks on about half of its rows, the match tables C -> B and D -> C (by row, -1: none, a
    tenth of them wrong), the planted poses X_C = R_CB X_B + t_CB and X_D = R_DC X_C + t_DC (the composition)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = KVEC
    px = np.stack([rng.uniform(60, FRAME_W - 60, npts), rng.uniform(60, FRAME_H - 60, npts)], 1)
    z = rng.uniform(4.0, 12.0, npts)
    xb = np.stack([(px[:, 0] - cx) / fx * z, (px[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    r_cb, t_cb = _rotation([1.0, -0.4, 0.3], np.deg2rad(6.0)), np.array([-1.3, 0.6, 0.4])
    r_db, t_db = _rotation([0.2, 1.0, 0.1], np.deg2rad(9.0)), np.array([1.2, -0.4, 0.5])
    r_dc = r_db @ r_cb.T
    t_dc = t_db - r_dc @ t_cb

    def project(r, t):
        pix = _project(camera_points(r, t, xb), KVEC).astype(np.int32)
        return pix, (pix[:, 0] >= 0) & (pix[:, 0] < FRAME_W) & (pix[:, 1] >= 0) & (pix[:, 1] < FRAME_H)
    pb, _ = project(np.eye(3), np.zeros(3))
    pc, in_c = project(r_cb, t_cb)
    pd, in_d = project(r_db, t_db)
    rows_b = rng.permutation(npts)[:800]
    rows_c = rng.permutation(np.flatnonzero(in_c))[:700]
    rows_d = rng.permutation(np.flatnonzero(in_d))[:600]
    where_b, where_c = np.full(npts, -1, np.int32), np.full(npts, -1, np.int32)
    where_b[rows_b] = np.arange(len(rows_b))
    where_c[rows_c] = np.arange(len(rows_c))
    has_b = rng.uniform(size=len(rows_b)) < 0.5
    m_cb, m_dc = where_b[rows_c].copy(), where_c[rows_d].copy()
    wrong_c = rng.choice(len(rows_c), 70, replace=False)
    m_cb[wrong_c] = rng.integers(0, len(rows_b), 70)
    wrong_d = rng.choice(len(rows_d), 60, replace=False)
    m_dc[wrong_d] = rng.integers(0, len(rows_c), 60)
    return Chain(pb[rows_b], pc[rows_c], pd[rows_d], rows_b, rows_c, rows_d, xb[rows_b], has_b, m_cb, m_dc, r_cb, t_cb,
                 r_dc, t_dc, wrong_c)


def restated_chain(kinds):
    """B's landmarks -> C's pose (pnp_rule) -> C's landmarks (landmarks_rule, the rows whose kind is in `kinds` kept) -> D's
    pose (pnp_rule) -> (rotation error in degrees, relative translation error) of D against the planted composition, and
    C's Landmarks."""
    ch = chain_scene()
    j = ch.m_cb
    use = (j >= 0) & ch.has_b[np.maximum(j, 0)]
    c_pose = pnp_rule(ch.pc[use], ch.lm_b[j[use]], CHAIN_PNP, 0)
    assert not c_pose.failed
    pair = np.flatnonzero(j >= 0)
    got = landmarks_rule(ch.pc[pair], ch.pb[j[pair]], ch.lm_b[j[pair]], ch.has_b[j[pair]], c_pose.R, c_pose.t)
    xyz_c, kind_c = np.zeros((len(ch.pc), 3), np.float32), np.zeros(len(ch.pc), np.uint8)
    xyz_c[pair], kind_c[pair] = got.xyz, got.kind
    keep = np.isin(kind_c, kinds)
    i = ch.m_dc
    use = (i >= 0) & keep[np.maximum(i, 0)]
    d_pose = pnp_rule(ch.pd[use], xyz_c[i[use]], CHAIN_PNP, 0)
    assert not d_pose.failed
    return pose_errors(d_pose.R, d_pose.t, (None, None, None, ch.r_dc, ch.t_dc)), got, c_pose


# ---- the boundary -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fpc.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"typedef struct fpc_landmark_params \{[^}]*float q_fx, q_fy, q_cx, q_cy;[^}]*float t_fx, t_fy, t_cx, t_cy;"
                     r"[^}]*float reproj_threshold;[^}]*float min_parallax_deg;[^}]*\} fpc_landmark_params;", hdr)
    assert [n for n, _ in _lib.FpcLandmarkParams._fields_] == ["q_fx", "q_fy", "q_cx", "q_cy", "t_fx", "t_fy", "t_cx", "t_cy",
                                                               "reproj_threshold", "min_parallax_deg"]
    assert ctypes.sizeof(_lib.FpcLandmarkParams) == 40
    assert re.search(r"#define FPC_ABI_VERSION 4\b", hdr) and lib.fpc_abi_version() == 4 == _lib.ABI_VERSION


def test_default_params():
    lib = _lib.load()
    p = _lib.FpcLandmarkParams()
    assert lib.fpc_default_landmark_params(ctypes.byref(p)) == 0
    assert (p.q_fx, p.q_fy, p.q_cx, p.q_cy) == KVEC and (p.t_fx, p.t_fy, p.t_cx, p.t_cy) == KVEC
    assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS
    assert lib.fpc_default_landmark_params(None) == FPC_E_INVALID


def test_null_context_is_refused():
    lib = _lib.load()
    p = _lib.FpcLandmarkParams()
    lib.fpc_default_landmark_params(ctypes.byref(p))
    buf = (ctypes.c_float * 64)()
    b = ctypes.addressof(buf)
    pp = ctypes.byref(p)
    assert lib.fpc_landmarks_pairs(None, 1, b, b, b, b, b, 1, b, b, pp, b, b, b) == FPC_E_INVALID
    assert lib.fpc_landmarks_frames(None, 1, b, b, b, b, b, b, b, pp, b, b, b) == FPC_E_INVALID
    assert lib.fpc_landmarks_bank(None, 1, b, b, b, b, pp, b, b, b) == FPC_E_INVALID


def test_landmarks_kernels_keep_their_registers(code_object):  # noqa: F811
    """The three instances of landmarks_kernel in the built code object: nothing in scratch, no spills, the block sum's 64
    bytes of LDS and plain stores only."""
    funcs, meta = code_object
    names = sorted(n for n in meta if "landmarks_kernel" in n)
    assert len(names) == 3 and all(tag in " ".join(names) for tag in ("LmExplicit", "LmKey", "LmBank")), names
    for name in names:
        m = meta[name]
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["vgpr_count"] <= 128 and m["agpr_count"] == 0 and m["group_segment_fixed_size"] == 64, m
        assert not any(i.startswith("scratch_") or "atomic" in i for _, i in funcs[name]), name


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_near_rows_stay_under_the_cap_on_every_planted_batch():
    """What the GPU comparison may leave out: at most 1 % of a frame's rows, on every batch test_gpu_landmarks.py uses."""
    worst = 0
    for i in range(len(SCENES)):
        s = planted_scene(i)
        got = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t)
        assert got.near.sum() <= NEAR_CAP * len(s.q_xy), (i, got.near.sum())
        worst = max(worst, got.near.sum())
    for f, frame in enumerate(explicit_batch()):
        got = rule_of(frame)
        assert got.near.sum() <= NEAR_CAP * max(frame.npairs, 1), (f, got.near.sum())
        worst = max(worst, got.near.sum())
    world = frames_world()
    for lists in (world_lists(world, len(world.key_xy), 1024), world_lists(world, 300, 1024),
                  world_lists(world, len(world.key_xy), 1024, key_valid=None),
                  world_lists(world, len(world.key_xy), 1024, with_landmarks=False)):
        q_xy, t_xy, t_xyz, t_valid, npairs, _ = lists
        for f, (_, _, r, t) in enumerate(world.views):
            k = npairs[f]
            got = landmarks_rule(q_xy[f, :k], t_xy[f, :k], t_xyz[f, :k], t_valid[f, :k], r, t, KQVGA, KQVGA)
            assert got.near.sum() <= NEAR_CAP * k, (f, got.near.sum())
            worst = max(worst, got.near.sum())
    (_, got, _) = restated_chain((1, 2))
    assert got.near.sum() <= NEAR_CAP * len(got.near)
    print("near rows: at most %d in any frame" % max(worst, got.near.sum()))


def test_wide_baselines_keep_every_right_pair():
    for i in WIDE:
        s = planted_scene(i)
        assert np.linalg.norm(s.t) >= 1.2
        got = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t)
        assert (got.kind == 2).all() and got.counts == (0, len(s.q_xy)), (i, got.counts)
        want = camera_points(s.R, s.t, s.xyz)                        # the planted points in the query camera's frame
        rel = np.linalg.norm(got.xyz - want, axis=1) / np.linalg.norm(want, axis=1)
        print("scene %d |t| %.2f: %d of %d kept, worst point error %.3e relative" % (i, np.linalg.norm(s.t), got.counts[1],
                                                                                      len(s.q_xy), rel.max()))
        assert np.median(rel) < 0.02                                 # rounded pixels: a depth error of half a pixel's parallax


def test_short_baselines_are_cut_by_the_parallax_gate():
    for i in SHORT:
        s = planted_scene(i)
        assert 0.2 <= np.linalg.norm(s.t) <= 0.6
        got = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t)
        ang = ray_angle_deg(s.q_xy, s.t_xy, s.R)
        clear = np.abs(ang - 1.0) > 1e-6
        np.testing.assert_array_equal((got.kind == 2)[clear], (ang > 1.0)[clear])     # the gate is all that cuts a right pair
        assert 0.2 * len(ang) < got.counts[1] < 0.95 * len(ang) and got.counts[0] == 0, (i, got.counts)
        free = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t, min_parallax_deg=0.0)
        assert free.counts[1] >= 0.97 * len(ang) and (free.kind >= got.kind).all()    # at 0 degrees only the floor is left
        print("scene %d |t| %.2f: %d of %d kept at 1 degree, %d at 0" % (i, np.linalg.norm(s.t), got.counts[1], len(ang),
                                                                         free.counts[1]))


def test_wrong_matches_and_points_behind_a_camera_get_kind_0():
    for f, frame in enumerate(explicit_batch()[:6]):
        full = frame._replace(npairs=STRIDE)
        got = rule_of(full)
        has = (full.t_valid != 0) & np.isfinite(full.t_xyz).all(1)
        wrong = ~full.right
        assert np.count_nonzero(got.kind[wrong]) <= 0.05 * wrong.sum(), (f, got.kind[wrong], wrong.sum())   # only by chance
        assert set(np.unique(got.kind[has])) <= {0, 1} and set(np.unique(got.kind[~has])) <= {0, 2}
        assert (got.kind[has & full.right] == 1).all()               # an exact landmark under the planted pose always passes
        assert not got.xyz[got.kind == 0].any()
        assert got.counts == ((got.kind == 1).sum(), (got.kind == 2).sum())
    s = planted_scene(0)
    # the mirror image of a landmark, behind the query camera at the same pixel: dropped, and not triangulated
    behind = ((-camera_points(s.R, s.t, s.xyz) - s.t) @ s.R).astype(np.float32)
    got = landmarks_rule(s.q_xy, s.t_xy, behind, None, s.R, s.t)
    assert not got.kind.any() and not got.xyz.any()
    # rays that meet behind the cameras: the two views' pixels swapped under the same pose
    got = landmarks_rule(s.t_xy, s.q_xy, None, None, s.R, s.t)
    assert not got.kind.any()
    # a valid landmark that fails the transfer test is not triangulated, although its two rays would pass
    off = s.xyz + np.float32(1.0)
    moved = landmarks_rule(s.q_xy, s.t_xy, off, None, s.R, s.t)
    assert not moved.kind.any()
    assert (landmarks_rule(s.q_xy, s.t_xy, off, np.zeros(len(off), np.uint8), s.R, s.t).kind == 2).all()


def test_failed_poses_give_nothing():
    s = planted_scene(1)
    nan_r = s.R.copy()
    nan_r[1, 1] = np.nan
    for r, t in ((np.zeros((3, 3)), np.zeros(3)), (np.zeros((3, 3)), s.t), (nan_r, s.t), (s.R, np.array([0.0, np.inf, 0.0]))):
        got = landmarks_rule(s.q_xy, s.t_xy, s.xyz, None, r, t)
        assert not got.kind.any() and not got.xyz.any() and got.counts == (0, 0) and not got.near.any()


def test_restated_chain_grows_the_map_at_one_scale():
    worst = np.zeros(2)
    for kinds in ((1, 2), (2,)):
        (rot, tr), got, c_pose = restated_chain(kinds)
        print("chain, kinds %s: C has %d carried over and %d triangulated rows (%d inliers); D: rotation %.4f deg, "
              "translation %.3e relative" % (kinds, *got.counts, c_pose.ninliers, rot, tr))
        assert got.counts[0] > 200 and got.counts[1] > 200
        worst = np.maximum(worst, (rot, tr))
    print("chain: worst rotation %.4f deg, worst relative translation %.3e; bars %.4f deg, %.3e"
          % (*worst, CHAIN_ROT_BAR, CHAIN_TRANS_BAR))
    # the docstring's figures, to the digits it gives: the bars are twice these and nothing else
    assert abs(worst[0] - CHAIN_ROT_BAR / 2) < 5e-5 and abs(worst[1] - CHAIN_TRANS_BAR / 2) < 5e-7, worst


@pytest.mark.parametrize("deg", [0.0, 1.0, 1.5])
def test_parallax_gate_is_monotone(deg):
    s = planted_scene(2)
    a = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t, min_parallax_deg=deg)
    b = landmarks_rule(s.q_xy, s.t_xy, None, None, s.R, s.t, min_parallax_deg=deg + 1.0)
    assert (b.kind <= a.kind).all() and b.counts[1] < a.counts[1]
