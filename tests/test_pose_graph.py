"""CPU checks of the pose graph (fpc_graph_reserve / _set_nodes / _clear / _get / _add_edges / _optimise / _apply_scale): the
header declares it, the binding binds it, the built library exports it -- and this file's float64 restatement of the rule of
include/fpc.h (`Graph`: the storage, the append rules and FPC_GRAPH_INIT_TO, apply_scale; `graph_rule`: the problem, E =
M o S_a o S_b^-1 and its seven-number residual, the first-order Jacobians, Marquardt's damping, block-Jacobi preconditioned
conjugate gradients with the fixed dot-product tree, the step rounded to fp32, accept / reject), which the GPU tests
(test_gpu_pose_graph.py) hold the kernels to, never raises the cost, removes the drift of planted rings and recovers the
truth of a consistent graph.

Measured on the restatement (ring_scene: N poses on a circle of radius 5, odometry with a scale drift of 1 + 0.3 / N per
edge, 2 mrad and 0.01 of noise, one exact loop edge, exact chords, the start composed from the odometry; defaults, 16
attempts of at most 256 CG iterations): see the constants below, each written beside its measured value."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_static_isa import code_object  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
NAMES = ("fpc_default_graph_params", "fpc_graph_reserve", "fpc_graph_get", "fpc_graph_clear", "fpc_graph_set_nodes",
         "fpc_graph_add_edges", "fpc_graph_optimise", "fpc_graph_apply_scale")
SINGULAR, STOP, LAMBDA_MIN, LAMBDA_MAX = 1e-14, 1e-6, 1e-10, 1e6         # include/fpc.h
MAX_NODES, MAX_EDGES, CHUNK = 1024, 16384, 64
DEFAULTS = dict(iterations=16, lambda0=1e-3, cg_iterations=256, cg_tol=1e-8, trans_unit=1.0)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


# ---- Sim(3) in float64 --------------------------------------------------------------------------------------------------------
def skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def exp_so3(w):
    """E(omega) of the PnP refit, rows of w [n,3] -> [n,3,3]."""
    w = np.asarray(w, np.float64)
    th2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    small = th2 < 1e-16
    th = np.sqrt(np.where(small, 1.0, th2))
    a = np.where(small, 1.0, np.sin(th) / th)
    b = np.where(small, 0.5, (1.0 - np.cos(th)) / np.where(small, 1.0, th2))
    k = skew(w)
    outer = w[:, :, None] * w[:, None, :]
    return np.eye(3)[None] + a[:, None, None] * k + b[:, None, None] * (outer - th2[:, None, None] * np.eye(3)[None])


def log_so3(r):
    v = 0.5 * np.stack([r[:, 2, 1] - r[:, 1, 2], r[:, 0, 2] - r[:, 2, 0], r[:, 1, 0] - r[:, 0, 1]], 1)
    sn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    cs = 0.5 * (r[:, 0, 0] + r[:, 1, 1] + r[:, 2, 2] - 1.0)
    small = sn < 1e-12
    f = np.where(small, 1.0, np.arctan2(sn, cs) / np.where(small, 1.0, sn))
    return f[:, None] * v


def compose(m, a):
    """M o A for similarity tuples (s, R [3,3], t [3])."""
    return m[0] * a[0], m[1] @ a[1], m[0] * (m[1] @ a[2]) + m[2]


def inverse(a):
    return 1.0 / a[0], a[1].T, -(a[1].T @ a[2]) / a[0]


def perturb(a, d):
    """D(delta) o A."""
    e, es = exp_so3(np.asarray(d[:3])[None])[0], np.exp(d[6])
    return es * a[0], e @ a[1], es * (e @ a[2]) + np.asarray(d[3:6])


def ordered_sum(terms, descending=False):
    terms = np.asarray(terms, np.float64)
    if len(terms) == 0:
        return np.zeros(terms.shape[1:])
    return np.cumsum(terms[::-1] if descending else terms, axis=0)[-1]


def chunked_sum(per, descending=False):
    """The cost's order: the edges of a chunk of 64 one after the other, then the chunks' sums one after the other."""
    pad = (-len(per)) % CHUNK
    rows = np.concatenate([per, np.zeros(pad)]).reshape(-1, CHUNK)
    parts = np.cumsum(rows[:, ::-1] if descending else rows, axis=1)[:, -1] if len(rows) else np.zeros(0)
    return float(ordered_sum(parts, descending))


def tree_dot(a, b):
    """sum over nodes of a_i . b_i: seven products in order onto 0 per node, then the fixed tree over 1024 leaves."""
    leaf = np.zeros(MAX_NODES)
    part = np.zeros(len(a))
    for k in range(7):
        part = part + a[:, k] * b[:, k]
    leaf[:len(a)] = part
    h = MAX_NODES // 2
    while h:
        leaf[:h] = leaf[:h] + leaf[h:2 * h]
        h //= 2
    return float(leaf[0])


# ---- the storage, restated ------------------------------------------------------------------------------------------------------
class Graph:
    """Nodes and edges as the reservation holds them (fp32), with the append rules and apply_scale."""

    def __init__(self, nodes, edges):
        self.nodes, self.edges = nodes, edges
        self.clear()

    def clear(self):
        n, e = self.nodes, self.edges
        self.s, self.R, self.t = np.zeros(n, np.float32), np.zeros((n, 3, 3), np.float32), np.zeros((n, 3), np.float32)
        self.efrom, self.eto = np.zeros(e, np.int32), np.zeros(e, np.int32)
        self.es, self.eR, self.et = np.zeros(e, np.float32), np.zeros((e, 3, 3), np.float32), np.zeros((e, 3), np.float32)
        self.ew = np.zeros(e, np.float32)
        self.count, self.dropped = 0, 0

    def copy(self):
        g = Graph(self.nodes, self.edges)
        for k, v in self.__dict__.items():
            setattr(g, k, v.copy() if isinstance(v, np.ndarray) else v)
        return g

    def set_nodes(self, first, R, t, s=None):
        n = len(R)
        self.s[first:first + n] = 1.0 if s is None else f32(s)
        self.R[first:first + n], self.t[first:first + n] = f32(R), f32(t)

    def is_set(self):
        with np.errstate(invalid="ignore"):
            return self.s > 0

    def add_edges(self, frm, to, R, t, s=None, ninliers=None, min_inliers=0, init_to=False):
        R, t = f32(R).reshape(-1, 3, 3), f32(t).reshape(-1, 3)
        first = self.count
        for f in range(len(R)):
            sv = np.float32(1.0) if s is None else np.float32(s[f])
            a, b = int(frm[f]), int(to[f])
            ok = 0 <= a < self.nodes and 0 <= b < self.nodes and a != b
            with np.errstate(invalid="ignore"):
                ok = ok and np.isfinite(sv) and sv > 0 and np.isfinite(R[f]).all() and np.isfinite(t[f]).all() and R[f].any()
            if ninliers is not None:
                ok = ok and int(ninliers[f]) >= min_inliers
            if not ok:
                continue
            if self.count >= self.edges:
                self.dropped += 1
                continue
            k = self.count
            self.efrom[k], self.eto[k], self.es[k], self.eR[k], self.et[k] = a, b, sv, R[f], t[f]
            self.ew[k] = 1.0 if ninliers is None else np.float32(int(ninliers[f]))
            self.count += 1
        if init_to:
            for k in range(first, self.count):
                a, b = self.efrom[k], self.eto[k]
                if not self.s[a] > 0 or self.s[b] > 0:
                    continue
                with np.errstate(all="ignore"):
                    sm, rm, tm = np.float64(self.es[k]), self.eR[k].astype(np.float64), self.et[k].astype(np.float64)
                    ra, ta = self.R[a].astype(np.float64), self.t[a].astype(np.float64)
                    # (the three products of an entry added in order, no fused multiply-add: the kernel's bits)
                    rn = (rm[:, 0, None] * ra[None, 0] + rm[:, 1, None] * ra[None, 1]) + rm[:, 2, None] * ra[None, 2]
                    tn = sm * ((rm[:, 0] * ta[0] + rm[:, 1] * ta[1]) + rm[:, 2] * ta[2]) + tm
                    sn, rn, tn = f32(sm * np.float64(self.s[a])), f32(rn), f32(tn)
                if np.isfinite(sn) and sn > 0 and np.isfinite(rn).all() and np.isfinite(tn).all():
                    self.s[b], self.R[b], self.t[b] = sn, rn, tn

    def apply_scale(self, lm, counts):
        """lm float32 [slots,rows,4] and the slots' counts, changed in place with the nodes and the edges."""
        sig = np.where(self.is_set(), self.s, np.float32(1.0)).astype(np.float64)
        k = self.count
        a, b = self.efrom[:k], self.eto[:k]
        self.es[:k] = f32(self.es[:k].astype(np.float64) * sig[a] / sig[b])
        self.et[:k] = f32(self.et[:k].astype(np.float64) / sig[b][:, None])
        for i in np.nonzero(self.is_set() & (self.s != 1))[0]:
            inv = 1.0 / np.float64(self.s[i])
            rows = np.arange(lm.shape[1]) < min(max(int(counts[i]), 0), lm.shape[1])
            rows &= lm[i, :, 3] != 0
            lm[i, rows, :3] = f32(lm[i, rows, :3].astype(np.float64) * inv)
            self.t[i] = f32(self.t[i].astype(np.float64) * inv)
            self.s[i] = 1.0

    def centres(self):
        """The camera centres -R^T t / s of the set nodes (NaN rows for the others)."""
        out = np.full((self.nodes, 3), np.nan)
        m = self.is_set()
        out[m] = -np.einsum("nji,nj->ni", self.R[m].astype(np.float64), self.t[m].astype(np.float64)) / self.s[m, None]
        return out


# ---- the optimiser, restated ----------------------------------------------------------------------------------------------------
def edge_frames(g, s, R, t, act):
    """E = M o S_a o S_b^-1 of the active edges from a state -> s_E [m], R_E [m,3,3], t_E [m,3]."""
    a, b = g.efrom[:g.count][act], g.eto[:g.count][act]
    ms, mr, mt = g.es[:g.count][act].astype(np.float64), g.eR[:g.count][act].astype(np.float64), g.et[:g.count][act].astype(np.float64)
    q = np.einsum("mij,mkj->mik", R[a], R[b])
    k = s[a] / s[b]
    u = t[a] - k[:, None] * np.einsum("mij,mj->mi", q, t[b])
    return ms * k, np.einsum("mij,mjk->mik", mr, q), ms[:, None] * np.einsum("mij,mj->mi", mr, u) + mt


def residuals(g, s, R, t, act, iu):
    se, re_, te = edge_frames(g, s, R, t, act)
    return np.concatenate([log_so3(re_), te * iu, np.log(se)[:, None]], 1), se, re_, te


def graph_cost(g, s, R, t, act, iu, descending=False):
    with np.errstate(all="ignore"):
        e = residuals(g, s, R, t, act, iu)[0]
        q = np.zeros(len(e))
        for k in range(7):
            q = q + e[:, k] * e[:, k]
        per = np.zeros(g.count)
        per[act] = g.ew[:g.count][act].astype(np.float64) * q
        return chunked_sum(per, descending)


def invert_blocks(blocks):
    """Gauss-Jordan with partial pivoting on the 7 x 14 tableaus [m,7,14] -> inverses [m,7,7], good [m]."""
    m = len(blocks)
    tab = np.concatenate([blocks, np.broadcast_to(np.eye(7), (m, 7, 7))], 2).copy()
    tiny = SINGULAR * np.abs(np.einsum("mii->mi", blocks)).max(1) if m else np.zeros(0)
    good = np.ones(m, bool)
    rows = np.arange(m)
    with np.errstate(all="ignore"):
        for c in range(7):
            pr = c + np.argmax(np.abs(tab[:, c:, c]), axis=1)                   # the first largest
            good &= np.abs(tab[rows, pr, c]) > tiny
            top, piv = tab[rows, c].copy(), tab[rows, pr].copy()
            tab[rows, pr], tab[rows, c] = top, piv
            tab[:, c] = tab[:, c] * (1.0 / tab[:, c, c])[:, None]
            for r in range(7):
                if r != c:
                    tab[:, r] = tab[:, r] - tab[:, r, c][:, None] * tab[:, c]
    return tab[:, :, 7:], good


class Result:
    def __init__(self):
        self.stats, self.failed = np.zeros(4), True
        self.costs, self.path, self.lambdas, self.cg = [], [], [], []


def graph_rule(g, fixed, iterations=16, lambda0=1e-3, cg_iterations=256, cg_tol=1e-8, trans_unit=1.0, descending=False):
    """include/fpc.h's optimiser in float64 on the Graph `g`, whose nodes change in place.  descending: every sum over edges
    runs the other way (the fallback margin of the device comparison)."""
    out = Result()
    n = g.nodes
    isset = g.is_set()
    if not (0 <= fixed < n) or not isset[fixed]:
        return out
    out.failed = False
    lam = float(np.float32(lambda0))
    tol2 = float(np.float32(cg_tol)) ** 2
    iu = 1.0 / float(np.float32(trans_unit))
    ea, eb = g.efrom[:g.count], g.eto[:g.count]
    act = isset[ea] & isset[eb]
    a, b = ea[act], eb[act]
    m = len(a)
    w = g.ew[:g.count][act].astype(np.float64)
    deg = np.bincount(np.concatenate([a, b]), minlength=n)
    member = (deg > 0) & isset
    member[fixed] = False
    # node i's contributions in ascending edge order: index 2 e (the `from` side) or 2 e + 1 (the `to` side); 2 m is a +0 row
    lists = [[] for _ in range(n)]
    for e in range(m):
        lists[a[e]].append(2 * e)
        lists[b[e]].append(2 * e + 1)
    width = max([len(v) for v in lists] + [1])
    table = np.full((n, width), 2 * m)
    for i, v in enumerate(lists):
        v = v[::-1] if descending else v
        table[i, :len(v)] = v

    def gather(ca, cb):
        both = np.zeros((2 * m + 1,) + ca.shape[1:])
        both[0:2 * m:2], both[1:2 * m:2] = ca, cb
        acc = np.zeros((n,) + ca.shape[1:])
        for d in range(width):
            acc = acc + both[table[:, d]]
        return acc

    s, R, t = g.s.astype(np.float64), g.R.astype(np.float64), g.t.astype(np.float64)
    cost = graph_cost(g, s, R, t, act, iu, descending)
    out.costs.append(cost)
    c0 = cost
    made = accepted = 0
    while made < iterations:
        with np.errstate(all="ignore"):
            e, se, re_, te = residuals(g, s, R, t, act, iu)
            ms, mr = g.es[:g.count][act].astype(np.float64), g.eR[:g.count][act].astype(np.float64)
            d = g.et[:g.count][act].astype(np.float64) - te
            ja, jb = np.zeros((m, 7, 7)), np.zeros((m, 7, 7))
            ja[:, 0:3, 0:3] = mr
            ja[:, 3:6, 0:3] = np.einsum("mij,mjk->mik", skew(d), mr) * iu
            ja[:, 3:6, 3:6] = ms[:, None, None] * mr * iu
            ja[:, 3:6, 6] = -d * iu
            ja[:, 6, 6] = 1.0
            jb[:, 0:3, 0:3] = -re_
            jb[:, 3:6, 3:6] = -(se[:, None, None] * re_) * iu
            jb[:, 6, 6] = -1.0
            grad = gather(w[:, None] * np.einsum("mrj,mr->mj", ja, e), w[:, None] * np.einsum("mrj,mr->mj", jb, e))
            hd = gather(w[:, None, None] * np.einsum("mrj,mrk->mjk", ja, ja), w[:, None, None] * np.einsum("mrj,mrk->mjk", jb, jb))
            dh = np.einsum("nii->ni", hd).copy()
            damped = hd + lam * np.einsum("ni,ij->nij", dh, np.eye(7))
            minv = np.zeros((n, 7, 7))
            minv[member], good = invert_blocks(damped[member])
            ok = bool(good.all())
            x = np.zeros((n, 7))
            its = 0
            if ok:
                mem = member[:, None]

                def precond(r):
                    z = np.zeros((n, 7))
                    for j in range(7):
                        z = z + minv[:, :, j] * r[:, j][:, None]
                    return np.where(mem, z, 0.0)

                def product(p):
                    q = w[:, None] * (np.einsum("mij,mj->mi", ja, p[a]) + np.einsum("mij,mj->mi", jb, p[b]))
                    ap = gather(np.einsum("mrj,mr->mj", ja, q), np.einsum("mrj,mr->mj", jb, q)) + lam * dh * p
                    return np.where(mem, ap, 0.0)

                r = np.where(mem, -grad, 0.0)
                z = precond(r)
                p = z.copy()
                rz = rz0 = tree_dot(r, z)
                if rz0 > 0:
                    for its in range(1, cg_iterations + 1):
                        ap = product(p)
                        pq = tree_dot(p, ap)
                        if not pq > 0:
                            break
                        alpha = rz / pq
                        x = x + alpha * p
                        r = r - alpha * ap
                        z = precond(r)
                        rzn = tree_dot(r, z)
                        if rzn <= tol2 * rz0:
                            break
                        p = z + (rzn / rz) * p
                        rz = rzn
            out.cg.append(its)
            new = np.inf
            if ok:
                ex, es = exp_so3(x[:, :3]), np.exp(x[:, 6])
                s1 = np.where(member, f32(es * s), g.s)
                r1 = np.where(member[:, None, None], f32(np.einsum("nij,njk->nik", ex, R)), g.R)
                t1 = np.where(member[:, None], f32(es[:, None] * np.einsum("nij,nj->ni", ex, t) + x[:, 3:6]), g.t)
                ok = bool(np.isfinite(s1).all() and (s1[member] > 0).all() and np.isfinite(r1).all() and np.isfinite(t1).all())
                if ok:
                    new = graph_cost(g, s1.astype(np.float64), r1.astype(np.float64), t1.astype(np.float64), act, iu, descending)
        made += 1
        out.lambdas.append(lam)
        if ok and new < cost:
            gain, before = cost - new, cost
            g.s, g.R, g.t = s1.astype(np.float32), r1.astype(np.float32), t1.astype(np.float32)
            s, R, t = g.s.astype(np.float64), g.R.astype(np.float64), g.t.astype(np.float64)
            cost = new
            accepted += 1
            lam = max(lam / 10.0, LAMBDA_MIN)
            out.path.append(1)
            out.costs.append(cost)
            if gain <= STOP * before:
                break
        else:
            lam = min(10.0 * lam, LAMBDA_MAX)
            out.path.append(0)
    out.stats = np.array([c0, cost, made, accepted], np.float64)
    return out


# ---- planted scenes -----------------------------------------------------------------------------------------------------------
class Scene:
    pass


def _truth(n, rng, radius=5.0):
    ang = 2 * np.pi * np.arange(n) / n
    cen = np.stack([radius * np.cos(ang), radius * np.sin(ang), 0.1 * rng.standard_normal(n)], 1)
    rot = exp_so3(np.stack([0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(n), ang], 1))
    return [(1.0, rot[i], -rot[i] @ cen[i]) for i in range(n)], cen


def _between(truth, a, b):
    """The exact measurement X_b = M X_a."""
    return compose(truth[b], inverse(truth[a]))


def _fill(sc, edges_cap, edges, start):
    g = Graph(sc.n, edges_cap)
    sc.frm = np.array([e[0] for e in edges], np.int32)
    sc.to = np.array([e[1] for e in edges], np.int32)
    sc.es = f32([e[2][0] for e in edges])
    sc.eR = f32([e[2][1] for e in edges])
    sc.et = f32([e[2][2] for e in edges])
    g.set_nodes(0, [p[1] for p in start], [p[2] for p in start], [p[0] for p in start])
    g.add_edges(sc.frm, sc.to, sc.eR, sc.et, sc.es)
    sc.graph = g
    return sc


def ring_scene(n, drift=True, chords=0, seed=0, edges_cap=None):
    """N poses on a circle.  Odometry edges i -> i + 1 carry a scale drift of 1 + 0.3 / N per edge (drift), 2 mrad of
    rotation noise and 0.01 of translation noise; one exact loop edge N - 1 -> 0 and `chords` exact chords.  Nodes start
    from composing the odometry (node 0 at the truth, the gauge)."""
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.n = n
    sc.truth, sc.centres = _truth(n, rng)
    edges, start = [], [sc.truth[0]]
    for i in range(n - 1):
        m = _between(sc.truth, i, i + 1)
        noise = np.concatenate([2e-3 * rng.standard_normal(3), 0.01 * rng.standard_normal(3), [np.log(1 + 0.3 / n) if drift else 0.0]])
        m = perturb(m, noise)
        m = (float(np.float32(m[0])), f32(m[1]).astype(np.float64), f32(m[2]).astype(np.float64))
        edges.append((i, i + 1, m))
        start.append(compose(m, start[-1]))
    if n > 2:
        edges.append((n - 1, 0, _between(sc.truth, n - 1, 0)))
    for _ in range(chords):
        i = int(rng.integers(0, n))
        j = int((i + rng.integers(2, n - 1)) % n)
        edges.append((i, j, _between(sc.truth, i, j)))
    return _fill(sc, edges_cap or 2 * n + 16, edges, start)


def exact_scene(n=16, seed=0, sigma=0.05):
    """Consistent edges (a ring and n / 2 chords, scales 0.7 .. 1.4 on the nodes), the start perturbed by N(0, sigma) per
    tangent coordinate; node 0 starts at the truth."""
    rng = np.random.default_rng(seed)
    sc = Scene()
    sc.n = n
    truth, _ = _truth(n, rng)
    scales = np.exp(rng.uniform(np.log(0.7), np.log(1.4), n))
    sc.truth = [(scales[i], p[1], scales[i] * p[2]) for i, p in enumerate(truth)]
    sc.truth = [(float(np.float32(p[0])), f32(p[1]).astype(np.float64), f32(p[2]).astype(np.float64)) for p in sc.truth]
    edges = [(i, (i + 1) % n, _between(sc.truth, i, (i + 1) % n)) for i in range(n)]
    for _ in range(n // 2):
        i = int(rng.integers(0, n))
        j = int((i + rng.integers(2, n - 1)) % n)
        edges.append((i, j, _between(sc.truth, i, j)))
    start = [sc.truth[0]] + [perturb(sc.truth[i], sigma * rng.standard_normal(7)) for i in range(1, n)]
    sc = _fill(sc, 2 * n + 16, edges, start)
    sc.centres = np.stack([-(p[1].T @ p[2]) / p[0] for p in sc.truth])
    return sc


def centre_error(g, sc):
    return float(np.linalg.norm(g.centres() - sc.centres, axis=1).max())


def run_scene(sc, **kw):
    g = sc.graph.copy()
    return g, graph_rule(g, 0, **kw)


RINGS = ((8, 0, 1), (65, 4, 2), (130, 8, 3))             # (nodes, chords, seed)


# ---- tests ----------------------------------------------------------------------------------------------------------------------
def header_text():
    return open(os.path.join(ROOT, "include", "fpc.h")).read()


def test_lib_exposes_every_new_symbol():
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(NAMES) <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))


def test_header_constants_equal_the_restatements_defaults():
    hdr = header_text()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in NAMES:
        nargs = len(re.search(r"\bint %s\s*\((.*?)\);" % name, code, flags=re.S).group(1).split(","))
        assert len(getattr(lib, name).argtypes) == nargs, name
    body = re.search(r"typedef struct fpc_graph_params \{(.*?)\} fpc_graph_params;", code, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(float|int)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_float if typ == "float" else ctypes.c_int) for n in names.split(",")]
    assert fields == list(_lib.FpcGraphParams._fields_)
    body = re.search(r"typedef struct fpc_graph_view \{(.*?)\} fpc_graph_view;", code, flags=re.S).group(1)
    names = [n.strip(" *") for _, group in re.findall(r"(float\*|int32_t\*|int|size_t)\s+([^;]+);", body) for n in group.split(",")]
    assert names == [n for n, _ in _lib.FpcGraphView._fields_]
    p = _lib.FpcGraphParams()
    assert lib.fpc_default_graph_params(ctypes.byref(p)) == 0
    assert {n: getattr(p, n) for n, _ in fields} == {k: (float(np.float32(v)) if isinstance(v, float) else v)
                                                     for k, v in DEFAULTS.items()}
    assert int(re.search(r"#define FPC_GRAPH_MAX_EDGES (\d+)", hdr).group(1)) == _lib.GRAPH_MAX_EDGES == MAX_EDGES
    assert int(re.search(r"#define FPC_GRAPH_INIT_TO (\d+)u", hdr).group(1)) == _lib.GRAPH_INIT_TO == 1
    assert int(re.search(r"#define FPC_BANK_MAX_SLOTS (\d+)", hdr).group(1)) == MAX_NODES
    for const in ("1e-14 of the largest diagonal entry", "max(lambda / 10, 1e-10)", "min(10 lambda, 1e6)", "C - C' <= 1e-6 C",
                  "accepted iff C' < C", "h = 512, 256, .. 1", "chunk of 64 edge", "|v| < 1e-12", "rz' <= cg_tol^2 rz0"):
        assert const in re.sub(r"\s*\n \*\s*", " ", hdr), const
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4
    assert lib.fpc_abi_version() == 4


def test_null_and_bad_arguments_are_refused():
    lib = _lib.load()
    p = _lib.FpcGraphParams()
    assert lib.fpc_default_graph_params(None) == FPC_E_INVALID
    assert lib.fpc_default_graph_params(ctypes.byref(p)) == 0
    d = np.zeros(64, np.float32).ctypes.data
    assert lib.fpc_graph_reserve(None, 4, 4, None) == FPC_E_INVALID
    assert lib.fpc_graph_get(None, None) == FPC_E_INVALID
    assert lib.fpc_graph_clear(None) == FPC_E_INVALID
    assert lib.fpc_graph_set_nodes(None, 0, 1, None, d, d) == FPC_E_INVALID
    assert lib.fpc_graph_add_edges(None, 1, d, d, None, d, d, None, 0, 0) == FPC_E_INVALID
    assert lib.fpc_graph_optimise(None, d, ctypes.byref(p), d) == FPC_E_INVALID
    assert lib.fpc_graph_apply_scale(None) == FPC_E_INVALID


# Measured on the restatement, per ring of RINGS (defaults: 16 attempts of at most 256 CG iterations):
#     8 nodes:            cost 2.86031 -> 0.00846852 (x 337.8),  4 of  6 attempts accepted, centre error 1.297 -> 0.1719
#    65 nodes, 4 chords:  cost 4.81755 -> 0.0016576  (x 2906.3), 7 of 12 attempts accepted, centre error 1.373 -> 0.09482
#   130 nodes, 8 chords:  cost 7.84027 -> 0.00202834 (x 3865.4), 6 of  6 attempts accepted, centre error 1.502 -> 0.1312
# (what is left is the odometry's own noise: 2 mrad and 0.01 per edge cannot be told from motion.)  The bars are four times
# what it achieves: the cost falls by at least a quarter of RING_GAIN, the centre error ends within four times RING_CENTRE.
RING_GAIN = {8: 337.8, 65: 2906.3, 130: 3865.4}
RING_CENTRE = {8: 0.1719, 65: 0.09482, 130: 0.1312}


@pytest.mark.parametrize("n,chords,seed", RINGS)
def test_rings_lose_their_drift(n, chords, seed):
    sc = ring_scene(n, True, chords, seed)
    g, out = run_scene(sc)
    before, after = centre_error(sc.graph, sc), centre_error(g, sc)
    print("ring %d: cost %.6g -> %.6g (x%.1f), %d of %d accepted, cg %s, centre error %.4g -> %.4g"
          % (n, out.stats[0], out.stats[1], out.stats[0] / out.stats[1], out.stats[3], out.stats[2], out.cg, before, after))
    assert not out.failed and out.stats[3] >= 1 and 1 in out.path                 # the accept path
    assert all(b < a for a, b in zip(out.costs, out.costs[1:]))                   # never rises
    assert out.stats[0] >= out.stats[1] * RING_GAIN[n] / 4, out.stats             # the cost falls
    assert after <= 4 * RING_CENTRE[n] and after < before, (before, after)        # the centre error falls


# the 16-node exact scene (start 0.16 off in the centres): cost 2.73463 -> 1.9e-12, 7 of 16 attempts accepted; the worst
# camera-centre error at the end measured 1.03e-06 and the worst |ln s - ln s_true| 9.87e-08: the fp32 state's rounding.
# Bars: four times these.
EXACT_CENTRE, EXACT_LNS = 1.03e-6, 9.87e-8


def test_exact_scene_recovers_the_ground_truth():
    sc = exact_scene()
    g, out = run_scene(sc)
    cen = centre_error(g, sc)
    lns = float(np.abs(np.log(g.s.astype(np.float64)) - np.log([p[0] for p in sc.truth])).max())
    print("exact: cost %.6g -> %.6g, %d of %d accepted, centre %.3g, ln s %.3g (start centre %.3g)"
          % (out.stats[0], out.stats[1], out.stats[3], out.stats[2], cen, lns, centre_error(sc.graph, sc)))
    assert out.stats[3] >= 1
    assert cen <= 4 * EXACT_CENTRE and lns <= 4 * EXACT_LNS, (cen, lns)


def test_a_call_without_an_accepted_attempt_leaves_the_nodes_bit_for_bit():
    sc = exact_scene(8, 3, 0.0)                                  # at the truth: fp32 rounding is all the cost there is
    g, out = run_scene(sc, iterations=3)
    again = g.copy()
    res = graph_rule(again, 0, iterations=3)
    if res.stats[3] == 0:
        for k in ("s", "R", "t"):
            np.testing.assert_array_equal(getattr(again, k).view(np.uint32), getattr(g, k).view(np.uint32))
    # a gauge that is unset or out of range: the call fails, nothing is written, the stats are zero
    for fixed in (-1, 8, 5):
        h = sc.graph.copy()
        if fixed == 5:
            h.s[5] = 0
        keep = h.copy()
        res = graph_rule(h, fixed)
        assert res.failed and not res.stats.any()
        for k in ("s", "R", "t"):
            np.testing.assert_array_equal(getattr(h, k).view(np.uint32), getattr(keep, k).view(np.uint32))
    # lambda at its ceiling and a truncated solve: every attempt of the rounding-level problem is rejected or accepted, but the
    # cost never rises and a rejected call returns the input bits
    h = sc.graph.copy()
    h.ew[:h.count] = 0                                           # weight 0 on every edge: g = 0, no step, no accept
    keep = h.copy()
    res = graph_rule(h, 0, iterations=4)
    assert res.stats[2] == 4 and res.stats[3] == 0 and res.path == [0, 0, 0, 0]
    for k in ("s", "R", "t"):
        np.testing.assert_array_equal(getattr(h, k).view(np.uint32), getattr(keep, k).view(np.uint32))


# The restatement with every sum over edges run the other way (per node and in the cost) against itself, worst over RINGS and
# the exact scene: |dR|, |dt| / max(1, |t|), |ds| / s.  Measured: all three exactly 0 -- the order moves the fp64 sums in their
# last bits, and the fp32 rounding of the state hides that unless a value lies within 1e-16 relative of a rounding boundary.
# The device comparison's fallback bound is four times these: the restatement's own fp32 values.
ORDER_MARGIN = np.array([0.0, 0.0, 0.0])


def order_difference(sc, **kw):
    ga, ra = run_scene(sc, **kw)
    gd, rd = run_scene(sc, descending=True, **kw)
    dr = np.abs(ga.R.astype(np.float64) - gd.R).max()
    dt = (np.abs(ga.t.astype(np.float64) - gd.t).max(1) / np.maximum(1.0, np.linalg.norm(ga.t.astype(np.float64), axis=1))).max()
    m = ga.is_set()
    ds = (np.abs(ga.s[m].astype(np.float64) - gd.s[m]) / ga.s[m]).max()
    return np.array([dr, dt, ds]), ra.path == rd.path


def test_descending_sums_bound_the_order_dependence():
    worst = np.zeros(3)
    for sc in [ring_scene(n, True, c, s) for n, c, s in RINGS] + [exact_scene()]:
        diff, same = order_difference(sc)
        assert same
        worst = np.maximum(worst, diff)
    print("order difference:", worst)
    assert (worst <= ORDER_MARGIN).all(), worst


def test_append_rules():
    g = Graph(6, 5)
    eye, z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    g.set_nodes(0, [eye], [z3])
    nan, inf = np.float32("nan"), np.float32("inf")
    bad_r, bad_t = eye.copy(), z3.copy()
    bad_r[1, 1], bad_t[2] = nan, inf
    cand = [  # (from, to, s, R, t, ninliers, taken)
        (0, 1, 1.0, eye, z3 + 1, 20, True),
        (0, 0, 1.0, eye, z3, 20, False),                         # from == to
        (-1, 1, 1.0, eye, z3, 20, False), (0, 6, 1.0, eye, z3, 20, False),       # out of range
        (1, 2, 0.0, eye, z3, 20, False), (1, 2, -1.0, eye, z3, 20, False), (1, 2, nan, eye, z3, 20, False),
        (1, 2, 1.0, bad_r, z3, 20, False), (1, 2, 1.0, eye, bad_t, 20, False),   # not finite
        (1, 2, 1.0, 0 * eye, z3, 20, False),                     # the RANSAC calls' failure output
        (1, 2, 1.0, eye, z3, 11, False),                         # under min_inliers
        (1, 2, 2.0, eye, z3 + 2, 12, True),
    ]
    cols = list(zip(*cand))
    g.add_edges(cols[0], cols[1], np.stack(cols[3]), np.stack(cols[4]), cols[2], cols[5], 12, init_to=True)
    assert g.count == 2 and g.dropped == 0
    assert g.efrom[:2].tolist() == [0, 1] and g.eto[:2].tolist() == [1, 2] and g.ew[:2].tolist() == [20.0, 12.0]
    # INIT_TO over a chain within one batch: node 1 from node 0, then node 2 from node 1
    assert g.s[:4].tolist() == [1.0, 1.0, 2.0, 0.0]
    np.testing.assert_array_equal(g.t[1], [1, 1, 1])
    np.testing.assert_array_equal(g.t[2], [4, 4, 4])             # 2 * (1, 1, 1) + (2, 2, 2)
    # a capacity overflow: five more candidates into three free places
    g.add_edges([2, 3, 4, 2, 3], [3, 4, 5, 4, 5], np.stack([eye] * 5), np.ones((5, 3), np.float32))
    assert g.count == 5 and g.dropped == 2 and g.eto[2:5].tolist() == [3, 4, 5]
    assert not g.s[3:].any()                                     # without INIT_TO no node is written
    g.clear()
    assert g.count == 0 and g.dropped == 0 and not g.s.any()


# apply_scale on the optimised 12-ring (node scales 1 .. 1.3): the worst relative change of a world point measured 4.81e-08 and
# the worst change of an edge's (e_omega, e_t sigma_b, e_sigma) 3.45e-07 -- one fp32 rounding of the landmarks, and of t and s
# of the nodes and edges; the cost went 0.00645602 -> 0.00645568 (its translation part rescaled).  Bars: four times these.
SCALE_WORLD, SCALE_RESIDUAL = 4.81e-8, 3.45e-7


def scale_check(g, lm, counts, unit=1.0):
    """-> (worst relative change of a world point, worst change of (e_omega, e_t sigma_b, e_sigma) per edge, cost before,
    cost after) of Graph.apply_scale on a copy."""
    def world(h, pts):
        out = []
        for i in range(h.nodes):
            r, t, s = h.R[i].astype(np.float64), h.t[i].astype(np.float64), np.float64(h.s[i])
            out.append((pts[i, :, :3].astype(np.float64) - t) @ r / s)
        return np.stack(out)

    def res(h):
        isset = h.is_set()
        act = isset[h.efrom[:h.count]] & isset[h.eto[:h.count]]
        e = residuals(h, h.s.astype(np.float64), h.R.astype(np.float64), h.t.astype(np.float64), act, 1.0 / unit)[0]
        return e, act, graph_cost(h, h.s.astype(np.float64), h.R.astype(np.float64), h.t.astype(np.float64), act, 1.0 / unit)

    h, pts = g.copy(), lm.copy()
    sig_b = np.where(g.is_set(), g.s, 1.0)[g.eto[:g.count]]
    w0, (e0, act, c0) = world(g, lm), res(g)
    h.apply_scale(pts, counts)
    w1, (e1, _, c1) = world(h, pts), res(h)
    valid = (np.arange(lm.shape[1])[None] < np.asarray(counts)[:, None]) & (lm[:, :, 3] != 0) & g.is_set()[:, None]
    dw = (np.linalg.norm(w1 - w0, axis=2) / np.maximum(1.0, np.linalg.norm(w0, axis=2)))[valid].max()
    e1 = e1.copy()
    e1[:, 3:6] *= sig_b[act][:, None]
    return float(dw), float(np.abs(e1 - e0).max()), c0, c1, h, pts


def scale_scene():
    sc = ring_scene(12, True, 2, 5)
    g, _ = run_scene(sc)
    rng = np.random.default_rng(9)
    lm = np.zeros((12, 40, 4), np.float32)
    lm[:, :, :3] = rng.uniform(-2, 2, (12, 40, 3)) + [0, 0, 6]
    lm[:, :, 3] = rng.random((12, 40)) < 0.8
    counts = rng.integers(20, 41, 12)
    return g, lm, counts


def test_apply_scale_keeps_the_world_points_and_the_scale_free_residuals():
    """Every world point R^T (X - t) / s is unchanged; so are e_omega and e_sigma of every edge, and e_t times its `to`
    node's scale: t_E becomes t_E / sigma_b (include/fpc.h), so the cost is unchanged exactly where the translation residuals
    are zero -- on a consistent graph -- and otherwise its translation part is rescaled edge by edge."""
    g, lm, counts = scale_scene()
    dw, de, c0, c1, h, pts = scale_check(g, lm, counts)
    print("apply_scale: world %.3g, residual %.3g, cost %.6g -> %.6g" % (dw, de, c0, c1))
    assert dw <= 4 * SCALE_WORLD and de <= 4 * SCALE_RESIDUAL, (dw, de)
    assert (h.s[h.is_set()] == 1).all()
    rows = np.arange(40)[None] >= counts[:, None]
    np.testing.assert_array_equal(pts[rows], lm[rows])                             # rows behind the count: untouched
    np.testing.assert_array_equal(pts[:, :, 3], lm[:, :, 3])                       # w kept
    # a consistent graph: the cost is unchanged up to the rounding of the fp32 state (both are that rounding)
    sc = exact_scene()
    for i, p in enumerate(sc.truth):
        sc.graph.set_nodes(i, [p[1]], [p[2]], [p[0]])
    lm16 = np.zeros((16, 40, 4), np.float32)
    lm16[:12] = lm
    _, de, c0, c1, _, _ = scale_check(sc.graph, lm16, np.concatenate([counts, [0] * 4]))
    print("apply_scale, consistent: residual %.3g, cost %.3g -> %.3g" % (de, c0, c1))
    # (24 edges of weight 1, seven residuals each, every one within the bar above of zero on either side)
    assert de <= 4 * SCALE_RESIDUAL and max(c0, c1) <= 24 * 7 * (4 * SCALE_RESIDUAL) ** 2


def test_code_object_keeps_the_kernels_out_of_scratch(code_object):  # noqa: F811
    _, meta = code_object
    names = [k for k in meta if re.match(r"_Z\d+pg_[a-z_]+_kernel", k)]
    # set_nodes, add_edges, degree, begin, fill, edges (two), decide, blocks, solve, retract, scale (edges, landmarks, nodes)
    assert len(names) == 14, names
    for k in names:
        m = meta[k]
        assert m["private_segment_fixed_size"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["group_segment_fixed_size"] <= 160 << 10, (k, m)
