"""The pose graph on the GPU (fpc_graph_reserve / _set_nodes / _clear / _get / _add_edges / _optimise / _apply_scale) against
the float64 restatement and the planted scenes of tests/test_pose_graph.py: the optimiser next to the restatement under the
same fp32 inputs at the smallest shapes at which a path changes (one edge, a ring of 8, 63 / 64 / 65 nodes across a wave
edge of the solve's workgroup, 257 nodes past four waves, 1024 nodes with 2048 edges), the append rules bit for bit,
apply_scale on both bank formats, the reservation, and the chain sim3_bank -> graph_add_edges -> graph_optimise ->
graph_apply_scale without a host call.  Every context runs under the canary zones.
Need a real MI355X: pytest -m gpu"""
import ctypes

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import _lib, synth

from tests.test_gpu_homography_ransac import H, N, W, engine
from tests.test_gpu_sim3_ransac import KQVGA, SIGMA
from tests.test_pose_graph import Graph, ORDER_MARGIN, exact_scene, graph_rule, ring_scene
from tests.test_sim3_ransac import _rotation

pytestmark = pytest.mark.gpu

# Device against restatement under the SAME fp32 inputs: test_gpu_refine_window.py's bar, for its reasons -- both sides evaluate
# the rule in fp64 and round the state to fp32 behind every attempt: 1e-5 for R, for t relative to max(1, |t|) and for s
# relative, with the same attempt and accept counts.  A scene off the restatement's path is reported and held to the fallback
# bound, four times the restatement's ascending-against-descending difference (tests/test_pose_graph.py: zero).
R_BAR = 1e-5
SHORT = dict(iterations=4, cg_iterations=64)           # the rings beyond 8 nodes: the attempts that remove the drift


@pytest.fixture(scope="module")
def graphs():
    """Small contexts under guard zones, one per (nodes, edges) reservation: the solve's workgroup is sized by the nodes.
    One is alive at a time; each is checked for damaged canaries before it is closed."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    live = {}

    def retire():
        for e in live.values():
            try:
                assert e.check_guards() == 0
            finally:
                e.close()
        live.clear()

    def get(nodes, edges):
        if (nodes, edges) not in live:
            retire()
            e = engine(64, 96, 1, descriptor_enabled=False, max_keypoints=64)
            live[(nodes, edges)] = e
            plan = e._l.fpc_plan_hash(e._ctx)
            with pytest.raises(_lib.FpcError):
                e.graph_optimise(0)                                                  # before the reservation: refused
            with pytest.raises(_lib.FpcError):
                e.graph_clear()
            assert e.graph_reserve(nodes, edges) >= nodes * 52 + edges * 64
            assert e._l.fpc_plan_hash(e._ctx) == plan                                # nothing is carved
            with pytest.raises(_lib.FpcError):
                e.graph_reserve(nodes, edges)                                        # a second reserve is refused
        return live[(nodes, edges)]

    yield get
    retire()


def _bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _load(e, g):
    """The restatement's Graph `g` onto the device: its nodes, then its edges through fpc_graph_add_edges."""
    e.graph_clear()
    e.graph_set_nodes(0, g.R, g.t, g.s)
    k = g.count
    if k:
        e.graph_add_edges_async(g.efrom[:k], g.eto[:k], g.eR[:k], g.et[:k], g.es[:k],
                                ninliers=None if (g.ew[:k] == 1).all() else g.ew[:k].astype(np.int32))


def _nodes(e):
    e.sync()
    return tuple(v.cpu().numpy() for v in e.graph_nodes())


def _edges(e):
    e.sync()
    return tuple(v.cpu().numpy() for v in e.graph_edges())


def _same_graph(e, g, tag=""):
    """The device's nodes, edges and counters bit for bit the restatement's."""
    s, r, t = _nodes(e)
    _bits(s, g.s), _bits(r, g.R), _bits(t, g.t)
    frm, to, es, er, et, ew, count = _edges(e)
    assert count.tolist() == [g.count, g.dropped], (tag, count, g.count, g.dropped)
    k = g.count
    np.testing.assert_array_equal(frm[:k], g.efrom[:k]), np.testing.assert_array_equal(to[:k], g.eto[:k])
    _bits(es[:k], g.es[:k]), _bits(er[:k], g.eR[:k]), _bits(et[:k], g.et[:k]), _bits(ew[:k], g.ew[:k])


def _compare(e, g, fixed=0, tag="", **params):
    """fpc_graph_optimise on the loaded graph next to graph_rule on `g` (changed in place) -> (stats, same path?)."""
    before = _nodes(e)
    stats = e.graph_optimise(fixed, **params)
    want = graph_rule(g, fixed, **params)
    s, r, t = _nodes(e)
    if want.failed:
        assert not stats.any(), (tag, stats)
        for a, b in zip(before, (s, r, t)):
            _bits(a, b)
        return stats, True
    assert abs(stats[0] - want.stats[0]) <= 1e-6 * want.stats[0] + 1e-30, (tag, stats, want.stats)
    assert stats[1] <= stats[0], (tag, stats)
    same = stats[2] == want.stats[2] and stats[3] == want.stats[3]
    m = g.is_set()
    np.testing.assert_array_equal(s > 0, m)
    dr = np.abs(r.astype(np.float64) - g.R).max()
    dt = (np.abs(t.astype(np.float64) - g.t).max(1) / np.maximum(1.0, np.linalg.norm(g.t.astype(np.float64), axis=1))).max()
    ds = (np.abs(s[m].astype(np.float64) - g.s[m]) / g.s[m]).max() if m.any() else 0.0
    print("%s: cost %.6g -> %.6g, %d of %d accepted (restatement %d of %d), |dR| %.2e, |dt| %.2e, |ds| %.2e"
          % (tag, stats[0], stats[1], stats[3], stats[2], want.stats[3], want.stats[2], dr, dt, ds))
    if same:
        assert dr <= R_BAR and dt <= R_BAR and ds <= R_BAR, (tag, dr, dt, ds)
        assert abs(stats[1] - want.stats[1]) <= 1e-3 * want.stats[1] + 1e-12, (tag, stats, want.stats)
    else:
        print("OFF THE RESTATEMENT'S PATH:", tag, stats, want.stats, want.path)
        assert dr <= 4 * ORDER_MARGIN[0] and dt <= 4 * ORDER_MARGIN[1] and ds <= 4 * ORDER_MARGIN[2], (tag, dr, dt, ds)
    if stats[3] == 0:
        for a, b in zip(before, (s, r, t)):
            _bits(a, b)                                                              # no accepted attempt: bit for bit
    return stats, same


def _two_nodes():
    sc = ring_scene(2, True, 0, 7)
    sc.graph.set_nodes(1, [np.eye(3)], [[0.3, -0.2, 0.1]], [1.2])                    # a start off the one edge
    return sc


SCENES = {
    "2 nodes, 1 edge": (_two_nodes, {}),
    "ring of 8": (lambda: ring_scene(8, True, 0, 1), {}),
    "63 nodes": (lambda: ring_scene(63, True, 0, 4), SHORT),
    "64 nodes": (lambda: ring_scene(64, True, 0, 5), SHORT),
    "65 nodes, 4 chords": (lambda: ring_scene(65, True, 4, 2), SHORT),
    "257 nodes, 3 chords": (lambda: ring_scene(257, True, 3, 6), SHORT),
    "1024 nodes, 2048 edges": (lambda: ring_scene(1024, True, 1024, 8, edges_cap=2048), dict(iterations=2, cg_iterations=32)),
    "exact, 16 nodes": (exact_scene, {}),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_device_against_the_restatement(graphs, name):
    make, params = SCENES[name]
    sc = make()
    g = sc.graph.copy()
    e = graphs(g.nodes, g.edges)
    _load(e, g)
    _same_graph(e, g, name)
    stats, _ = _compare(e, g, 0, name, **params)
    assert stats[3] >= 1 and stats[1] < stats[0], (name, stats)
    # repeated sequences are bit-identical
    first = _nodes(e)
    _load(e, sc.graph)
    again = e.graph_optimise(0, **params)
    _bits(again, stats)
    for a, b in zip(first, _nodes(e)):
        _bits(a, b)


def test_other_cases(graphs):
    sc = ring_scene(8, True, 0, 1)
    e = graphs(sc.graph.nodes, sc.graph.edges)
    # cg_iterations = 1: a truncated solve is still an attempt
    g = sc.graph.copy()
    _load(e, g)
    _compare(e, g, 0, "cg_iterations = 1", iterations=6, cg_iterations=1)
    # a trans_unit, a gauge other than node 0, the gauge as a device tensor
    import torch
    g = sc.graph.copy()
    _load(e, g)
    stats = e._host((e.graph_optimise_async(torch.tensor([3], dtype=torch.int32, device=e.torch_device), trans_unit=5.0),))[0]
    want = graph_rule(g, 3, trans_unit=5.0)
    assert stats[2] == want.stats[2] and stats[3] == want.stats[3] and abs(stats[1] - want.stats[1]) <= 1e-3 * want.stats[1]
    _bits(_nodes(e)[1][3], sc.graph.R[3])                                            # the gauge stays
    # an isolated set node and an unset node: neither changes; a duplicate edge; an edge of weight 0
    big = ring_scene(10, True, 1, 11, edges_cap=24)
    e = graphs(12, 24)
    g = Graph(12, 24)
    g.set_nodes(0, big.graph.R, big.graph.t, big.graph.s)
    g.set_nodes(10, [_rotation([1, 2, 3], 0.4)], [[1, 2, 3]], [0.8])                 # isolated; node 11 stays unset
    k = big.graph.count
    ninl = np.full(k + 3, 30, np.int32)
    ninl[k + 1] = 0                                                                  # weight 0
    frm = np.concatenate([big.frm, [big.frm[2], 4, 11]]).astype(np.int32)            # a duplicate; weight 0; to an unset node
    to = np.concatenate([big.to, [big.to[2], 7, 3]]).astype(np.int32)
    er = np.concatenate([big.eR, big.eR[2:3], big.eR[:2]])
    et = np.concatenate([big.et, big.et[2:3], big.et[:2]])
    es = np.concatenate([big.es, big.es[2:3], big.es[:2]])
    g.add_edges(frm, to, er, et, es, ninl, 0)
    assert g.count == k + 3
    e.graph_clear()
    e.graph_set_nodes(0, g.R[:11], g.t[:11], g.s[:11])
    e.graph_add_edges_async(frm, to, er, et, es, ninliers=ninl, min_inliers=0)
    _same_graph(e, g, "other cases")
    start = g.copy()
    stats, _ = _compare(e, g, 0, "isolated, unset, duplicate, weight 0")
    s, r, t = _nodes(e)
    assert stats[3] >= 1
    for i in (0, 10, 11):
        _bits(s[i], start.s[i]), _bits(r[i], start.R[i]), _bits(t[i], start.t[i])
    # a fixed node that is unset, or out of range: the call fails, no node is written, the stats are zero
    for fixed in (11, 12, -1):
        keep = _nodes(e)
        stats = e.graph_optimise(fixed)
        assert not stats.any(), stats
        for a, b in zip(keep, _nodes(e)):
            _bits(a, b)


def test_tails_and_bad_arguments(graphs):
    import torch
    sc = ring_scene(8, True, 0, 1)
    e = graphs(sc.graph.nodes, sc.graph.edges)
    _load(e, sc.graph)
    dev = e.torch_device
    p = _lib.FpcGraphParams()
    e._l.fpc_default_graph_params(ctypes.byref(p))
    fixed = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((16 + 64,), 0xFF, dtype=torch.uint8, device=dev)               # stats, pre-filled and longer
    torch.cuda.synchronize()
    e._call("fpc_graph_optimise", fixed, ctypes.byref(p), out, inputs=(fixed,))
    e.sync()
    host = out.cpu().numpy()
    assert (host[16:] == 0xFF).all()
    stats = host[:16].view(np.float32)
    assert stats[3] >= 1 and stats[1] < stats[0]
    lib, ctx, pp = e._l, e._ctx, ctypes.byref(p)
    d = out.data_ptr()
    keep = _nodes(e)
    bad = []
    for field, value in (("iterations", 0), ("iterations", 17), ("lambda0", 0.0), ("lambda0", float("nan")), ("cg_iterations", 0),
                         ("cg_iterations", 1025), ("cg_tol", -1.0), ("trans_unit", 0.0), ("trans_unit", float("inf"))):
        q = _lib.FpcGraphParams()
        lib.fpc_default_graph_params(ctypes.byref(q))
        setattr(q, field, value)
        bad.append(lib.fpc_graph_optimise(ctx, fixed.data_ptr(), ctypes.byref(q), d))
    bad += [lib.fpc_graph_optimise(ctx, None, pp, d), lib.fpc_graph_optimise(ctx, fixed.data_ptr(), None, d),
            lib.fpc_graph_optimise(ctx, fixed.data_ptr(), pp, None),
            lib.fpc_graph_set_nodes(ctx, -1, 1, None, d, d), lib.fpc_graph_set_nodes(ctx, 0, 0, None, d, d),
            lib.fpc_graph_set_nodes(ctx, 1, 8, None, d, d), lib.fpc_graph_set_nodes(ctx, 0, 1, None, None, d),
            lib.fpc_graph_add_edges(ctx, 0, d, d, None, d, d, None, 0, 0),
            lib.fpc_graph_add_edges(ctx, _lib.GRAPH_MAX_EDGES + 1, d, d, None, d, d, None, 0, 0),
            lib.fpc_graph_add_edges(ctx, 1, None, d, None, d, d, None, 0, 0), lib.fpc_graph_add_edges(ctx, 1, d, d, None, d, d, None, 0, 2),
            lib.fpc_graph_get(ctx, None), lib.fpc_graph_apply_scale(ctx),           # (no bank)
            lib.fpc_graph_reserve(ctx, 0, 4, None), lib.fpc_graph_reserve(ctx, 4, _lib.GRAPH_MAX_EDGES + 1, None)]
    assert bad == [-1] * len(bad), bad
    for a, b in zip(keep, _nodes(e)):
        _bits(a, b)                                                                  # nothing was written


def test_add_edges_matches_the_restatement_bit_for_bit(graphs):
    """Refusals, min_inliers, an overflow with the dropped counter, INIT_TO over a chain within one batch, and a batch longer
    than the kernel's tile of 256 candidates."""
    rng = np.random.default_rng(17)
    n = 700
    e = graphs(40, 300)
    g = Graph(40, 300)
    frm, to = rng.integers(-1, 41, n).astype(np.int32), rng.integers(-1, 41, n).astype(np.int32)
    frm[:39], to[:39] = np.arange(39), np.arange(1, 40)                             # a chain first: INIT_TO walks it
    er = np.stack([_rotation(rng.normal(size=3), rng.uniform(0, 1)) for _ in range(n)]).astype(np.float32)
    et = rng.normal(size=(n, 3)).astype(np.float32)
    es = rng.uniform(0.5, 2.0, n).astype(np.float32)
    ninl = rng.integers(0, 60, n).astype(np.int32)
    ninl[:39] = 50
    er[rng.choice(np.arange(39, n), 40, replace=False)] = 0                          # the RANSAC calls' failure output
    es[rng.choice(np.arange(39, n), 20, replace=False)] = [0.0, -1.0, np.nan, np.inf] * 5
    et[rng.choice(np.arange(39, n), 10, replace=False), 1] = np.nan
    er[rng.choice(np.arange(39, n), 10, replace=False), 2, 2] = np.inf
    start = (np.eye(3, dtype=np.float32)[None], np.array([[0.5, -1.0, 2.0]], np.float32), np.array([1.5], np.float32))
    e.graph_clear()
    e.graph_set_nodes(0, *start)
    g.set_nodes(0, *start)
    g.add_edges(frm, to, er, et, es, ninl, 12, init_to=True)
    e.graph_add_edges_async(frm, to, er, et, es, ninliers=ninl, min_inliers=12, init_to=True)
    assert g.count == 300 and g.dropped > 50 and g.is_set().all(), (g.count, g.dropped)
    _same_graph(e, g, "first batch")
    g.add_edges(frm[:50], to[:50], er[:50], et[:50])                                 # a full graph: every taken edge is dropped
    held, dropped = e.graph_add_edges(frm[:50], to[:50], er[:50], et[:50])
    assert (held, dropped) == (g.count, g.dropped)
    _same_graph(e, g, "second batch")
    e.graph_clear()
    g.clear()
    g.add_edges(frm[:300], to[:300], er[:300], et[:300], es[:300])                   # no start: INIT_TO has nothing to do
    e.graph_add_edges_async(frm[:300], to[:300], er[:300], et[:300], es[:300], init_to=True)
    assert 100 < g.count < 300 and not g.is_set().any()
    _same_graph(e, g, "after a clear")


@pytest.mark.parametrize("fmt", ("f32", "bf16"))
def test_apply_scale_on_either_bank_format(fmt):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(64, 96, 1, max_keypoints=64)
    try:
        cap, slots = e.capacity, 12
        e.bank_create(slots, cap, format=fmt)
        e.bank_landmarks_reserve()
        with pytest.raises(_lib.FpcError):
            e.graph_apply_scale()                                                    # no graph reservation
        e.graph_reserve(slots, 40)
        sc = ring_scene(slots - 1, True, 2, 5)                                       # slot 11: an unset node
        g = Graph(slots, 40)
        g.set_nodes(0, sc.graph.R, sc.graph.t, sc.graph.s)
        g.add_edges(sc.frm, sc.to, sc.eR, sc.et, sc.es)
        g.add_edges([3], [11], sc.eR[:1], sc.et[:1], [1.3])                          # an edge to the unset node
        _load(e, g)
        rng = np.random.default_rng(9)
        counts = rng.integers(cap // 2, cap + 1, slots)
        lm = np.zeros((slots, cap, 4), np.float32)
        desc = rng.normal(size=(cap, e.desc_dim)).astype(np.float32)
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        for s in range(slots):
            xyz = (rng.uniform(-2, 2, (cap, 3)) + [0, 0, 6]).astype(np.float32)
            valid = rng.random(cap) < 0.8
            e.bank_store_rows(s, desc[:counts[s]], rng.integers(0, 64, (counts[s], 2)).astype(np.int32))
            e.bank_store_landmarks(s, xyz, valid)
        e.sync()
        lm = e.bank_landmarks().cpu().numpy().copy()
        for twice in range(2):                                                       # (the second call finds every s = 1)
            stats = e.graph_optimise(0, iterations=3) if not twice else None
            if stats is not None:
                assert stats[3] >= 1
                s, r, t = _nodes(e)
                g.s, g.R, g.t = s.copy(), r.copy(), t.copy()                         # the device's own state goes on
            e.graph_apply_scale()
            g.apply_scale(lm, counts)
            _same_graph(e, g, fmt)
            _bits(e.bank_landmarks().cpu().numpy(), lm)
        assert (g.s[:11] == 1).all() and g.s[11] == 0
        assert e.check_guards() == 0
    finally:
        e.close()


def test_loop_closing_chain_without_a_host_call():
    """test_gpu_sim3_ransac.py's planted loop closing, carried on: the frame is aligned with the loop candidate in slot 1
    (fpc_sim3_bank), that similarity becomes the edge slot 1 -> slot 0 of the graph, FPC_GRAPH_INIT_TO gives node 0 its
    start from node 1, the optimiser runs and fpc_graph_apply_scale brings slot 0's landmarks (the frame's own, at SIGMA
    times slot 1's scale) to slot 1's scale -- nothing returns to the host in between."""
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    e = engine(conf_thresh=0.001)
    try:
        e.pnp_reserve()
        e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
        e.detect(synth.make_batch(300, N, H, W))
        cap, dev = e.capacity, e.torch_device
        rng = np.random.default_rng(31)
        fx, fy, cx, cy = KQVGA
        npts = 800
        px = np.stack([rng.uniform(30, W - 30, npts), rng.uniform(30, H - 30, npts)], 1)
        z = rng.uniform(4.0, 12.0, npts)
        pa = np.round(px).astype(np.int32)
        xa = np.stack([(pa[:, 0] - cx) / fx * z, (pa[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
        r0, t0 = _rotation([0.3, 1.0, -0.2], np.deg2rad(7.0)), np.array([1.6, -0.4, 0.5])
        xc = xa.astype(np.float64) @ r0.T + t0
        pc = np.round(np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)).astype(np.int32)
        seen = np.flatnonzero((pc[:, 0] >= 0) & (pc[:, 0] < W) & (pc[:, 1] >= 0) & (pc[:, 1] < H))
        rows_c = rng.permutation(seen)[:600]
        desc = rng.normal(size=(npts, e.desc_dim)).astype(np.float32)
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        lm1 = np.zeros((cap, 3), np.float32)
        lm1[:npts] = (xa.astype(np.float64) / SIGMA).astype(np.float32)              # the loop candidate's scale
        qxyz = np.zeros((N, cap, 3), np.float32)
        qxyz[0, :len(rows_c)] = xc[rows_c]                                           # the frame's own landmarks, its own scale
        qvalid = np.zeros((N, cap), np.uint8)
        qvalid[0, :len(rows_c)] = 1
        xy, count = e._points_view()
        dview, _ = e._results_view()
        hx, hd = np.zeros((N, cap, 2), np.int32), np.zeros((N, cap, e.desc_dim), np.float32)
        hx[0, :len(rows_c)], hd[0, :len(rows_c)] = pc[rows_c], desc[rows_c]
        e.bank_create(2, cap)
        e.bank_landmarks_reserve()
        e.graph_reserve(2, 8)
        xy[:N].copy_(torch.from_numpy(hx))
        dview[:N].copy_(torch.from_numpy(hd))
        count[:N].copy_(torch.tensor([len(rows_c)] + [0] * (N - 1), dtype=torch.int32))
        qx, qv = torch.from_numpy(qxyz).to(dev), torch.from_numpy(qvalid).to(dev)
        to = torch.zeros(N, dtype=torch.int32, device=dev)                           # the frame goes into slot 0
        torch.cuda.synchronize()
        # ---- from here on nothing returns to the host until the results are read
        e.bank_store_rows(1, desc, pa)
        e.bank_store_landmarks(1, lm1, None)
        e.graph_set_nodes(1, np.eye(3)[None], np.zeros((1, 3)))                      # slot 1 is the map's frame
        _, loop, match, _ = e.match_bank_async(N, cross_check=True, max_dist=0.7)
        sv, rm, tv, ni, _ = e.sim3_bank_async(N, loop, match, qx, qv, K_query=KQVGA, K_train=KQVGA, iterations=512, seed=5)
        e.bank_store_rows(0, hd[0, :len(rows_c)], hx[0, :len(rows_c)])               # the frame becomes key frame 0
        e.bank_store_landmarks(0, qx[0], qv[0])
        e.graph_add_edges_async(loop, to, rm, tv, sv, ninliers=ni, min_inliers=12, init_to=True)
        stats = e.graph_optimise_async(1)
        e.graph_apply_scale()
        loop, sv, rm, tv, ni, stats = e._host((loop, sv, rm, tv, ni, stats))
        s, r, t = _nodes(e)
        frm, eto, es, er, et, ew, cnt = _edges(e)
        lm = e.bank_landmarks().cpu().numpy()
        print("chain: loop slot %d, s %.5f (planted %.2f), %d inliers, stats %s, edges %s" % (loop[0], sv[0], SIGMA, ni[0], stats, cnt))
        assert loop[0] == 1 and (loop[1:] == -1).all() and ni[0] > 400
        assert abs(sv[0] / SIGMA - 1) < 1e-2
        assert cnt.tolist() == [1, 0] and frm[0] == 1 and eto[0] == 0 and ew[0] == ni[0]
        assert stats[2] >= 1 and stats[1] <= stats[0] and stats[0] < 1e-8              # one consistent edge: nothing to spread
        assert s.tolist() == [1.0, 1.0]
        # one edge that INIT_TO satisfies: the optimiser may move node 0 by roundings only (the fp32 R is not exactly
        # orthonormal), so node, edge and landmarks are the similarity's own values within a few fp32 roundings
        inv, tol = 1.0 / np.float64(sv[0]), 1e-6
        assert np.abs(r[0] - rm[0]).max() <= tol and np.abs(t[0] - tv[0] * inv).max() <= tol * max(1.0, np.abs(tv[0]).max())
        assert abs(es[0] - 1.0) <= tol and np.abs(et[0] - tv[0] * inv).max() <= tol * max(1.0, np.abs(tv[0]).max())
        scaled = qxyz[0, :len(rows_c)].astype(np.float64) * inv
        assert (np.abs(lm[0, :len(rows_c), :3] - scaled) <= tol * np.abs(scaled) + 1e-30).all()
        assert (lm[0, :len(rows_c), 3] == 1).all()
        _bits(lm[1, :npts, :3], lm1[:npts])                                          # slot 1 was at scale 1: untouched
        # one scale: slot 0's landmarks are now the loop candidate's under the edge's rigid part
        want = lm1[rows_c].astype(np.float64) @ r[0].astype(np.float64).T + t[0]
        rel = np.linalg.norm(lm[0, :len(rows_c), :3] - want, axis=1) / np.linalg.norm(want, axis=1)
        assert np.median(rel) < 1e-3, np.median(rel)
        assert e.check_guards() == 0
    finally:
        e.close()
