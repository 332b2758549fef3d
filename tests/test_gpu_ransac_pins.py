"""The geometry chain's device results, pinned bit for bit to tests/golden/ransac_pins.json.

The RANSAC kernels (csrc/ransac_parts.h and the three model headers) can be reorganised without changing what they compute;
the other GPU tests compare them to float64 restatements within bars, which such a change could move inside of.  This test
is what says it moved nothing: for every case the model's floats (as uint32 bit patterns), the inlier counts and the SHA-256
of the masks equal the fixture -- explicit pairs through fpc_ransac_homography / _fundamental / _pnp at the pair counts,
iteration counts and refit counts where the kernels change path, and the gather paths (frames, bank, top-K, pose, landmarks)
on planted keypoints of a QVGA context.

A pull request that MEANS to change a result (another sampler, another tolerance, another summation order) regenerates the
fixture with tests/golden/make_golden_ransac.py and says so; any other pull request passes this test with the fixture as it
is.  Need a real MI355X: pytest -m gpu"""
import hashlib
import json
import os

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth

from tests.test_pnp_ransac import _rotation, camera_points

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_pins.json")
H, W, N = 240, 320, 3                  # the gather paths' context: the QVGA geometry of the RANSAC tests, three frames
KVEC = (250.0, 250.0, 160.0, 120.0)
KPAIRS = (500.0, 500.0, 320.0, 240.0)  # the explicit pairs' camera (a 640 x 480 frame)
RHO = {"homography": 0.3, "fundamental": 0.3, "pnp": 0.1}           # the planted frames' share of outliers
# family -> (hypotheses per workgroup of its score kernel, sample size, engine call, the seed of its T = 1 case: one under
# which, by the float64 restatements, hypothesis 0 of both planted frames of pair set "b" is drawn from inliers only)
FAMILIES = {"homography": (256, 4, "ransac_homography", 20), "fundamental": (128, 8, "ransac_fundamental", 143),
            "pnp": (64, 6, "ransac_pnp", 8)}
SEED = 5
GATHER = ("homography_frames", "homography_bank", "homography_bank_topk", "fundamental_frames", "fundamental_bank",
          "pose_frames", "pnp_frames", "pnp_bank")


def cases():
    """(id, family or None, arguments).  Explicit pairs: two four-frame pair sets per family -- "a": sample - 1, sample, 257
    (one past the refit's stride) and 1 024 pairs (one LDS chunk); "b": 1 025 pairs, the context's capacity, outliers only,
    exactly collinear points -- under T in {1, THREADS - 1, THREADS, THREADS + 1}, refits in {0, 1, 3} and one min_inliers
    that rejects the 257-pair frame's best hypothesis.  Then the eight gather paths."""
    out = []
    for fam, (threads, sample, _, seed1) in FAMILIES.items():
        for pairs, t, refits, min_inliers in (("a", threads, 0, sample), ("a", threads, 1, sample), ("a", threads + 1, 3, sample),
                                              ("b", threads - 1, 1, sample), ("b", 1, 3, sample), ("a", threads, 1, 600)):
            out.append(("%s-%s-T%d-r%d-m%d" % (fam, pairs, t, refits, min_inliers), fam,
                        dict(pairs=pairs, iterations=t, refits=refits, min_inliers=min_inliers, seed=seed1 if t == 1 else SEED)))
    return out + [("gather-" + name, None, name) for name in GATHER]


# ---- planted inputs (numpy only; pixels are rounded, so the last bit of a cosine does not reach them) ---------------------------
_TRUTH_H = np.array([[1.05, 0.03, 12.0], [-0.02, 0.97, -8.0], [2e-5, -3e-5, 1.0]])
_TRUTH_R, _TRUTH_T = _rotation([0.2, 1.0, 0.1], np.deg2rad(5.0)), np.array([0.8, 0.1, 0.05])


def _project(r, t, xyz, kvec, exact=False):
    fx, fy, cx, cy = kvec
    xc = camera_points(r, t, xyz)
    pix = np.stack([fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy], 1)
    return pix if exact else np.round(pix)


def _frame(fam, kind, m, rng):
    """One frame's pairs (a float32 [m,2], b float32 [m,2] or [m,3]): planted -- rounded pixels with a share RHO of outliers
    or, below 100 pairs, unrounded ones without: a frame of exactly one sample must be that sample's inliers --, outliers
    only, or exactly collinear on both sides."""
    k = np.arange(m, dtype=np.float64)
    exact = m < 100
    if kind == "collinear":
        if fam == "pnp":
            return np.stack([3 * k + 2, 2 * k + 5], 1).astype(np.float32), np.stack([0.5 * k - 3, 0.25 * k + 1, 0.125 * k + 4], 1).astype(np.float32)
        return np.stack([k, 2 * k + 3], 1).astype(np.float32), np.stack([k + 5, 2 * k + 1], 1).astype(np.float32)
    px = np.stack([rng.integers(0, 640, m), rng.integers(0, 480, m)], 1).astype(np.float64)
    noise = np.stack([rng.integers(0, 640, m), rng.integers(0, 480, m)], 1).astype(np.float64)
    z = rng.uniform(4.0, 12.0, m)
    out = rng.uniform(size=m) < (0.0 if exact else RHO[fam])
    if kind == "outliers":
        out[:] = True
    if fam == "homography":
        q = np.concatenate([px, np.ones((m, 1))], 1) @ _TRUTH_H.T
        a, b = px, q[:, :2] / q[:, 2:] if exact else np.round(q[:, :2] / q[:, 2:])
        b[out] = noise[out]
    elif fam == "fundamental":
        xyz = np.stack([(px[:, 0] - 320.0) / 500.0 * z, (px[:, 1] - 240.0) / 500.0 * z, z], 1)
        a, b = px, _project(_TRUTH_R, _TRUTH_T, xyz, KPAIRS, exact)
        b[out] = noise[out]
    else:
        xyz = np.stack([(px[:, 0] - 320.0) / 500.0 * z, (px[:, 1] - 240.0) / 500.0 * z, z], 1).astype(np.float32)
        a, b = _project(_TRUTH_R, _TRUTH_T, xyz, KPAIRS, exact), xyz
        a[out] = noise[out]
    return a.astype(np.float32), b.astype(np.float32)


def _pairs(fam, which, cap):
    sample = FAMILIES[fam][1]
    rng = np.random.default_rng(1000 * sorted(FAMILIES).index(fam) + (which == "b"))
    frames = ((("planted", sample - 1), ("planted", sample), ("planted", 257), ("planted", 1024)) if which == "a" else
              (("planted", 1025), ("planted", cap), ("outliers", 300), ("collinear", 200)))
    lists = [_frame(fam, kind, m, rng) for kind, m in frames]
    a = np.zeros((4, cap, 2), np.float32)
    b = np.zeros((4, cap, lists[0][1].shape[1]), np.float32)
    for f, (u, v) in enumerate(lists):
        a[f, :len(u)], b[f, :len(v)] = u, v
    return a, b, np.array([len(u) for u, _ in lists], np.int32)


def _world(kind, cap):
    """The gather paths' planted keypoints: a key frame of 700 rows (pixels kxy int32, landmarks key_xyz float32 in its camera
    frame with three rows that are not finite, key_valid) and N views of it -> per view (xy int32 [k,2], match int32 [k]): a
    fifth of a view's matches is wrong, some rows have none, some point behind the key's rows.  kind "plane": the views see
    the key through homographies; "scene": through rigid motions."""
    rng = np.random.default_rng(7 if kind == "plane" else 8)
    nkey = 700
    kxy = np.stack([rng.integers(20, W - 20, nkey), rng.integers(20, H - 20, nkey)], 1).astype(np.float64)
    z = rng.uniform(4.0, 12.0, nkey)
    fx, fy, cx, cy = KVEC
    key_xyz = np.stack([(kxy[:, 0] - cx) / fx * z, (kxy[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    valid = rng.uniform(size=nkey) > 0.1
    views = []
    for f in range(N):
        if kind == "plane":
            g = np.array([[1.0 + 0.02 * f, 0.03, 4.0 - 3 * f], [-0.02, 0.98, 2.0 + f], [1e-5 * f, -2e-5, 1.0]])
            q = np.concatenate([kxy, np.ones((nkey, 1))], 1) @ g.T
            pix = np.round(q[:, :2] / q[:, 2:])
        else:
            pix = _project(_rotation([0.3 * f, 1.0, 0.2], np.deg2rad(2.0 + 2 * f)), np.array([0.4, -0.1 * f, 0.05]), key_xyz, KVEC)
        seen = np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < W) & (pix[:, 1] >= 0) & (pix[:, 1] < H))
        rows = rng.permutation(seen)[:600 - 40 * f]
        match = rows.astype(np.int32)
        wrong = rng.choice(len(rows), len(rows) // 5, replace=False)
        match[wrong] = rng.integers(0, nkey, len(wrong))
        match[rng.choice(len(rows), 20, replace=False)] = -1
        match[rng.choice(len(rows), 5, replace=False)] = nkey + 3
        views.append((pix[rows].astype(np.int32), match))
    key_xyz[5, 1], key_xyz[17, 0], key_xyz[40, 2] = np.nan, np.inf, -np.inf
    valid[[5, 17]] = True
    return kxy.astype(np.int32), key_xyz, valid, views


# ---- what a case records --------------------------------------------------------------------------------------------------------
def _bits(a):
    return ["%08x" % v for v in np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel().tolist()]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def _model(out, names=("model", "ninliers", "mask")):
    """(floats ..., an int32 count, a bool mask) -> the floats' bits, the counts, the mask's hash."""
    rec = {name: _bits(v) for name, v in zip(names[:-2], out[:-2])}
    rec[names[-2]] = [int(v) for v in np.asarray(out[-2]).ravel()]
    rec[names[-1]] = _sha(np.asarray(out[-1]).astype(np.uint8))
    return rec


class Rig:
    """The two contexts the cases run on, made when first needed: `pairs` (four frames, no descriptor head, 1 280 keypoints so
    that a pair list crosses the 1 024-record LDS chunk) and `frames` (the QVGA context of the RANSAC tests with synthetic
    weights and one detect of N frames, whose keypoints the gather cases replace by planted ones)."""

    def __init__(self):
        self._pairs = self._frames = None
        self._inputs = {}

    def pairs(self):
        from tests.test_gpu_homography_ransac import engine
        if self._pairs is None:
            self._pairs = engine(480, 640, 4, descriptor_enabled=False, max_keypoints=1280)
            assert self._pairs.pnp_reserve() > 0 and self._pairs.capacity >= 1100
        return self._pairs

    def frames(self):
        from tests.test_gpu_homography_ransac import engine
        if self._frames is None:
            e = self._frames = engine(H, W, N, conf_thresh=0.001)
            assert e.pnp_reserve() > 0
            e.load_state_dict(synth.make_state_dict(21, dustbin_bias=7.0))
            e.detect(synth.make_batch(300, N, H, W))
        return self._frames

    def close(self):
        engines = [e for e in (self._pairs, self._frames) if e is not None]
        try:
            assert all(e.check_guards() == 0 for e in engines)
        finally:
            for e in engines:
                e.close()

    def explicit(self, fam, pairs, **params):
        e = self.pairs()
        if (fam, pairs) not in self._inputs:
            self._inputs[fam, pairs] = _pairs(fam, pairs, e.capacity)
        a, b, npairs = self._inputs[fam, pairs]
        kw = dict(params, reproj_threshold=2.0)
        if fam == "pnp":
            kw["K"] = KPAIRS
        out = getattr(e, FAMILIES[fam][2])(a, b, npairs, **kw)
        rec = _model(out, ("R", "t", "ninliers", "mask") if fam == "pnp" else ("model", "ninliers", "mask"))
        rec["inputs"] = _sha(np.concatenate([a.ravel(), b.ravel(), npairs.astype(np.float32)]))
        return rec

    def _plant(self, e, views):
        """The views' pixels and counts in place of the last detect's -> the match table (device, int32 [N,cap])."""
        import torch
        cap = e.capacity
        xy, count = e._points_view()
        hx, hm = np.zeros((N, cap, 2), np.int32), np.full((N, cap), -1, np.int32)
        for f, (pix, match) in enumerate(views):
            hx[f, :len(pix)], hm[f, :len(match)] = pix, match
            hm[f, len(match):len(match) + 8] = 3                                    # rows past the count are never pairs
        xy[:N].copy_(torch.from_numpy(hx))
        count[:N].copy_(torch.tensor([len(v[0]) for v in views], dtype=torch.int32))
        torch.cuda.synchronize()
        return hm, torch.from_numpy(hm).to(e.torch_device)

    def gather(self, name):
        import torch
        e = self.frames()
        cap, dev = e.capacity, e.torch_device
        kxy, key_xyz, valid, views = _world("plane" if name.startswith("homography") else "scene", cap)
        nkey = len(kxy)
        hm, match = self._plant(e, views)
        ransac = dict(iterations=256, seed=11, reproj_threshold=2.0, min_inliers=8)
        pnp = dict(K=KVEC, iterations=256, seed=11, reproj_threshold=3.0, min_inliers=12)
        rec = {"inputs": _sha(np.concatenate([kxy.ravel(), hm.ravel(), np.nan_to_num(key_xyz).ravel().view(np.int32),
                                              np.concatenate([v[0].ravel() for v in views])]))}
        if name.endswith("_frames"):
            if name == "homography_frames":
                rec.update(_model(e.homography_frames(N, match, key_xy=kxy, **ransac)))
            elif name == "fundamental_frames":
                rec.update(_model(e.fundamental_frames(N, match, key_xy=kxy, **ransac)))
            elif name == "pose_frames":                     # reads the gathered rows with a null mask
                fm = e.fundamental_frames_async(N, match, key_xy=kxy, **ransac)[0]
                rm, tv, nf, xyz, front = e.pose_frames(N, match, fm, key_xy=kxy, K_query=KVEC, K_train=KVEC, reproj_threshold=2.0)
                rec.update(_model((rm, tv, nf, front), ("R", "t", "nfront", "front")))
                rec["xyz"] = _sha(np.where(front[..., None], xyz, 0.0).astype(np.float32))
            else:                                           # key_valid clears a tenth of the rows
                rec.update(_model(e.pnp_frames(N, match, key_xyz, valid, **pnp), ("R", "t", "ninliers", "mask")))
            return rec
        # the bank: slots 0 and 1 hold the key's rows, slot 2 its first 300 (matches behind them are no pairs)
        e.bank_create(3, cap)
        try:
            desc = np.random.default_rng(1).normal(size=(nkey, e.desc_dim)).astype(np.float32)
            for s, k in ((0, nkey), (1, nkey), (2, 300)):
                e.bank_store_rows(s, desc[:k], kxy[:k])
            slot = torch.tensor([0, 2, -1], dtype=torch.int32, device=dev)
            if name == "homography_bank":
                rec.update(_model(e.homography_bank(N, slot, match, **ransac)))
            elif name == "fundamental_bank":
                rec.update(_model(e.fundamental_bank(N, slot, match, **ransac)))
            elif name == "homography_bank_topk":            # two problems per frame
                assert e.bank_topk_reserve(2) > 0
                cand = torch.tensor([[0, 1], [2, 0], [1, -1]], dtype=torch.int32, device=dev)
                hm2, ni, mask, pick, best = e.homography_bank_topk(N, cand, match[:, None, :].repeat(1, 2, 1).contiguous(), **ransac)
                rec.update(_model((hm2, ni, mask)))
                rec["pick"], rec["best"] = [int(v) for v in pick], [int(v) for v in best]
            else:
                assert e.bank_landmarks_reserve() > 0
                full_xyz, full_valid = np.ones((cap, 3), np.float32), np.ones(cap, bool)
                full_xyz[:nkey], full_valid[:nkey] = key_xyz, valid
                for s in range(3):
                    e.bank_store_landmarks(s, full_xyz, full_valid if s != 1 else None)
                slot = torch.tensor([1, 2, 0], dtype=torch.int32, device=dev)
                rec.update(_model(e.pnp_bank(N, slot, match, **pnp), ("R", "t", "ninliers", "mask")))
        finally:
            e.bank_destroy()
        return rec


def record(rig, fam, args):
    """What the fixture holds for one case, from the library the package loads."""
    return rig.gather(args) if fam is None else rig.explicit(fam, **args)


@pytest.fixture(scope="module")
def rig():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    r = Rig()
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_ransac_pins(rig, case):
    with open(FIXTURE) as f:
        want = json.load(f)[case[0]]
    got = record(rig, *case[1:])
    assert got["inputs"] == want["inputs"], "%s: the planted inputs differ from the fixture's (numpy?)" % case[0]
    for key in want:
        assert got[key] == want[key], "%s: %s differs from tests/golden/ransac_pins.json" % (case[0], key)
    assert sorted(got) == sorted(want)
