"""bench.py's plain run and --dump-outputs: the arrays it writes (CPU, with a stand-in engine) and, on the GPU, that a
plain run writes what Engine.detect returns for the same seeded frames and checkpoint, and nothing of --full."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FetchOnly:
    """Engine.fetch's return value without a GPU: per frame (xy int32 [K,2], conf float32 [K], desc float32 [K,D] or
    None, candidates)."""

    def __init__(self, counts, desc_dim=128, seed=0):
        rng = np.random.default_rng(seed)
        self.res = [(rng.integers(0, 640, (k, 2)).astype(np.int32), rng.random(k, np.float32),
                     rng.random((k, desc_dim), np.float32) if desc_dim else None, 2 * k) for k in counts]

    def fetch(self, n):
        assert n == len(self.res)
        return self.res


def test_dump_outputs_writes_the_fetched_arrays(tmp_path):
    bench = _bench_module()
    eng = FetchOnly([3, 0, 5])
    bench.dump_outputs(str(tmp_path), eng, 3)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["candidates_per_frame", "descriptor_rows", "descriptors", "keypoints_conf",
                           "keypoints_per_frame", "keypoints_xy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["keypoints_per_frame"], [3, 0, 5])
    np.testing.assert_array_equal(got["candidates_per_frame"], [6, 0, 10])
    np.testing.assert_array_equal(got["keypoints_xy"], np.concatenate([r[0] for r in eng.res]))
    np.testing.assert_array_equal(got["keypoints_conf"], np.concatenate([r[1] for r in eng.res]))
    np.testing.assert_array_equal(got["descriptor_rows"], np.arange(8))
    np.testing.assert_array_equal(got["descriptors"], np.concatenate([r[2] for r in eng.res]))


def test_dump_outputs_samples_descriptors_within_the_budget(tmp_path):
    """32 VGA frames carry ~4 000 keypoints each: all their descriptors would exceed 64 MB, so a seeded sample of the
    rows is written -- the same rows on every run with the same number of keypoints."""
    bench = _bench_module()
    eng = FetchOnly([4100] * 32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, 32)
    rows = np.load(tmp_path / "a" / "descriptor_rows.npy")
    assert rows.shape == (bench.DUMP_DESC_ROWS,) and np.all(np.diff(rows) > 0) and rows[-1] < 4100 * 32
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "descriptor_rows.npy"))
    desc = np.concatenate([r[2] for r in eng.res])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "descriptors.npy"), desc[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    eng = FetchOnly([10, 20], desc_dim=0)                     # detector only (MagicPoint): no descriptors
    bench.dump_outputs(str(tmp_path / "c"), eng, 2)
    assert not os.path.exists(tmp_path / "c" / "descriptors.npy")


@pytest.mark.gpu
def test_plain_run_dumps_what_detect_returns(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`: one line with the headline fields and none of
    --full's passes; the dumped keypoints are Engine.detect's on the bench's seeded frames and checkpoint."""
    import torch
    from fpc_amd.engine import Engine
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "frames/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    for k in ("roofline", "steady_state", "single_context", "latency_b1", "host_fed", "other_workloads", "cpu_baseline"):
        assert k not in out, k
    e = Engine(480, 640, max_batch=32, num_streams=1)          # the headline's plan: one sub-batch per context
    e.load_state_dict(synth.make_state_dict(0, dustbin_bias=7.0))
    res = e.detect(synth.make_batch(100, 32, 480, 640))
    e.close()
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    np.testing.assert_array_equal(got["keypoints_per_frame"], [len(r_[1]) for r_ in res])
    np.testing.assert_array_equal(got["candidates_per_frame"], [r_[3] for r_ in res])
    np.testing.assert_array_equal(got["keypoints_xy"], np.concatenate([r_[0] for r_ in res]))
    np.testing.assert_array_equal(got["keypoints_conf"], np.concatenate([r_[1] for r_ in res]))
    desc = np.concatenate([r_[2] for r_ in res])[got["descriptor_rows"].astype(np.int64)]
    np.testing.assert_allclose(got["descriptors"], desc, rtol=0, atol=1e-6)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
