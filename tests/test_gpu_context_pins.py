"""What a context allocates and how many streams it opens, pinned to tests/golden/context_pins.json.

The host code of fpc_create, of the calls that reserve device memory (fpc_bank_create_ex, fpc_bank_topk_reserve,
fpc_pnp_reserve, fpc_bank_landmarks_reserve) and of fpc_bank_destroy can be reorganised without touching a kernel; this
test is what says such a change moved no byte and no stream: per case the streams of fpc_stream_report, the packed size
and the bytes every reserving call reports equal the fixture, a destroyed bank can be reserved again at the same sizes,
and in a FPC_PLAN_GUARD_ZONES context a detect, a bank match, a PnP call and a landmark call leave every canary zone of
all five allocations whole.

The fixture is recorded with tests/golden/make_golden_context.py from the build BEFORE such a change, never from the
changed one."""
import json
import os

import numpy as np
import pytest

import fpc_amd  # noqa: F401
from fpc_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "context_pins.json")
H, W, MAX_BATCH = 32, 48, 4
SLOTS, KMAX = 4, 4
NUM_STREAMS = (0, 1, 2, 3, 5)
K = (40.0, 40.0, 24.0, 16.0)

_cache = {}


def _shared(key, make, *args, **kw):
    if key not in _cache:
        _cache[key] = make(*args, **kw)
    return _cache[key]


def cases():
    return [("guard%d-streams%d" % (guard, ns), bool(guard), ns) for guard in (0, 1) for ns in NUM_STREAMS]


def record(guard, num_streams):
    """What the fixture holds for one case, from the library the package loads; `guards_bad` (never in the fixture) is
    the canary words a guarded context lost to the calls at the end."""
    import torch
    from fpc_amd.engine import Engine

    eng = Engine(H, W, max_batch=MAX_BATCH, num_streams=num_streams, plan_flags=["guard_zones"] if guard else [])
    try:
        rec = {"n_streams": len(eng.stream_report()["streams"]), "packed_size": int(eng.packed_size())}

        def bank(fmt):
            return {"bank": int(eng.bank_create(SLOTS, format=fmt)), "topk": eng.bank_topk_reserve(KMAX),
                    "landmarks": eng.bank_landmarks_reserve()}
        rec["f32"] = bank("f32")
        eng.bank_destroy()
        rec["bf16"] = bank("bf16")
        eng.bank_destroy()
        rec["f32_again"] = bank("f32")              # a destroyed bank and what went with it: reserved again
        rec["pnp"] = eng.pnp_reserve()
        # one call of each chain that uses the five allocations
        eng.load_state_dict(_shared("sd", synth.make_state_dict, seed=0))
        eng.detect(_shared("frames", synth.make_batch, 11, MAX_BATCH, H, W))
        rows, dev = eng.bank_info()["rows"], eng.torch_device
        for slot in range(SLOTS):
            eng.bank_store(slot % MAX_BATCH, slot)
            eng.bank_store_landmarks(slot, torch.from_numpy(np.random.default_rng(slot).uniform(1, 5, (rows, 3)).astype(np.float32)).to(dev))
        score, best, match, dist = eng.match_bank_async(MAX_BATCH, max_dist=1.5)
        rm, tv, ninl, mask = eng.pnp_bank_async(MAX_BATCH, best, match, K=K)
        eng.landmarks_bank_async(MAX_BATCH, best, match, rm, tv, K_query=K, K_train=K)
        eng.match_bank_topk_async(MAX_BATCH, KMAX, max_dist=1.5)
        eng.sync()
        if guard:
            rec["guards_bad"] = eng.check_guards()
    finally:
        eng.close()
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_context_pins(case):
    with open(FIXTURE) as f:
        want = _shared("pins", json.load, f)[case[0]]
    got = record(*case[1:])
    assert got.pop("guards_bad", 0) == 0, "a kernel stored into a canary zone"
    assert got["f32_again"] == got["f32"], "after fpc_bank_destroy the same reservations report other sizes"
    assert got == want, "%s differs from tests/golden/context_pins.json" % case[0]
