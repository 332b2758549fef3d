"""CPU checks of the bf16 key-frame bank (fpc_bank_create_ex / fpc_bank_format, include/fpc.h): the two entry points exist,
refuse a NULL context and are declared by the binding, and `bank_rule_bf16` -- tests/test_match_bank.py's float64 `bank_rule`
on inputs rounded to bf16 (round to nearest even), the restatement the GPU tests (test_gpu_match_bank_bf16.py) hold the
kernels to -- ranks the slots of planted data exactly as the fp32 rule does under max_dist or a ratio."""
import ctypes
import os
import re
import subprocess

import numpy as np

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_match_bank import bank_rule, planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPC_E_INVALID = -1
BANK_F32, BANK_BF16 = 0, 1
# (cross_check, max_dist, ratio): the option sets the header recommends.  NOT the bare cross check: it does not tell slots
# apart (the header's warning), and the two formats differ there.
OPTIONS = ((True, 0.7, 0.0), (False, 0.7, 0.0), (True, 0.0, 0.8), (False, 0.0, 0.8))


def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even; a NaN -> 0x7FC0."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC0
    return r


def bf16_round(x):
    """float32 array -> float32 array of the values bf16 storage keeps."""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def bank_rule_bf16(desc, counts, slots, cross_check=True, max_dist=0.0, ratio=0.0, min_score=0):
    """bank_rule on the rounded rows (float64 arithmetic on exactly the values the device stores)."""
    return bank_rule(bf16_round(desc), counts, [bf16_round(t) for t in slots], cross_check, max_dist, ratio, min_score)


def test_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 3.4e38, np.inf, np.nan, 0.0, -0.0, 1e-40], np.float32)
    #             exact  tie -> even (down)  tie -> even (up)  tie, negative   fits   overflows -> inf
    got = bf16_bits(x)
    assert list(got[:7]) == [0x3F80, 0x3F80, 0x3F82, 0xBF80, 0x7F62, 0x7F80, 0x7F80]
    assert got[7] == 0x7FC0 and got[8] == 0 and got[9] == 0x8000
    import torch
    rng = np.random.Generator(np.random.PCG64(3))
    v = np.concatenate([rng.normal(size=4096).astype(np.float32), x[~np.isnan(x)]])   # (what a NaN becomes is the library's choice)
    want = torch.from_numpy(v).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(bf16_bits(v), want)


def test_entry_points_refuse_a_null_context():
    lib = _lib.load()
    fmt = ctypes.c_int(-7)
    ptr = ctypes.c_void_p(0x1234)
    assert lib.fpc_bank_create_ex(None, 4, 16, BANK_F32) == FPC_E_INVALID
    assert lib.fpc_bank_create_ex(None, 4, 16, BANK_BF16) == FPC_E_INVALID
    assert lib.fpc_bank_format(None, ctypes.byref(fmt), ctypes.byref(ptr)) == FPC_E_INVALID
    assert fmt.value == -7 and ptr.value == 0x1234                 # nothing was written


def test_header_binding_and_library_agree():
    lib = _lib.load()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert lib.fpc_bank_create_ex.argtypes == [vp, ci, ci, ci]
    assert lib.fpc_bank_format.argtypes == [vp, ctypes.POINTER(ci), ctypes.POINTER(vp)]
    assert lib.fpc_bank_create.argtypes == [vp, ci, ci]            # unchanged
    hdr = open(os.path.join(ROOT, "include", "fpc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = ("fpc_bank_create_ex", "fpc_bank_format")
    for name in names:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"#define FPC_BANK_F32\s+0\b", code) and re.search(r"#define FPC_BANK_BF16\s+1\b", code)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(names) <= set(re.findall(r" T (fpc_[a-z_0-9]+)", out))
    assert int(re.search(r"#define FPC_ABI_VERSION (\d+)", hdr).group(1)) == 4 and lib.fpc_abi_version() == 4
    from fpc_amd.engine import Engine
    assert Engine.BANK_FORMATS == {"f32": BANK_F32, "bf16": BANK_BF16}
    import inspect
    assert inspect.signature(Engine.bank_create).parameters["format"].default == "f32"


def test_bf16_rule_ranks_planted_slots_as_the_fp32_rule_does():
    desc, counts, slots, origin = planted(seed=7)
    for cross, md, ratio in OPTIONS:
        score, best, match, d1 = bank_rule(desc, counts, slots, cross, md, ratio)
        score16, best16, match16, d16 = bank_rule_bf16(desc, counts, slots, cross, md, ratio)
        fin = np.isfinite(d1)
        assert (fin == np.isfinite(d16)).all()
        moved = float(np.abs(d1[fin] - d16[fin]).max())
        print("options", (cross, md, ratio), "score difference", int(np.abs(score - score16).max()),
              "nearest distance moves by at most", moved)
        np.testing.assert_array_equal(score16, score)
        np.testing.assert_array_equal(best16, best)
        np.testing.assert_array_equal(best16, origin)              # the planted slot is recovered
        np.testing.assert_array_equal(match16, match)
        # bf16 keeps 8 significant bits: a unit row moves by at most 2^-9 in norm, a distance by at most twice that
        assert moved <= 2 * 2.0 ** -9
        for f, s in enumerate(origin):
            assert (match16[f, :counts[f]] >= 0).sum() == score16[f, s]
        assert (score16[:, 5] == 0).all()                          # the empty slot
