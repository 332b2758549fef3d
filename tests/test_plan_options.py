"""The launch-plan options of a context (csrc/plan_options.h), checked without a GPU.

resolve_plan_options is plain C++: tests/plan_options_driver.cc, a stand-alone program that includes nothing but that
header, is compiled with the host compiler and run as a child process with the config on its command line and the
FPC_* variables in ITS environment; it prints every field of the resolved PlanOptions.  `restated` below is the block
of fpc_create that the resolver replaced, line for line and in its order, in Python integers -- the flag first, then the
variable over it, the stream options last.  Stream options change no result bit, so nothing on the GPU sees a wrong
default here: this test is what does."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "feature-point-cnn_amd", "csrc")

F32, BF16, F32_SPLIT, F32_SPLIT_F16 = range(4)
RESNET, VGG = 0, 1
# include/fpc.h
FLAGS = {
    "NO_FUSED_BLOCKS": 1 << 0, "NO_WINOGRAD": 1 << 1, "NO_WINOGRAD_DETECTOR": 1 << 2, "NO_WINOGRAD_LAYER_IN1": 1 << 3,
    "NO_XCD_ORDER": 1 << 4, "NO_FUSED_STEM_POOL": 1 << 5, "SPLIT_HEADS": 1 << 6, "NMS_IN_LINE": 1 << 7,
    "NO_PERSISTENT_GRID": 1 << 8, "LAYER1_TILE_8x16": 1 << 9, "WINOGRAD_GEN1": 1 << 10, "NO_LATENCY_TILES": 1 << 11,
    "NMS_ONE_WORKGROUP": 1 << 12, "NO_FUSED_SOFTMAX": 1 << 13, "WINOGRAD_GEN2": 1 << 14, "GUARD_ZONES": 1 << 15,
    "DETECTOR_GEN1": 1 << 16, "HEADS_IN_LINE": 1 << 17, "W36_ONE_WAVE": 1 << 18, "CONVT_PHASES": 1 << 19,
    "STEM_ROUND3": 1 << 20, "CONV_ROUND1": 1 << 21, "TILES_ROUND5": 1 << 22,
}
VARIABLES = (
    "FPC_GUARD_ZONES", "FPC_W36_PAIRED", "FPC_TILES_ROUND6", "FPC_W36_CUS", "FPC_WINOGRAD_DET_GEN", "FPC_CONV_LEAN",
    "FPC_STEM_LEAN", "FPC_WINOGRAD_GEN", "FPC_LATENCY_TILES", "FPC_CONVT_FUSED", "FPC_FUSE_SOFTMAX", "FPC_NMS_CHUNKED",
    "FPC_STREAMS", "FPC_FUSE", "FPC_WINOGRAD", "FPC_XCD_ORDER", "FPC_MIN_SUB", "FPC_PERSIST_MIN", "FPC_WINOGRAD_DET",
    "FPC_WINOGRAD_IN1", "FPC_FUSE_STEM", "FPC_NMS_PASSES", "FPC_NMS_G", "FPC_L1_T816", "FPC_SPLIT_HEADS", "FPC_NMS_ASIDE",
    "FPC_BF16_GRID",
)
# each flag with the variable that sets the same option, and the value of it that means the OTHER way
FLAG_AGAINST_VARIABLE = (
    ("NO_FUSED_BLOCKS", "FPC_FUSE", "1"), ("NO_WINOGRAD", "FPC_WINOGRAD", "1"), ("NO_WINOGRAD_DETECTOR", "FPC_WINOGRAD_DET", "1"),
    ("NO_WINOGRAD_LAYER_IN1", "FPC_WINOGRAD_IN1", "1"), ("NO_XCD_ORDER", "FPC_XCD_ORDER", "1"),
    ("NO_FUSED_STEM_POOL", "FPC_FUSE_STEM", "1"), ("SPLIT_HEADS", "FPC_SPLIT_HEADS", "0"), ("HEADS_IN_LINE", "FPC_SPLIT_HEADS", "1"),
    ("NMS_IN_LINE", "FPC_NMS_ASIDE", "1"), ("NO_PERSISTENT_GRID", "FPC_PERSIST_MIN", "1"), ("WINOGRAD_GEN1", "FPC_WINOGRAD_GEN", "3"),
    ("WINOGRAD_GEN2", "FPC_WINOGRAD_GEN", "3"), ("NO_LATENCY_TILES", "FPC_LATENCY_TILES", "1"),
    ("NMS_ONE_WORKGROUP", "FPC_NMS_CHUNKED", "1"), ("NO_FUSED_SOFTMAX", "FPC_FUSE_SOFTMAX", "1"), ("GUARD_ZONES", "FPC_GUARD_ZONES", "0"),
    ("DETECTOR_GEN1", "FPC_WINOGRAD_DET_GEN", "3"), ("W36_ONE_WAVE", "FPC_W36_PAIRED", "1"), ("CONVT_PHASES", "FPC_CONVT_FUSED", "1"),
    ("STEM_ROUND3", "FPC_STEM_LEAN", "1"), ("CONV_ROUND1", "FPC_CONV_LEAN", "1"), ("TILES_ROUND5", "FPC_TILES_ROUND6", "1"),
    # (FPC_L1_T816 cannot say "off": its presence turns the option on -- test_quirks)
)


def atoi(text):
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def restated(dtype=F32, arch=RESNET, num_streams=0, pf=0, nms_round_launches=0, min_sub_batch=0, env=None):
    """fpc_create's option block as it stood before plan_options.h, statement by statement."""
    env = env or {}
    get = env.get
    vgg, bf16, split = arch == VGG, dtype == BF16, dtype in (F32_SPLIT, F32_SPLIT_F16)
    on = lambda name: bool(pf & FLAGS[name])                                             # noqa: E731
    # the defaults of fpc_ctx's members
    o = dict(nms_aside=1, split_heads=0, min_sub=8, persist_min_tiles=1, xcd_order=1, nms_passes=2, fuse_softmax=1,
             convt_fused=1, nms_one_workgroup=0, nms_g=0, fuse_stem_pool=1, conv_lean=1, stem_lean=1, stem2=0, layer1_t816=0,
             winograd_in1=1, winograd_det=1, w36_cus=0, tiles_round6=1, w36_paired=1, winograd_det_gen3=1, winograd=1,
             latency_tiles=1, winograd_gen=3, fuse_blocks=1, guard_zones=0, bf16_grid=0)
    nsub = min(8, num_streams) if num_streams > 0 else (3 if split else 2)
    o["fuse_blocks"] = not on("NO_FUSED_BLOCKS")
    o["guard_zones"] = on("GUARD_ZONES")
    if get("FPC_GUARD_ZONES") is not None: o["guard_zones"] = atoi(get("FPC_GUARD_ZONES")) != 0
    o["winograd_det_gen3"] = not on("DETECTOR_GEN1")
    o["w36_paired"] = not on("W36_ONE_WAVE")
    if get("FPC_W36_PAIRED") is not None: o["w36_paired"] = atoi(get("FPC_W36_PAIRED")) != 0
    o["tiles_round6"] = not on("TILES_ROUND5")
    if get("FPC_TILES_ROUND6") is not None: o["tiles_round6"] = atoi(get("FPC_TILES_ROUND6")) != 0
    if get("FPC_W36_CUS") is not None: o["w36_cus"] = max(0, atoi(get("FPC_W36_CUS")))
    if get("FPC_BF16_GRID") is not None: o["bf16_grid"] = max(0, atoi(get("FPC_BF16_GRID")))      # (added with the option)
    if get("FPC_WINOGRAD_DET_GEN") is not None: o["winograd_det_gen3"] = atoi(get("FPC_WINOGRAD_DET_GEN")) >= 3
    o["winograd"] = not on("NO_WINOGRAD")
    o["winograd_det"] = not on("NO_WINOGRAD_DETECTOR")
    o["winograd_in1"] = not on("NO_WINOGRAD_LAYER_IN1")
    o["xcd_order"] = not on("NO_XCD_ORDER")
    o["fuse_stem_pool"] = not on("NO_FUSED_STEM_POOL")
    o["stem_lean"] = not on("STEM_ROUND3")
    o["conv_lean"] = not on("CONV_ROUND1")
    if get("FPC_CONV_LEAN") is not None: o["conv_lean"] = atoi(get("FPC_CONV_LEAN")) != 0
    if get("FPC_STEM_LEAN") is not None: o["stem_lean"] = atoi(get("FPC_STEM_LEAN")) != 0
    o["split_heads"] = on("SPLIT_HEADS")
    if on("NO_PERSISTENT_GRID"): o["persist_min_tiles"] = 0
    o["layer1_t816"] = on("LAYER1_TILE_8x16")
    o["winograd_gen"] = 1 if on("WINOGRAD_GEN1") else 2 if on("WINOGRAD_GEN2") else 3
    if get("FPC_WINOGRAD_GEN") is not None: o["winograd_gen"] = min(3, max(1, atoi(get("FPC_WINOGRAD_GEN"))))
    o["latency_tiles"] = not on("NO_LATENCY_TILES")
    if get("FPC_LATENCY_TILES") is not None: o["latency_tiles"] = atoi(get("FPC_LATENCY_TILES")) != 0
    o["fuse_softmax"] = not on("NO_FUSED_SOFTMAX")
    o["convt_fused"] = not on("CONVT_PHASES")
    if get("FPC_CONVT_FUSED") is not None: o["convt_fused"] = atoi(get("FPC_CONVT_FUSED")) != 0
    if get("FPC_FUSE_SOFTMAX") is not None: o["fuse_softmax"] = atoi(get("FPC_FUSE_SOFTMAX")) != 0
    o["nms_one_workgroup"] = on("NMS_ONE_WORKGROUP")
    if get("FPC_NMS_CHUNKED") is not None: o["nms_one_workgroup"] = atoi(get("FPC_NMS_CHUNKED")) == 0
    if min_sub_batch > 0: o["min_sub"] = min_sub_batch
    if nms_round_launches > 0: o["nms_passes"] = min(64, nms_round_launches)
    elif nms_round_launches < 0: o["nms_passes"] = 0
    if get("FPC_STREAMS") is not None: nsub = max(1, min(8, atoi(get("FPC_STREAMS"))))
    if not on("HEADS_IN_LINE") and nsub >= 2 and not vgg and not bf16 and not split: o["split_heads"] = True
    if get("FPC_FUSE") is not None: o["fuse_blocks"] = atoi(get("FPC_FUSE")) != 0
    if get("FPC_WINOGRAD") is not None: o["winograd"] = atoi(get("FPC_WINOGRAD")) != 0
    if get("FPC_XCD_ORDER") is not None: o["xcd_order"] = atoi(get("FPC_XCD_ORDER")) != 0
    if get("FPC_MIN_SUB") is not None: o["min_sub"] = max(1, atoi(get("FPC_MIN_SUB")))
    if get("FPC_PERSIST_MIN") is not None: o["persist_min_tiles"] = atoi(get("FPC_PERSIST_MIN"))
    if get("FPC_WINOGRAD_DET") is not None: o["winograd_det"] = atoi(get("FPC_WINOGRAD_DET")) != 0
    if get("FPC_WINOGRAD_IN1") is not None: o["winograd_in1"] = atoi(get("FPC_WINOGRAD_IN1")) != 0
    if get("FPC_FUSE_STEM") is not None: o["fuse_stem_pool"] = atoi(get("FPC_FUSE_STEM")) != 0
    if get("FPC_NMS_PASSES") is not None: o["nms_passes"] = max(0, min(64, atoi(get("FPC_NMS_PASSES"))))
    if get("FPC_NMS_G") is not None: o["nms_g"] = max(0, min(64, atoi(get("FPC_NMS_G"))))
    if get("FPC_L1_T816") is not None: o["layer1_t816"] = True
    if get("FPC_SPLIT_HEADS") is not None: o["split_heads"] = atoi(get("FPC_SPLIT_HEADS")) != 0
    o["nms_aside"] = not split
    if on("NMS_IN_LINE"): o["nms_aside"] = False
    if get("FPC_NMS_ASIDE") is not None: o["nms_aside"] = atoi(get("FPC_NMS_ASIDE")) != 0
    if o["split_heads"]: o["nms_aside"] = False
    o["nsub"] = nsub
    o["nside"] = nsub if 2 * nsub <= 4 else 1
    return {k: int(v) for k, v in o.items()}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_options") / "plan_options_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-o", exe, os.path.join(HERE, "plan_options_driver.cc")],
                   check=True)
    return exe


def resolved(driver, dtype=F32, arch=RESNET, num_streams=0, pf=0, nms_round_launches=0, min_sub_batch=0, env=None):
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("FPC_")}
    child_env.update(env or {})
    out = subprocess.run([driver] + [str(v) for v in (dtype, arch, num_streams, pf, nms_round_launches, min_sub_batch)],
                         env=child_env, check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split("=") for line in out.split())}


def check(driver, **case):
    got, want = resolved(driver, **case), restated(**case)
    assert got == want, (case, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
    return got


def test_defaults(driver):
    got = check(driver)
    assert got["nsub"] == 2 and got["nside"] == 2 and got["split_heads"] == 1 and got["nms_aside"] == 0
    assert got["min_sub"] == 8 and got["nms_passes"] == 2 and got["winograd_gen"] == 3 and got["persist_min_tiles"] == 1
    assert len(got) == 29 and got["bf16_grid"] == 0


@pytest.mark.parametrize("flag", sorted(FLAGS))
def test_every_flag_alone(driver, flag):
    moved = False
    for arch in (RESNET, VGG):       # (the Python network splits its heads by default: two of the flags show on the other)
        moved |= check(driver, arch=arch, pf=FLAGS[flag]) != resolved(driver, arch=arch)
    assert moved, flag


@pytest.mark.parametrize("name", VARIABLES)
@pytest.mark.parametrize("value", ("0", "1", "99", "-7", "x"))
def test_every_variable_alone(driver, name, value):
    check(driver, env={name: value})
    check(driver, dtype=F32_SPLIT, env={name: value})


@pytest.mark.parametrize("flag,name,value", FLAG_AGAINST_VARIABLE)
def test_variable_overrides_its_flag(driver, flag, name, value):
    # (on the C++ network, whose heads are in line by default, so that every one of these pairs shows)
    alone = check(driver, arch=VGG, pf=FLAGS[flag])
    both = check(driver, arch=VGG, pf=FLAGS[flag], env={name: value})
    assert both != alone, (flag, name, value)
    assert both == check(driver, arch=VGG, env={name: value}), "the variable decides, whatever the flag says"


def test_quirks(driver):
    # FPC_L1_T816: its presence turns the option on, whatever its value
    for v in ("0", "1", "", "no"):
        assert check(driver, env={"FPC_L1_T816": v})["layer1_t816"] == 1
    # FPC_NMS_CHUNKED names the opposite of the field
    assert check(driver, env={"FPC_NMS_CHUNKED": "0"})["nms_one_workgroup"] == 1
    assert check(driver, pf=FLAGS["NMS_ONE_WORKGROUP"], env={"FPC_NMS_CHUNKED": "1"})["nms_one_workgroup"] == 0
    # FPC_WINOGRAD_DET_GEN: generation 3 from 3 up
    for v, want in (("1", 0), ("2", 0), ("3", 1), ("4", 1), ("0", 0)):
        assert check(driver, env={"FPC_WINOGRAD_DET_GEN": v})["winograd_det_gen3"] == want
    # FPC_WINOGRAD_GEN clamped to 1..3 over the flags; the gen1 flag wins over the gen2 flag
    for v, want in (("0", 1), ("-4", 1), ("1", 1), ("2", 2), ("3", 3), ("9", 3)):
        assert check(driver, env={"FPC_WINOGRAD_GEN": v})["winograd_gen"] == want
        assert check(driver, pf=FLAGS["WINOGRAD_GEN1"] | FLAGS["WINOGRAD_GEN2"], env={"FPC_WINOGRAD_GEN": v})["winograd_gen"] == want
    assert check(driver, pf=FLAGS["WINOGRAD_GEN1"] | FLAGS["WINOGRAD_GEN2"])["winograd_gen"] == 1
    assert check(driver, pf=FLAGS["WINOGRAD_GEN2"])["winograd_gen"] == 2
    # FPC_PERSIST_MIN unclamped
    for v in ("-3", "0", "7", "100000"):
        assert check(driver, env={"FPC_PERSIST_MIN": v})["persist_min_tiles"] == int(v)
    assert check(driver, pf=FLAGS["NO_PERSISTENT_GRID"])["persist_min_tiles"] == 0
    # FPC_MIN_SUB at least 1, over min_sub_batch
    for v, want in (("0", 1), ("-2", 1), ("1", 1), ("5", 5), ("1000", 1000)):
        assert check(driver, min_sub_batch=3, env={"FPC_MIN_SUB": v})["min_sub"] == want
    assert check(driver, min_sub_batch=3)["min_sub"] == 3 and check(driver, min_sub_batch=-1)["min_sub"] == 8
    # FPC_NMS_PASSES, FPC_NMS_G: 0..64
    for name, field in (("FPC_NMS_PASSES", "nms_passes"), ("FPC_NMS_G", "nms_g")):
        for v, want in (("-1", 0), ("0", 0), ("3", 3), ("64", 64), ("65", 64)):
            assert check(driver, nms_round_launches=5, env={name: v})[field] == want
    # nms_round_launches: a positive value capped at 64, a negative one gives 0
    for v, want in ((0, 2), (1, 1), (64, 64), (65, 64), (1000, 64), (-1, 0), (-9, 0)):
        assert check(driver, nms_round_launches=v)["nms_passes"] == want
    # FPC_W36_CUS at least 0
    for v, want in (("-8", 0), ("0", 0), ("96", 96)):
        assert check(driver, env={"FPC_W36_CUS": v})["w36_cus"] == want
    # FPC_BF16_GRID at least 0
    for v, want in (("-8", 0), ("0", 0), ("8", 8), ("16", 16), ("1000000", 1000000)):
        assert check(driver, dtype=BF16, env={"FPC_BF16_GRID": v})["bf16_grid"] == want
    # FPC_STREAMS clamped to 1..8, over num_streams
    for v, want in (("0", 1), ("-1", 1), ("1", 1), ("4", 4), ("8", 8), ("9", 8)):
        assert check(driver, num_streams=3, env={"FPC_STREAMS": v})["nsub"] == want


@pytest.mark.parametrize("arch", (RESNET, VGG))
@pytest.mark.parametrize("dtype", (F32, BF16, F32_SPLIT, F32_SPLIT_F16))
def test_stream_options(driver, arch, dtype):
    """nsub, split_heads, nms_aside and nside over num_streams 0..9 and the three flags that steer them."""
    steering = ("HEADS_IN_LINE", "SPLIT_HEADS", "NMS_IN_LINE")
    for num_streams in range(10):
        for picked in itertools.product((0, 1), repeat=3):
            pf = sum(FLAGS[f] for f, p in zip(steering, picked) if p)
            got = check(driver, dtype=dtype, arch=arch, num_streams=num_streams, pf=pf)
            # the rules, once more in words
            nsub = min(8, num_streams) if num_streams > 0 else 3 if dtype in (F32_SPLIT, F32_SPLIT_F16) else 2
            assert got["nsub"] == nsub and got["nside"] == (nsub if nsub <= 2 else 1)
            default_split = not picked[0] and nsub >= 2 and arch == RESNET and dtype == F32
            assert got["split_heads"] == int(bool(picked[1] or default_split))
            assert got["nms_aside"] == int(not got["split_heads"] and not picked[2] and dtype in (F32, BF16))
    # the variables over all of it: FPC_STREAMS is the nsub that split_heads sees; split_heads is what nms_aside sees
    for env in ({"FPC_STREAMS": "1"}, {"FPC_STREAMS": "2"}, {"FPC_SPLIT_HEADS": "0"}, {"FPC_SPLIT_HEADS": "1"},
                {"FPC_NMS_ASIDE": "1"}, {"FPC_NMS_ASIDE": "0"}, {"FPC_SPLIT_HEADS": "1", "FPC_NMS_ASIDE": "1"},
                {"FPC_SPLIT_HEADS": "0", "FPC_NMS_ASIDE": "1"}, {"FPC_STREAMS": "1", "FPC_NMS_ASIDE": "1"}):
        for num_streams in (0, 1, 3):
            got = check(driver, dtype=dtype, arch=arch, num_streams=num_streams, env=env)
            assert not (got["split_heads"] and got["nms_aside"])


def test_bf16_persistent_grid(driver):
    """bf16_persistent_grid(tiles, resident, parts, cap): cap 0 is the rule as it stood -- min(ceil8(T), max(8, resident /
    parts / 8 * 8)) -- and a cap stands in for `resident`, never below 8 per part, always a multiple of 8."""
    def grid(tiles, resident, parts, cap):
        out = subprocess.run([driver, "grid"] + [str(v) for v in (tiles, resident, parts, cap)], check=True, capture_output=True,
                             text=True).stdout
        return int(out)

    for tiles in (1, 7, 8, 9, 50, 175, 512, 513, 5000):
        for resident in (256, 512, 768):
            for parts in (1, 2):
                old = min((tiles + 7) // 8 * 8, max(8, resident // parts // 8 * 8))
                assert grid(tiles, resident, parts, 0) == old
                for cap in (1, 8, 15, 16, 17, 24, 100000):
                    want = min((tiles + 7) // 8 * 8, max(8, cap // parts // 8 * 8))
                    assert grid(tiles, resident, parts, cap) == want and want % 8 == 0 and want >= 8
    assert grid(175, 512, 1, 8) == 8 and grid(175, 512, 1, 16) == 16 and grid(10, 512, 2, 8) == 8 and grid(10, 512, 2, 16) == 8
