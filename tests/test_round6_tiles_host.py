"""Round 6, CPU suite: the plan's tile choices (fpc_tile_choice: the library's own choice functions, no device needed)
and the new entry points in the SHIPPED gfx950 code object -- wblock36s_kernel<2, 4, 4> (the stacked walk) and
wconv36p_kernel<8, 2, 3> (conv-only, 8 x 2 Winograd tiles) -- with the scanner of tests/test_static_isa.py: the
128-channel body keeps all sixteen MFMAs of a step inside one asm statement, and that scan is what makes it safe.
"""
import re

import fpc_amd  # noqa: F401
from fpc_amd import _lib

from tests.test_static_isa import _back_edges, _chunk_loop, _scan, code_object  # noqa: F401  (code_object: the fixture)

R5 = _lib.PLAN_FLAGS["tiles_round5"]


def choice(what, h, w, frames=1, flags=0):
    return _lib.load().fpc_tile_choice(what, h, w, frames, flags)


def test_plan_flag_is_declared_everywhere():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fpc.h")).read()
    assert re.search(r"FPC_PLAN_TILES_ROUND5 = 1 << 22\b", hdr)
    assert R5 == 1 << 22 and list(_lib.PLAN_FLAGS.values()).count(R5) == 1
    assert "FPC_PLAN_TILES_ROUND5" in open(os.path.join(root, "INTEGRATION.md")).read()


def test_stacked_walk_is_chosen_only_where_it_needs_fewer_tile_rows():
    # 60-row maps: 18.75 tile rows per frame instead of 20 -- 16 frames (a sub-batch of the headline) 60 instead of 64,
    # 32 frames 120 instead of 128; one to three frames are as many rows either way
    assert [choice(0, 60, 80, n) for n in (1, 2, 3, 4, 16, 32)] == [0, 0, 0, 15, 60, 120]
    # 20 x 24 maps are 3 tiles of 8 x 32 per frame: stacked on 16 x 16 (two tile columns) 3 frames are 8 tiles instead of 9,
    # 5 frames 14 instead of 15, 7 frames 18 instead of 21; one or two frames are no fewer
    assert [choice(0, 20, 24, n) for n in (1, 2, 3, 4, 5, 7)] == [0, 0, 4, 5, 7, 9]
    # 28-row maps: 3 frames are 6 rows either way, 4 frames 7 instead of 8
    assert [choice(0, 28, 24, n) for n in (3, 4)] == [0, 7]
    # heights that are a multiple of 16 (nothing to gain), no multiple of 4 (a Winograd tile would straddle a seam) or
    # under 16 (two seams in a tile) stay frame by frame; so does everything under tiles_round5
    for hf in (16, 32, 64, 30, 22, 12, 8):
        assert choice(0, hf, 40, 32) == 0, hf
    assert choice(0, 60, 80, 32, R5) == 0


def test_conv_8x2_is_chosen_only_where_it_needs_fewer_tiles():
    assert choice(1, 30, 40) == 3208          # 5 tiles against 6 (4 x 4) and 8 (2 x 8)
    assert choice(1, 18, 8) == 3208           # 1 against 2 and 3
    assert choice(1, 30, 8) == 3208           # 1 against 2 and 4
    assert choice(1, 14, 10) == 1616          # 2 against 1
    assert choice(1, 32, 16) == 1616          # 2 against 2: a tie keeps round 5's choice
    assert choice(1, 8, 64) == 832            # round 5's 2 x 8 where it wins
    assert choice(1, 30, 40, 1, R5) == 1616 and choice(1, 18, 8, 1, R5) == 1616


def test_block_4x16_is_chosen_only_where_it_issues_fewer_rows():
    assert choice(2, 60, 80) == 416           # 75 tiles of 64 rows against 80
    assert choice(2, 22, 26) == 416           # 6 x 2 against 8 x 2
    assert choice(2, 8, 12) == 416            # 2 against 3
    assert choice(2, 6, 20) == 320            # 2 x 2 against 2 x 1
    assert choice(2, 9, 20) == 320            # 3 x 2 against 3 x 1: more tiles
    assert choice(2, 12, 80) == 416           # 3 x 5 against 4 x 4
    assert choice(2, 3, 16) == 320            # 1 against 1: a tie keeps round 5's choice
    assert choice(2, 60, 80, 1, R5) == 320
    assert choice(3, 60, 80) < 0 and choice(0, 0, 80) < 0


# What DESIGN.md section 3.1 ("Round 6") states, as measured with -Rpass-analysis=kernel-resource-usage:
# (sgpr_spill_count max, vgpr_spill_count max, private_segment_fixed_size max, MFMAs per chunk loop, chunk loops)
NEW_ENTRY_POINTS = {
    "_ZN3fpc16wblock36s_kernelILi2ELi4ELi4EEEvNS_10WBlockArgsE": (96, 0, 0, 2 * 36 * 4 * 2, 1),
    "_ZN3fpc15wconv36p_kernelILi8ELi2ELi3EEEvNS_10WBlockArgsE": (0, 0, 0, 2 * 18 * 4, 2),
}


def test_new_entry_points_exist_and_use_only_the_8_pass_mfma(code_object):
    funcs, _ = code_object
    for name in NEW_ENTRY_POINTS:
        assert name in funcs, name
        ops = {i.split()[0] for _, i in funcs[name] if i.startswith("v_mfma")}
        assert ops == {"v_mfma_f32_16x16x4_f32"}, (name, ops)
    # exactly these: no other instance of the two new templates rides along
    new = [n for n in funcs if re.match(r"_ZN3fpc(16wblock36s_kernel|15wconv36p_kernel)I", n)]
    assert sorted(new) == sorted(NEW_ENTRY_POINTS), new


def test_new_entry_points_touch_no_mfma_result_too_early(code_object):
    """(i) of tests/test_static_isa.py: straight line and every back edge."""
    funcs, _ = code_object
    for name in NEW_ENTRY_POINTS:
        body = funcs[name]
        seq = [i for _, i in body]
        bad = _scan(seq)
        assert not bad, "%s: %s" % (name, [(seq[j], ins, ws) for _, ins, j, ws in bad[:5]])
        edges = _back_edges(body)
        assert len(edges) >= 2, (name, edges)          # the chunk loop(s) and the tile loop at least
        for head, k in edges:
            bad = _scan(seq[max(0, k - 40):k] + seq[head:head + 40])
            assert not bad, "%s back edge at %d: %s" % (name, k, bad[:3])


def test_new_entry_points_spill_what_design_md_says_and_nothing_inside_a_chunk_loop(code_object):
    """(ii) of tests/test_static_isa.py."""
    funcs, meta = code_object
    for name, (s_max, v_max, p_max, n_mfma, n_loops) in NEW_ENTRY_POINTS.items():
        m, body = meta[name], funcs[name]
        assert m["sgpr_spill_count"] <= s_max, (name, m)
        assert m["vgpr_spill_count"] <= v_max, (name, m)
        assert m["private_segment_fixed_size"] <= p_max, (name, m)
        assert not [i for _, i in body if i.startswith("scratch_")], name
        loop = _chunk_loop(body)
        assert loop is not None and loop[2] == n_mfma, (name, loop)
        edges = _back_edges(body)
        loops = [(h, k) for h, k in edges
                 if sum(1 for _, i in body[h:k] if i.startswith("v_mfma")) == n_mfma
                 and not any(h2 >= h and k2 <= k and (h2, k2) != (h, k) for h2, k2 in edges)]
        assert len(loops) == n_loops, (name, loops)
        for h, k in loops:
            inside = [i for _, i in body[h:k] if i.startswith(("v_readlane", "v_writelane", "scratch_"))]
            assert not inside, (name, inside[:5])
        if "wconv36p" in name:
            assert m["agpr_count"] == 0 and m["vgpr_count"] <= 256, (name, m)


def test_round6_block_instance_keeps_its_registers(code_object):
    """block_mfma_kernel<4, 16, 2, 32, 1, 4, 2, 1, 128> (layer2.0): two workgroups per CU as the 3 x 20 instance it replaces --
    no more than 256 registers, nothing spilled, nothing in scratch."""
    funcs, meta = code_object
    name = "_ZN3fpc17block_mfma_kernelILi4ELi16ELi2ELi32ELi1ELi4ELi2ELi1ELi128EEEvNS_9BlockArgsE"
    assert name in funcs
    m = meta[name]
    assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert not [i for _, i in funcs[name] if i.startswith("scratch_")]
