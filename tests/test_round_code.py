"""The round code around the walk of stage 2 (trace_bvh_spheres_kernel<false, 2, 2>: the refill from the survivors' queue, the set-up of
the walk's ray, one iteration of the exact loop, the shading block), counted in the ISA without a GPU by tools/isa_round_count.py: the
figures the product build reached, with those of the parent commit (2fd0e97, counted by the same tool) beside them.  What a region is
and what a column counts stands at the head of the tool.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_round_count.py --json on the parent commit
PARENT = {
    "refill": {"valu": 149, "f64": 3, "quarter": 31, "v_mov": 36, "salu": 41, "s_load": 19, "global": 6, "flat": 3, "scratch": 2, "lds": 0, "waitcnt": 21, "branches": 12},
    "setup": {"valu": 257, "f64": 151, "quarter": 8, "v_mov": 20, "salu": 40, "s_load": 4, "global": 0, "flat": 0, "scratch": 0, "lds": 0, "waitcnt": 6, "branches": 8},
    "exact_iter": {"valu": 66, "f64": 49, "quarter": 2, "v_mov": 3, "salu": 21, "s_load": 0, "global": 3, "flat": 0, "scratch": 0, "lds": 2, "waitcnt": 6, "branches": 8},
    "shading": {"valu": 498, "f64": 348, "quarter": 36, "v_mov": 41, "salu": 132, "s_load": 9, "global": 2, "flat": 11, "scratch": 1, "lds": 0, "waitcnt": 14, "branches": 27},
    "round": {"valu": 970, "f64": 551, "quarter": 77, "v_mov": 100, "salu": 234, "s_load": 32, "global": 11, "flat": 14, "scratch": 3, "lds": 2, "waitcnt": 47, "branches": 55},
    "kernel": {"vgpr_count": 128, "vgpr_spill_count": 4, "sgpr_count": 106, "sgpr_spill_count": 6, "private_segment_fixed_size": 20, "instructions": 2630},
}
# ... and on this tree
NOW = {
    "refill": {"valu": 57, "f64": 3, "quarter": 2, "v_mov": 29, "salu": 36, "s_load": 2, "global": 9, "flat": 0, "scratch": 1, "lds": 0, "waitcnt": 11, "branches": 9},
    "setup": {"valu": 257, "f64": 151, "quarter": 8, "v_mov": 20, "salu": 40, "s_load": 4, "global": 0, "flat": 0, "scratch": 0, "lds": 0, "waitcnt": 6, "branches": 8},
    "exact_iter": {"valu": 66, "f64": 49, "quarter": 2, "v_mov": 3, "salu": 21, "s_load": 0, "global": 3, "flat": 0, "scratch": 0, "lds": 2, "waitcnt": 6, "branches": 8},
    "shading": {"valu": 499, "f64": 348, "quarter": 36, "v_mov": 41, "salu": 132, "s_load": 9, "global": 13, "flat": 0, "scratch": 1, "lds": 0, "waitcnt": 11, "branches": 27},
    "round": {"valu": 879, "f64": 551, "quarter": 48, "v_mov": 93, "salu": 229, "s_load": 15, "global": 25, "flat": 0, "scratch": 2, "lds": 2, "waitcnt": 34, "branches": 52},
    "kernel": {"vgpr_count": 127, "vgpr_spill_count": 2, "sgpr_count": 106, "sgpr_spill_count": 6, "private_segment_fixed_size": 12, "instructions": 2489},
}


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_isa_round_count", os.path.join(ROOT, "tools", "isa_round_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def asm(tool):
    return tool.ivc.compile_asm()


@pytest.fixture(scope="module")
def now(tool, asm):
    return tool.summary(tool.round_counts(asm))


def test_the_tool_finds_the_round(tool, asm):
    """The regions are what they are taken for: the refill holds the queue's atomic and the record's loads, the exact loop reads its
    candidate from LDS and tests it in f64, and the walk between them is not counted."""
    c = tool.round_counts(asm)
    print({k: c[k] for k in tool.REGIONS})
    assert c["walk_blocks"] > 10 and c["other_loop_count"] == 3, (c["walk_blocks"], c["other_loop_count"])      # every sphere, planes, triangles
    assert c["refill"]["global"] >= 5 and c["setup"]["global"] == 0 and c["setup"]["f64"] > 100, (c["refill"], c["setup"])
    assert c["exact_iter"]["lds"] == 2 and c["exact_iter"]["f64"] > 40, c["exact_iter"]
    assert c["shading"]["f64"] > 300, c["shading"]
    assert all(c["round"][f] == sum(c[r][f] for r in tool.REGIONS) for f in tool.FIELDS)


def test_the_round_costs_what_it_reached(now):
    for r in ("refill", "setup", "exact_iter", "shading", "round", "kernel"):
        print(r, "now", now[r], "| parent", PARENT[r])
    for r in ("refill", "setup", "exact_iter", "shading", "round"):
        assert now[r] == NOW[r], (r, now[r], NOW[r])
    assert {k: now["kernel"][k] for k in NOW["kernel"]} == NOW["kernel"], now["kernel"]


def test_the_round_issues_no_more_than_the_parents(now):
    assert now["round"]["valu"] <= PARENT["round"]["valu"], (now["round"]["valu"], PARENT["round"]["valu"])
    for r in ("refill", "setup", "exact_iter"):
        assert now[r]["valu"] <= PARENT[r]["valu"], (r, now[r]["valu"], PARENT[r]["valu"])
    assert now["shading"]["valu"] <= PARENT["shading"]["valu"] + 2, now["shading"]            # (+2: the RNG cursor made from the bounce count)
    assert now["round"]["quarter"] <= PARENT["round"]["quarter"] and now["round"]["v_mov"] <= PARENT["round"]["v_mov"], now["round"]
    assert now["round"]["waitcnt"] <= PARENT["round"]["waitcnt"] and now["round"]["s_load"] <= PARENT["round"]["s_load"], now["round"]


def test_the_round_reads_the_scenes_records_as_global_memory(now):
    """RTX_ROUND_GLOBAL: no flat_ access is left in the round (the parent had 14: the material's, the sphere's, the plane's and the
    triangle's record, the nonzero bit), so none of its waits also waits for the LDS."""
    assert all(now[r]["flat"] == 0 for r in ("refill", "setup", "exact_iter", "shading")), now
    assert now["round"]["global"] >= PARENT["round"]["global"] + PARENT["round"]["flat"] - 3, now["round"]      # (the refill's sq.perm load went nowhere)


def test_scratch_did_not_grow(now):
    """Zero scratch was the aim and was not reached: 12 bytes remain of the parent's 20, 8 of them the RNG key (stored by the refill,
    reloaded by the shading block); the spilled constant pair of the refill's key arithmetic is gone with that arithmetic."""
    assert now["kernel"]["private_segment_fixed_size"] <= 12 < PARENT["kernel"]["private_segment_fixed_size"], now["kernel"]
    assert now["kernel"]["vgpr_spill_count"] <= 2 and now["kernel"]["sgpr_spill_count"] <= PARENT["kernel"]["sgpr_spill_count"], now["kernel"]
    assert now["round"]["scratch"] <= 2 and now["setup"]["scratch"] == 0 and now["exact_iter"]["scratch"] == 0, now
