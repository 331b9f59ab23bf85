"""The 64-byte sphere node with its links interleaved (rtx_bvh.h BvhQ3Node: {link0, ox, link1, oy} {link2, oz, link3, sx} {sy, sz, lox, loy}
{loz, hix, hiy, hiz}), without a GPU.

The host check of rtx_debug_host_scene decodes every 64-byte node field by field, as the device does, and holds it against the 128-byte
node it was made from: links, types, empty slots and the decoded boxes.  A word the builder put in the wrong place fails it.  The count
of the visit (tools/isa_visit_count.py) is pinned at what the layout, the room test `sp <= STACK - 3` and the bound's min as one
instruction reached.
"""
import importlib.util
import os

import pytest

from test_stage2_visit import _scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_visit_count.py with this layout: 147 before it; 143 with the four link copies gone; 142 with the room test's add gone; 141
# with the bound's min written as the instruction (rtx_min_f32_bits: no canonicalising v_max of best_up).
VISIT_VALU = 141
VISIT_VALU_SCALAR_OPERAND = 22


def _host_scene(rtx, objs):
    from rust_raytracing_amd import scenes
    return rtx.debug_host_scene(rtx.Scene.from_packed(rtx.Config(), rtx.Camera(*scenes.CAMERA), objs))


def _layout_scenes():
    from rust_raytracing_amd import scenes
    s = _scenes()
    return {"few3": s["few3"], "few5": s["few5"], "few6": s["few6"],            # nodes with empty slots
            "random200": scenes.random_spheres(200, 11, box=0.2),               # (the scene of tests/golden/spheres200_48x27.npz)
            "deep": s["deep"]}


@pytest.mark.parametrize("name", ["few3", "few5", "few6", "random200", "deep"])
def test_every_64_byte_node_decodes_to_its_128_byte_node(rtx, name):
    objs = _layout_scenes()[name]
    st = _host_scene(rtx, objs)                                                 # raises when the check fails
    assert st["quantised_nodes"] == st["wide_nodes"], st
    if len(objs) <= 4:                                                          # (rtx_pack.hip pack_scene: four spheres or fewer get no tree)
        assert st["wide_nodes"] == 0 and st["flags"] == 0, st
        return
    assert st["flags"] == 1 + 16, st                                            # a sphere tree in its 64-byte form
    assert st["wide_nodes"] >= 1 and st["sphere_leaf_entries"] == len(objs), st


def _isa_tool():
    spec = importlib.util.spec_from_file_location("_isa_visit_count", os.path.join(ROOT, "tools", "isa_visit_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_visit_builds_its_sort_pairs_in_place():
    tool = _isa_tool()
    now = tool.visit_counts(tool.compile_asm())
    assert now["global"] == 4 and now["lds"] >= 3, now                          # the path found is the visit: one node fetched, pushed, popped
    assert now["valu"] <= VISIT_VALU, (now["valu"], now["mnemonics"])
    assert now["valu_sgpr_or_literal"] <= VISIT_VALU_SCALAR_OPERAND, (now["valu_sgpr_or_literal"], now["mnemonics"])
    old = tool.visit_counts(tool.compile_asm(["-DRTX_Q3_PUSH_ALL=0"]))          # the counted pushes still build, and count more
    assert old["global"] == 4 and old["valu"] > now["valu"], (old["valu"], now["valu"])
    fmin = tool.visit_counts(tool.compile_asm(["-DRTX_Q3_MIN_BITS=0"]))         # so does the fminf form: by the one v_max
    assert fmin["global"] == 4 and fmin["valu"] > now["valu"], (fmin["valu"], now["valu"])
