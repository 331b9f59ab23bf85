"""The node visit of the sphere walk (rtx_traverse.h sphere_node_step_q3: all four links written to the stack, the nearest read back).

Without a GPU: the cost of the visit, counted in the ISA of trace_bvh_spheres_kernel<false, 2, 2> (tools/isa_visit_count.py), may not
rise above what this form reached.  On the GPU: the frames of RTX_KERNEL_AUTO equal those of the exhaustive f64 kernel bit for bit on
the scenes and ray classes a visit can tell apart, and the work the walk counts (segments, exact tests, box tests) is what the former
form of the visit counted on the same scenes -- a visiting order that differed would show in the box tests.
"""
import importlib.util
import os

import numpy as np
import pytest

from helpers import hip_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_visit_count.py on the form this file came with: VALU instructions of a wave's iteration of the walk loop that visits
# nodes, and how many of them read an SGPR, an SGPR pair or a literal.  The form before it (-DRTX_Q3_PUSH_ALL=0) counts 163 and 32 by
# the same rules (126 of them between the node's fetch and the pop, counted by hand).
VISIT_VALU = 147
VISIT_VALU_SCALAR_OPERAND = 22


def _isa_tool():
    spec = importlib.util.spec_from_file_location("_isa_visit_count", os.path.join(ROOT, "tools", "isa_visit_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_node_visit_costs_no_more_instructions_than_it_did():
    tool = _isa_tool()
    now = tool.visit_counts(tool.compile_asm())
    assert now["global"] == 4 and now["lds"] >= 3, now                      # the path found is the visit: one node fetched, pushed, popped
    assert now["valu"] <= VISIT_VALU, (now["valu"], now["mnemonics"])
    assert now["valu_sgpr_or_literal"] <= VISIT_VALU_SCALAR_OPERAND, (now["valu_sgpr_or_literal"], now["mnemonics"])
    # the A/B macros still build the former form, and the tool tells the two apart
    old = tool.visit_counts(tool.compile_asm(["-DRTX_Q3_PUSH_ALL=0"]))
    assert old["valu"] > now["valu"] and old["valu_sgpr_or_literal"] > now["valu_sgpr_or_literal"], (old["valu"], now["valu"])


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _scenes():
    from rust_raytracing_amd import scenes
    c2 = scenes.random_spheres(10000, 1)
    clustered = scenes.light_every(scenes.compact(scenes.random_spheres(4000, 7)))
    deep = scenes.random_spheres(3000, 2).copy()
    deep["geom"][:, :3] *= np.logspace(0, 1.5, len(deep))[:, None]             # sizes over 1.5 decades: a deeper tree
    out = {"c2": c2, "clustered": clustered, "deep": deep}
    for n in (3, 5, 6):                                                        # nodes with empty slots
        few = scenes.light_every(scenes.compact(scenes.random_spheres(n, 30 + n)), n=2)
        out["few%d" % n] = few
    return out


def _origin_limit(objs):
    """rtx_bvh.h build_bvh: 4 x the largest |coordinate| of a sphere's box + 1 (to the padding of the boxes)."""
    g = objs["geom"]
    return 4.0 * float(np.max(np.abs(g[:, :3]) + np.abs(g[:, 3:4]))) + 1.0


def _cameras(objs):
    from rust_raytracing_amd import scenes
    g = objs["geom"]
    mid = g[:, :3].mean(axis=0)
    lim = _origin_limit(objs)
    cams = [("bench", scenes.CAMERA, {}),
            ("inside", (tuple(mid), (0.0, 0.0, 1.0), 1.2), {}),
            ("along+y", ((float(mid[0]), -lim * 0.3, float(mid[2])), (0.0, 1.0, 0.0), 1e-9), dict(focal_offset=0.0, non_focal_offset=0.0)),
            ("along-x", ((lim * 0.5, float(mid[1]), float(mid[2])), (-1.0, 0.0, 0.0), 1e-9), dict(focal_offset=0.0, non_focal_offset=0.0))]
    for name, f in (("under the limit", 0.999), ("on the limit", 1.0), ("over the limit", 1.001), ("far over it", 37.0)):
        o = (-lim * f, float(mid[1]) * 0.5, float(mid[2]) * 0.5)
        d = tuple(float(x) for x in (mid - np.array(o)))
        cams.append((name, (o, d, 0.4 / f), {}))
    return cams


def _render(gpu, objs, cam, kernel, tuning, w, h, spp, **cfg):
    import torch
    hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel, rays_per_pixel=spp, seed=42, tuning=tuning, **cfg).upload(0)
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    hnd.close()
    return buf.cpu().numpy(), st


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c2", "clustered", "deep", "few3", "few5", "few6"])
def test_auto_equals_the_exhaustive_kernel_bit_for_bit(gpu, name):
    """RTX_KERNEL_AUTO in one stage, in two stages (packets, then the queue-fed stage 2) and in two stages walked per lane (the primary
    rays of a far origin then take the visit with the slack of the f64 range) against RTX_KERNEL_EXACT: the frames bit for bit and the
    segment counts, from the benchmark's camera, inside the scene, along two axes, and from origins under, on and over the tree's
    origin limit."""
    objs = _scenes()[name]
    w, h, spp = (96, 54, 2) if len(objs) > 100 else (64, 36, 3)
    for cname, cam, cfg in _cameras(objs):
        ref, st_ref = _render(gpu, objs, cam, gpu.RTX_KERNEL_EXACT, 0, w, h, spp, **cfg)
        for tune in (0, gpu.RTX_TUNE_TWO_STAGE, gpu.RTX_TUNE_TWO_STAGE | gpu.RTX_TUNE_NO_PACKETS):
            img, st = _render(gpu, objs, cam, gpu.RTX_KERNEL_AUTO, tune, w, h, spp, **cfg)
            assert np.array_equal(img.view(np.int64), ref.view(np.int64)), (name, cname, tune, float(np.nanmax(np.abs(img - ref))))
            assert st.segments == st_ref.segments, (name, cname, tune)


# ---- the work the walk counts ------------------------------------------------------------------------------------------------------
# (segments, exact tests, box tests) of RTX_KERNEL_AUTO | RTX_TUNE_TWO_STAGE | RTX_TUNE_NO_PACKETS at 160 x 90, 2 rays per pixel, seed 42,
# from the benchmark's camera, counted on an MI355X by the library of the commit this file was added on top of (twice: the counts do
# not vary from run to run).  The order in which a walk visits the children decides how early its bound shrinks, hence its box tests;
# segments and exact tests follow from the bits.
COUNTS_BEFORE = {
    "c2": (60911, 34510, 5720032),
    "clustered": (58474, 43932, 3591140),
    "deep": (30202, 1793, 5012812),
}
COUNTED_SCENES = tuple(sorted(COUNTS_BEFORE))


def counted(gpu, name):
    from rust_raytracing_amd import scenes
    _, st = _render(gpu, _scenes()[name], scenes.CAMERA, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE | gpu.RTX_TUNE_NO_PACKETS, 160, 90, 2)
    return (int(st.segments), int(st.exact_tests), int(st.box_tests))


@pytest.mark.gpu
@pytest.mark.parametrize("name", COUNTED_SCENES)
def test_the_walk_counts_what_it_counted_before(gpu, name):
    got = counted(gpu, name)
    print(name, "segments, exact tests, box tests:", got, "before:", COUNTS_BEFORE[name])
    assert got == COUNTS_BEFORE[name]
