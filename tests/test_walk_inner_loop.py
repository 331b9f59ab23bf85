"""The sphere walk with consecutive node visits in an inner loop (rtx_traverse.h sphere_walk_phased<.., INNER = true>, the form of the
four trace_bvh_spheres_kernel instances; -DRTX_WALK_INNER=0 builds the former two-arm loop).

Without a GPU: what an iteration that visits nodes costs in the ISA of stage 2 (tools/isa_visit_count.py, which follows the control
flow: the block with the pushes lies behind the loop's back-branch in this form), that the former form still builds and still counts
what it counted, and that the path found in the new form holds the two row-pair writes and the read-back.
On the GPU: RTX_KERNEL_AUTO against the exhaustive f64 kernel bit for bit where the new loop has exits the former did not have -- waves
with a few lanes (no cut can happen: the run of node visits ends because nobody walks any more, or because everybody left holds a leaf),
and frames under the cut with rays of one segment each --, and the work the walk counts against what the parent commit's library counted.
The query kernels (rtx_query.hip) did not take the new form: they call sphere_walk_phased with INNER = false, the former body.
"""
import importlib.util
import os

import numpy as np
import pytest

from test_stage2_visit import _cameras, _render, _scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tools/isa_visit_count.py on this form: 141 VALU / 66 SALU / 14 branches before it (the two-arm loop, which -DRTX_WALK_INNER=0 still is).
# The issue that asked for the inner loop set 133 as the most the visit may cost.
VISIT_VALU = 131
VISIT_SALU = 49
VISIT_VALU_LIMIT = 133
FORMER_VALU, FORMER_SALU = 141, 66


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("_isa_visit_count", os.path.join(ROOT, "tools", "isa_visit_count.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def now(tool):
    return tool.visit_counts(tool.compile_asm())


def test_the_node_visit_of_the_inner_loop_costs_what_it_reached(now):
    print("visit:", {k: now[k] for k in ("valu", "valu_sgpr_or_literal", "salu", "lds", "global", "branches")})
    assert now["global"] == 4 and now["lds"] >= 3, now
    assert now["valu"] <= VISIT_VALU_LIMIT, (now["valu"], now["mnemonics"])
    assert now["valu"] <= VISIT_VALU, (now["valu"], now["mnemonics"])
    assert now["salu"] <= VISIT_SALU, now["salu"]


def test_the_path_holds_the_pushes_and_the_read_back(now):
    """All four links written as two row pairs, the nearest read back: the block behind the back-branch is on the path."""
    assert now["mnemonics"].get("ds_write2st64_b32") == 2, now["mnemonics"]
    assert now["mnemonics"].get("ds_read_b32") == 1, now["mnemonics"]


def test_the_former_loop_still_builds_and_counts_what_it_counted(tool):
    old = tool.visit_counts(tool.compile_asm(["-DRTX_WALK_INNER=0"]))
    print("former:", {k: old[k] for k in ("valu", "valu_sgpr_or_literal", "salu", "lds", "global", "branches")})
    assert (old["valu"], old["salu"]) == (FORMER_VALU, FORMER_SALU), old
    assert old["global"] == 4 and old["lds"] == 3 and old["valu_sgpr_or_literal"] == 22, old


# ---- on the GPU --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _random200():
    from rust_raytracing_amd import scenes
    return scenes.random_spheres(200, 11, box=0.2)                               # (the scene of tests/golden/spheres200_48x27.npz)


def _objects(name):
    return _random200() if name == "random200" else _scenes()[name]


def _tunings(gpu):
    return (0, gpu.RTX_TUNE_TWO_STAGE, gpu.RTX_TUNE_TWO_STAGE | gpu.RTX_TUNE_NO_PACKETS)


def _auto_equals_exact(gpu, objs, cam, w, h, spp, what, **cfg):
    ref, st_ref = _render(gpu, objs, cam, gpu.RTX_KERNEL_EXACT, 0, w, h, spp, **cfg)
    for tune in _tunings(gpu):
        img, st = _render(gpu, objs, cam, gpu.RTX_KERNEL_AUTO, tune, w, h, spp, **cfg)
        assert np.array_equal(img.view(np.int64), ref.view(np.int64)), (what, tune, float(np.nanmax(np.abs(img - ref))))
        assert st.segments == st_ref.segments, (what, tune, st.segments, st_ref.segments)
    return st_ref.segments


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["few3", "few5", "few6", "random200"])
def test_partly_filled_waves_equal_the_exhaustive_kernel(gpu, name):
    """Frames of 1, 35, 72 and 6912 rays: waves with fewer live rays than the cut asks for, so every run of node visits ends by the
    walkers' ballot being empty or by the leaf rule with fewer than `leaf_lanes` walkers."""
    objs = _objects(name)
    cams = {c[0]: c for c in _cameras(objs)}
    for cname in ("bench", "inside"):
        _, cam, cfg = cams[cname]
        for w, h, spp in ((1, 1, 1), (7, 5, 1), (9, 8, 1), (64, 36, 3)):
            _auto_equals_exact(gpu, objs, cam, w, h, spp, (name, cname, w, h, spp), **cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("bounces", [10, 0, 1])
@pytest.mark.parametrize("name", ["deep", "clustered"])
def test_the_cut_inside_a_run_of_node_visits(gpu, name, bounces):
    """Full waves under the cut (two stages), from outside and from inside the cloud.  With max_bounces 0 and 1 every survivor of
    stage 1 takes exactly one segment: every round of stage 2 refills."""
    objs = _objects(name)
    cams = {c[0]: c for c in _cameras(objs)}
    segs = 0
    for cname in ("bench", "inside"):
        _, cam, cfg = cams[cname]
        segs += _auto_equals_exact(gpu, objs, cam, 96, 54, 2, (name, cname, bounces), max_bounces=bounces, **cfg)
    assert segs >= 2 * 96 * 54 * 2, segs                                       # (every primary ray is a segment)


# (segments, exact tests, box tests) of RTX_KERNEL_AUTO | RTX_TUNE_TWO_STAGE | RTX_TUNE_NO_PACKETS, seed 42, from the benchmark's camera,
# counted on an MI355X by the library of the parent commit 0acc6fa (the two-arm loop), loaded through RTX_HIP_LIB in the GPU visit that
# then ran this file on the new library.  Four box tests per node visit: a visit more, fewer or earlier against best_up shows here.
COUNTS_PARENT = {
    ("random200", 48, 27, 2): (2849, 277, 55188),
    ("deep", 96, 54, 2): (10869, 638, 1804080),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(COUNTS_PARENT))
def test_the_walk_counts_what_the_parent_counted(gpu, case):
    from rust_raytracing_amd import scenes
    name, w, h, spp = case
    _, st = _render(gpu, _objects(name), scenes.CAMERA, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE | gpu.RTX_TUNE_NO_PACKETS, w, h, spp)
    got = (int(st.segments), int(st.exact_tests), int(st.box_tests))
    print(case, "segments, exact tests, box tests:", got, "parent:", COUNTS_PARENT[case])
    assert got == COUNTS_PARENT[case]
