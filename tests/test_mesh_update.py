"""RTX_UPDATE_DEFORM, host half (no GPU): rtx_debug_host_refit_mesh of the lab library runs pack_scene, the path decision and
refit_packed -- the host reference that compiles from the same header text as scene_update_kernel (csrc/rtx_refit.h) -- and then
rtx_debug_host_scene's invariant walk over the refitted arrays and the updated object list: every footprint inside its leaf's
rectangle, every child inside its parent, the free axis of every tree record the one its TriX rows name, every 64-byte footprint
node's decoded rectangles around the 128-byte node's.  A walk that fails raises.  `how` must be what the class rule, restated in
tests/mesh_update_cases.py, says.  tests/test_mesh_update_gpu.py holds the device to these digests."""
import struct

import numpy as np
import pytest

import mesh_update_cases as mc

NODES, TRIS, TRI_F32, TRI_GEO, QNODES, TRI_EXTENT = 0, 8, 9, 10, 11, 12      # digest slots (include/rtx_hip.h)
EMPTY = np.zeros(0, dtype=np.uint64)


def _scene(rtx, objs):
    return rtx.Scene.from_packed(rtx.Config(rays_per_pixel=3, max_bounces=3), rtx.Camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.pi / 2), objs)


_base = {}


def _base_pack(rtx, name):
    """(stats, digests, info) of the scene as uploaded: an empty update"""
    if name not in _base:
        objs = mc.cached_scene(name)
        how, stats, digests, info = rtx.debug_host_refit_mesh(_scene(rtx, objs), EMPTY, objs[:0])
        assert how == "nothing"
        _base[name] = (stats, digests, info)
    return _base[name]


def _bits(x):
    return struct.pack("<d", x)


def test_the_scenes_are_the_trees_the_cases_were_chosen_for(rtx):
    """records in the tree, flags, depth, flat nodes: the table of the cases' docstring, and the restated class rule counts the same
    records and tree records as pack_scene on every scene"""
    want = {"t6": (0, 0, 0), "t40": (19, 14, 2), "t300": (164, 14, 3), "t1100": (622, 14, 5), "cubes25": (196, 2, 5), "mixed": (22, 3, 4)}
    for name in mc.SCENES:
        stats, _, info = _base_pack(rtx, name)
        objs = mc.cached_scene(name)
        assert (stats["tri_in_tree"], stats["flags"], stats["depth"]) == want[name], name
        assert stats["tri_in_tree"] == len(mc.in_tree(objs)), name
        assert stats["tri_filter_records"] == sum(1 for c in mc.classes(objs).values() if c[0] != "none"), name
        assert [info["centre_x"], info["centre_y"], info["centre_z"]] == list(mc.centre_of(objs)), name
        assert info["scale"] == mc.build_scale(objs), name
    assert _base_pack(rtx, "t300")[0]["flat_nodes"] == 21 and _base_pack(rtx, "cubes25")[0]["tri_other_footprints"] == 128
    assert _base_pack(rtx, "t40")[0]["quantised_nodes"] == _base_pack(rtx, "t40")[0]["wide_nodes"]
    assert _base_pack(rtx, "cubes25")[0]["quantised_nodes"] == 0


@pytest.mark.parametrize("name,case", mc.pairs())
def test_host_deform_keeps_the_invariants_and_takes_the_path_the_class_rule_names(rtx, name, case):
    objs, idx, new, want, mode = mc.case_of(name, case)
    before, base, base_info = _base_pack(rtx, name)
    how, stats, digests, info = rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode)     # (raises when the walk fails)
    assert how == want, (name, case, how)
    for k in ("spheres", "triangles", "tri_filter_records", "tri_in_tree", "wide_nodes", "depth", "binary_nodes", "flags", "sphere_leaf_entries",
              "tri_leaf_entries", "flat_nodes", "tri_xy_footprints", "tri_other_footprints", "quantised_nodes"):
        assert stats[k] == before[k], (name, case, k)
    assert digests != base and digests[13:] == (0, 0, 0)
    # tri_extent: the largest |v - centre| coordinate of the qualified triangles of the UPDATED list against the KEPT centre, to the bit
    centre = np.array([base_info["centre_x"], base_info["centre_y"], base_info["centre_z"]])
    assert [info["centre_x"], info["centre_y"], info["centre_z"]] == list(centre)
    now = mc.apply(objs, idx, new)
    assert _bits(info["tri_extent"]) == _bits(mc.tri_extent(now, centre)), (name, case, info["tri_extent"])
    assert (info["abs_pad"], info["scale"]) == (base_info["abs_pad"], base_info["scale"])
    if case == "shrink":
        assert info["tri_extent"] <= base_info["tri_extent"]
        if name != "cubes25":                                   # (the cubes' extreme face shrinks within its own plane, which is the extreme)
            assert info["tri_extent"] < base_info["tri_extent"], name
    if case == "grow":
        assert info["tri_extent"] > base_info["tri_extent"] and digests[TRI_EXTENT] != base[TRI_EXTENT]
    if case == "material_only":
        assert [k for k in range(13) if digests[k] != base[k]] == [6]
    elif how == "refit" and case not in ("grow", "one"):
        assert digests[NODES] != base[NODES] and digests[TRIS] != base[TRIS] and digests[TRI_F32] != base[TRI_F32] and digests[TRI_GEO] != base[TRI_GEO]
        if before["flags"] & 8:
            assert digests[QNODES] != base[QNODES], (name, case)


def test_a_triangle_update_of_the_joint_scene_leaves_the_sphere_arrays(rtx):
    """of the first eight digests (rtx_debug_host_refit's) a triangles-only update changes the wide nodes alone"""
    _, base, _ = _base_pack(rtx, "mixed")
    for case in ("shrink", "slide", "jitter"):
        objs, idx, new, want, mode = mc.case_of("mixed", case)
        how, _, digests, _ = rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode)
        assert how == "refit" and [k for k in range(8) if digests[k] != base[k]] == [NODES], case
        # and rtx_debug_host_refit (8 digests) takes the new mode too
        how8, _, digests8 = rtx.debug_host_refit(_scene(rtx, objs), idx, new, mode=mode)
        assert how8 == how and digests8 == digests[:8]


@pytest.mark.parametrize("name,case", mc.pairs())
def test_one_update_is_the_same_update_in_two_halves_and_its_inverse_restores_the_pack(rtx, name, case):
    objs, idx, new, want, mode = mc.case_of(name, case)
    _, base, _ = _base_pack(rtx, name)
    whole = rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode)
    if len(idx) >= 2:
        halves = rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode, split=len(idx) // 2)
        assert halves[0] == whole[0] and halves[2] == whole[2] and halves[3] == whole[3], (name, case)
    # there and back: the centre is the kept one in both updates, so every array is the base pack's again
    back = objs[idx.astype(np.int64)].copy()
    how, _, digests, _ = rtx.debug_host_refit_mesh(_scene(rtx, objs), np.concatenate([idx, idx]), np.concatenate([new, back]), mode=mode, split=len(idx))
    assert how == want and digests == base, (name, case, [k for k in range(13) if digests[k] != base[k]])


@pytest.mark.parametrize("name", mc.SCENES)
def test_fallbacks_rebuild(rtx, name):
    for case in mc.fallbacks_for(name):
        objs, idx, new, want, mode = mc.case_of(name, case)
        how, _, digests, _ = rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode)
        assert how == want == "rebuilt", (name, case, how)
        # a rebuild IS a fresh pack of the updated list
        now = mc.apply(objs, idx, new)
        _, _, fresh, _ = rtx.debug_host_refit_mesh(_scene(rtx, now), EMPTY, now[:0])
        assert digests == fresh, (name, case)
        if case != "auto_tri_vertex":                           # the same entries under AUTO and REBUILD rebuild too
            for other in ("auto", "rebuild"):
                assert rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=other)[0] == "rebuilt", (name, case, other)


def test_every_deform_case_still_rebuilds_under_auto(rtx):
    """RTX_UPDATE_AUTO keeps its behaviour: a triangle's new vertices rebuild, whatever their class"""
    for name in ("t6", "t40", "mixed"):
        for case in ("shrink", "one", "grow"):
            objs, idx, new, _, _ = mc.case_of(name, case)
            assert rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode="auto")[0] == "rebuilt", (name, case)


def test_unknown_modes_are_still_refused_and_the_product_library_has_no_hook(rtx):
    objs, idx, new, _, _ = mc.case_of("t40", "one")
    assert rtx.abi.RTX_UPDATE_DEFORM == 2
    for mode in (3, 7, 0xFFFF):
        with pytest.raises(rtx.RtxError) as e:
            rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode=mode)
        assert e.value.status == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    with pytest.raises(KeyError):
        rtx.debug_host_refit_mesh(_scene(rtx, objs), idx, new, mode="morph")
    import ctypes as C
    lib = rtx.load_library()
    assert lib.rtx_debug_host_refit_mesh(None, None, None, 0, 2, None, None, None, None) == rtx.abi.RTX_ERR_UNSUPPORTED
    assert lib.rtx_debug_resident_mesh_digests(None, (C.c_uint64 * 16)()) == rtx.abi.RTX_ERR_UNSUPPORTED
