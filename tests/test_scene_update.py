"""rtx_scene_update_objects, host half (no GPU): rtx_debug_host_refit of the lab library runs pack_scene, the path decision and
refit_packed -- the host reference that compiles from the same header text as scene_update_kernel (csrc/rtx_refit.h) -- and then
rtx_debug_host_scene's invariant walk over the refitted arrays and the updated object list: every sphere's box inside its leaf
child's box, every child inside its parent's, every 64-byte node's decoded child box around the 128-byte child's.  A walk that fails
raises; `how` must be the path include/rtx_hip.h prescribes.  tests/test_scene_update_gpu.py holds the device to these digests."""
import numpy as np
import pytest

import update_cases as uc

HOST_SCENES = ["s%d" % n for n in uc.HOST_SPHERE_COUNTS] + ["c2", "mixed"]


def _scene(rtx, objs):
    return rtx.Scene.from_packed(rtx.Config(rays_per_pixel=3, max_bounces=3), rtx.Camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.pi / 2), objs)


def _pairs():
    return [(s, c) for s in HOST_SCENES for c in uc.cases_for(uc.scene(s))]


@pytest.mark.parametrize("name,case", _pairs())
def test_host_refit_keeps_the_invariants_and_takes_the_documented_path(rtx, name, case):
    objs = uc.scene(name)
    idx, new, want = uc.update(objs, case)
    before = rtx.debug_host_scene(_scene(rtx, objs))
    how, stats, digests = rtx.debug_host_refit(_scene(rtx, objs), idx, new)            # (raises when the walk fails)
    assert how == want, (name, case, how)
    # the tree kept its shape, and every sphere is still in exactly one leaf
    for k in ("spheres", "triangles", "wide_nodes", "depth", "binary_nodes", "flags", "sphere_leaf_entries", "tri_leaf_entries"):
        assert stats[k] == before[k], (name, case, k)
    assert stats["flags"] & 1 and stats["sphere_leaf_entries"] == stats["spheres"]
    if name != "mixed":
        # a sphere tree has the 64-byte form, and the refit encoded every node again (or `how` would read "rebuilt")
        assert stats["flags"] & 16 and stats["quantised_nodes"] == stats["wide_nodes"]
    # the digests are those of the updated arrays, not of the old ones
    _, _, unchanged = rtx.debug_host_refit(_scene(rtx, objs), idx[:0], new[:0])
    assert digests != unchanged


def test_the_deep_scene_has_more_levels_than_the_breadth_first_top(rtx):
    assert rtx.debug_host_scene(_scene(rtx, uc.scene("c2")))["depth"] > 6


@pytest.mark.parametrize("name", ["s9", "s300", "mixed"])
def test_fallbacks_rebuild(rtx, name):
    objs = uc.scene(name)
    for case in uc.fallbacks_for(objs):
        idx, new, want = uc.update(objs, case)
        how, stats, digests = rtx.debug_host_refit(_scene(rtx, objs), idx, new, mode="rebuild" if case == "rebuild" else "auto")
        assert how == want == "rebuilt", (name, case, how)
        # a rebuild IS a fresh pack of the updated list
        _, _, fresh = rtx.debug_host_refit(_scene(rtx, uc.apply(objs, idx, new)), idx[:0], new[:0])
        assert digests == fresh, (name, case)


def test_the_edge_cases_are_what_their_names_say(rtx):
    """on the inputs alone: grow enlarges the largest reach (a stale sphere_cmax would be too small) and keeps every box in the build's
    range; neg_zero writes a -0.0 on y and z (x does not reach 0 in these scenes' move boxes); scale_in / scale_out put one padded
    hi.x 0.1 % inside / outside the build's scale, everything else of the update inside it"""
    for name in ("s9", "s65", "s300", "mixed"):
        objs = uc.scene(name)
        sph = objs["kind"] == 0
        idx, new, _ = uc.update(objs, "grow")
        assert uc.inside_build_range(objs, new), name
        assert (np.abs(new["geom"][:, 3]) >= np.abs(objs["geom"][sph, 3])).all()
        assert (np.abs(new["geom"][:, 3]) > 1.04 * np.abs(objs["geom"][sph, 3])).sum() * 2 > len(new), name
        idx, new, _ = uc.update(objs, "neg_zero")
        signed = [a for a in range(3) if (np.signbit(new["geom"][:, a]) & (new["geom"][:, a] == 0.0)).any()]
        assert signed == [1, 2], (name, signed, "the move box excludes 0 on an axis other than x")
        scale = uc.build_scale(objs)
        for case, f in (("scale_in", 0.999), ("scale_out", 1.001)):
            idx, new, _ = uc.update(objs, case)
            g = new["geom"][0]
            hi = g[0] + abs(g[3]) + (abs(g[0]) + abs(g[3])) / 1048576.0
            assert abs(hi / scale - f) < 1e-9 and np.array_equal(g[1:4], objs["geom"][int(idx[0]), 1:4]), (name, case, hi / scale)


@pytest.mark.parametrize("name", uc.ONEPOINT_SCENES)
def test_the_fallback_only_the_refit_itself_can_find(rtx, name):
    """collapse8 / onepoint_tiny: plan_update would refit them -- nothing leaves the range the tree was built for, and the same
    indices at the same place with radius 1e-4 DO refit -- but mode B meets a 64-byte node without an encoding (kUpdateStatusNoQ3)
    and the host rebuilds over the half-written arrays: the result is a fresh pack of the updated list.  That pack has lost the
    64-byte form (flags & 16 == 0, no quantised node): a few co-located tiny spheres cost the whole tree its 64-byte nodes until
    the next forced rebuild of a scene without them.  onepoint (every sphere at one point, r = 1e-4) still refits, 64-byte form kept."""
    objs = uc.scene(name)
    for case in uc.DEVICE_FALLBACK_CASES:
        idx, new, want = uc.update(objs, case)
        assert uc.inside_build_range(objs, new), (name, case)
        how, stats, digests = rtx.debug_host_refit(_scene(rtx, objs), idx, new)
        assert how == want == "rebuilt", (name, case, how)
        milder = uc.collapse(objs, idx.astype(np.int64), 1.0e-4)
        how_m, stats_m, _ = rtx.debug_host_refit(_scene(rtx, objs), idx, milder)
        assert how_m == "refit" and stats_m["flags"] & 16 and stats_m["quantised_nodes"] == stats_m["wide_nodes"], (name, case, how_m)
        _, _, fresh = rtx.debug_host_refit(_scene(rtx, uc.apply(objs, idx, new)), idx[:0], new[:0])
        assert digests == fresh, (name, case)
        assert stats["flags"] & 1 and stats["flags"] & 16 == 0 and stats["quantised_nodes"] == 0, (name, case, stats["flags"])
    idx, new, want = uc.update(objs, "onepoint")
    how, stats, _ = rtx.debug_host_refit(_scene(rtx, objs), idx, new)
    assert how == want == "refit" and stats["flags"] & 16 and stats["quantised_nodes"] == stats["wide_nodes"], (name, how)


@pytest.mark.parametrize("name", ["s9", "s300"])
def test_a_refit_of_the_tree_without_64_byte_nodes_and_the_way_back(rtx, name):
    """after collapse8 the resident tree is a sphere tree WITHOUT the 64-byte form (q3nodes == null in mode B): an ordinary move on it
    refits and keeps the invariants; a forced rebuild of an update that spreads the eight spheres out again brings the form back"""
    objs = uc.scene(name)
    i1, n1, _ = uc.update(objs, "collapse8")
    now = uc.apply(objs, i1, n1)
    i2, n2, _ = uc.update(now, "third", seed=4)
    how, stats, digests = rtx.debug_host_refit(_scene(rtx, objs), np.concatenate([i1, i2]), np.concatenate([n1, n2]), split=len(i1))
    assert how == "rebuilt" and stats["flags"] & 16 == 0, (name, how, stats["flags"])         # (of a split call: the stronger of the two)
    how, stats, direct = rtx.debug_host_refit(_scene(rtx, now), i2, n2)
    assert how == "refit" and stats["flags"] == 1 and stats["quantised_nodes"] == 0, (name, how, stats["flags"])
    assert digests == direct                                 # (the rebuilt tree is the fresh pack's: the same refit from either start)
    back = objs[i1.astype(np.int64)].copy()
    how, stats, _ = rtx.debug_host_refit(_scene(rtx, now), i1, back, mode="rebuild")
    assert how == "rebuilt" and stats["flags"] & 16 and stats["quantised_nodes"] == stats["wide_nodes"], (name, stats["flags"])


def test_a_rebuild_and_a_refit_agree_on_everything_but_the_tree(rtx):
    """the shape, plane and material records of a refit are those of a fresh pack; nodes, leaf order and the f32 records (offsets from
    the kept centre) may differ"""
    objs = uc.scene("s65")
    idx, new, _ = uc.update(objs, "all")
    _, _, a = rtx.debug_host_refit(_scene(rtx, objs), idx, new)
    _, _, b = rtx.debug_host_refit(_scene(rtx, objs), idx, new, mode="rebuild")
    assert a[4:7] == b[4:7] and a[0] != b[0]


@pytest.mark.parametrize("name", ["s9", "s300", "c2", "mixed"])
def test_a_refit_back_to_the_first_geometry_gives_the_builders_arrays(rtx, name):
    """move every sphere, then move it back (two refits): nodes, 64-byte nodes, leaf records, f32 records and shapes are the bits
    pack_scene built for that geometry -- the refit reproduces the builder for the same topology, the 64-byte step included"""
    objs = uc.scene(name)
    sc = _scene(rtx, objs)
    i1, n1, _ = uc.update(objs, "all")
    back = objs[i1.astype(np.int64)].copy()
    how, _, there_and_back = rtx.debug_host_refit(sc, np.concatenate([i1, i1]), np.concatenate([n1, back]), split=len(i1))
    _, _, built = rtx.debug_host_refit(sc, i1[:0], n1[:0])
    assert how == "refit" and there_and_back == built


def test_errors_and_the_empty_update(rtx):
    objs = uc.scene("s9")
    idx, new, _ = uc.update(objs, "one")
    how, _, _ = rtx.debug_host_refit(_scene(rtx, objs), idx[:0], new[:0])
    assert how == "nothing"
    with pytest.raises(rtx.RtxError) as e:
        rtx.debug_host_refit(_scene(rtx, objs), np.array([len(objs)], dtype=np.uint64), new)
    assert e.value.status == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    bad = new.copy()
    bad["kind"] = 9
    with pytest.raises(rtx.RtxError) as e:
        rtx.debug_host_refit(_scene(rtx, objs), idx, bad)
    assert e.value.status == rtx.abi.RTX_ERR_UNSUPPORTED
    bad = new.copy()
    bad["reserved"] = 1
    with pytest.raises(rtx.RtxError) as e:
        rtx.debug_host_refit(_scene(rtx, objs), idx, bad)
    assert e.value.status == rtx.abi.RTX_ERR_UNSUPPORTED
    with pytest.raises(rtx.RtxError) as e:
        rtx.debug_host_refit(_scene(rtx, objs), idx, new, mode=7)
    assert e.value.status == rtx.abi.RTX_ERR_INVALID_ARGUMENT


def test_the_product_library_has_no_host_refit_hook(rtx):
    import ctypes as C
    lib = rtx.load_library()
    how, stats, digests = C.c_uint32(0), (C.c_uint64 * 16)(), (C.c_uint64 * 8)()
    assert lib.rtx_debug_host_refit(None, None, None, 0, 0, stats, C.byref(how), digests) == rtx.abi.RTX_ERR_UNSUPPORTED
    assert lib.rtx_debug_resident_digests(None, digests) == rtx.abi.RTX_ERR_UNSUPPORTED


@pytest.mark.parametrize("name", ["s17", "s300", "mixed"])
def test_two_updates_in_a_row_equal_both_at_once(rtx, name):
    """a refit is a function of the geometry it ends with: (base, update 1, then update 2) leaves the arrays of (base, both in one call) --
    the two lists overlap, so the one-call form also exercises "the last entry wins" """
    objs = uc.scene(name)
    i1, n1, _ = uc.update(objs, "third", seed=1)
    i2, n2, _ = uc.update(objs, "all", seed=2)
    i3, n3, _ = uc.update(objs, "material", seed=3)
    idx, new = np.concatenate([i1, i2, i3]), np.concatenate([n1, n2, n3])
    how_a, _, once = rtx.debug_host_refit(_scene(rtx, objs), idx, new)
    how_b, _, twice = rtx.debug_host_refit(_scene(rtx, objs), idx, new, split=len(i1))
    assert how_a == how_b == "refit"
    assert once == twice
