"""rtx_scene_set_visible, host half (no GPU).  rtx_debug_host_set_visible of the lab library runs a handle's life on the host -- pack,
hide / show / update / append steps with refit_packed (csrc/rtx_refit.h: the text scene_update_kernel compiles too) in place of the
launches -- and then the invariant walk, which for a hidden shape asks nothing and for every visible one its leaf's box and exactly
one leaf (a walk that fails raises).  Held here: the path (`how`) per case, the restated contract on the node words
(visibility_cases.check_slots), that hide followed by show restores every digest of the base pack, that halves equal the whole, that
sphere_cmax / tri_extent are numpy's max over the visible shapes to the bit, that every rebuild equals a fresh pack plus the hide
pass -- and, with the oracle, that all-NaN geometry is "never hit" in the reference's text for all three kinds, which is what makes
L_nan the deleted list.  tests/test_visibility_gpu.py holds the device to these digests."""
import math

import numpy as np
import pytest

import mesh_update_cases as mc
import update_cases as uc
import visibility_cases as vc
from helpers import oracle_render, same


def _scene(rtx, objs):
    return rtx.Scene.from_packed(rtx.Config(rays_per_pixel=3, max_bounces=3), rtx.Camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.pi / 2), objs)


def _run(rtx, objs, steps, dump=False):
    return rtx.debug_host_set_visible(_scene(rtx, objs), steps, dump=dump)


def test_the_stated_cases_are_the_ones_the_trees_have(rtx):
    for name in vc.SCENES:
        objs = vc.scene(name)
        sets = vc.hide_sets(vc.tree_of(rtx, _scene(rtx, objs)), objs)
        assert [c for c in vc.HIDE_CASES if c in sets] == list(vc.CASES_OF[name]), name


@pytest.mark.parametrize("name", ["mixed", "s9"])
def test_nan_geometry_is_never_hit_in_the_reference(oracle, name):
    """the oracle's frame of L_nan is its frame of the list with those objects deleted, bit for bit -- one hidden object of every kind
    the scene has -- and another frame than the full scene's"""
    objs = vc.scene(name)
    hidden = [int(np.nonzero(objs["kind"] == k)[0][j]) for k in range(3) for j in (0, 3) if (objs["kind"] == k).sum() > j]
    cfg = dict(rays_per_pixel=2, max_bounces=3, seed=11)
    a = oracle_render(oracle, vc.l_nan(objs, hidden), 40, 24, **cfg)
    b = oracle_render(oracle, vc.deleted(objs, hidden), 40, 24, **cfg)
    assert same(a, b)
    assert not same(a, oracle_render(oracle, objs, 40, 24, **cfg)), "the hidden objects were not in view: the comparison shows nothing"


@pytest.mark.parametrize("name,case", vc.PAIRS)
def test_hide_takes_the_documented_path_and_keeps_the_contract(rtx, name, case):
    objs = vc.scene(name)
    tree = vc.tree_of(rtx, _scene(rtx, objs))
    idx = vc.hide_sets(tree, objs)[case]
    base = _run(rtx, objs, [])
    hows, stats, digests, info, mask, dump = _run(rtx, objs, [("hide", idx)], dump=True)           # (raises when the walk fails)
    assert hows == [vc.how_of(tree, idx)], (name, case, hows)
    if case in ("leaf", "leaf_but_one", "node4", "all_tree"):
        assert hows == ["refit"]
    if case in ("plane", "outside"):
        assert hows == ["records"]
    assert np.array_equal(np.nonzero(~mask)[0], sorted(set(idx)))
    n_empty, n_live = vc.check_slots(tree, objs, idx, dump)
    pack_empty, _ = vc.check_slots(tree, objs, [], tree.dump)
    if case in ("leaf", "node4", "all_tree"):
        assert n_empty > pack_empty, "the case emptied no slot"
    if case == "leaf_but_one":
        assert n_empty == pack_empty
    if case == "all_tree":
        assert n_live == 0 and stats["sphere_leaf_entries"] == stats["tri_leaf_entries"] == 0
    if case == "node4" and len(tree.children) > 1:
        # the empty slot climbed: the node's own slot in its parent reads empty
        assert n_empty >= pack_empty + 2
    assert digests != base[2]
    # the topology and the record counts are the pack's
    for k in ("spheres", "triangles", "tri_filter_records", "tri_in_tree", "wide_nodes", "binary_nodes", "flags"):
        assert stats[k] == base[1][k], (name, case, k)
    # hide followed by show: every digest of the base pack, every object visible
    hows2, _, digests2, _, mask2 = _run(rtx, objs, [("hide", idx), ("show", idx[::-1])])
    assert hows2 == hows * 2 and digests2 == base[2] and mask2.all(), (name, case)
    # repeated indices and entries already in the state are no-ops
    hows3, _, digests3, _, _ = _run(rtx, objs, [("hide", list(idx) + list(idx)), ("hide", idx), ("show", [])])
    assert hows3 == hows + ["nothing", "nothing"] and digests3 == digests


@pytest.mark.parametrize("name", vc.SCENES)
def test_halves_equal_the_whole_and_the_order_does_not_matter(rtx, name):
    objs = vc.scene(name)
    tree = vc.tree_of(rtx, _scene(rtx, objs))
    idx = vc.hide_sets(tree, objs)["third"]
    whole = _run(rtx, objs, [("hide", idx)])[2]
    h = len(idx) // 2
    assert _run(rtx, objs, [("hide", idx[:h]), ("hide", idx[h:])])[2] == whole
    assert _run(rtx, objs, [("hide", idx[h:]), ("hide", idx[:h])])[2] == whole
    # hide A, hide B, show A: B alone
    a, b = idx[:h], idx[h:]
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", a), ("hide", b), ("show", a)])
    assert digests == _run(rtx, objs, [("hide", b)])[2] and np.array_equal(np.nonzero(~mask)[0], sorted(b))
    # ten steps in a row end where one step ends
    rng = np.random.default_rng(4)
    hidden, steps = set(), []
    for k in range(10):
        pick = [int(x) for x in rng.choice(len(objs), max(len(objs) // 4, 1), replace=False)]
        steps.append(("show" if k % 3 == 2 else "hide", pick))
        hidden = hidden - set(pick) if k % 3 == 2 else hidden | set(pick)
    hows, _, digests, _, mask = _run(rtx, objs, steps)
    assert np.array_equal(np.nonzero(~mask)[0], sorted(hidden))
    assert digests == _run(rtx, objs, [("hide", sorted(hidden))])[2], name


@pytest.mark.parametrize("name", vc.SCENES)
def test_the_scene_wide_bounds_are_those_of_the_visible_shapes(rtx, name):
    """sphere_cmax = max |c - centre| + |r| over the visible spheres and tri_extent = max |v - centre| over the visible qualified
    triangles, against the KEPT centre, to the bit; everything hidden: 0, and still below plan_update's 1e14"""
    objs = vc.scene(name)
    tree = vc.tree_of(rtx, _scene(rtx, objs))
    sets = vc.hide_sets(tree, objs)
    for case in ("third", "all_tree", "everything"):
        idx = list(range(len(objs))) if case == "everything" else sets.get(case)
        if idx is None:
            continue
        _, _, _, info, mask = _run(rtx, objs, [("hide", idx)])
        centre = np.array([info["centre_x"], info["centre_y"], info["centre_z"]])
        assert np.array_equal(centre, mc.centre_of(objs)), "the centre moved"
        cmax = 0.0
        for k in np.nonzero((objs["kind"] == 0) & mask)[0]:
            cx, cy, cz = (float(objs["geom"][k, a]) - float(centre[a]) for a in range(3))
            cmax = max(cmax, math.sqrt(cx * cx + cy * cy + cz * cz) + abs(float(objs["geom"][k, 3])))
        ext = max([mc.reach(objs["geom"][k], centre) for k, c in mc.classes(objs, centre).items() if c[0] == "qualified" and mask[k]], default=0.0)
        assert info["sphere_cmax"] == cmax and info["tri_extent"] == ext, (name, case)
        if case == "everything":
            assert cmax == 0.0 and ext == 0.0
            # ... and a show after it is taken in place
            assert _run(rtx, objs, [("hide", idx), ("show", idx)])[0][1] in ("refit", "records")


@pytest.mark.parametrize("name", ["s9", "s300", "mixed", "t40", "cubes25"])
def test_every_rebuild_is_a_fresh_pack_plus_the_hide_pass(rtx, name):
    objs = vc.scene(name)
    tree = vc.tree_of(rtx, _scene(rtx, objs))
    sets = vc.hide_sets(tree, objs)
    hid = sets["third"]
    want = _run(rtx, objs, [("hide", hid)])
    # RTX_UPDATE_REBUILD of an untouched entry: the same list packed again, the same hidden set
    k = [i for i in range(len(objs)) if i not in hid][:1]
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", hid), ("rebuild", k, objs[k])])
    assert hows[1] == "rebuilt" and digests == want[2] and np.array_equal(mask, want[4]), name
    # ... and a show after it is taken in place and restores the base pack
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", hid), ("rebuild", k, objs[k]), ("show", hid)])
    assert hows[2] in ("refit", "records") and digests == _run(rtx, objs, [])[2] and mask.all()
    # an append: the new objects are visible, the old hidden set is kept
    extra = objs[:3].copy()
    extra["geom"][:, :3] += 0.25
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", hid), ("append", extra)])
    assert hows[1] == "rebuilt" and np.array_equal(np.nonzero(~mask)[0], sorted(hid))
    assert digests == _run(rtx, np.concatenate([objs, extra]), [("hide", hid)])[2], name
    # an update of a VISIBLE object that falls back (a kind change) with objects hidden
    new = objs[k].copy()
    new["kind"] = 1 if int(objs["kind"][k[0]]) != 1 else 0
    hows, _, digests, _, _ = _run(rtx, objs, [("hide", hid), ("auto", k, new)])
    assert hows[1] == "rebuilt" and digests == _run(rtx, uc.apply(objs, np.asarray(k), new), [("hide", hid)])[2]


@pytest.mark.parametrize("name", ["s9", "s300", "mixed"])
def test_an_update_of_a_hidden_object_is_judged_when_it_is_shown(rtx, name):
    objs = vc.scene(name)
    idx, new, want = uc.update(objs, "one")
    k = [int(idx[0])]
    assert want == "refit"
    # hidden, moved, shown: it appears at the NEW place -- the arrays of the move alone
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", k), ("auto", idx, new), ("show", k)])
    assert hows == ["refit", "records", "refit"] and mask.all()
    assert digests == _run(rtx, objs, [("auto", idx, new)])[2], name
    # while it is hidden the update writes the material alone: geometry records are the hidden ones
    moved_only = _run(rtx, objs, [("hide", k), ("auto", idx, new)])[2]
    hidden_only = _run(rtx, objs, [("hide", k)])[2]
    assert [a == b for a, b in zip(moved_only, hidden_only)].count(False) <= 1          # (the material digest may differ)
    # moved beyond the build's range while hidden: the show rebuilds, and is the fresh pack of the moved list
    idx, far, _ = uc.update(objs, "far")
    k = sorted(set(int(i) for i in idx))
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", k), ("auto", idx, far), ("show", k)])
    assert hows == ["refit", "records", "rebuilt"] and mask.all()
    assert digests == _run(rtx, uc.apply(objs, idx, far), [])[2]
    # a kind change of a hidden object rebuilds at once, and the object stays hidden
    new = objs[k[:1]].copy()
    new["kind"] = 1
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", k), ("auto", k[:1], new)])
    assert hows[1] == "rebuilt" and np.array_equal(np.nonzero(~mask)[0], k)


def test_a_triangle_shown_with_another_class_rebuilds(rtx):
    objs, idx, new, want, mode = mc.case_of("t300", "flip")
    assert want == "rebuilt"
    k = sorted(set(int(i) for i in idx))
    hows, _, digests, _, mask = _run(rtx, objs, [("hide", k), (mode, idx, new), ("show", k)])
    assert hows == ["refit", "records", "rebuilt"] and mask.all()
    assert digests == _run(rtx, mc.apply(objs, idx, new), [])[2]
    # ... and one that keeps its class is taken in place, at the new place
    objs, idx, new, want, mode = mc.case_of("t300", "slide")
    k = sorted(set(int(i) for i in idx))
    hows, _, digests, _, _ = _run(rtx, objs, [("hide", k), (mode, idx, new), ("show", k)])
    assert hows == ["refit", "records", "refit"]
    assert digests == _run(rtx, objs, [(mode, idx, new)])[2]


def test_errors_are_found_before_anything_is_written(rtx):
    objs = vc.scene("s9")
    for steps in ([("hide", [len(objs)])], [("hide", [0]), ("show", [1 << 40])]):
        with pytest.raises(rtx.RtxError) as e:
            _run(rtx, objs, steps)
        assert e.value.status == rtx.abi.RTX_ERR_INVALID_ARGUMENT
