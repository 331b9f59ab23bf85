"""The tree walks' f32 bounds on trees refitted under RTX_UPDATE_DEFORM, held to the f64 text on rays aimed at the deformed triangles.

tests/test_walk_bounds.py holds the bounds of freshly built trees, tests/test_update_bounds.py those of trees refitted by a sphere
move.  A deform rewrites on the device everything the triangle side of the walk reads -- a triangle's A, B, g0, g1 records against
the KEPT centre, its f32 footprint widened by the KEPT abs_pad, the rectangles and boxes above it level by level, the 64-byte
BvhQNode encoding with a step of the refit's own, tri_extent (mode D) -- and what checks it elsewhere (tests/test_mesh_update*.py) is
a host reference that compiles from the same header, the host invariant walk and equality with a fresh upload on random rays.  Here
the deformed tree meets the generator of tests/bounds_cases.py:

  inputs -- (scene, update) PAIRS: tests/mesh_update_cases.py's scenes and updates, bounds_cases' planes_mesh ((x, z) and (y, z)
    faces in a joint tree) through the same update builder, and one SEQUENCE, t300 / ten: the ten alternating slide / shrink steps of
    test_mesh_update_gpu.test_ten_deform_steps_in_a_row, the property taken on the scene after step 10 (its rectangles are unions
    accumulated over ten refits; its model is deform() of the base by the accumulated update, the last entry of an index winning).
    `base` is the uploaded list, `now` the updated one.  The rays are bounds_cases.aimed(label, now, regime, pk = the BASE pack):
    origin_limit and the in-tree flags are the base pack's, which a deform keeps; the answers are bounds_cases.text_distances(now, ...).
  the deform's model -- bounds_model.deform(): what a deform must leave, written from the documented contract (DESIGN.md 3.13 "Moving
    triangles", include/rtx_hip.h "Triangles") in numpy f64; pack() and deform() share ONE per-triangle text (bounds_model.tri_record).
  CPU part -- the premises of aiming with the base pack; the generator's conditions on these rays; the model of the deformed tree (the
    deform model's records, own boxes and tri_extent, the base topology as bounds_model.own_steps reads it) has test_walk_bounds'
    property with the shipped margins; records told the FRESH pack's centre, STALE own boxes and a STALE B rectangle are each seen on
    a named set of pairs; a stale tri_extent is not -- the finding below.
  gpu part -- a lab handle uploaded with `base` and deformed ("refit"): the property on the device for every form the tree has; the
    resident records, rectangles, boxes and scene constants are the deform model's, bit for bit; AUTO == RTX_KERNEL_EXACT == AUTO on a
    fresh upload on the same rays.

Findings of the first run are in the docstrings below and in DESIGN.md 3.13; the measured shares and counts in
profiles/bounds_margin_use.txt."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import bounds_cases as bc
import bounds_model as bm
import mesh_update_cases as mc
from helpers import check_equal, hip_scene
from test_update_bounds import _best, model_violations, sub
from test_walk_bounds import FORMS, device_observation

PAIRS = (("t40", "shrink"), ("t40", "grow"), ("t300", "jitter"), ("planes_mesh", "slide"), ("mixed", "with_spheres"), ("cubes25", "slide"),
         ("t300", "ten"))
REGIMES = ("inside", "edge", "outside", "far10", "surface")
# the cells that cannot meet the generator's conditions, left out by name.  The bar is not lowered: the cells are not used, and
# test_generator_conditions_on_the_deformed_scenes keeps the figure honest (a cell that turns good is noticed).
#   cubes25 / slide / surface: the surface regime puts the origin on the centroid of the nearest other triangle -- on a cube that is
#       mostly the other half of the target's own face, and a ray inside the target's plane is not a hit: the text reports 0.296 of
#       the aimed pairs, below half.
CROWDED = {(("cubes25", "slide"), "surface")}
CPU_PAIRS = 1000
PACK_DIGESTS = os.path.join(bc.GOLDEN, "bounds_model_pack_digests.json")


def _label(pair):
    return "%s/%s" % pair


def regimes_of(pair):
    return tuple(r for r in REGIMES if (pair, r) not in CROWDED)


CASES = [(p, r) for p in PAIRS for r in regimes_of(p)]
IDS = ["%s-%s" % (_label(p), r) for p, r in CASES]


def _scene(name):
    if name == "planes_mesh":
        import rust_raytracing_amd as rtx
        return dict(bc.scenes(rtx.OBJECT_DTYPE))[name]
    return mc.cached_scene(name)


@functools.lru_cache(maxsize=None)
def steps(pair):
    """(base, ((indices, new), ...)): the update calls of a pair in order -- one, or the ten of the sequence"""
    name, what = pair
    base = _scene(name)
    if what != "ten":
        idx, new, how, mode = mc.update(base, what, name=name)
        assert (how, mode) == ("refit", "deform"), pair
        return base, ((idx, new),)
    now, out = base, []
    for k in range(10):                                     # test_mesh_update_gpu.test_ten_deform_steps_in_a_row's steps
        idx, new, how, mode = mc.update(now, "shrink" if k % 2 else "slide", seed=100 + k, name=name)
        m = mc.kept(base, idx, new)                         # (the class is judged against the kept centre: the base scene's)
        idx, new = idx[m], new[m]
        assert (how, mode) == ("refit", "deform") and len(idx), (pair, k)
        now = mc.apply(now, idx, new)
        out.append((idx, new))
    return base, tuple(out)


@functools.lru_cache(maxsize=None)
def lists(pair):
    """(base, indices, new, now) of a pair: a sequence as ONE accumulated update (the last entry of an index wins)"""
    base, calls = steps(pair)
    idx, new = np.concatenate([c[0] for c in calls]), np.concatenate([c[1] for c in calls])
    assert mc.kept(base, idx, new).all(), pair              # the premise of an in-place update, by the restated class rule
    return base, idx, new, mc.apply(base, idx, new)


@functools.lru_cache(maxsize=None)
def packs(pair):
    """(the base pack, the deform model's pack of the updated list)"""
    base, idx, new, _ = lists(pair)
    return bm.pack_for(base), bm.deform(base, idx, new)


@functools.lru_cache(maxsize=None)
def case(pair, regime):
    """bounds_cases._case for a deformed tree: the rays aimed at `now` with the BASE pack's origin_limit and in-tree flags, the surface
    regime's second pair appended, the text's answers on `now` -- computed once per process"""
    _, _, _, now = lists(pair)
    base_pk, _ = packs(pair)
    rays = bc.aimed(_label(pair), now, regime, pk=base_pk)
    o, d, target, sign, extra = rays["o"], rays["d"], rays["target"], rays["sign"], rays["extra"]
    has = extra >= 0
    o = np.concatenate([o, o[has]]); d = np.concatenate([d, d[has]])
    target = np.concatenate([target, extra[has]])
    aimed = np.concatenate([np.ones(len(sign), dtype=bool), np.zeros(int(has.sum()), dtype=bool)])
    sign = np.concatenate([sign, np.zeros(int(has.sum()))])
    t, rep, _ = bc.text_distances(now, o, d, target)
    out = {"o": o, "d": d, "target": target, "sign": sign, "aimed": aimed, "t": t, "reported": rep}
    for v in out.values():
        v.setflags(write=False)
    return out


def _bits(pk):
    """every entry of a pack as bytes: arrays whole, scalars as f64"""
    return {k: (np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else np.float64(v).tobytes()) for k, v in pk.items() if k != "objs"}


def _moved_xy(pair):
    """does an in-tree (x, y) triangle's B rectangle change at all / reach beyond the base one (centre +- half) on some side"""
    base_pk, ref = packs(pair)
    xy = base_pk["in_tree"] & (base_pk["free"] == 2)
    b0, b1 = base_pk["rec"][xy][:, 4:8].astype(np.float64), ref["rec"][xy][:, 4:8].astype(np.float64)
    out = ((b1[:, 0:2] - b1[:, 2:4]) < (b0[:, 0:2] - b0[:, 2:4])) | ((b1[:, 0:2] + b1[:, 2:4]) > (b0[:, 0:2] + b0[:, 2:4]))
    return bool((b0 != b1).any()), bool(out.any())


# ---- the CPU part -----------------------------------------------------------------------------------------------------------------------
def test_pack_is_the_parents_pack_and_an_empty_deform_is_pack():
    """pack() went through a refactoring for deform() (the per-triangle text is now bounds_model.tri_record): on every scene of
    bounds_cases.scenes and mesh_update_cases.SCENES its output has the SHA-256 it had before (tests/golden/
    bounds_model_pack_digests.json, taken from the parent commit's pack()), and deform() of an EMPTY update -- which writes every
    sphere again, takes tri_extent again and asserts every class -- is pack() bit for bit, every key"""
    import rust_raytracing_amd as rtx
    with open(PACK_DIGESTS) as fh:
        want = json.load(fh)
    every = [("bc/" + n, o) for n, o in bc.scenes(rtx.OBJECT_DTYPE)] + [("mc/" + n, mc.cached_scene(n)) for n in mc.SCENES]
    assert sorted(want) == sorted(n for n, _ in every)
    for name, objs in every:
        pk = bm.pack_for(objs)
        h = hashlib.sha256()
        for k in ("centre", "cmax", "limit32", "limit", "abs_pad", "inv_max32", "tri_extent", "in_tree", "kind", "rec", "lo", "hi", "free"):
            h.update(_bits(pk)[k])
        assert h.hexdigest() == want[name], name
        same = bm.deform(objs, np.zeros(0, dtype=np.uint64), objs[:0])
        a, b = _bits(pk), _bits(same)
        assert [k for k in a if a[k] != b[k]] == [], name
        assert sorted(set(b) - set(a)) == ["filt", "fw", "sweep"], name        # (sweep: the LDS sweep's records, tests/test_sweep_filters.py)


def test_a_deform_keeps_what_the_rays_are_built_from():
    """the premises of aiming with the base pack: the updated list's fresh pack puts the same objects in the tree with the same free
    axes; the model keeps centre, origin_limit and abs_pad, and every triangle the update does not name keeps pack()'s bits.  The
    fresh pack has ANOTHER centre on all seven pairs (it moves by 0.01 on mixed / with_spheres ... 0.35 on t300 / ten, 0.51 on t40 /
    grow), so "records against the fresh centre" is a different scene on each; t40 / grow is the one pair whose tri_extent GROWS
    (4.05 to 5.06: a stale one would be too small); on the shrinks and on t300 / ten it falls, slide and jitter are clipped to the
    vertex box and leave it."""
    differ = set()
    for pair in PAIRS:
        base, idx, new, now = lists(pair)
        base_pk, ref = packs(pair)
        fresh = bm.pack(now)
        assert np.array_equal(fresh["in_tree"], base_pk["in_tree"]) and np.array_equal(fresh["free"], base_pk["free"]), pair
        assert np.array_equal(ref["in_tree"], base_pk["in_tree"]) and np.array_equal(ref["free"], base_pk["free"]), pair
        assert ref["limit32"] == base_pk["limit32"] and np.array_equal(ref["centre"], base_pk["centre"]) and ref["abs_pad"] == base_pk["abs_pad"]
        assert ref["tri_extent"] == mc.tri_extent(now, base_pk["centre"]), pair      # (the second restatement, to the bit)
        named = np.zeros(len(base), dtype=bool)
        named[idx.astype(np.int64)] = True
        rest = ~named & (base_pk["kind"] == 2)
        for k in ("rec", "lo", "hi"):                       # a triangle the update does not name keeps pack()'s bits
            assert np.array_equal(ref[k][rest].view(np.uint32), base_pk[k][rest].view(np.uint32)), (pair, k)
        moved = named & base_pk["in_tree"] & (base_pk["kind"] == 2)
        assert moved.any() and (ref["rec"][moved].view(np.uint32) != base_pk["rec"][moved].view(np.uint32)).any(), pair
        if not np.array_equal(fresh["centre"], base_pk["centre"]):
            differ.add(_label(pair))
        print("%s: %d entries, %d in-tree triangles moved, tri_extent %.4f -> %.4f, centre shift %.3g" % (
            _label(pair), len(idx), int(moved.sum()), base_pk["tri_extent"], ref["tri_extent"], np.abs(fresh["centre"] - base_pk["centre"]).max()))
    assert differ == {_label(p) for p in PAIRS}
    grows = {_label(p) for p in PAIRS if packs(p)[1]["tri_extent"] > packs(p)[0]["tri_extent"]}
    assert grows == {"t40/grow"}
    assert packs(("t40", "grow"))[1]["tri_extent"] > 1.2 * packs(("t40", "grow"))[0]["tri_extent"]
    base_pk, ref = packs(("mixed", "with_spheres"))         # the spheres named in the same call: new records (cmax stays: 5.772, the
    sph = base_pk["kind"] == 0                              # sphere that reaches furthest is not among the moved third)
    assert (ref["rec"][sph].view(np.uint32) != base_pk["rec"][sph].view(np.uint32)).any() and ref["cmax"] == base_pk["cmax"]


def test_generator_conditions_on_the_deformed_scenes():
    """On the reference alone, as test_update_bounds.test_generator_conditions_on_the_updated_scenes: in every pair x regime used
    (CROWDED excepted, by name) at least half of the aimed pairs are reported by the text, each displacement sign occurs among the
    reported and among the unreported pairs, and no case exceeds bounds_cases.MAX_PAIRS.  The measured shares per cell are in
    profiles/bounds_margin_use.txt: 0.61 to 0.71 on the 34 cells used, 0.296 on cubes25 / slide / surface, the cell left out."""
    for pair, regime in CASES + sorted(CROWDED):
        cs = case(pair, regime)
        am, rep, sg = cs["aimed"], cs["reported"], cs["sign"]
        assert am.sum() <= bc.MAX_PAIRS, (pair, regime)
        print("%s %s: %d aimed pairs, reported share %.3f" % (_label(pair), regime, am.sum(), rep[am].mean()))
        if (pair, regime) in CROWDED:                       # (the record of why it is left out: a cell that turns good is noticed)
            assert 2 * rep[am].sum() < am.sum(), (pair, regime, rep[am].mean())
            continue
        assert 2 * rep[am].sum() >= am.sum(), (pair, regime, rep[am].mean())
        for s in (-1, 1):
            assert (~rep[am & (sg == s)]).any(), (pair, regime, s)
            assert rep[am & (sg == s)].any(), (pair, regime, s)


def _stride(cs):
    return max(1, len(cs["t"]) // CPU_PAIRS)


def test_the_deform_models_tree_has_the_property():
    """the deform model's records, boxes and tri_extent with the kept centre and the shipped margins: no violation on any pair x
    regime, for the 128-byte and (t40, t300: the pure (x, y) trees) the 64-byte one-node paths, best_up = round_up32(t) and +inf"""
    looked = 0
    for pair, regime in CASES:
        cs = sub(case(pair, regime), _stride(case(pair, regime)))
        _, ref = packs(pair)
        for node_form in (0, 2):
            for tight in (True, False):
                bad, n = model_violations(cs, ref, node_form, tight)
                assert not any(bad.values()), (pair, regime, node_form, tight, bad)
                looked += n
    assert looked > 40000


def _weakened(which):
    """a wrong deform, on WHOLE cases (a weakening can show on one pair in 20 000): -> {(pair label, regime, node form, property):
    violations}.  centre: the walk is told the FRESH pack's centre, the records are offsets from the kept one.  boxes: every own box
    and rectangle is the base pack's (mode A's tribox32 or mode B not run).  B: the filter rectangle of every (x, y) triangle is the
    base pack's.  extent / extent0: tri_extent is the base pack's / 0 (mode D not run)."""
    total = {}
    for pair, regime in CASES:
        base_pk, ref = packs(pair)
        pk, over = ref, {}
        if which == "centre":
            over = dict(centre=bm.pack(lists(pair)[3])["centre"])
            if np.array_equal(over["centre"], ref["centre"]):
                continue
        elif which == "boxes":
            pk = dict(ref, lo=base_pk["lo"], hi=base_pk["hi"], lo128=base_pk["lo"], hi128=base_pk["hi"])
        elif which == "B":
            rec = ref["rec"].copy()
            xy = ref["free"] == 2
            rec[xy, 4:8] = base_pk["rec"][xy, 4:8]
            pk = dict(ref, rec=rec)
        elif which == "extent":
            if not ref["tri_extent"] > base_pk["tri_extent"]:
                continue                                    # (a stale tri_extent that is LARGER only loosens the bounds)
            pk = dict(ref, tri_extent=base_pk["tri_extent"])
        else:
            pk = dict(ref, tri_extent=0.0)
        cs = case(pair, regime)
        for node_form in (0, 2):
            bad, _ = model_violations(cs, pk, node_form, True, **over)
            for k, v in bad.items():
                if v:
                    total[(_label(pair), regime, node_form, k)] = v
    print("%s: %d violations in %d pair x regime x form x property cells" % (which, sum(total.values()), len(total)))
    per = {}
    for k, v in total.items():
        per[(k[0], k[3])] = per.get((k[0], k[3]), 0) + v
    for k in sorted(per):
        print("   ", k, per[k])
    return total


def _unseen(total):
    """the cells of CASES with no violation"""
    return {"%s-%s" % (_label(p), r) for p, r in CASES} - {"%s-%s" % (k[0], k[1]) for k in total}


def test_records_against_the_fresh_centre_are_caught():
    """the walk told the FRESH pack's centre while the records are offsets from the kept one (or the reverse: a deform that wrote its
    records against a recomputed centre): 762 961 violations, on every pair -- all seven centres differ -- and in every cell but
    far10 of the three pairs whose centre moves least (mixed / with_spheres 0.010, t300 / jitter 0.013, t40 / shrink 0.032: there
    |p|_1 is 5e4 and the margins, which scale with S = tri_extent + |p|_1 + 1, are wider than the shift)"""
    total = _weakened("centre")
    assert {k[0] for k in total} == {_label(p) for p in PAIRS}
    assert {k[3] for k in total} >= {"not a candidate", "t_lo above t", "t_hi below t", "certain but unreported"}
    assert _unseen(total) == {"mixed/with_spheres-far10", "t300/jitter-far10", "t40/shrink-far10"}


def test_stale_boxes_and_rectangles_are_caught():
    """the own boxes and rectangles of the BASE pack under the deformed records (a deform that did not write tribox32, or whose
    level passes did not run): "path not entered" (61 414, and 42 "entry bound above t") in every cell of every pair except the two
    of t40 -- on t40 / shrink and t40 / grow the stale box still contains every deformed footprint (a shrink stays inside; grow
    moves one vertex along its triangle's FREE axis), so it is only looser, which these rays cannot see and no answer depends on"""
    total = _weakened("boxes")
    assert {k[0] for k in total} == {_label(p) for p in PAIRS} - {"t40/shrink", "t40/grow"}
    assert _unseen(total) == {"%s-%s" % (_label(p), r) for p, r in CASES if p[0] == "t40"}
    assert {"path not entered"} <= {k[3] for k in total} <= {"path not entered", "entry bound above t"}
    assert {k[0] for k in total if k[3] == "path not entered"} == {k[0] for k in total}
    for pair in (("t40", "shrink"), ("t40", "grow")):       # the reason, checked: every deformed own box lies inside the stale one
        base_pk, ref = packs(pair)
        tree = base_pk["in_tree"]
        assert (base_pk["lo"][tree] <= ref["lo"][tree]).all() and (base_pk["hi"][tree] >= ref["hi"][tree]).all(), pair


def test_a_stale_filter_rectangle_is_caught():
    """B of the BASE pack in the record of every (x, y) triangle (a deform that wrote A, g0, g1 and forgot the grown rectangle): "not
    a candidate" (42 234) exactly on the pairs where the rectangle of an (x, y) triangle reaches beyond its old one -- t300 / jitter,
    planes_mesh / slide, t300 / ten, cubes25 / slide; not on the shrinks (t40 / shrink, mixed / with_spheres: the old rectangle
    contains the new one) and not on t40 / grow (the vertex moves along z: no rectangle changes)"""
    total = _weakened("B")
    seen = {k[0] for k in total}
    assert {k[3] for k in total} == {"not a candidate"}
    outward = {_label(p) for p in PAIRS if _moved_xy(p)[1]}
    assert seen == outward, (seen, outward)
    assert seen >= {"t300/jitter", "planes_mesh/slide"} and not seen & {"t40/shrink", "t40/grow", "mixed/with_spheres"}
    assert not _moved_xy(("t40", "grow"))[0] and _moved_xy(("t40", "shrink"))[0]
    assert not any(k[1] == "far10" for k in total)          # at 2^10 origin_limit the filter's margin A = 64uS, S = 5e4, is wider than these moves


def test_a_stale_tri_extent_is_not_seen_by_these_rays():
    """tri_extent of the BASE pack where the deform's is larger (t40 / grow: 4.05 against 5.06, 25 %) -- and even tri_extent = 0 on
    every pair: NO violation on any aimed pair.  A finding, not a failure, as test_update_bounds records it for sphere_cmax.
    tri_extent enters the walk only through S = tri_extent + |p|_1 + 1 (p = origin - centre), the scale of tri_filter_sign's margin
    A = 64uS and of tri_bounds' e_nv = 16uS and (a, b) margins, and the aimed origins keep |p|_1 large: its median is 3.4 to 11.4 in
    the inside and surface regimes (tri_extent is 3.1 to 5.1), 14 and more from `edge` outward.  Measured over every triangle pair of
    the 34 cells: the stale value makes S smaller by at most 15 % (t40 / grow, inside); tri_extent = 0 leaves 0.23 of S on the worst
    pair (t300 / ten, inside: |p|_1 = 0.30), 0.55 to 0.95 in the median, and 1.000 on far10.  Against that the worst aimed pair of a
    fresh tree uses 0.25 of e_nv and the others below 0.09 (profiles/bounds_margin_use.txt, "device triangle t_lo", surface's t = 0
    pairs aside): the pair that starts next to the centre and the pair that needs its margin are not the same pair.  A ray that
    needed the term would start within a fraction of a unit of the centre and graze a triangle at the scene's rim with the
    roundings of n . (v0 - p) all on one side; the generator does not aim there.
    What holds a stale tri_extent is therefore not this property but the bit comparison of info[6] with the deform model's value in
    test_the_deform_left_the_models_records, slot 12 of the digests of tests/test_mesh_update_gpu.py, and tests/test_mesh_update.py's
    comparison with numpy's max to the bit."""
    assert packs(("t40", "grow"))[1]["tri_extent"] > packs(("t40", "grow"))[0]["tri_extent"]
    assert not _weakened("extent")
    assert not _weakened("extent0")


# ---- the gpu part ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """the deformed resident scenes of this module's gpu tests are shared among them and freed when the module is done"""
    yield
    for h in _OPEN:
        h.close()
    del _OPEN[:]
    _handle.cache_clear()
    _product_handle.cache_clear()
    _fresh_handle.cache_clear()


_OPEN = []


def _deformed(pair, **how):
    import rust_raytracing_amd as rtx
    base, calls = steps(pair)
    hnd = hip_scene(rtx, base, rays_per_pixel=1, **how.pop("cfg", {})).upload(0, **how)
    _OPEN.append(hnd)
    for k, (idx, new) in enumerate(calls):
        assert hnd.update_objects(idx, new, mode="deform") == "refit", (pair, k)
    return hnd


@functools.lru_cache(maxsize=None)
def _handle(pair):
    return _deformed(pair, lab=True)


@functools.lru_cache(maxsize=None)
def _product_handle(pair, kernel):
    return _deformed(pair, cfg=dict(kernel=kernel))


@functools.lru_cache(maxsize=None)
def _fresh_handle(pair):
    import rust_raytracing_amd as rtx
    _OPEN.append(hip_scene(rtx, lists(pair)[3], kernel=rtx.RTX_KERNEL_AUTO, rays_per_pixel=1).upload(0))
    return _OPEN[-1]


def _has_64(pk):
    """the tree has 64-byte nodes: a pure (x, y)-footprint tree (BvhQNode; none of the pairs is a sphere-only tree)"""
    return bool((pk["free"][pk["in_tree"]] == 2).all())


@pytest.mark.gpu
@pytest.mark.parametrize("pair,regime", CASES, ids=IDS)
def test_the_walks_bounds_hold_after_a_deform(gpu, pair, regime):
    """rtx_debug_path_bounds on the DEFORMED handle, every node / ray / leaf form the tree has (the 64-byte forms on t40 and t300;
    the sphere-only leaf forms flag a triangle 64 and are looked at on mixed's spheres), best_up = round_up32(t) and +inf: the
    property of test_walk_bounds.test_the_walks_bounds_hold_on_the_device, no tolerance.  The in-tree flag is the base pack's and NO
    WALK follows the base origin_limit."""
    hnd = _handle(pair)
    base_pk, _ = packs(pair)
    cs = case(pair, regime)
    o, d, tg = cs["o"], cs["d"], cs["target"]
    form_m, _ = bm.ray_form(o, d, base_pk["limit32"])
    looked = 0
    with np.errstate(all="ignore"):
        for form, what in FORMS:
            if (form & 2) and not _has_64(base_pk):
                continue
            for tight in (True, False):
                out = hnd.debug_path_bounds(o, d, tg, _best(cs, tight), form=form)
                flags, entered, bound, leaf = device_observation(out)
                assert np.array_equal((flags & 3) == 3, form_m == 3), (pair, regime, what)
                walked = (flags & 3) != 3
                assert np.array_equal(((flags & 4) != 0)[walked], base_pk["in_tree"][tg][walked]), (pair, regime, what)
                far_form = np.where((form & 1) != 0, 2, 1)
                assert np.array_equal((flags & 3)[walked], np.where(form_m == 0, 0, far_form)[walked]), (pair, regime, what)
                active = walked & ((flags & 4) != 0) & ((flags & 64) == 0)
                bad = bm.check(cs["t"], cs["reported"], entered, bound, leaf, active)
                n_bad = {k: int(v.sum()) for k, v in bad.items() if v.any()}
                first = {k: int(np.nonzero(v)[0][0]) for k, v in bad.items() if v.any()}
                assert not n_bad, (pair, regime, what, "tight" if tight else "+inf", n_bad, first)
                looked += int(active.sum())
    assert looked > 0


def _path_boxes(path, k, live):
    """step k of the rows `live` of a 128-byte path as (lo, hi) (m, 3) f64: a footprint child is unbounded along z"""
    f = path.view(np.float32)
    flat = path[live, k, 0] == 1
    assert (flat | (path[live, k, 0] == 0)).all()
    ninf, pinf = np.full(int(live.sum()), -np.inf, dtype=np.float32), np.full(int(live.sum()), np.inf, dtype=np.float32)
    lo = np.where(flat[:, None], np.stack([f[live, k, 1], f[live, k, 2], ninf], axis=1), f[live, k, 1:4])
    hi = np.where(flat[:, None], np.stack([f[live, k, 3], f[live, k, 4], pinf], axis=1), f[live, k, 4:7])
    return lo.astype(np.float64), hi.astype(np.float64), flat


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=[_label(p) for p in PAIRS])
def test_the_deform_left_the_models_records(gpu, pair):
    """On the RESIDENT data of the deformed handle (the hook's scene_info, records and path boxes), on every 4th pair of `inside` and
    `far10`: centre, origin_limit and inv_max are the base pack's; tri_extent is the deform model's BIT FOR BIT (mode D's maximum
    against the kept centre) and sphere_cmax the model's; the 16-word records of every triangle are the model's, the sphere and filter
    records as test_update_bounds checks them; on every step of a triangle's path the rectangle or box contains the triangle's own
    model footprint on its two bounded axes (a footprint child only above an (x, y) triangle); the fma-only slab tests (box_entry32,
    rect_entry32, qrect_entry) equal bounds_model.walk_steps on the returned path bit for bit; t_lo, t_hi and the candidate flag of
    the phased and the inline triangle leaf equal bounds_model.leaf_bounds on the MODEL's records bit for bit (the f32 division taken
    as correctly rounded); on t40 and t300 every decoded BvhQNode child rectangle contains the 128-byte rectangle of the same step.
    (No equality with bounds_model.q_node: the refit picks its own origin and step.)"""
    hnd = _handle(pair)
    base_pk, ref = packs(pair)
    for regime in ("inside", "far10"):
        cs = sub(case(pair, regime), 4)
        o, d, tg = cs["o"], cs["d"], cs["target"]
        best = _best(cs, True)
        _, in32 = bm.ray_form(o, d, base_pk["limit32"])
        q = bm.make_ray32(o, d, base_pk["inv_max32"], in32)
        tri = ref["kind"][tg] == 2
        free = ref["free"][tg]
        own_lo, own_hi = ref["lo"][tg].astype(np.float64), ref["hi"][tg].astype(np.float64)
        bounded = free[:, None] != np.arange(3)[None, :]
        boxes = None
        for form in (0, 2):
            if (form & 2) and not _has_64(base_pk):
                continue
            out, info, rec, path = hnd.debug_path_bounds(o, d, tg, best, form=form | 0x800, path_steps=12)
            flags, entered, bound, leaf = device_observation(out)
            act = ((flags & 3) != 3) & ((flags & 4) != 0)
            assert np.array_equal(info[:3], base_pk["centre"]), (pair, info[:3])
            assert info[4] == float(base_pk["limit32"]) and info[5] == float(base_pk["inv_max32"]), (pair, info[:8])
            assert np.float64(info[6]).view(np.uint64) == np.float64(ref["tri_extent"]).view(np.uint64), (pair, info[6], ref["tri_extent"])
            assert np.float64(info[3]).view(np.uint64) == np.float64(ref["cmax"]).view(np.uint64), (pair, info[3], ref["cmax"])
            assert act.any() and (act & tri).any() and out[act, 1].max() <= 12
            sph = act & ~tri
            assert sph.any() == (pair[0] == "mixed")
            assert np.array_equal(rec[act & tri], ref["rec"][tg][act & tri].view(np.uint32)), (pair, regime)
            assert np.array_equal(rec[sph][:, :4], ref["rec"][tg][sph][:, :4].view(np.uint32)), (pair, regime)
            filt = np.ascontiguousarray(ref["filt"][tg][sph]).view(np.uint32)
            assert np.array_equal(rec[sph][:, 4:8], filt) and np.array_equal(rec[sph][:, 8:12], filt), (pair, regime)
            assert not rec[sph][:, 12:].any()
            lens = np.where(act, out[:, 1], 0).astype(int)
            m_entered, m_bound = bm.walk_steps(bm.device_steps(path, lens), q, best)
            assert np.array_equal(entered[act], m_entered[act]), (pair, regime, form)
            assert np.array_equal(bound[act].view(np.uint32), m_bound[act].view(np.uint32)), (pair, regime, form)
            f = path.view(np.float32)
            if form == 0:
                boxes = path
                last = path[np.arange(len(tg)), np.maximum(lens - 1, 0)].view(np.float32)
                assert np.array_equal(last[sph][:, 1:4], ref["lo"][tg][sph]) and np.array_equal(last[sph][:, 4:7], ref["hi"][tg][sph]), (pair, regime)
                for k in range(path.shape[1]):
                    live = act & (k < lens)
                    if not live.any():
                        continue
                    lo, hi, flat = _path_boxes(path, k, live)
                    assert (free[live][flat] == 2).all(), (pair, regime, k)      # a footprint child only above an (x, y) triangle
                    b = bounded[live]
                    assert (lo[b] <= own_lo[live][b]).all() and (hi[b] >= own_hi[live][b]).all(), (pair, regime, k)
            else:
                g = boxes.view(np.float32)
                for k in range(path.shape[1]):
                    live = act & (k < lens)
                    if not live.any():
                        continue
                    assert (path[live, k, 0] == 3).all() and (boxes[live, k, 0] == 1).all(), (pair, regime, k)
                    assert np.array_equal(path[live, k, 15], boxes[live, k, 15]), (pair, regime, k)
                    org, stp = f[live, k, 1:3].astype(np.float64), f[live, k, 3:5].astype(np.float64)
                    ql = np.stack([path[live, k, 5] & 0xFFFF, path[live, k, 6] & 0xFFFF], axis=1).astype(np.float64)
                    qh = np.stack([path[live, k, 5] >> 16, path[live, k, 6] >> 16], axis=1).astype(np.float64)
                    dlo, dhi = org + ql * stp, org + qh * stp      # (exact in f64: an f32, an integer below 2^16, a power of two)
                    assert (dlo <= g[live, k, 1:3].astype(np.float64)).all() and (dhi >= g[live, k, 3:5].astype(np.float64)).all(), (pair, regime, k)
                    assert (dlo <= own_lo[live][:, :2]).all() and (dhi >= own_hi[live][:, :2]).all(), (pair, regime, k)
        mleaf = bm.leaf_bounds(ref["kind"][tg], ref["rec"][tg], o, d, base_pk["centre"], ref["cmax"], ref["tri_extent"], best)
        for lform in (0x000, 0x200):                        # the phased walks' tri_filter_sign + tri_bounds, mesh_step's inline leaf
            out = hnd.debug_path_bounds(o, d, tg, best, form=lform)
            flags, entered, bound, leaf = device_observation(out)
            t_c = ((flags & 3) != 3) & ((flags & 4) != 0) & ((flags & 64) == 0) & tri
            cand = leaf["cand"]
            assert t_c.any() and cand[t_c].any()
            assert np.array_equal(cand[t_c], mleaf["cand"][t_c]), (pair, regime, lform)
            assert np.array_equal(leaf["tlo_hi"][t_c & cand].view(np.uint32), mleaf["tlo_hi"][t_c & cand].view(np.uint32)), (pair, regime, lform)
            assert np.array_equal(leaf["thi_lo"][t_c & cand].view(np.uint32), mleaf["thi_lo"][t_c & cand].view(np.uint32)), (pair, regime, lform)


@pytest.mark.gpu
@pytest.mark.parametrize("pair,regime", CASES, ids=IDS)
def test_auto_equals_exact_on_rays_aimed_at_the_deformed_scene(gpu, pair, regime):
    """the end-to-end anchor on the deformed handle (the product library): query under AUTO -- the real walk of the refitted tree --
    equals RTX_KERNEL_EXACT bit for bit on every 4th ray of the case, and AUTO on a FRESH upload of the updated list"""
    o, d = case(pair, regime)["o"][::4], case(pair, regime)["d"][::4]
    got = [_product_handle(pair, kernel).query(o, d) for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT)]
    check_equal(got[0], got[1], "%s, %s" % (_label(pair), regime))
    check_equal(got[0], _fresh_handle(pair).query(o, d), "%s, %s: a fresh upload" % (_label(pair), regime))
