"""The tree walks' f32 bounds on REFITTED trees (rtx_scene_update_objects), held to the f64 text on rays aimed at their margins.

tests/test_walk_bounds.py holds the bounds of freshly built trees.  A refit keeps origin_limit, abs_pad, bvh_inv_max and sphere_center
of the OLD pack, takes sphere_cmax again on the device and encodes the 64-byte nodes with a step of its own -- and the walks' margins
are functions of exactly these numbers.  The frame and query tests of tests/test_scene_update_gpu.py aim random rays at updated scenes;
the device's arrays are compared with a host reference that compiles from the same header (csrc/rtx_refit.h), so an expression that
is wrong there is wrong on both sides of that comparison.  Here the refitted tree meets the generator of tests/bounds_cases.py:

  inputs -- (scene, update) PAIRS of tests/update_cases.py; `base` is the uploaded list, `now` the updated one.  The rays are
    bounds_cases.aimed(label, now, regime, pk = the BASE pack): origin_limit and the in-tree flags are the base pack's, which a refit
    keeps; the expected answers are bounds_cases.text_distances(now, ...).
  the refit's model -- bounds_model.refit(): the records, own boxes and sphere_cmax a refit must leave, written from the documented
    contract (include/rtx_hip.h) in numpy f64.
  CPU part -- the generator's conditions on these rays; the model of the refitted tree (the refit model's records and cmax, the base
    topology as bounds_model.own_steps reads it: the leaf of one record whose box is the refitted own box, the 64-byte grid spanned
    with the next sphere's refitted box) has test_walk_bounds' property with the shipped margins; with a STALE sphere_cmax or with
    the FRESH pack's centre in place of the kept one it must not -- or the finding is that these rays cannot tell.
  gpu part -- a lab handle uploaded with `base` and updated ("refit"): the property on the device for every form the scene has; the
    resident records, boxes and scene constants are the refit model's; AUTO == RTX_KERNEL_EXACT on the same rays.

Findings of the first run are in the docstrings below and in DESIGN.md 3.13."""
import functools

import numpy as np
import pytest

import bounds_cases as bc
import bounds_model as bm
import update_cases as uc
from helpers import check_equal, hip_scene
from test_walk_bounds import FORMS, device_observation

PAIRS = (("s9", "inbox"), ("s65", "inbox"), ("s300", "all"), ("mixed", "inbox"), ("s65", "grow"))
REGIMES = ("inside", "edge", "outside", "far10", "surface")
# the surface cells that cannot meet the generator's conditions, left out by name.  The bar is not lowered: the cells are not used, and
# test_generator_conditions_on_the_updated_scenes keeps both figures honest (a cell that turns good is noticed).
#   s300 / all: the surface regime puts the origin ON the nearest other sphere; after the `all` jitter the spheres of the compacted
#       scene overlap, the origin then often lies inside the target or behind its tangent point: the text reports 0.498 of the aimed
#       pairs, below half;
#   s65 / inbox: 0.664 are reported, but NO outward ray is (0 of 4680): the origins lie within a few radii of the target, where the
#       f64 text resolves even the smallest outward delta -- test_walk_bounds' EXACT_OUTSIDE on spheres200, correctly so.
CROWDED = {(("s300", "all"), "surface"), (("s65", "inbox"), "surface")}
CPU_PAIRS = 1000


def _label(pair):
    return "%s/%s" % pair


def regimes_of(pair):
    return tuple(r for r in REGIMES if (pair, r) not in CROWDED)


CASES = [(p, r) for p in PAIRS for r in regimes_of(p)]
IDS = ["%s-%s" % (_label(p), r) for p, r in CASES]


@functools.lru_cache(maxsize=None)
def lists(pair):
    """(base, indices, new, now) of a pair"""
    base = uc.scene(pair[0])
    idx, new, how = uc.update(base, pair[1])
    assert how == "refit"
    return base, idx, new, uc.apply(base, idx, new)


@functools.lru_cache(maxsize=None)
def packs(pair):
    """(the base pack, the refit model's pack of the updated list)"""
    base, idx, new, _ = lists(pair)
    return bm.pack_for(base), bm.refit(base, idx, new)


@functools.lru_cache(maxsize=None)
def case(pair, regime):
    """bounds_cases._case for a refitted tree: the rays aimed at `now` with the BASE pack's origin_limit and in-tree flags, the surface
    regime's second pair appended, the text's answers on `now` -- computed once per process"""
    _, _, _, now = lists(pair)
    base_pk, _ = packs(pair)
    rays = bc.aimed(_label(pair), now, regime, pk=base_pk)
    o, d, target, sign, what, extra = rays["o"], rays["d"], rays["target"], rays["sign"], rays["what"], rays["extra"]
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


def sub(cs, stride):
    """a seeded random 1 / stride of a case (a fixed stride would alias with the deltas' order)"""
    n = len(cs["t"])
    if stride <= 1:
        return cs
    sel = np.sort(np.random.default_rng(5).choice(n, max(1, n // int(stride)), replace=False))
    return {k: v[sel] for k, v in cs.items()}


def _best(cs, tight):
    return np.where(cs["reported"] & tight, bm.round_up32(np.where(cs["reported"], cs["t"], 0.0)), bm.INF32).astype(np.float32)


def model_violations(cs, pk, node_form, tight, centre=None, cmax=None):
    """test_walk_bounds.model_violations on a given pack; centre / cmax: what the walk's leaf bounds are TOLD (default: the pack's own)"""
    o, d, tg = cs["o"], cs["d"], cs["target"]
    form, in32 = bm.ray_form(o, d, pk["limit32"])
    active = (form != 3) & pk["in_tree"][tg]
    steps = bm.own_steps(pk, tg, node_form)
    if steps is None:
        return {}, 0
    if steps[0][0] != "mixed":
        active = active & steps[0][5]
    q = bm.make_ray32(o, d, pk["inv_max32"], in32)
    best = _best(cs, tight)
    entered, bound = bm.walk_steps(steps, q, best)
    leaf = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"] if centre is None else centre,
                          pk["cmax"] if cmax is None else cmax, pk["tri_extent"], best)
    bad = bm.check(cs["t"], cs["reported"], entered, bound, leaf, active)
    return {k: int(v.sum()) for k, v in bad.items()}, int(active.sum())


# ---- the CPU part -----------------------------------------------------------------------------------------------------------------------
def test_a_refit_keeps_what_the_rays_are_built_from():
    """the premises of aiming with the base pack: the updated list's fresh pack puts the same objects in the tree; the refit model of
    an empty update IS pack(); s9 / inbox is the pair whose fresh pack has another origin_limit (42.21 against the kept 46.83) and
    another centre; s65 / grow is the pair whose sphere_cmax GROWS (a stale one would be too small)"""
    for pair in PAIRS:
        base, idx, new, now = lists(pair)
        base_pk, ref = packs(pair)
        assert np.array_equal(bm.pack(now)["in_tree"], base_pk["in_tree"]), pair
        same = bm.refit(base, idx[:0], new[:0])
        tree = base_pk["in_tree"]
        for k in ("rec", "lo", "hi"):
            assert np.array_equal(same[k][tree].view(np.uint32), base_pk[k][tree].view(np.uint32)), (pair, k)
        assert same["cmax"] == base_pk["cmax"]
        assert ref["limit32"] == base_pk["limit32"] and np.array_equal(ref["centre"], base_pk["centre"])
    fresh = bm.pack(lists(("s9", "inbox"))[3])
    assert abs(float(fresh["limit32"]) - 42.21) < 0.01 and abs(float(packs(("s9", "inbox"))[0]["limit32"]) - 46.83) < 0.01
    assert np.abs(fresh["centre"] - packs(("s9", "inbox"))[0]["centre"]).max() > 0.1
    assert packs(("s65", "grow"))[1]["cmax"] > packs(("s65", "grow"))[0]["cmax"] * 1.01


def test_generator_conditions_on_the_updated_scenes():
    """On the reference alone, as test_walk_bounds.test_generator_conditions: in every pair x regime used (CROWDED excepted, by name)
    at least half of the aimed pairs are reported by the text, each displacement sign occurs among the reported and among the
    unreported pairs, and no case exceeds bounds_cases.MAX_PAIRS.  Measured: the reported share is 0.62 to 0.74 on inside / edge /
    outside / far10, 0.60 to 0.70 on the three surface cells used; 0.498 on s300 / all / surface and no reported outward ray on
    s65 / inbox / surface, the two cells left out."""
    for pair, regime in CASES + sorted(CROWDED):
        cs = case(pair, regime)
        am, rep, sg = cs["aimed"], cs["reported"], cs["sign"]
        assert am.sum() <= bc.MAX_PAIRS, (pair, regime)
        print("%s %s: %d aimed pairs, reported share %.3f" % (_label(pair), regime, am.sum(), rep[am].mean()))
        if (pair, regime) in CROWDED:                       # (the record of why it is left out: a cell that turns good is noticed)
            assert 2 * rep[am].sum() < am.sum() or not rep[am & (sg == 1)].any(), (pair, regime, rep[am].mean())
            continue
        assert 2 * rep[am].sum() >= am.sum(), (pair, regime, rep[am].mean())
        for s in (-1, 1):
            assert (~rep[am & (sg == s)]).any(), (pair, regime, s)
            assert rep[am & (sg == s)].any(), (pair, regime, s)


def _stride(cs):
    return max(1, len(cs["t"]) // CPU_PAIRS)


def test_the_refit_models_tree_has_the_property():
    """the refit model's records, boxes and cmax with the kept centre and the shipped margins: no violation on any pair x regime, for
    the 128-byte and the 64-byte one-node paths, best_up = round_up32(t) and +inf"""
    looked = 0
    for pair, regime in CASES:
        cs = sub(case(pair, regime), _stride(case(pair, regime)))
        _, ref = packs(pair)
        for node_form in (0, 2):
            for tight in (True, False):
                bad, n = model_violations(cs, ref, node_form, tight)
                assert not any(bad.values()), (pair, regime, node_form, tight, bad)
                looked += n
    assert looked > 20000


def _weakened_total(which):
    total = {}
    for pair, regime in CASES:
        base_pk, ref = packs(pair)
        if which == "cmax":
            if not ref["cmax"] > base_pk["cmax"]:
                continue                                    # (a stale cmax that is LARGER only loosens the bounds)
            over = dict(cmax=base_pk["cmax"])
        else:
            over = dict(centre=bm.pack(lists(pair)[3])["centre"])
            if np.array_equal(over["centre"], ref["centre"]):
                continue
        cs = case(pair, regime)                             # whole: a weakening that shows on one pair in 20 000 must be seen
        for node_form in (0, 2):
            bad, _ = model_violations(cs, ref, node_form, True, **over)
            for k, v in bad.items():
                if v:
                    total[(_label(pair), regime, node_form, k)] = v
    print("%s: %d violations in %d pair x regime x form x property cells" % (which, sum(total.values()), len(total)))
    for k in sorted(total, key=lambda k: -total[k])[:6]:
        print("   ", k, total[k])
    return total


def test_a_record_against_the_wrong_centre_is_caught():
    """the walk told the FRESH pack's centre while the records are offsets from the kept one (or the reverse: a refit that wrote its
    records against a recomputed centre): violations on s9 / inbox and s65 / inbox, the two pairs whose centres differ"""
    total = _weakened_total("centre")
    assert total
    assert {k[0] for k in total} >= {"s9/inbox", "s65/inbox"}


def test_a_stale_sphere_cmax_is_not_seen_by_these_rays():
    """sphere_cmax of the BASE pack where the refit's is larger (s65 / grow: 5.949 against 6.023, 1.2 % -- the growth is clipped to the
    box the tree was built for, so cmax can grow by little): NO violation on any aimed pair.  A finding, not a failure, recorded as
    test_walk_bounds records its LOOSE margins: cmax enters the sphere bounds only through M = cmax + |p| in K = 24uM and G = 128uMr
    + ..., and G's share of the bound is several times what the worst aimed ray uses (profiles/bounds_margin_use.txt); a 1.2 % smaller
    M is far inside that.  What holds a stale cmax is therefore not this property but the bit comparison of info[3] with the refit
    model's cmax in test_the_refit_left_the_models_records (and the digest of tests/test_scene_update_gpu.py)."""
    assert not _weakened_total("cmax")


# ---- the gpu part ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """the updated resident scenes of this module's gpu tests are shared among them and freed when the module is done"""
    yield
    for h in _OPEN:
        h.close()
    del _OPEN[:]
    _handle.cache_clear()
    _product_handle.cache_clear()


_OPEN = []


@functools.lru_cache(maxsize=None)
def _handle(pair):
    import rust_raytracing_amd as rtx
    base, idx, new, _ = lists(pair)
    hnd = hip_scene(rtx, base, rays_per_pixel=1).upload(0, lab=True)
    _OPEN.append(hnd)
    assert hnd.update_objects(idx, new) == "refit"
    return hnd


@functools.lru_cache(maxsize=None)
def _product_handle(pair, kernel):
    import rust_raytracing_amd as rtx
    base, idx, new, _ = lists(pair)
    hnd = hip_scene(rtx, base, kernel=kernel, rays_per_pixel=1).upload(0)
    _OPEN.append(hnd)
    assert hnd.update_objects(idx, new) == "refit"
    return hnd


def _has_q3(pk):
    return bool((pk["kind"][pk["in_tree"]] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("pair,regime", CASES, ids=IDS)
def test_the_walks_bounds_hold_after_a_refit(gpu, pair, regime):
    """rtx_debug_path_bounds on the UPDATED handle, every node / ray / leaf form the scene has, best_up = round_up32(t) and +inf: the
    property of test_walk_bounds.test_the_walks_bounds_hold_on_the_device, no tolerance.  The in-tree flag is the base pack's and NO
    WALK follows the base origin_limit (no ray of these regimes is beyond 2^27 of it; the non-unit directions of `inside` are).

    What this test found (first run, MI355X): no violation on any of the 23 cells -- the kept origin_limit, abs_pad and centre and
    the refitted boxes leave the margins what they were derived for.  It does NOT see a stale sphere_cmax (it passes on a scratch
    build that drops mode C's result): test_a_stale_sphere_cmax_is_not_seen_by_these_rays says why, the next test holds cmax."""
    hnd = _handle(pair)
    base_pk, _ = packs(pair)
    cs = case(pair, regime)
    o, d, tg = cs["o"], cs["d"], cs["target"]
    form_m, _ = bm.ray_form(o, d, base_pk["limit32"])
    looked = 0
    with np.errstate(all="ignore"):
        for form, what in FORMS:
            if (form & 2) and not _has_q3(base_pk):
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


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS, ids=[_label(p) for p in PAIRS])
def test_the_refit_left_the_models_records(gpu, pair):
    """On the RESIDENT data of the updated handle (the hook's scene_info, records and path boxes): the centre, origin_limit and inv_max
    are the base pack's; sphere_cmax is the refit model's BIT FOR BIT (mode C's maximum against the kept centre); the leaf records
    and both copies of the filter record {c - centre, |c - centre|^2 - r^2} are the model's; a sphere leaf's box equals the model's own box and every box on the sphere's path contains it; the 128-byte slab
    tests equal bounds_model.walk_steps on the returned path bit for bit; every decoded 64-byte child box contains the 128-byte
    child's after the further abs_pad.  (No equality with bounds_model.q3_node: the refit may pick another step.)

    The further abs_pad is held up to the f64 roundings of the encoder's own (l - abs_pad - o) / s: two roundings of 2^-53 of a
    coordinate below origin_limit, against abs_pad = 2^-22 origin_limit: a share of 2^-30; the test allows 2^-28 of abs_pad.

    What this test found (first run, MI355X): every item holds.  On a scratch build whose host drops mode C's result it fails on
    all five pairs at sphere_cmax (s9 / inbox: resident 5.0313, the model's 3.4391; s65 / grow: 5.9490 against 6.0229)."""
    hnd = _handle(pair)
    base_pk, ref = packs(pair)
    pad = base_pk["abs_pad"] * (1.0 - 2.0 ** -28)
    for regime in ("inside", "far10"):
        cs = sub(case(pair, regime), 4)
        o, d, tg = cs["o"], cs["d"], cs["target"]
        best = _best(cs, True)
        _, in32 = bm.ray_form(o, d, base_pk["limit32"])
        q = bm.make_ray32(o, d, base_pk["inv_max32"], in32)
        boxes = None
        for form in (0, 2):
            if (form & 2) and not _has_q3(base_pk):
                continue
            out, info, rec, path = hnd.debug_path_bounds(o, d, tg, best, form=form | 0x800, path_steps=12)      # (+ the filter records)
            flags, entered, bound, leaf = device_observation(out)
            act = ((flags & 3) != 3) & ((flags & 4) != 0)
            assert np.array_equal(info[:3], base_pk["centre"]), (pair, info[:3])
            assert np.float64(info[3]).view(np.uint64) == np.float64(ref["cmax"]).view(np.uint64), (pair, info[3], ref["cmax"])
            assert info[4] == float(base_pk["limit32"]) and info[5] == float(base_pk["inv_max32"]) and info[6] == base_pk["tri_extent"]
            assert act.any() and out[act, 1].max() <= 12
            sph = act & (ref["kind"][tg] == 0)
            assert np.array_equal(rec[sph][:, :4], ref["rec"][tg][sph][:, :4].view(np.uint32)), (pair, regime)
            assert np.array_equal(rec[act & ~sph], ref["rec"][tg][act & ~sph].view(np.uint32)), (pair, regime)
            filt = np.ascontiguousarray(ref["filt"][tg][sph]).view(np.uint32)
            assert np.array_equal(rec[sph][:, 4:8], filt) and np.array_equal(rec[sph][:, 8:12], filt), (pair, regime)
            assert not rec[sph][:, 12:].any()
            lens = np.where(act, out[:, 1], 0).astype(int)
            steps = bm.device_steps(path, lens)
            m_entered, m_bound = bm.walk_steps(steps, q, best)
            assert np.array_equal(entered[act], m_entered[act]), (pair, regime, form)
            assert np.array_equal(bound[act].view(np.uint32), m_bound[act].view(np.uint32)), (pair, regime, form)
            own_lo, own_hi = ref["lo"][tg].astype(np.float64), ref["hi"][tg].astype(np.float64)
            f = path.view(np.float32)
            if form == 0:
                boxes = path
                last = path[np.arange(len(tg)), np.maximum(lens - 1, 0)].view(np.float32)
                assert (path[sph][:, 0, 0] == 0).all()
                assert np.array_equal(last[sph][:, 1:4], ref["lo"][tg][sph]) and np.array_equal(last[sph][:, 4:7], ref["hi"][tg][sph]), (pair, regime)
                for k in range(path.shape[1]):
                    live = sph & (k < lens)
                    assert (path[live, k, 0] == 0).all(), (pair, regime, k)              # a sphere's path has no footprint node
                    assert (f[live, k, 1:4] <= own_lo[live]).all() and (f[live, k, 4:7] >= own_hi[live]).all(), (pair, regime, k)
            else:
                g = boxes.view(np.float32)
                for k in range(path.shape[1]):
                    live = act & (k < lens)
                    assert (path[live, k, 0] == 2).all() and np.array_equal(path[live, k, 15], boxes[live, k, 15]), (pair, regime, k)
                    org, stp = f[live, k, 1:4].astype(np.float64), f[live, k, 4:7].astype(np.float64)
                    dlo = org + path[live, k, 7:10].astype(np.float64) * stp
                    dhi = org + path[live, k, 10:13].astype(np.float64) * stp
                    assert (dlo == dlo.astype(np.float32)).all() and (dhi == dhi.astype(np.float32)).all()      # exact in f32
                    assert (dlo <= g[live, k, 1:4].astype(np.float64) - pad).all(), (pair, regime, k)
                    assert (dhi >= g[live, k, 4:7].astype(np.float64) + pad).all(), (pair, regime, k)


@pytest.mark.gpu
@pytest.mark.parametrize("pair,regime", CASES, ids=IDS)
def test_auto_equals_exact_on_rays_aimed_at_the_updated_scene(gpu, pair, regime):
    """the end-to-end anchor on the updated handle (the product library): query under AUTO -- the real walk of the refitted tree --
    equals RTX_KERNEL_EXACT bit for bit on every 4th ray of the case"""
    o, d = case(pair, regime)["o"][::4], case(pair, regime)["d"][::4]
    got = [_product_handle(pair, kernel).query(o, d) for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT)]
    check_equal(got[0], got[1], "%s, %s" % (_label(pair), regime))
