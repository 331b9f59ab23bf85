"""The tree walks' f32 bounds, held to the f64 text of the reference on rays aimed at their margins.

Every result of the library is decided in f64; WHICH shapes reach the f64 test is decided in f32 by slab tests and distance bounds
whose margins were derived by hand.  A margin that is a factor too small prunes the true winner -- but only for a ray
within a few f32 ulps of a box face, a tangent or an edge, which the frame and query tests (random rays, or rays aimed at the f64
thresholds of the text) meet about once in 10^7 ray-box pairs.  Here the bounds themselves are looked at, on tests/bounds_cases.py's rays:

  the property (for every pair (ray, object j) the walk would take, j in the tree; t = the text's distance, tests/text_shapes.py F64):
    the text reports t (Some, normal, positive), with best_up = round_up32(t) and with best_up = +inf:
        every step of j's path enters j's child, the largest entry bound is <= t, j is a candidate, t_lo <= t, certain => t <= t_hi;
    the text does not report j (None, negative, zero, subnormal, NaN, culled): "certain" is false.
    f32 bounds and f64 distances are compared exactly (an f32 is an f64 value).

  CPU part -- tests/bounds_model.py: every f32 operation exact and rounded once, every margin a factor.  The model with the shipped
  margins has the property on the generator's rays; with ONE margin set to zero it must not, or the rays are not sharp enough to
  notice that margin.  SHARP lists the margins a weakening of which is caught, LOOSE the ones for which no ray of the generator can
  be made to violate -- a finding, not a failure: the margin is larger than what the worst aimed ray needs, see
  profiles/bounds_margin_use.txt for the measured shares.

  gpu part -- rtx_debug_path_bounds (the lab library) runs the walks' own device functions along j's path: the same property on the
  device; the no-walk flag is set exactly beyond 2^27 origin_limit, for a NaN origin and a non-unit direction; the fma-only slab tests
  equal the model bit for bit on the resident boxes, the sqrt and division paths lie in the model's intervals, and the resident records
  are the ones the model's restated builder makes -- so the CPU part speaks about the device's code; AUTO == RTX_KERNEL_EXACT on the
  same rays ties the scenes to the real walk.

Findings of the first run (MI355X, ROCm 7.2) are in the docstrings of the tests below and in profiles/bounds_margin_use.txt."""
import functools

import numpy as np
import pytest

import bounds_cases as bc
import bounds_model as bm
from helpers import check_equal, hip_scene

CPU_PAIRS = 1000                                          # pairs per scene x regime in the CPU part (every k-th ray of the case)
SCENES = ("s5", "s6", "spheres200", "cloud", "dust", "tris300", "planes_mesh", "mixed", "s6_big", "s6_tiny")
# scene x regime combinations that walk but cannot meet the generator's conditions (at least half of the aimed rays reported), by name:
# at these distances the TEXT's own discriminant b^2 - 4ac has an ulp far above r^2, Sphere::distance reports noise (about one ray in
# nine) whatever the ray is aimed at.  They stay in the property tests -- what is reported must still be found -- and out of the conditions.
NOISE = {(s, "far26") for s in ("s5", "s6", "spheres200", "cloud", "dust", "mixed")} | {("dust", "far10"), ("cloud", "far10")}
# ... and the one whose outward rays are never reported: the origins of spheres200's surface regime lie within a few radii of the
# target, where the f64 text resolves even the smallest delta (1 ulp of f64 at the SCENE's scale is 16 ulps there) -- correctly so.
EXACT_OUTSIDE = {("spheres200", "surface")}
# Margins whose weakening the aimed rays catch / do not catch (module docstring; measured shares: profiles/bounds_margin_use.txt).
# slack is sharp through its SECOND term alone (one pair of cloud-far10, which is why that case runs whole in the CPU part): what it
# covers there is not a rounding of the f32 side but the reference's own f64 roundings, see test_the_walks_bounds_hold_on_the_device.
# The four loose ones are covered TWICE on every ray the generator can build, which is why no ray needs any ONE of them:
#   widen -- inside origin_limit the slab distance's roundings (noi, inv, the fma: 2^-23 |t| together, 2^-23 origin_limit of position
#       at most) are within abs_pad = 2^-22 origin_limit; beyond it within ray32_slack's two terms;
#   abs_pad, abs_pad2 -- the 2^-21 |t| widening is 8 x the 2^-24 |o * inv| rounding of noi whenever the box is at least |o| / 8
#       away, nearer boxes have the builder's RELATIVE padding 2^-20 (|c| + r), 16 x the 2^-24 |o| shift, because |o| is then
#       about |c|; the 64-byte visit's extra rounding of O is 2^-24 of a distance inside the node, again within the widening; the
#       knob is live (test_every_margin_knob_reaches_the_model: the quantised boxes change);
#   K -- G enlarges sqrt(Delta) by at least G / 2r = 64uM, four times beta's 16uM that K was derived for; also on near ties
#       (test_near_ties_in_the_model: pairs less than K apart, each under the other's t_hi, with K = 0).
#   A (the triangle filter's allowance 64uS, tri_filter_from_ray; tests/test_sweep_filters.py holds it on the sweep) is sharp: with
#       A = 0 the filter drops reported triangles at edges and vertices before tri_bounds is asked.
SHARP = ("slack", "G", "e_nv", "e_dn", "e_ab", "A")
LOOSE = ("widen", "abs_pad", "abs_pad2", "K")


def _cases():
    for name in SCENES:
        for regime in bc.regimes_of(name):
            yield name, regime


def _stride(name, regime):
    if (name, regime) == ("cloud", "far10"):                # whole: the one pair that showed the far-origin hole is in it (index 16012)
        return 1
    n = {"spheres200": 20000, "tris300": 20000}.get(name, 6000) * (2 if regime == "surface" else 1)
    return max(1, n // CPU_PAIRS)


@functools.lru_cache(maxsize=None)
def _pack(name, m):
    import rust_raytracing_amd as rtx
    return bm.pack_for(dict(bc.scenes(rtx.OBJECT_DTYPE))[name], m)


def model_violations(cs, node_form, m, tight):
    """the property's violations of one case in the model: {property: count}, and the number of pairs looked at"""
    pk = _pack(cs["name"], m)
    o, d, tg = cs["o"], cs["d"], cs["target"]
    form, in32 = bm.ray_form(o, d, pk["limit32"])
    active = (form != 3) & pk["in_tree"][tg]
    steps = bm.own_steps(pk, tg, node_form, m)
    if steps is None:
        return {}, 0
    if steps[0][0] != "mixed":
        active = active & steps[0][5]
    q = bm.make_ray32(o, d, pk["inv_max32"], in32, m)
    best = np.where(cs["reported"] & tight, bm.round_up32(np.where(cs["reported"], cs["t"], 0.0)), bm.INF32).astype(np.float32)
    entered, bound = bm.walk_steps(steps, q, best, m)
    leaf = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], best, m)
    bad = bm.check(cs["t"], cs["reported"], entered, bound, leaf, active)
    return {k: int(v.sum()) for k, v in bad.items()}, int(active.sum())


def test_model_operations_round_once():
    """fma32 / add32 / mul32 against fractions.Fraction on magnitudes 1e-20 ... 1e20 with cancelling sums, ties and subnormal
    results; a * b + c through one f64 addition (two roundings) differs on some of them, so the check can tell."""
    rng = np.random.default_rng(1)
    n = 4000
    a = (rng.normal(size=n) * 10.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.normal(size=n) * 10.0 ** rng.integers(-10, 10, n)).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.choice([0, 1e-7, 3e-8, 1e-3, 1], n))).astype(np.float32)
    # c + a * b = (1 + 2^-23) + 2^-24 - 2^-60 lies just below the middle of two f32: one rounding gives c, an f64 addition first
    # rounds to the middle itself and the tie then goes to the even neighbour, 1 + 2^-22; and two subnormal results
    a = np.concatenate([a, np.float32([2.0 ** -12 * (1.0 + 2.0 ** -18), 2.0 ** -100, 2.0 ** -75])])
    b = np.concatenate([b, np.float32([2.0 ** -12 * (1.0 - 2.0 ** -18), 2.0 ** -40, 1.5 * 2.0 ** -74])])
    c = np.concatenate([c, np.float32([1.0 + 2.0 ** -23, 0.0, 2.0 ** -149])])
    want = np.array([bm.exact_fma32(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(bm.fma32(a, b, c).view(np.uint32), want.view(np.uint32))
    with np.errstate(all="ignore"):
        twice = (a.astype(np.float64) * b + c).astype(np.float32)
    assert (twice.view(np.uint32) != want.view(np.uint32)).any()
    assert np.array_equal(bm.add32(a, c).view(np.uint32), np.array([bm.exact_fma32(x, 1.0, z) for x, z in zip(a, c)]).view(np.uint32))
    assert np.array_equal(bm.mul32(a, b).view(np.uint32), np.array([bm.exact_fma32(x, y, 0.0) for x, y in zip(a, b)]).view(np.uint32))


def test_generator_conditions():
    """On the reference alone: in every scene x origin regime that walks (NOISE excepted, by name), at least half of the aimed rays are
    reported by the text for their target, and each displacement sign occurs among the reported and among the unreported rays; no case
    exceeds bounds_cases.MAX_PAIRS aimed pairs."""
    for name, regime in _cases():
        cs = bc.case(name, regime)                          # (the whole case, as the gpu part uses it)
        am, rep, sg = cs["aimed"], cs["reported"], cs["sign"]
        assert am.sum() <= bc.MAX_PAIRS, (name, regime)
        if regime == "nowalk" or (name, regime) in NOISE:
            continue
        assert 2 * rep[am].sum() >= am.sum(), (name, regime, rep[am].mean())
        for s in (-1, 1):
            assert (~rep[am & (sg == s)]).any(), (name, regime, s)
            assert rep[am & (sg == s)].any() or (s == 1 and (name, regime) in EXACT_OUTSIDE), (name, regime, s)


def test_shipped_margins_hold_in_the_model():
    """the model with the shipped constants has the property on every scene x regime, for the 128-byte and the 64-byte one-node paths,
    with best_up = round_up32(t) and +inf"""
    looked = 0
    for name, regime in _cases():
        cs = bc.case(name, regime, _stride(name, regime))
        for node_form in (0, 2):
            for tight in (True, False):
                bad, n = model_violations(cs, node_form, bm.SHIPPED, tight)
                assert not any(bad.values()), (name, regime, node_form, tight, bad)
                looked += n
    assert looked > 50000


@pytest.mark.parametrize("margin", SHARP + LOOSE)
def test_each_weakened_margin_is_caught(margin):
    """one margin set to zero, the others as shipped, the same rays: at least one violation for a margin in SHARP.  (A margin in LOOSE
    has none on any ray of the generator: reported, not asserted.)"""
    total = {}
    for name, regime in _cases():
        if regime == "nowalk":
            continue
        cs = bc.case(name, regime, _stride(name, regime))
        for node_form in (0, 2):
            bad, _ = model_violations(cs, node_form, bm.WEAKENED[margin], True)
            for k, v in bad.items():
                if v:
                    total[(name, regime, node_form, k)] = v
    print("margin %s = 0: %d violations in %d scene x regime x form x property cells" % (margin, sum(total.values()), len(total)))
    for k in sorted(total, key=lambda k: -total[k])[:6]:
        print("   ", k, total[k])
    if margin in SHARP:
        assert total, margin
    else:                                                   # the record of what was measured: a margin that turns sharp is noticed
        assert not total, (margin, total)


def _fingerprint(cs, node_form, m):
    pk = _pack(cs["name"], m)
    o, d, tg = cs["o"], cs["d"], cs["target"]
    _, in32 = bm.ray_form(o, d, pk["limit32"])
    steps = bm.own_steps(pk, tg, node_form, m)
    if steps is None:
        return []
    q = bm.make_ray32(o, d, pk["inv_max32"], in32, m)
    entered, bound = bm.walk_steps(steps, q, np.float32(np.inf), m)
    leaf = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], np.float32(np.inf), m)
    arrays = [entered, bound, q["e"], leaf["tlo_hi"], leaf["thi_lo"], leaf["cand"], leaf["certain_any"]]
    arrays += [np.asarray(x) for x in steps[0][1:5] if not isinstance(x, bool)]
    return [np.asarray(a).astype(np.float64) for a in arrays]


@pytest.mark.parametrize("margin", SHARP + LOOSE)
def test_every_margin_knob_reaches_the_model(margin):
    """a weakened Margins changes what the model computes (the boxes of the one-node paths, the ray's slack, or a bound) on some aimed
    ray: a knob that reaches nothing would make "no violation" an empty statement"""
    changed = False
    for name, regime in (("spheres200", "far10"), ("spheres200", "inside"), ("tris300", "inside")):
        cs = bc.case(name, regime, _stride(name, regime))
        for node_form in (0, 2):
            a, b = _fingerprint(cs, node_form, bm.SHIPPED), _fingerprint(cs, node_form, bm.WEAKENED[margin])
            with np.errstate(all="ignore"):
                changed = changed or any(not np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    assert changed, margin


# ---- near ties --------------------------------------------------------------------------------------------------------------------------
def tie_violations(objs, o, d, a, b, observe):
    """each shape of a near-tie pair under best_up = the other's t_hi (+inf where the other is not certain): it stays entered and a
    candidate.  observe(target, best_up) -> (entered_all, candidate, t_hi from +inf).  -> the number of violations"""
    bad = 0
    inf = np.full(len(o), np.inf, dtype=np.float32)
    for first, second in ((a, b), (b, a)):
        _, _, thi = observe(second, inf)
        entered, cand, _ = observe(first, thi)
        bad += int((~entered).sum()) + int((~cand).sum())
    return bad


def _model_observer(objs, o, d, m, node_form):
    pk = bm.pack_for(objs, m)
    _, in32 = bm.ray_form(o, d, pk["limit32"])
    q = bm.make_ray32(o, d, pk["inv_max32"], in32, m)

    def observe(target, best):
        steps = bm.own_steps(pk, target, node_form, m)
        if steps is None:
            return np.ones(len(o), dtype=bool), np.ones(len(o), dtype=bool), np.full(len(o), np.inf, dtype=np.float32)
        entered, _ = bm.walk_steps(steps, q, best, m)
        leaf = bm.leaf_bounds(pk["kind"][target], pk["rec"][target], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], best, m)
        inf_leaf = bm.leaf_bounds(pk["kind"][target], pk["rec"][target], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], np.float32(np.inf), m)
        thi = np.where(inf_leaf["certain_any"], inf_leaf["thi_lo"], np.float32(np.inf)).astype(np.float32)    # (the end that prunes most)
        return entered, leaf["cand"], thi
    return observe


def test_near_ties_in_the_model(rtx):
    """pairs whose reported distances differ by less than K (spheres) / e_nv / D (triangles): with the shipped margins neither makes the
    other a non-candidate -- nor with K = 0 (G's share of t_hi, 64uM, is above any distance below K = 24uM: K stays loose on near
    ties too), nor with e_nv = 0 for the sphere pairs; the triangle pairs DO lose each other with e_nv = 0"""
    seen = {}
    for name, objs, o, d, a, b in bc.near_ties(rtx.OBJECT_DTYPE):
        ta, ra, _ = bc.text_distances(objs, o, d, a)
        tb, rb, _ = bc.text_distances(objs, o, d, b)
        assert ra.all() and rb.all() and (np.abs(ta - tb) < 24.0 * bm.U * 5.0).all() and (ta != tb).any(), name
        for label, m in (("shipped", bm.SHIPPED), ("K", bm.WEAKENED["K"]), ("e_nv", bm.WEAKENED["e_nv"])):
            seen[(name, label)] = sum(tie_violations(objs, o, d, a, b, _model_observer(objs, o, d, m, nf)) for nf in (0, 2))
    print(seen)
    assert seen[("sphere_ties", "shipped")] == 0 and seen[("triangle_ties", "shipped")] == 0
    assert seen[("sphere_ties", "K")] == 0 and seen[("triangle_ties", "K")] == 0
    assert seen[("triangle_ties", "e_nv")] > 0


def test_product_library_has_no_path_bounds_hook(rtx):
    """rtx_lab_build() == 0 => RTX_ERR_UNSUPPORTED, before anything is looked at (no device is needed)"""
    lib = rtx.load_library()
    assert lib.rtx_lab_build() == 0
    assert lib.rtx_debug_path_bounds(None, None, None, None, 0, 0, None, None, None, None, 0) == rtx.abi.RTX_ERR_UNSUPPORTED


# ---- the gpu part ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    """the resident scenes of this module's gpu tests are shared among them and freed when the module is done"""
    yield
    for h in _OPEN:
        h.close()
    del _OPEN[:]
    _handle.cache_clear()
    _product_handle.cache_clear()


_OPEN = []


@functools.lru_cache(maxsize=None)
def _handle(name):
    import rust_raytracing_amd as rtx
    objs = dict(bc.scenes(rtx.OBJECT_DTYPE))[name]
    _OPEN.append(hip_scene(rtx, objs, rays_per_pixel=1).upload(0, lab=True))
    return _OPEN[-1]


def _f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def device_observation(out):
    """the hook's eight words as the arrays bounds_model.check takes"""
    flags = out[:, 0]
    tlo, thi = _f32(out[:, 4]), _f32(out[:, 5])
    leaf = {"cand": (flags & 8) != 0, "tlo_hi": tlo, "certain_any": (flags & 16) != 0, "thi_lo": thi}
    return flags, out[:, 2] == out[:, 1], _f32(out[:, 3]), leaf


FORMS = ((0x000, "128-byte nodes, Ray32 / Ray32S, the phased leaf tests"), (0x300, "the packet kernel's sph_packet_leaf_test"), (0x001, "... Ray64 beyond origin_limit"),
         (0x002, "64-byte nodes"), (0x100, "sphere_step's inline leaf"), (0x200, "mesh_step's inline leaf"), (0x203, "64-byte nodes, Ray64, mesh_step's leaf"))


CASES = [(n, r) for n in SCENES for r in bc.regimes_of(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime", CASES)
def test_the_walks_bounds_hold_on_the_device(gpu, name, regime):
    """rtx_debug_path_bounds on one scene x origin regime, every node / ray / leaf form the scene has, best_up = round_up32(t) and
    +inf: the property of the module docstring, no tolerance.  Also: the object is flagged in-tree exactly where the restated builder
    puts it there, and NO WALK exactly beyond 2^27 origin_limit / for a NaN origin / a direction that is not of unit length.

    What this test found (first run, MI355X, before ray32_slack had its second term): cloud-far10, one pair of 20 000 -- a sphere of
    r = 1e-3 at |c| = 5, the origin 2.1e4 away (1000 x origin_limit), the ray passing 3.05e-5 OUTSIDE the sphere: the text reports it
    all the same, t = 21415.5034, because b^2 - 4ac cancels 1.8e9 against itself and is positive by rounding; the ray is 2.1e-5
    outside the leaf's padded box (total padding 1e-5), the slack covered 1e-6 of position on that axis (d_x = -1.9e-4), box_entry32
    returned +inf and the walk dropped a shape the exhaustive kernel reports.  What the derivation had missed is not an f32 rounding:
    "a reported sphere is a real intersection" (rtx_bvh.h) holds only up to the REFERENCE'S f64 roundings, which let it report a
    sphere the ray misses by up to 2^-24.3 |o - c|.  Inside origin_limit that is within abs_pad; beyond it ray32_slack (and Ray64's
    e) now move every slab out by 2^-22 |o|_inf (rtx_traverse.h)."""
    hnd = _handle(name)
    pk = _pack(name, bm.SHIPPED)
    looked = 0
    with np.errstate(all="ignore"):
        cs = bc.case(name, regime)
        o, d, tg = cs["o"].copy(), cs["d"], cs["target"]
        if regime == "nowalk":
            o[::7, 0] = np.nan                              # NaN origins: no walk
        form_m, _ = bm.ray_form(o, d, pk["limit32"])
        for form, what in FORMS:
            if (form & 2) and not (pk["kind"][pk["in_tree"]] == 0).all() and not (pk["free"][pk["in_tree"]] == 2).all():
                continue                                    # a joint tree has no 64-byte nodes (the hook refuses: tested below)
            for tight in (True, False):
                best = np.where(cs["reported"] & tight, bm.round_up32(np.where(cs["reported"], cs["t"], 0.0)), bm.INF32).astype(np.float32)
                out = hnd.debug_path_bounds(o, d, tg, best, form=form)
                flags, entered, bound, leaf = device_observation(out)
                assert np.array_equal((flags & 3) == 3, form_m == 3), (name, regime, what)
                walked = (flags & 3) != 3
                assert np.array_equal(((flags & 4) != 0)[walked], pk["in_tree"][tg][walked]), (name, regime, what)
                far_form = np.where((form & 1) != 0, 2, 1)
                assert np.array_equal((flags & 3)[walked], np.where(form_m == 0, 0, far_form)[walked]), (name, regime, what)
                active = walked & ((flags & 4) != 0) & ((flags & 64) == 0)
                if regime == "nowalk":
                    assert not (out[~walked, 1:] != np.array([0, 0, 0, 0, 0, 0, 0xFFFFFFFF], dtype=np.uint32)).any()
                bad = bm.check(cs["t"], cs["reported"], entered, bound, leaf, active)
                n_bad = {k: int(v.sum()) for k, v in bad.items() if v.any()}
                first = {k: int(np.nonzero(v)[0][0]) for k, v in bad.items() if v.any()}
                assert not n_bad, (name, regime, what, "tight" if tight else "+inf", n_bad, first)
                looked += int(active.sum())
    assert looked > 0 or regime == "nowalk"


@pytest.mark.gpu
def test_forms_a_tree_does_not_have_are_refused(gpu):
    hnd = _handle("mixed")
    with pytest.raises(gpu.abi.RtxError):
        hnd.debug_path_bounds(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), [0], np.inf, form=2)
    with pytest.raises(gpu.abi.RtxError):
        hnd.debug_path_bounds(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), [0], np.inf, form=0x400)
    with pytest.raises(gpu.abi.RtxError):
        hnd.debug_path_bounds(np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]]), [10 ** 6], np.inf)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_the_model_is_the_devices_arithmetic(gpu, name):
    """On the RESIDENT data (the hook's records and path boxes): the records are the ones bounds_model.pack restates; the object's own
    box lies inside its leaf's box; the fma-only slab tests (box_entry32 for Ray32 / Ray32S, rect_entry32, qrect_entry: the largest
    entry distance on the path, and which steps are entered -- also for the 64-byte sphere visit, which returns no distance) equal the
    model BIT FOR BIT; t_lo and t_hi of the sphere bounds lie in the model's sqrt intervals; the triangle bounds, whose only inexact
    operation is the f32 division taken as correctly rounded, equal the model bit for bit."""
    hnd = _handle(name)
    pk = _pack(name, bm.SHIPPED)
    for regime in bc.regimes_of(name):
        if regime == "nowalk":
            continue
        cs = bc.case(name, regime, 4)
        o, d, tg = cs["o"], cs["d"], cs["target"]
        best = np.where(cs["reported"], bm.round_up32(np.where(cs["reported"], cs["t"], 0.0)), bm.INF32).astype(np.float32)
        form_m, in32 = bm.ray_form(o, d, pk["limit32"])
        q = bm.make_ray32(o, d, pk["inv_max32"], in32)
        for form in (0, 2):
            if (form & 2) and not (pk["kind"][pk["in_tree"]] == 0).all() and not (pk["free"][pk["in_tree"]] == 2).all():
                continue
            out, info, rec, path = hnd.debug_path_bounds(o, d, tg, best, form=form, path_steps=12)
            flags, entered, bound, leaf = device_observation(out)
            act = ((flags & 3) != 3) & ((flags & 4) != 0)
            assert info[4] == float(pk["limit32"]) and info[5] == float(pk["inv_max32"]) and info[3] == pk["cmax"], (name, info[:8])
            assert np.array_equal(info[:3], pk["centre"]) and info[6] == pk["tri_extent"]
            assert out[act, 1].max() <= 12
            assert np.array_equal(rec[act], pk["rec"][tg][act].view(np.uint32)), (name, regime)
            steps = bm.device_steps(path, np.where(act, out[:, 1], 0))
            m_entered, m_bound = bm.walk_steps(steps, q, best)
            assert np.array_equal(entered[act], m_entered[act]), (name, regime, form)
            assert np.array_equal(bound[act].view(np.uint32), m_bound[act].view(np.uint32)), (name, regime, form)
            if form == 0:                                   # the leaf's box holds the object's own box (equal when the leaf has one record)
                last = path[np.arange(len(tg)), np.maximum(out[:, 1].astype(int) - 1, 0)]
                f = last.view(np.float32)
                flat = last[:, 0] == 1
                lo = np.where(flat[:, None], np.stack([f[:, 1], f[:, 2], np.full(len(f), -np.inf, dtype=np.float32)], axis=1), f[:, 1:4])
                hi = np.where(flat[:, None], np.stack([f[:, 3], f[:, 4], np.full(len(f), np.inf, dtype=np.float32)], axis=1), f[:, 4:7])
                own_lo, own_hi = pk["lo"][tg], pk["hi"][tg]
                fin = np.isfinite(own_lo) & act[:, None] & ~(flat[:, None] & (np.arange(3) == 2)[None, :])
                assert (lo[fin] <= own_lo[fin]).all() and (hi[fin] >= own_hi[fin]).all(), (name, regime)
                sph = act & (pk["kind"][tg] == 0)
                assert np.array_equal(lo[sph], own_lo[sph]) and np.array_equal(hi[sph], own_hi[sph])      # (sphere leaves hold one record)
        mleaf = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], best)
        tri = pk["kind"][tg] == 2
        for lform in (0x000, 0x100, 0x200, 0x300):          # every copy of the leaf arithmetic: phased, sphere_step, mesh_step, packet
            out = hnd.debug_path_bounds(o, d, tg, best, form=lform)
            flags, entered, bound, leaf = device_observation(out)
            act = ((flags & 3) != 3) & ((flags & 4) != 0) & ((flags & 64) == 0)
            if lform in (0x100, 0x300):
                assert not (act & tri).any() and (((flags & 64) != 0) == (((flags & 3) != 3) & ((flags & 4) != 0) & tri)).all()
            cand = leaf["cand"]
            # spheres: inside the intervals wherever both ends agree that it is a candidate / certain
            s_c = act & ~tri & cand & mleaf["cand"] & mleaf["cand_best"]
            with np.errstate(all="ignore"):
                assert (mleaf["tlo_lo"][s_c] <= leaf["tlo_hi"][s_c]).all() and (leaf["tlo_hi"][s_c] <= mleaf["tlo_hi"][s_c]).all(), (name, regime)
                assert not (act & ~tri & mleaf["cand"] & ~cand).any() and not (act & ~tri & cand & ~mleaf["cand_best"]).any(), (name, regime)
                s_h = act & ~tri & leaf["certain_any"] & mleaf["certain_all"]
                assert (mleaf["thi_lo"][s_h] <= leaf["thi_lo"][s_h]).all() and (leaf["thi_lo"][s_h] <= mleaf["thi_hi"][s_h]).all(), (name, regime)
                assert not (act & ~tri & mleaf["certain_all"] & ~leaf["certain_any"]).any(), (name, regime)
                assert not (act & ~tri & leaf["certain_any"] & ~mleaf["certain_any"]).any(), (name, regime)
            t_c = act & tri
            assert np.array_equal(cand[t_c], mleaf["cand"][t_c]), (name, regime)
            assert np.array_equal(leaf["tlo_hi"][t_c & cand].view(np.uint32), mleaf["tlo_hi"][t_c & cand].view(np.uint32)), (name, regime)
            assert np.array_equal(leaf["thi_lo"][t_c & cand].view(np.uint32), mleaf["thi_lo"][t_c & cand].view(np.uint32)), (name, regime)


@functools.lru_cache(maxsize=None)
def _product_handle(name, kernel):
    import rust_raytracing_amd as rtx
    _OPEN.append(hip_scene(rtx, dict(bc.scenes(rtx.OBJECT_DTYPE))[name], kernel=kernel, rays_per_pixel=1).upload(0))
    return _OPEN[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime", CASES)
def test_auto_equals_the_exhaustive_kernel_on_the_aimed_rays(gpu, name, regime):
    """the end-to-end anchor: hnd.query on AUTO (the real walk of the same scene, the product library) equals RTX_KERNEL_EXACT bit for
    bit on the regime's rays (every 4th).

    What this test found (first run, MI355X, before ray32_slack had its second term): the far26 regime of s5, s6, cloud, dust and
    mixed, 2 to 8 rays of 1500 ... 6600 each -- at |o| = 2^26 origin_limit the text's Sphere::distance reports spheres the ray misses
    by tens of units (f64 cancellation in b^2 - 4ac), the exhaustive kernel reports them with it, and the walk's boxes did not let them
    through: s6, ray 7521: EXACT 1491493973.478789, AUTO +inf; s5, ray 6396: EXACT 1345463209.9160147, AUTO 1345463213.3667912 (the
    next sphere).  The cause and the repair are the ones test_the_walks_bounds_hold_on_the_device names."""
    o, d = bc.case(name, regime)["o"][::4], bc.case(name, regime)["d"][::4]
    got = [_product_handle(name, kernel).query(o, d) for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT)]
    check_equal(got[0], got[1], "%s, %s" % (name, regime))


@pytest.mark.gpu
def test_near_ties_on_the_device(gpu):
    """bounds_cases.near_ties on the device's own functions: every shape of a pair, run with best_up = its partner's device t_hi,
    stays entered and a candidate -- for the 128-byte and (spheres) the 64-byte nodes and every leaf form the pair's kind has"""
    for name, objs, o, d, a, b in bc.near_ties(gpu.OBJECT_DTYPE):
        hnd = hip_scene(gpu, objs, rays_per_pixel=1).upload(0, lab=True)
        forms = (0x000, 0x002, 0x100, 0x200, 0x300, 0x302) if name == "sphere_ties" else (0x000, 0x200)
        for form in forms:
            def observe(target, best, form=form):
                out = hnd.debug_path_bounds(o, d, target, best, form=form)
                assert ((out[:, 0] & 3) == 0).all() and ((out[:, 0] & 0x44) == 4).all(), (name, hex(form))
                return out[:, 2] == out[:, 1], (out[:, 0] & 8) != 0, _f32(out[:, 5])
            assert tie_violations(objs, o, d, a, b, observe) == 0, (name, hex(form))
            _, _, thi = observe(a, np.full(len(o), np.inf, dtype=np.float32))
            assert np.isfinite(thi).any(), (name, hex(form))                        # (some partner IS certain: the bound is a real one)
        hnd.close()
