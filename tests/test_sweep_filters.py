"""The LDS sweep's two f32 filters (trace_mixed_kernel: filter_from_ray / filter_disc2 over sphere_f32, tri_filter_from_ray /
tri_filter_sign over tri_f32), held to the f64 text of the reference on rays aimed at them.

Every result is decided in f64; which shapes reach the f64 test of the sweep is decided by these two filters, whose allowances E =
64uM^2 and A = 64uS were derived by hand (rtx_device.h).  tests/test_walk_bounds.py holds the tree walks' bounds; the sweep -- AUTO's
path for every scene without a tree, for more than 64 shapes outside it, and the product's for a sphere tree without 64-byte nodes --
was seen only through frames of random rays.

  the property (no tolerance; f32 values compared as f64): for every pair (ray, object) the text reports (tests/text_shapes.py F64:
    Some, normal, positive), the ray's filter is pass-all or the record's sign bit is clear.  Nothing is asked of unreported pairs.  A
    hidden record and a pad record are never candidates unless the ray is pass-all.  The pass-all flag is set exactly by
    !(M < 1e14) || !(M > 1e-12) (spheres; a NaN origin included) resp. !(S < 1e14) (triangles).

  CPU part -- tests/bounds_model.py sweep_record / sweep_params / sweep_disc / tri_params / tri_filter_sxy on tests/sweep_cases.py's
    rays: the shipped margins have the property on every family; E = 0 and A = 0 each lose reported pairs on the aimed families of
    every scene with such shapes; model mutations (CAUGHT / NOT_CAUGHT below); the margin use per cell
    (profiles/sweep_filter_margin_use.txt is this module's print-out: `python tests/test_sweep_filters.py`).

  gpu part -- rtx_debug_sweep_filter (the lab library) runs the sweep's own device functions on the resident records: the property on
    the device; FilterParams, TriFilterParams, D of filter_disc2 and of filter_disc1 and tri_filter_sign's word equal the model bit
    for bit; the resident records are sweep_record()'s and pack()'s -- after a refit, a deform, a hide and a hide + show too; and the
    hook's counts tie it to the launch: RtxStats.exact_tests of a MIXED frame equals what the hook counts on the transcript's segments.

  the real kernel -- limb frames (sweep_cases.limb_cameras) through RTX_KERNEL_MIXED_VERIFY, RTX_KERNEL_MIXED and AUTO against
    RTX_KERNEL_EXACT, bit for bit.

What the first runs found (MI355X): no reported pair is lost by the shipped allowances, in the model or on the device; the worst use
is 0.12 of E and 0.04 of A (profiles/sweep_filter_margin_use.txt); scratch builds with E = 0, A = 0, the refit's interleave index
swapped and a short LDS load each turn tests of this module red ("The sweep's f32 filters").
"""
import functools

import numpy as np
import pytest

import bounds_cases as bc
import bounds_model as bm
import sweep_cases as sc
from helpers import hip_scene

U = bm.U
SCENES = ("s5", "s6", "spheres200", "cloud", "dust", "tris300", "planes_mesh", "mixed", "s6_big", "s6_tiny", "s4t4", "nan200", "mixed3")
CELLS = [(n, r) for n in SCENES for r in sc.regimes_of(n)]
# the mutations of the model the rays catch / do not catch (test_model_mutations); what is not caught is a finding about the rays and
# the allowances, written down so that a change is noticed
CAUGHT = ("p2 without the factor 2", "pair swapped", "stale cmax")
NOT_CAUGHT = ("w from the f32 centre", "stale tri_extent")


# ---- one case through the model -------------------------------------------------------------------------------------------------------------
class Geo:
    """what the sweep reads of one resident scene: centre, cmax, tri_extent, the sweep's sphere records, the triangle records"""
    def __init__(self, objs, centre, cmax, tri_extent, sweep, tri_rec, has_tri_rec, hidden=None):
        self.objs, self.centre, self.cmax, self.tri_extent = objs, np.asarray(centre, dtype=np.float64), cmax, tri_extent
        self.sweep, self.tri_rec, self.has_tri_rec = sweep, tri_rec, has_tri_rec
        kind = np.asarray(objs["kind"]).astype(int)
        self.kind = kind
        self.local = np.cumsum(kind == 0) - 1                   # object -> its row of the sweep's records (scene order)
        self.hidden = np.zeros(len(kind), dtype=bool) if hidden is None else np.asarray(hidden, dtype=bool)


@functools.lru_cache(maxsize=None)
def geo_of(name):
    objs, centre, cmax, tri_extent, pk = sc.geometry(name)
    return Geo(objs, centre, cmax, tri_extent, bm.sweep_record(objs, centre), pk["rec"][:, :8], pk["free"] >= 0)


def evaluate(cs, g, m=bm.SHIPPED, mutation=None):
    """-> dict of (n,) arrays: sphere / tri (the pair has a modelled record), pass_all, cand, D, sx, sy, words (n, 8), rec (n, 8), M, A"""
    o, d, tg = cs["o"], cs["d"], cs["target"]
    sph = g.kind[tg] == 0
    tri = (g.kind[tg] == 2) & g.has_tri_rec[tg]
    loc = np.where(sph, g.local[tg], 0)
    if mutation == "pair swapped":
        loc = loc ^ 1
    srec = g.sweep[loc] if len(g.sweep) else np.zeros((len(tg), 4), dtype=np.float32)
    if mutation == "w from the f32 centre":
        c32 = srec[:, :3].astype(np.float64)
        r = np.asarray(g.objs["geom"], dtype=np.float64)[tg, 3]
        srec = srec.copy()
        srec[:, 3] = (((c32[:, 0] * c32[:, 0] + c32[:, 1] * c32[:, 1]) + c32[:, 2] * c32[:, 2]) - r * r).astype(np.float32)
    words, s_all, M = bm.sweep_params(o, d, g.centre, g.cmax, m)
    if mutation == "p2 without the factor 2":
        words = words.copy()
        words[:, 4:7] = words[:, 4:7] * np.float32(0.5)
    D = bm.sweep_disc(srec, words)
    tp = bm.tri_params(o, d, g.centre, g.tri_extent, m)
    trec = g.tri_rec[tg]
    sx, sy = bm.tri_filter_sxy(trec[:, 0:4], trec[:, 4:8], tp)
    cand = np.where(sph, ~np.signbit(D), ~(np.signbit(sx) | np.signbit(sy)))
    rec = np.zeros((len(tg), 8), dtype=np.float32)
    rec[:, :4] = srec
    rec = np.where(sph[:, None], rec, trec)
    twords = np.concatenate([tp["d"], tp["np"], tp["A"][:, None], np.zeros((len(tg), 1), dtype=np.float32)], axis=1).astype(np.float32)
    return {"sphere": sph, "tri": tri, "pass_all": np.where(sph, s_all, tp["off"]), "cand": cand, "D": D, "sx": sx, "sy": sy,
            "words": np.where(sph[:, None], words, twords), "rec": rec, "M": M, "A": tp["A"], "s_all": s_all, "t_all": tp["off"]}


def lost(cs, ev):
    """the property's violations: reported pairs with a record whose filter is not pass-all and whose sign bit is set"""
    return cs["reported"] & (ev["sphere"] | ev["tri"]) & ~ev["pass_all"] & ~ev["cand"]


def cells():
    for name, regime in CELLS:
        yield name, regime, sc.case(name, regime, sc.stride_of(name, regime))
    for name in sc.SPHERE_SCENES:
        yield name, "centre", sc.centre_case(name)
        yield name, "adversarial spheres", sc.adversarial_case(name, "spheres")
    for name in sc.TRI_SCENES:
        yield name, "adversarial triangles", sc.adversarial_case(name, "triangles")


# ---- the CPU part ---------------------------------------------------------------------------------------------------------------------------
def test_the_model_restates_the_pack():
    """sweep_record against the refit model's filter records (bounds_model.refit of an empty update: written from pack_scene's text
    for tests/test_update_bounds.py), the sentinel rows, the -1e30 rows of nan200 and its NaN cmax"""
    for name in ("s5", "s6", "spheres200", "mixed"):
        g = geo_of(name)
        pk = bm.refit(g.objs, np.zeros(0, dtype=np.uint64), g.objs[:0])
        n = int((g.kind == 0).sum())
        assert np.array_equal(g.sweep[:n].view(np.uint32), pk["filt"][g.kind == 0].view(np.uint32)), name
        assert np.array_equal(pk["sweep"].view(np.uint32), g.sweep.view(np.uint32)) and pk["cmax"] == g.cmax, name
        assert len(g.sweep) % 4 == 0 and (g.sweep[n:] == np.float32([0, 0, 0, 1e30])).all(), name
    assert len(geo_of("s5").sweep) == 8 and len(geo_of("s5").sweep[5:]) == 3
    g = geo_of("nan200")
    assert np.isnan(g.cmax) and (g.sweep == np.float32([0, 0, 0, -1e30])).all() and len(g.sweep) == 204
    g = geo_of("s6")
    hid = np.zeros(6, dtype=bool); hid[2] = True
    rec = bm.sweep_record(g.objs, g.centre, hid)
    assert (rec[2] == np.float32([0, 0, 0, 1e30])).all() and np.array_equal(np.delete(rec, 2, 0), np.delete(g.sweep, 2, 0))
    assert bm.sweep_cmax(g.objs, g.centre, hid) <= g.cmax


def test_pass_all_is_set_by_the_two_gates():
    """M on both sides of 1e14 and of 1e-12 (s6_big / s6_tiny, medge), a NaN origin, a NaN cmax: the flag and the words"""
    for name in ("s6_big", "s6_tiny"):
        cs, g = sc.case(name, "medge"), geo_of(name)
        ev = evaluate(cs, g)
        assert ev["s_all"].any() and (~ev["s_all"]).any(), name
        with np.errstate(all="ignore"):
            assert np.array_equal(ev["s_all"], ~(ev["M"] < 1e14) | ~(ev["M"] > 1e-12))
        assert (ev["words"][ev["s_all"]] == np.float32([0, 0, 0, 0, 0, 0, 0, 1e30])).all()
        assert ev["cand"][ev["s_all"]].all()                    # D = 0 * 0 + (1e30 - w) >= 0 for every record, the pads' w = 1e30 too
    cs, g = sc.case("s6", "inside", 6), geo_of("s6")
    o = cs["o"].copy(); o[::3, 1] = np.nan
    ev = evaluate(dict(cs, o=o), g)
    assert np.array_equal(ev["s_all"], np.isnan(o).any(axis=1)) and ev["cand"][ev["s_all"]].all()
    ev = evaluate(sc.case("nan200", "inside", 20), geo_of("nan200"))
    assert ev["s_all"].all() and ev["cand"][ev["sphere"]].all()


def test_shipped_margins_have_the_property():
    """no reported pair is lost on any family: every scene x regime (far26 and nowalk included: the sweep has no "no walk" form), the
    adversarial searches; the pad and hidden sentinels are no candidates for any ray that is not pass-all"""
    looked = reported = 0
    for name, regime, cs in cells():
        g = geo_of(name)
        ev = evaluate(cs, g)
        bad = lost(cs, ev)
        assert not bad.any(), (name, regime, int(bad.sum()), int(np.nonzero(bad)[0][0]))
        looked += int((ev["sphere"] | ev["tri"]).sum()); reported += int((cs["reported"] & (ev["sphere"] | ev["tri"])).sum())
        pad = np.tile(np.float32([0, 0, 0, 1e30]), (len(cs["o"]), 1))
        assert not (~np.signbit(bm.sweep_disc(pad, ev["words"])) & ev["sphere"] & ~ev["s_all"]).any(), (name, regime)
    assert looked > 60000 and reported > 30000, (looked, reported)


@pytest.mark.parametrize("margin", ("E", "A"))
def test_a_zero_allowance_loses_reported_pairs(margin):
    """E = 0 resp. A = 0, everything else as shipped: reported pairs are lost on the aimed families of EVERY scene that has such
    shapes (the pass-all scenes excepted: nan200 has no filter to weaken) -- the rays do see the allowance"""
    seen = {}
    for name, regime, cs in cells():
        if "adversarial" in regime:
            continue
        ev = evaluate(cs, geo_of(name), bm.WEAKENED[margin])
        kind = ev["sphere"] if margin == "E" else ev["tri"] & (geo_of(name).tri_rec[cs["target"], 6] < 1e29)
        if (kind & ~ev["pass_all"]).any():
            seen[name] = seen.get(name, 0) + int((lost(cs, ev) & kind).sum())
    print(margin, seen)
    assert seen and all(v > 0 for v in seen.values()), seen
    want = {"E": ("s5", "s6", "spheres200", "cloud", "dust", "mixed", "s4t4", "mixed3"), "A": ("tris300", "planes_mesh", "mixed", "s4t4", "mixed3")}[margin]
    assert set(want) <= set(seen), seen


def _refit_outward():
    """a cluster of twelve spheres around (100, 100, 100), every one moved to centre - 8 |c - centre|: outward 8 x from the kept centre,
    every coordinate still below the build's scale.  -> (base, indices, new)"""
    import rust_raytracing_amd as rtx
    rng = np.random.default_rng(31)
    base = bc._sphere_objs(rtx.OBJECT_DTYPE, 100.0 + rng.uniform(-1.0, 1.0, (12, 3)), rng.uniform(0.1, 0.3, 12))
    centre = bm.pack(base)["centre"]
    new = base.copy()
    new["geom"][:, :3] = centre - 8.0 * np.abs(base["geom"][:, :3] - centre)
    assert np.abs(new["geom"][:, :3]).max() + 0.3 < np.abs(base["geom"][:, :3]).max()
    return base, np.arange(12, dtype=np.uint64), new


def _deform_outward():
    """s4t4's four triangles scaled 8 x about the origin (n . v0 keeps its sign, so class and free axis are kept:
    bounds_model.deform asserts it); the centre the records are relative to is the pack's"""
    base = sc.scenes()["s4t4"]
    idx = np.nonzero(base["kind"] == 2)[0]
    new = base[idx].copy()
    new["geom"][:, :9] = 8.0 * new["geom"][:, :9]
    return base, idx.astype(np.uint64), new


def _updated_case(label, now, regime="inside"):
    rays = bc.aimed(label, now, regime, None)
    t, rep, _ = bc.text_distances(now, rays["o"], rays["d"], rays["target"])
    return {"o": rays["o"], "d": rays["d"], "target": rays["target"], "t": t, "reported": rep}


def mutation_counts():
    """{mutation: reported pairs lost} on the aimed families"""
    out = {k: 0 for k in CAUGHT + NOT_CAUGHT}
    for name, regime, cs in cells():
        if "adversarial" in regime or name == "nan200":
            continue
        for mut in ("w from the f32 centre", "p2 without the factor 2", "pair swapped"):
            ev = evaluate(cs, geo_of(name), mutation=mut)
            out[mut] += int((lost(cs, ev) & ev["sphere"]).sum())
    base, idx, new = _refit_outward()
    pk = bm.refit(base, idx, new)
    assert pk["cmax"] > 7.0 * bm.pack(base)["cmax"]
    for regime in ("inside", "centre"):
        cs = _updated_case("refit outward", pk["objs"], regime) if regime == "inside" else sc.centre_tangents("refit outward", pk["objs"], pk["centre"])
        fresh = Geo(pk["objs"], pk["centre"], pk["cmax"], 0.0, pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
        assert not lost(cs, evaluate(cs, fresh)).any()
        stale = Geo(pk["objs"], pk["centre"], bm.pack(base)["cmax"], 0.0, pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
        out["stale cmax"] += int(lost(cs, evaluate(cs, stale)).sum())
    base, idx, new = _deform_outward()
    pk = bm.deform(base, idx, new)
    assert pk["tri_extent"] > 5.0 * bm.pack(base)["tri_extent"]
    for regime in ("inside", "edge"):
        cs = _updated_case("deform outward", pk["objs"], regime)
        fresh = Geo(pk["objs"], pk["centre"], pk["cmax"], pk["tri_extent"], pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
        assert not lost(cs, evaluate(cs, fresh)).any()
        stale = Geo(pk["objs"], pk["centre"], pk["cmax"], bm.pack(base)["tri_extent"], pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
        out["stale tri_extent"] += int((lost(cs, evaluate(cs, stale))).sum())
    return out


def test_model_mutations():
    """Each mutation of the model by name: w formed from the f32-rounded centre, p2 without its factor 2, the two records of a pair
    swapped, a cmax left stale by a refit that moves spheres outward 8 x, a tri_extent left stale by a deform that scales the
    triangles 8 x.  CAUGHT ones lose reported pairs (the stale cmax only on the tangents from the centre, where |p| adds nothing to
    M).  NOT_CAUGHT ones lose none on any ray of the generator -- findings about the allowances, not failures:
      w from the f32 centre -- moves w by about 2u |c - centre|^2 <= 2uM^2, and E = 64uM^2 has 56uM^2 to spare over the 7.5uM^2 the
          worst ray of the search needs (profiles/sweep_filter_margin_use.txt);
      stale tri_extent -- S = tri_extent + |p|_1 + 1 shrinks by 5 x at most while the worst reported pair needs 0.04 of A."""
    got = mutation_counts()
    print(got)
    for k in CAUGHT:
        assert got[k] > 0, (k, got)
    for k in NOT_CAUGHT:
        assert got[k] == 0, (k, got)


# ---- margin use: measured, not fixed in advance ---------------------------------------------------------------------------------------------
def margin_use(cs, g, exact_top=8):
    """-> (e_need, e_err, a_share, n_s, n_t) of one cell:
    e_need  the largest -D_f32(E = 0) / (u M^2) over the REPORTED sphere pairs: the allowance a reported pair needs (E ships 64)
    e_err   the largest (D_exact - D_f32(E = 0)) / (u M^2) over the reported pairs, D_exact the discriminant of the f64 inputs in
            exact rational arithmetic (fractions.Fraction) for the exact_top pairs the f64 ruler ranks worst
    a_share the largest share of A = 64uS a reported triangle pair needs: max(-sx, -sy) computed with A = 0, over A"""
    e0 = evaluate(cs, g, bm.WEAKENED["E"])
    a0 = evaluate(cs, g, bm.WEAKENED["A"])
    ship = evaluate(cs, g)
    rep = cs["reported"]
    s = rep & e0["sphere"] & ~e0["pass_all"]
    e_need = e_err = a_share = float("nan")
    with np.errstate(all="ignore"):
        uM2 = U * e0["M"] * e0["M"]
        if s.any():
            need = -e0["D"].astype(np.float64) / uM2
            e_need = float(need[s].max())
            ruler = (sc.disc_f64(g.objs, cs["target"], cs["o"], cs["d"]) - e0["D"].astype(np.float64)) / uM2
            top = np.nonzero(s)[0][np.argsort(-ruler[s])[:exact_top]]
            geom = np.asarray(g.objs["geom"], dtype=np.float64)
            e_err = max((sc.exact_disc(geom[cs["target"][i], :3], geom[cs["target"][i], 3], cs["o"][i], cs["d"][i]) - float(e0["D"][i])) / uM2[i] for i in top)
        t = rep & a0["tri"] & ~a0["pass_all"] & (g.tri_rec[cs["target"], 6] < 1e29)
        if t.any():
            share = np.maximum(-a0["sx"].astype(np.float64), -a0["sy"].astype(np.float64)) / ship["A"].astype(np.float64)
            a_share = float(share[t].max())
    return e_need, e_err, a_share, int(s.sum()), int((rep & a0["tri"]).sum())


def margin_table():
    rows = []
    for name, regime, cs in cells():
        if name == "nan200":
            continue
        rows.append((name, regime) + margin_use(cs, geo_of(name)))
    return rows


def test_margin_use_is_within_the_allowances():
    """the figures of profiles/sweep_filter_margin_use.txt on the adversarial cells (the aimed cells are in the file): no reported
    pair needs the whole allowance -- which is the property once more, read as a share; the figures themselves are printed"""
    for name, regime, cs in cells():
        if "adversarial" not in regime:
            continue
        e_need, e_err, a_share, n_s, n_t = margin_use(cs, geo_of(name))
        print("%-12s %-22s E needed %8.3f uM^2  error %8.3f uM^2  share of A %7.4f  (%d / %d reported)" % (name, regime, e_need, e_err, a_share, n_s, n_t))
        assert not e_need >= 64.0 and not a_share >= 1.0, (name, regime, e_need, a_share)


def test_product_library_has_no_sweep_filter_hook(rtx):
    lib = rtx.load_library()
    assert lib.rtx_lab_build() == 0
    assert lib.rtx_debug_sweep_filter(None, None, None, 0, None, None) == rtx.abi.RTX_ERR_UNSUPPORTED


# ---- the gpu part ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _OPEN:
        h.close()
    del _OPEN[:]
    _handle.cache_clear()


@functools.lru_cache(maxsize=None)
def _handle(name):
    import rust_raytracing_amd as rtx
    _OPEN.append(hip_scene(rtx, sc.scenes()[name], rays_per_pixel=1).upload(0, lab=True))
    return _OPEN[-1]


def _f32(words):
    return np.ascontiguousarray(words).view(np.float32)


def check_device(hnd, cs, g, what, hidden_objects=()):
    """one hook launch on a case: the scene constants, the property, the flags, and every word against the model bit for bit"""
    out, info = hnd.debug_sweep_filter(cs["o"], cs["d"], cs["target"])
    assert np.array_equal(info[:3], g.centre) and (info[3] == g.cmax or (np.isnan(info[3]) and np.isnan(g.cmax))), (what, info[:5])
    assert info[4] == g.tri_extent and info[5] == (g.kind == 0).sum() and info[7] == 8 and info[8] == 24, (what, info[:9])
    ev = evaluate(cs, g)
    flags = out[:, 0]
    is_tri, has, p_all, cand = (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0
    assert has[ev["sphere"] | ev["tri"]].all() and np.array_equal(is_tri[has], (g.kind[cs["target"]] == 2)[has]), what
    bad = cs["reported"] & has & ~p_all & ~cand
    assert not bad.any(), (what, "reported pairs lost on the device", int(bad.sum()), int(np.nonzero(bad)[0][0]))
    m = ev["sphere"] | ev["tri"]
    assert np.array_equal(p_all[m], ev["pass_all"][m]), what
    assert np.array_equal(cand[m], ev["cand"][m]), what
    assert np.array_equal(out[m, 1:9], ev["words"][m].view(np.uint32)), (what, "FilterParams / TriFilterParams")
    assert np.array_equal(out[m, 9:17], ev["rec"][m].view(np.uint32)), (what, "the resident records")
    s, t = ev["sphere"], ev["tri"]
    fin = s & ~np.isnan(ev["D"])
    assert np.array_equal(out[fin, 17], ev["D"][fin].view(np.uint32)) and np.array_equal(out[fin, 18], ev["D"][fin].view(np.uint32)), (what, "D")
    assert np.array_equal(out[s, 19], g.local[cs["target"]][s].astype(np.uint32)), what
    sg = ev["sx"].view(np.uint32) | ev["sy"].view(np.uint32)
    tf = t & ~np.isnan(ev["sx"]) & ~np.isnan(ev["sy"])
    assert np.array_equal(out[tf, 17], sg[tf]), (what, "tri_filter_sign")
    for j in hidden_objects:
        sel = (cs["target"] == j) & ~p_all
        assert not cand[sel].any(), (what, "a hidden record is a candidate", j)
    return out


def _gpu_case(name, regime):
    cs = sc.case(name, regime)
    return cs if len(cs["t"]) <= 20000 else sc.case(name, regime, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime", CELLS)
def test_the_filters_hold_on_the_device(gpu, name, regime):
    """rtx_debug_sweep_filter on one scene x regime: the property on the device, every word the model's (module docstring)"""
    cs = _gpu_case(name, regime)
    assert len(cs["t"]) <= 20000
    if regime == "nowalk":
        cs = dict(cs, o=cs["o"].copy())
        cs["o"][::7, 0] = np.nan                               # NaN origins: pass-all
    check_device(_handle(name), cs, geo_of(name), (name, regime))


@pytest.mark.gpu
@pytest.mark.parametrize("name,what", [(n, w) for n in sc.SPHERE_SCENES for w in ("spheres", "centre")] + [(n, "triangles") for n in sc.TRI_SCENES])
def test_the_filters_hold_on_the_adversarial_rays(gpu, name, what):
    """the kept rays of the model's searches and the tangents from the centre, on the device"""
    cs = sc.centre_case(name) if what == "centre" else sc.adversarial_case(name, what)
    check_device(_handle(name), cs, geo_of(name), (name, "adversarial", what))


@pytest.mark.gpu
def test_the_resident_records_are_the_models(gpu):
    """every record of s5 (its last pair: a sphere and a sentinel), s1030 (the chunk's ragged tail) and mixed3 / tris300 through the
    hook, one pair per object: sweep_record's and pack()'s bits"""
    for name in ("s5", "s1030", "mixed3", "tris300", "s4t4"):
        g = geo_of(name)
        tg = np.nonzero((g.kind == 0) | ((g.kind == 2) & g.has_tri_rec))[0]
        o = np.tile(g.centre + np.array([0.3, -0.2, 0.1]), (len(tg), 1))
        cs = {"o": o, "d": np.tile(np.array([0.0, 0.6, 0.8]), (len(tg), 1)), "target": tg, "reported": np.zeros(len(tg), dtype=bool)}
        check_device(_handle(name), cs, g, (name, "records"))
    cnt, info = _handle("s5").debug_sweep_filter(g.centre[None, :] + 1e3, np.array([[1.0, 0.0, 0.0]]))
    assert cnt.shape == (1, 4)


@pytest.mark.gpu
def test_the_filters_hold_after_a_refit_a_deform_and_a_hide(gpu):
    """one update_cases pair (s65 / grow: cmax grows), one mesh_update_cases pair (t40 / grow: tri_extent grows), one
    visibility_cases scene (s65: a third of the spheres hidden, then shown): the resident records and constants are the refit / deform
    model's, the property holds on rays aimed at the updated scene, and a hidden sphere is never a candidate"""
    import mesh_update_cases as mc
    import update_cases as uc
    base = uc.scene("s65")
    idx, new, how = uc.update(base, "grow")
    pk = bm.refit(base, idx, new)
    hnd = hip_scene(gpu, base, rays_per_pixel=1).upload(0, lab=True)
    assert hnd.update_objects(idx, new) == how == "refit"
    g = Geo(pk["objs"], pk["centre"], pk["cmax"], pk["tri_extent"], pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
    assert g.cmax > bm.pack(base)["cmax"]
    check_device(hnd, _updated_case("s65/grow", pk["objs"]), g, "s65 / grow")
    # hide a third, then show them again
    sph = np.nonzero(g.kind == 0)[0]
    hide = sph[::3]
    hnd.hide(hide)
    hidden = np.zeros(len(g.kind), dtype=bool); hidden[hide] = True
    gh = Geo(pk["objs"], pk["centre"], bm.sweep_cmax(pk["objs"], pk["centre"], hidden), pk["tri_extent"],
             bm.sweep_record(pk["objs"], pk["centre"], hidden), pk["rec"][:, :8], pk["free"] >= 0, hidden)
    cs = _updated_case("s65/grow", pk["objs"])
    rep = cs["reported"] & ~hidden[cs["target"]]           # (a pair's distance is the pair's alone: the text of the others stands)
    check_device(hnd, dict(cs, reported=rep), gh, "s65 / grow / hide", hidden_objects=hide[:8])
    hnd.show(hide)
    check_device(hnd, cs, g, "s65 / grow / hide / show")
    hnd.close()
    base = mc.cached_scene("t40")
    idx, new, how, mode = mc.update(base, "grow", name="t40")
    pk = bm.deform(base, idx, new)
    hnd = hip_scene(gpu, base, rays_per_pixel=1).upload(0, lab=True)
    assert hnd.update_objects(idx, new, mode=mode) == how
    g = Geo(pk["objs"], pk["centre"], pk["cmax"], pk["tri_extent"], pk["sweep"], pk["rec"][:, :8], pk["free"] >= 0)
    assert g.tri_extent > bm.pack(base)["tri_extent"]
    check_device(hnd, _updated_case("t40/grow", pk["objs"]), g, "t40 / grow")
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("s1030", "mixed3", "s5"))
def test_the_hooks_counts_are_the_launchs(gpu, name):
    """Ties the hook to the launch: a 32 x 32 frame, 1 spp, default bounces, RTX_KERNEL_MIXED.  Every segment of rtx_debug_paths'
    transcripts goes through the hook's counts mode; RtxStats.exact_tests of the frame equals, to the unit, the sum over the segments
    of the candidates (n_spheres + n_tris where they exceed Q + kOverflowQ) plus n_planes per segment.  A wrong chunk tail, pair
    index or pad shows here."""
    import torch
    objs = sc.scenes()[name].copy()
    objs["emission_color"][::3] = 1.0
    g = geo_of(name)
    cam = (tuple(g.centre + np.array([-2.5 * max(g.cmax, 1.0), 0.3, 0.2])), (1.0, 0.0, 0.0), 0.9)
    w = h = 32
    lab = hip_scene(gpu, objs, cam, rays_per_pixel=1).upload(0, lab=True)
    segs = []
    for row in range(h):
        steps, counts = lab.debug_paths(w, h, row, 64)
        assert counts.max() <= 64
        for x in range(w):
            segs.append(steps[x, 0, :counts[x, 0]])
    segs = np.concatenate(segs)
    cnt, info = lab.debug_sweep_filter(segs["position"], segs["direction"])
    lab.close()
    assert not (cnt[:, 2] != 0).any(), "a pass-all ray"
    n_s, n_t, n_p = int((g.kind == 0).sum()), int((g.kind == 2).sum()), int((g.kind == 1).sum())
    cap = int(info[7] + info[8])
    per = cnt[:, 0].astype(np.int64) + cnt[:, 1]
    want = int(np.where(per > cap, n_s + n_t, per).sum()) + n_p * len(segs)
    hnd = hip_scene(gpu, objs, cam, kernel=gpu.RTX_KERNEL_MIXED, rays_per_pixel=1).upload(0)
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    hnd.close()
    assert st.segments == len(segs), (st.segments, len(segs))
    assert (per > 0).mean() > 0.05, "the frame does not see the scene"
    assert st.exact_tests == want, (name, st.exact_tests, want)


LIMB_SCENES = ("s4t4", "nan200", "s5", "mixed3")
SWEEPS_ON_AUTO = ("s4t4", "nan200")                            # no tree / more than 64 shapes outside it: AUTO is the sweep


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIMB_SCENES)
def test_limb_frames_equal_the_exhaustive_kernel(gpu, name):
    """The real kernel on frames whose pixels straddle a silhouette (sweep_cases.limb_cameras: 32 x 32, 1 spp, no lens jitter,
    neighbouring rays one f32 ulp of the scene's scale apart at the tangent point, every object its own dyadic emission):
    RTX_KERNEL_MIXED_VERIFY, RTX_KERNEL_MIXED and AUTO equal RTX_KERNEL_EXACT bit for bit, segment counts included, with
    filter_mismatches == 0, for max_bounces 0 and the default.  The builder's claim is asserted on the exhaustive frame: at least 10 %
    of the pixels show the target and at least 10 % do not.  On s4t4 and nan200 AUTO must have taken the sweep."""
    import torch
    objs = sc.limb_objects(name)
    cams = sc.limb_cameras(name)
    assert len(cams) >= 4 * min(6, int(((objs["kind"] == 0) | (objs["kind"] == 2)).sum()) - 1), len(cams)
    n = sc.LIMB_SIZE
    kernels = (gpu.RTX_KERNEL_EXACT, gpu.RTX_KERNEL_MIXED_VERIFY, gpu.RTX_KERNEL_MIXED, gpu.RTX_KERNEL_AUTO)
    cfg = lambda k, b: gpu.Config(rays_per_pixel=1, max_bounces=b, focal_offset=0.0, non_focal_offset=0.0, kernel=k)
    hnd = gpu.Scene.from_packed(cfg(kernels[0], 0), gpu.Camera(*cams[0][:3]), objs).upload(0)
    buf = torch.zeros((n, n, 3), dtype=torch.float64, device="cuda:0")
    try:
        for pos, d, fov, target, regime in cams:
            hnd.set_camera(gpu.Camera(pos, d, fov))
            for bounces in (0, gpu.Config().max_bounces):
                got = {}
                for k in kernels:
                    hnd.set_config(cfg(k, bounces))
                    buf.zero_()
                    st = hnd.render_rows(n, n, 0, 1, n, buf.data_ptr())
                    got[k] = (buf.cpu().numpy().copy(), st.segments, st.filter_mismatches, st.kernel)
                want = got[gpu.RTX_KERNEL_EXACT]
                shows = (want[0][:, :, 0] == sc.limb_emission(target)).mean()
                assert 0.1 <= shows <= 0.9, (name, target, regime, shows)
                for k in kernels[1:]:
                    assert np.array_equal(got[k][0], want[0]), (name, target, regime, bounces, k, int((got[k][0] != want[0]).any(axis=2).sum()))
                    assert got[k][1] == want[1] and got[k][2] == 0, (name, target, regime, bounces, k, got[k][1:3], want[1])
                if name in SWEEPS_ON_AUTO:
                    assert got[gpu.RTX_KERNEL_AUTO][3] == gpu.RTX_KERNEL_MIXED, (name, got[gpu.RTX_KERNEL_AUTO][3])
    finally:
        hnd.close()


if __name__ == "__main__":                                      # the print-out kept as profiles/sweep_filter_margin_use.txt
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("# the sweep's f32 filters: margin use per cell (tests/test_sweep_filters.py margin_table; the model, CPU only)")
    print("# E needed: the largest -D_f32(E = 0) / (u M^2) over the reported sphere pairs (E ships 64 u M^2)")
    print("# error:    the largest (D exact - D_f32(E = 0)) / (u M^2) over them, D exact in rational arithmetic on the f64 inputs")
    print("# share A:  the largest share of A = 64 u S a reported triangle pair needs;  nan: the cell has no such pair")
    for row in margin_table():
        print("%-12s %-22s E needed %8.3f  error %8.3f  share A %8.4f   reported: %5d spheres %5d triangles" % row)
    print("# mutations, reported pairs lost:", mutation_counts())
