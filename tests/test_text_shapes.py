"""tests/text_shapes.py -- the reference's intersection arithmetic, closest_object, shading and avg, restated once over a number type --
checked on the CPU, three ways:

  1. its f64 evaluation equals the oracle BIT FOR BIT (distance, winner, hit point, normal; NaN equals NaN) on the fuzz and on every
     crafted family of tests/shape_families.py: the oracle is pinned against a second, independent reading of the text;
  2. the reading MEANS what it should: on inputs built from known answers (a point chosen on the shape, a ray aimed at it, unit
     direction) the point the text reports lies on the sphere / in the plane, is the NEAR intersection, is reported from the right
     side only, and lies inside or outside the triangle as barycentric coordinates from cross-product areas at 400 bits say.  No bound
     is chosen: the same routine evaluated in 53-bit interval arithmetic (outward rounding) encloses the real value and any
     round-to-nearest f64 evaluation; the f64 and the 400-bit results must lie inside it and each residual is compared with the
     width of its enclosure.  A ray whose enclosure straddles one of the text's comparisons is left out, at most 5 % of a family;
  3. the averaging set of tests/closed_form.py catches the usual wrong implementations.

The text's quirks have no geometric meaning -- phantom hits behind the ray (triangle.rs:118), the un-normalised direction in the hit
point (triangle.rs:122, scene.rs:234), the cull by direction (triangle.rs:115) -- so (2) keeps away from them (facing triangles, the
plane in front, unit directions): the text alone pins them, through the bit-for-bit comparisons of (1) and of
tests/test_shapes_from_text.py.  mpmath must be importable: a failed import fails these tests, it does not skip them."""
import math
from fractions import Fraction

import numpy as np

import closed_form as cf
import shape_families as sf
import text_shapes as ts
from helpers import check_equal, oracle_render, same

MAX_LEFT_OUT = 0.05


# ---- 1. the f64 reading equals the oracle -------------------------------------------------------------------------------------------------
def _oracle_answers(oracle, objs, origins, dirs):
    """closest_object of the oracle, scene.rs:234's hit point (plain f64 products and sums) and the oracle's normal_at there"""
    import ctypes as C
    L = oracle.lib()
    L.rtxo_object_normal_at.restype = oracle.Vec3
    L.rtxo_object_normal_at.argtypes = [C.c_void_p, oracle.Vec3]
    objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
    sc = oracle.make_scene(objs, ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0))
    n = len(origins)
    dist, obj = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    pos, nrm = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    with np.errstate(all="ignore"):
        for k in range(n):
            i, d = oracle.closest_object(sc, origins[k], dirs[k])
            if i < 0:
                continue
            dist[k], obj[k] = d, i
            pos[k] = origins[k] + dirs[k] * d
            nrm[k] = L.rtxo_object_normal_at(objs.ctypes.data + i * objs.itemsize, oracle.vec(pos[k])).tuple()
    return dist, obj, pos, nrm


def test_f64_reading_equals_the_oracle_bit_for_bit(oracle):
    """the fuzz scenes of the query test (all 150, 200 rays of each: its own first 160 -- zero and NaN directions among them -- and 40
    aimed at the shapes), every crafted family, every tie scene"""
    n_rays = n_odd = 0
    for s, objs, cam, o, d in sf.fuzz_cases(oracle.OBJECT_DTYPE):
        o, d = o[:sf.FUZZ_RAYS + 40], d[:sf.FUZZ_RAYS + 40]
        check_equal(ts.answers(objs, o, d), _oracle_answers(oracle, objs, o, d), "fuzz scene %d" % s)
        n_rays += len(o)
        n_odd += int((~np.isfinite(d).all(axis=1) | ~d.any(axis=1)).sum())
    assert n_rays >= 20000 and n_odd >= 20, (n_rays, n_odd)
    for name, objs, o, d in sf.families(oracle.OBJECT_DTYPE):
        check_equal(ts.answers(objs, o, d), _oracle_answers(oracle, objs, o, d), name)
    n = 0
    for name, objs, o, d, first in sf.tie_scenes(oracle.OBJECT_DTYPE):
        want = _oracle_answers(oracle, objs, o, d)
        check_equal(ts.answers(objs, o, d), want, name)
        assert want[1][0] == first, name
        n += 1
    assert n == 30


# ---- 2. the reading means what it should ----------------------------------------------------------------------------------------------------
_NS = []


def _namespaces():
    if not _NS:
        _NS.extend((ts.F64, ts.MPF(400), ts.IV(53)))
    return tuple(_NS)


def _bounds(mp, x):
    """the end points of a 53-bit interval as numbers of the 400-bit context (exact)"""
    return mp.ctx.make_mpf(x._mpi_[0]), mp.ctx.make_mpf(x._mpi_[1])


def _inside(mp, x, enclosure):
    lo, hi = _bounds(mp, enclosure)
    return lo <= mp.ctx.mpf(float(x)) <= hi if isinstance(x, (float, np.floating)) else lo <= x <= hi


def _width(mp, enclosure):
    lo, hi = _bounds(mp, enclosure)
    return hi - lo


def _three(fn, *args):
    """fn(ns, *args converted) on f64, 400 bits and intervals -> (f, m, i); i is the string "undecided" where an interval straddles
    a comparison of the text"""
    out = []
    for ns in _namespaces():
        conv = [tuple(ns.num(x) for x in a) if isinstance(a, (tuple, list, np.ndarray)) else a for a in args]
        try:
            with np.errstate(all="ignore"):
                out.append(fn(ns, *conv))
        except ts.Undecided:
            out.append("undecided")
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


def _perp(rng, n):
    """a unit vector perpendicular to the unit vector n"""
    t = np.cross(n, rng.normal(size=3))
    return _unit(t)


def _check_value(mp, f, m, i, what):
    assert _inside(mp, f, i), (what, "the f64 value is outside its enclosure", f, i)
    assert _inside(mp, m, i), (what, "the 400-bit value is outside the enclosure", m, i)


def _check_residual(mp, residual, args, t, what):
    """residual(ns, *args, t) at the three evaluations: the f64 one inside the enclosure, the 400-bit one no larger than its width"""
    f64, mpf, iv = _namespaces()
    conv = lambda ns: [tuple(ns.num(x) for x in a) for a in args]
    with np.errstate(all="ignore"):
        rf = residual(f64, *conv(f64), t[0])
    rm = residual(mpf, *conv(mpf), t[1])
    ri = residual(iv, *conv(iv), t[2])
    assert _inside(mp, rf, ri), (what, "the f64 residual is outside its enclosure", rf, ri)
    assert abs(rm) <= _width(mp, ri), (what, "the point is off the surface by more than the enclosure is wide", rm, ri)


def _on_sphere(ns, g, o, d, t):
    p = ts.sub(ts.hit_point(o, d, t), g[:3])
    return ts.dot(p, p) - g[3] * g[3]


def _on_plane(ns, p0, normal, o, d, t):
    return ts.dot(ts.sub(ts.hit_point(o, d, t), p0), normal)


def test_sphere_reading_reports_the_near_point_on_the_sphere():
    """400 rays aimed at a point chosen on a sphere from outside, at least 0.1 rad inside the tangent cone.  Left out: 0 %."""
    mp = _namespaces()[1]
    rng = np.random.default_rng(101)
    n = left_out = 0
    while n < 400:
        c, r = rng.uniform(-5.0, 5.0, 3), float(rng.uniform(0.2, 3.0))
        nrm = _unit(rng.normal(size=3))
        p = c + r * nrm
        phi = float(rng.uniform(0.0, math.pi / 2 - 0.15))
        o = p + float(rng.uniform(0.5, 20.0)) * (math.cos(phi) * nrm + math.sin(phi) * _perp(rng, nrm))
        d = _unit(p - o)
        axis = c - o
        beta = math.atan2(float(np.linalg.norm(np.cross(d, axis))), float(d @ axis))
        if math.asin(r / float(np.linalg.norm(axis))) - beta < 0.1:
            continue
        n += 1
        g = tuple(c) + (r,)
        tf, tm, ti = _three(ts.sphere_distance, g, o, d)
        if isinstance(ti, str):
            left_out += 1
            continue
        assert tf is not None and tm is not None and ti is not None and tm > 0
        _check_value(mp, tf, tm, ti, ("sphere", n))
        # the NEAR intersection, from the known answer and from a formula that is not the text's quadratic: with u the unit
        # direction and m = (c - o) . u the closest approach, the two intersections are m -+ sqrt(r^2 - (|c - o|^2 - m^2)).  The
        # enclosure of the text's distance holds the nearer and not the farther, and the chosen point P (the near one by
        # construction: O lies on its outward side) is closer to the reported distance than to the far intersection.
        gm, om, um = tuple(mp.num(x) for x in g), ts.vec(mp, o), ts.norm(mp, ts.vec(mp, d))
        to_c = ts.sub(gm[:3], om)
        m = ts.dot(to_c, um)
        half = mp.sqrt(gm[3] * gm[3] - (ts.dot(to_c, to_c) - m * m))
        near, far = m - half, m + half
        assert _inside(mp, near, ti) and not _inside(mp, far, ti), (n, near, far, ti)
        to_p = ts.length(mp, ts.sub(ts.vec(mp, p), om))
        assert abs(to_p - tm) < abs(to_p - far) and abs(to_p - tf) < abs(to_p - far), (n, to_p, tm, far)
        _check_residual(mp, _on_sphere, (g, o, d), (tf, tm, ti), ("sphere", n))
    print("sphere family: %d rays, %d left out" % (n, left_out))
    assert left_out <= MAX_LEFT_OUT * n


def test_plane_reading_reports_a_point_of_the_plane_from_the_normal_side_only():
    """400 rays at a point chosen on a plane whose normal has length 1e-3 ... 1e3: from the side the normal points to (a hit, and the
    point lies on the plane), the same ray reversed, and both again from behind (plane.rs:25: none of the three).  At least 0.1 rad
    off the plane.  Left out: 0 %."""
    mp = _namespaces()[1]
    rng = np.random.default_rng(103)
    n = left_out = hits = 0
    for _ in range(100):
        p0 = rng.uniform(-5.0, 5.0, 3)
        nhat = _unit(rng.normal(size=3))
        normal = nhat * 10.0 ** float(rng.uniform(-3.0, 3.0))
        p = p0 + float(rng.uniform(-4.0, 4.0)) * _perp(rng, nhat) + float(rng.uniform(-4.0, 4.0)) * _perp(rng, nhat)
        phi = float(rng.uniform(0.0, math.pi / 2 - 0.15))
        away = math.cos(phi) * nhat + math.sin(phi) * _perp(rng, nhat)
        length = float(rng.uniform(0.5, 20.0))
        for side in (1.0, -1.0):
            o = p + side * length * away
            for towards in (1.0, -1.0):
                d = _unit(p - o) * towards
                n += 1
                tf, tm, ti = _three(ts.plane_distance, tuple(p0) + tuple(normal), o, d)
                if isinstance(ti, str):
                    left_out += 1
                    continue
                # the side, at 400 bits, by the plain geometric statement: in front of the plane and heading towards it
                front = ts.dot(ts.sub(ts.vec(mp, o), ts.vec(mp, p0)), ts.vec(mp, normal)) > 0
                heading = ts.dot(ts.vec(mp, d), ts.vec(mp, normal)) < 0
                assert front == (side > 0) and heading == (side * towards > 0)
                want_hit = front and heading
                assert (tf is not None) == (tm is not None) == (ti is not None) == want_hit, (n, tf, tm, ti, want_hit)
                if want_hit:
                    hits += 1
                    _check_value(mp, tf, tm, ti, ("plane", n))
                    _check_residual(mp, _on_plane, (p0, normal, o, d), (tf, tm, ti), ("plane", n))
    print("plane family: %d rays, %d hits, %d left out" % (n, hits, left_out))
    assert left_out <= MAX_LEFT_OUT * n and hits >= 90


def _plane_distance_of_triangle(ns, g, o, d):
    return ns.abs(ts._triangle_plane_distance(ns, g, o, d))


def _in_triangle_plane(ns, g, o, d, t):
    _, r, s = ts._plane_vectors(g)
    return ts.dot(ts.sub(ts.hit_point(o, d, t), g[:3]), ts.cross(r, s))


def test_triangle_reading_agrees_with_cross_product_barycentrics():
    """600 rays at a point a r + b s chosen inside or outside a triangle -- at least 0.05 from every edge in (a, b), the triangle
    facing (n . v0 > 1.1: triangle.rs:115 never culls a unit direction), the plane in front, the (x, y) rows the text solves well
    conditioned (|n.z| >= 0.2, |r.x| >= 0.2 |r|) -- from either side, at least 0.15 rad off the plane.  The point the text's plane
    distance gives lies in the plane, and the text says inside exactly when the barycentric coordinates from cross-product areas at
    400 bits -- NOT the two-row elimination -- do.  Left out: 0 %."""
    mp = _namespaces()[1]
    rng = np.random.default_rng(107)
    n = left_out = inside_n = 0
    while n < 600:
        v0 = rng.uniform(-4.0, 4.0, 3)
        r, s = rng.normal(size=3) * rng.uniform(0.5, 2.0), rng.normal(size=3) * rng.uniform(0.5, 2.0)
        nrm = np.cross(r, s)
        if float(np.linalg.norm(nrm)) < 0.3 * float(np.linalg.norm(r)) * float(np.linalg.norm(s)):
            continue
        nhat = _unit(nrm)
        if float(nhat @ v0) < 0.0:
            r, s, nhat = s, r, -nhat
        if float(nhat @ v0) <= 1.1 or abs(nhat[2]) < 0.2 or abs(r[0]) < 0.2 * float(np.linalg.norm(r)):
            continue
        a, b = rng.uniform(-0.6, 1.6, 2)
        if min(abs(a), abs(b), abs(1.0 - a - b)) < 0.05:
            continue
        want_inside = bool(a > 0 and b > 0 and a + b < 1)
        if want_inside != (n % 2 == 0):                            # half of each
            continue
        g = tuple(v0) + tuple(v0 + r) + tuple(v0 + s)
        p = v0 + a * r + b * s
        phi = float(rng.uniform(0.0, math.pi / 2 - 0.2))
        side = 1.0 if rng.random() < 0.5 else -1.0
        o = p + side * float(rng.uniform(0.5, 20.0)) * (math.cos(phi) * nhat + math.sin(phi) * _perp(rng, nhat))
        d = _unit(p - o)
        n += 1
        tf, tm, ti = _three(ts.triangle_distance, g, o, d)
        qf, qm, qi = _three(_plane_distance_of_triangle, g, o, d)
        if isinstance(ti, str) or isinstance(qi, str):
            left_out += 1
            continue
        _check_value(mp, qf, qm, qi, ("triangle plane distance", n))
        _check_residual(mp, _in_triangle_plane, (g, o, d), (qf, qm, qi), ("triangle", n))
        # barycentric coordinates of the point the text tests, from cross-product areas at 400 bits
        gm = tuple(mp.num(x) for x in g)
        _, rm, sm = ts._plane_vectors(gm)
        pm = ts.sub(ts.hit_point(ts.vec(mp, o), ts.vec(mp, d), qm), gm[:3])
        big = ts.cross(rm, sm)
        am = ts.dot(ts.cross(pm, sm), big) / ts.dot(big, big)
        bm = ts.dot(ts.cross(rm, pm), big) / ts.dot(big, big)
        inside = bool(am >= 0 and bm >= 0 and am + bm <= 1)
        assert inside == want_inside, (n, a, b, am, bm)                                 # (the construction)
        assert (tf is not None) == (tm is not None) == (ti is not None) == inside, (n, a, b, tf, tm, ti)
        if inside:
            inside_n += 1
            _check_value(mp, tf, tm, ti, ("triangle", n))
            assert tf == qf
    print("triangle family: %d rays, %d inside, %d left out" % (n, inside_n, left_out))
    assert left_out <= MAX_LEFT_OUT * n and inside_n >= 250


# ---- 3. shading and averaging ----------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c with ONE rounding (math.fma where the Python has it)"""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _pairwise(xs):
    if len(xs) <= 2:
        return sum(xs, 0.0)
    h = len(xs) // 2
    return _pairwise(xs[:h]) + _pairwise(xs[h:])


def _kahan(xs):
    total = comp = 0.0
    for x in xs:
        y = x - comp
        t = total + y
        comp = (t - total) - y
        total = t
    return total


def test_averaging_set_catches_the_usual_wrong_implementations():
    """For the (k, n) of the lens cases and the n of the closed box: pairwise summation, Kahan summation and `sum * (1.0 / n)` each
    produce at least one value outside the allowed set {fold(E, j) / n}; a fused `res = fma(light, e, res)` produces a closed-box
    sample that is not the text's."""
    caught = {"pairwise": 0, "kahan": 0, "reciprocal": 0}
    for n in cf.LENS_COLOUR_SPP + cf.COLOUR_SPP:
        allowed = cf.lens_allowed(n)
        for c, e in enumerate(cf.COLOUR_EMIT):
            ok = set(allowed[:, c].tolist())
            for k in range(n + 1):
                xs = [e] * k + [0.0] * (n - k)
                caught["pairwise"] += _pairwise(xs) / float(n) not in ok
                caught["kahan"] += _kahan(xs) / float(n) not in ok
                caught["reciprocal"] += cf.fold(e, k) * (1.0 / n) not in ok
    assert all(v > 0 for v in caught.values()), caught
    for mb in cf.COLOUR_BOUNCES:
        fused = 0
        want = cf.coloured_sample(mb)
        for c, (e, b) in enumerate(zip(cf.COLOUR_EMIT, cf.COLOUR_BASE)):
            res, light = 0.0, 1.0
            for _ in range(mb + 1):
                res = _fma(light, e, res)
                light = light * b
            fused += res != want[c]
        assert fused > 0 or mb == 0, mb                               # (one hit: 0 + 1 * e, nothing to fuse)
    # ... and text_shapes' own two routines are the plain ones
    with np.errstate(all="ignore"):
        for mb in cf.COLOUR_BOUNCES:
            for c, (e, b) in enumerate(zip(cf.COLOUR_EMIT, cf.COLOUR_BASE)):
                res, light = np.float64(0.0), np.float64(1.0)
                for _ in range(mb + 1):
                    res, light = ts.ray_hit_colours(res, light, np.float64(e), np.float64(b))
                assert float(res) == cf.coloured_sample(mb)[c]
                for n in cf.COLOUR_SPP:
                    assert float(ts.avg(ts.F64, [res] * n)) == cf.coloured_pixel(mb, n)[c]


def test_oracle_shading_and_averaging_from_the_text(oracle):
    """the oracle renders closed_form's non-dyadic scenes as the text says: the coloured closed box bit for bit for every
    (max_bounces, samples, spheres), the coloured lens cases inside the allowed set with a common k per pixel, and at least half of
    the possible k occur"""
    w, h = 24, 16
    cam = ((0.3, -0.2, 0.1), (1.0, 0.1, -0.05), 1.5)
    for n_sph in (0, 40):
        box = cf.closed_box_coloured(oracle.OBJECT_DTYPE, n_sph)
        for mb in cf.COLOUR_BOUNCES:
            for spp in cf.COLOUR_SPP:
                img = oracle_render(oracle, box, w, h, cam=cam, rays_per_pixel=spp, max_bounces=mb, seed=17 + spp + mb)
                assert same(img, np.broadcast_to(np.array(cf.coloured_pixel(mb, spp)), img.shape)), (n_sph, mb, spp)
    seen = {n: set() for n in cf.LENS_COLOUR_SPP}
    for name, objs, lcam, cfg in cf.lens_coloured_cases(oracle.OBJECT_DTYPE):
        for n in cf.LENS_COLOUR_SPP:
            img = oracle_render(oracle, objs, cf.LENS_COLOUR_FRAME, cf.LENS_COLOUR_FRAME, cam=lcam, rays_per_pixel=n, seed=100 + n, **cfg)
            k = cf.lens_lit_counts(img, n)
            assert (k >= 0).all(), (name, n)
            seen[n] |= set(k.ravel().tolist())
    for n in cf.LENS_COLOUR_SPP:
        assert 2 * len(seen[n]) >= n + 1, (n, len(seen[n]))
