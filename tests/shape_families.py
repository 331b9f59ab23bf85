"""Crafted scenes and rays for the shapes' arithmetic, with BOTH sides of every threshold of the text: tests/test_text_shapes.py runs
them through the oracle, tests/test_shapes_from_text.py through the device, and both compare with tests/text_shapes.py's f64 reading
bit for bit.  Where a decision flips between two neighbouring f64 inputs, the two are found by bisection on the f64 reading, and every
family asserts -- here, on the reading alone -- that it holds the outcomes it was built for.

Every scene carries filler shapes far from the action (six spheres and six triangles around y = 900), so that an upload builds a tree.
A family is (name, objects, origins [n][3], directions [n][3])."""
import itertools
import math
import types

import numpy as np

import text_shapes as ts
from helpers import fuzz_rays, fuzz_scene

S, P, T = ts.SPHERE, ts.PLANE, ts.TRIANGLE
MIN_NORMAL = ts.F64_MIN_NORMAL


# ---- the f64 reading of one shape / one scene -------------------------------------------------------------------------------------------
def _shape(shape):
    return (shape[0], tuple(np.float64(x) for x in shape[1]))


def dist(shape, o, d):
    """Some(dst) of the f64 reading as a float, or None"""
    with np.errstate(all="ignore"):
        r = ts.distance(ts.F64, _shape(shape), ts.vec(ts.F64, o), ts.vec(ts.F64, d))
    return None if r is None else float(r)


def kept(t):
    """passes closest_object's filter (scene.rs:249)"""
    return t is not None and math.isfinite(t) and t >= MIN_NORMAL


def winner(shapes, o, d):
    """(index, distance) of the f64 reading's closest_object, (-1, None) for none"""
    with np.errstate(all="ignore"):
        best = ts.closest_object(ts.F64, [_shape(s) for s in shapes], ts.vec(ts.F64, o), ts.vec(ts.F64, d))
    return (-1, None) if best is None else (best[1], float(best[0]))


def sphere_discriminant(g, o, d):
    """sphere.rs:20-25 up to the discriminant, f64 (to AIM rays at its thresholds; the expectation never uses it)"""
    with np.errstate(all="ignore"):
        ns = ts.F64
        g, o, d = tuple(ns.num(x) for x in g), ts.vec(ns, o), ts.vec(ns, d)
        offset = ts.sub(o, g[:3])
        dn = ts.norm(ns, d)
        a = ts.dot(dn, dn)
        b = ns.num(2.0) * ts.dot(offset, dn)
        c = ts.dot(offset, offset) - g[3] * g[3]
        return float(b * b - ns.num(4.0) * a * c)


def flip_pair(pred, lo, hi):
    """the two NEIGHBOURING f64 values in [lo, hi] between which pred changes (pred(lo) != pred(hi)), by bisection"""
    lo, hi = float(lo), float(hi)
    a = pred(lo)
    assert a != pred(hi), "no flip between %r and %r" % (lo, hi)
    while True:
        mid = lo + (hi - lo) / 2.0
        if mid == lo or mid == hi:
            break
        if pred(mid) == a:
            lo = mid
        else:
            hi = mid
    assert hi == np.nextafter(lo, hi) and pred(lo) == a and pred(hi) != a
    return lo, hi


# ---- packing ----------------------------------------------------------------------------------------------------------------------------------
def filler_shapes():
    """six spheres and six small triangles far from every ray of the families (a phantom triangle hit, triangle.rs:118, can still
    reach them: the f64 reading of the whole scene, fillers included, is what the answers are compared with).  The triangles are wound
    so that no unit direction is culled: an upload keeps them in its tree."""
    out = []
    for k in range(6):
        out.append((S, (3.0 * k - 7.0, 940.0 + k, 25.0, 1.0)))
    for k in range(6):
        b = np.array([2.0 + k, 900.0 + 3.0 * k, 0.3 * k])
        out.append((T, tuple(np.concatenate([b, b + (0.1, 0.6, 0.2), b + (0.5, 0.1, 0.0)]))))
    return out


def pack(dtype, shapes):
    o = np.zeros(len(shapes), dtype=dtype)
    for k, (kind, g) in enumerate(shapes):
        o[k]["kind"] = kind
        o[k]["geom"][:len(g)] = g
    o["base_color"] = 0.5
    o["emission_color"] = 1.0
    o["roughness"] = 1.0
    return o


def _family(dtype, name, shapes, rays):
    o = np.array([r[0] for r in rays], dtype=np.float64).reshape(-1, 3)
    d = np.array([r[1] for r in rays], dtype=np.float64).reshape(-1, 3)
    return name, pack(dtype, list(shapes) + filler_shapes()), np.ascontiguousarray(o), np.ascontiguousarray(d)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


# ---- spheres --------------------------------------------------------------------------------------------------------------------------------
def sphere_origins(dtype):
    """origin outside (hit), inside (the near root is negative: dropped, scene.rs:249) and ON the surface -- a previous hit point, as
    a bounced ray starts: the near root is 0 but for rounding, a last-place positive (kept: the ray hits the surface it stands on)
    or negative (dropped)"""
    sph = (S, (5.0, 0.3, -0.2, 1.3))
    c = np.array(sph[1][:3])
    rays, labels = [], []
    rng = np.random.default_rng(41)
    for j in (-9, -3, -2, -1, 0, 1, 2, 3, 9):
        d = _unit((5.0, 0.3 + 0.2 * j, -0.2 + 0.11 * j))
        rays.append(((0.0, 0.0, 0.0), d))
        t = dist(sph, (0.0, 0.0, 0.0), d)
        labels.append("outside:" + ("kept" if kept(t) else "dropped"))
        if t is None:
            continue
        p = np.zeros(3) + d * t                                   # a hit point (scene.rs:234)
        for k in range(6):
            w = _unit(rng.normal(size=3))
            for e in (_unit(p - c + 0.7 * w), _unit(c - p + 0.7 * w), _unit(np.cross(p - c, w)), _unit(c - p)):
                rays.append((p, e))
                labels.append("surface:" + ("kept" if kept(dist(sph, p, e)) else "dropped"))
    for k in range(12):
        o = c + rng.uniform(-0.6, 0.6, 3)
        e = _unit(rng.normal(size=3))
        rays.append((o, e))
        t = dist(sph, o, e)
        assert t is not None and t < 0.0
        labels.append("inside:dropped")
    assert {"outside:kept", "outside:dropped", "surface:kept", "surface:dropped", "inside:dropped"} <= set(labels), set(labels)
    return _family(dtype, "spheres: origin outside, inside, on the surface", [sph], rays)


def sphere_grazing(dtype):
    """sphere.rs:26, `discriminant <= 1e-100`: a unit-scale sphere (the discriminant moves in steps of 1e-14: hit / miss between two
    neighbouring directions) and a sphere of radius 1e-50 at 5e-50, where the discriminant moves in steps of 1e-114: neighbours on
    both sides of 1e-100, and on both sides of 0"""
    big, tiny = (S, (5.0, 0.0, 0.0, 1.0)), (S, (5e-50, 0.0, 0.0, 1e-50))
    o = (0.0, 0.0, 0.0)
    rays = []

    def dirn(y):
        return (5.0, y, 0.3)

    for sph in (big, tiny):
        lo, hi = flip_pair(lambda y: dist(sph, o, dirn(y)) is not None, 0.5, 2.0)
        assert dist(sph, o, dirn(lo)) is not None and dist(sph, o, dirn(hi)) is None
        rays += [(o, dirn(lo)), (o, dirn(hi)), (o, dirn(0.5)), (o, dirn(2.0))]
    dl, dh = sphere_discriminant(tiny[1], o, dirn(lo)), sphere_discriminant(tiny[1], o, dirn(hi))
    assert dl > 1e-100 >= dh > 0.0 and dl < 1.001e-100 and dh > 0.999e-100, (dl, dh)
    zlo, zhi = flip_pair(lambda y: sphere_discriminant(tiny[1], o, dirn(y)) < 0.0, 0.5, 2.0)
    dl, dh = sphere_discriminant(tiny[1], o, dirn(zlo)), sphere_discriminant(tiny[1], o, dirn(zhi))
    assert 0.0 <= dl < 1e-110 and -1e-110 < dh < 0.0, (dl, dh)
    rays += [(o, dirn(zlo)), (o, dirn(zhi))]
    for y in (0.9, 1.0, 1.01, 1.02, 1.03):                        # around the tangent of both
        rays.append((o, _unit(dirn(y))))
    return _family(dtype, "spheres: grazing rays", [big, tiny], rays)


def sphere_radii(dtype):
    """radius negative (only its square enters, sphere.rs:24: hit like |r|), zero and -0.0 (a point: the discriminant is 0 but for
    rounding -- a miss, or a last-place hit)"""
    shapes = [(S, (5.0, 0.0, 0.0, -0.7)), (S, (0.0, 6.0, 0.5, 0.0)), (S, (0.3, 0.2, 7.0, -0.0))]
    rays, hits = [], [0, 0, 0]
    rng = np.random.default_rng(43)
    for k, sh in enumerate(shapes):
        c = np.array(sh[1][:3])
        for j in range(40):
            o = rng.uniform(-1.0, 1.0, 3) if j % 2 else np.zeros(3)
            aim = c + (rng.normal(size=3) * 0.5 if j % 4 == 3 else 0.0)
            d = aim - o if j % 8 < 4 else _unit(aim - o)
            rays.append((o, d))
            hits[k] += kept(dist(sh, o, d))
    assert hits[0] >= 20 and hits[1] + hits[2] > 0 and hits[1] + hits[2] < 80, hits
    return _family(dtype, "spheres: radius negative and zero", shapes, rays)


DIRECTION_LENGTHS = (1e-160, 1e-3, 0.3, 7.0, 1e3, 1e160)


def sphere_direction_lengths(dtype):
    """sphere.rs:21 normalises the direction, so its length drops out -- until len under- or overflows: at 1e160 the squares are
    +inf, norm() is (0, 0, 0), a = b = 0 and the discriminant 0: no hit; at 1e-160 the squares are subnormal and norm() is a vector of
    length 0.98 ... 1.03.  The hit POINT uses the direction as given (scene.rs:234)."""
    sph = (S, (5.0, 0.3, -0.2, 1.3))
    rays, labels = [], []
    for j in range(-3, 4):
        u = _unit((5.0, 0.3 + 0.5 * j, -0.2 + 0.1 * j))
        for s in DIRECTION_LENGTHS + (1.0,):
            rays.append(((0.0, 0.0, 0.0), u * s))
            labels.append((s, kept(dist(sph, (0.0, 0.0, 0.0), u * s))))
    for s in DIRECTION_LENGTHS:
        assert (s, False) in labels
        assert ((s, True) in labels) == (s != 1e160), s
    return _family(dtype, "spheres: direction lengths", [sph], rays)


# ---- planes ---------------------------------------------------------------------------------------------------------------------------------
def planes(dtype):
    """plane.rs:25's two decisions on the normal as given -- origin exactly on the plane (offset . normal == 0: miss), direction exactly
    parallel (== 0: miss), their neighbours on both sides, origin behind -- with normals of length 1e-3 ... 1e3 and a -0.0 among the
    components"""
    p_small = (P, (4.0, 0.0, 0.0, -0.8e-3, 0.5e-3, 0.33e-3))      # |normal| = 0.9994e-3
    p_large = (P, (0.0, -6.0, 1.0, 3e2, 9.3e2, -2.2e2))            # |normal| = 1.0016e3
    p_zero = (P, (0.0, 0.0, -7.0, -0.0, 0.0, 2.0))
    p_exact = (P, (2.0, 2.0, 2.0, 1.0, 2.0, 0.0))
    shapes = [p_small, p_large, p_zero, p_exact]
    rays = []
    rng = np.random.default_rng(47)
    seen = set()
    for j in range(60):
        o = rng.uniform(-3.0, 3.0, 3)
        d = rng.normal(size=3)
        if j % 3 == 0:
            d = _unit(d)
        if j % 5 == 0:
            d[j % 3] = -0.0
        if j % 7 == 0:
            o[(j + 1) % 3] = -0.0
        rays.append((o, d))
        for k, sh in enumerate(shapes):
            seen.add((k, dist(sh, o, d) is not None))
    assert all((k, b) in seen for k in range(4) for b in (True, False)), seen
    # origin exactly on the plane, and its neighbours along z
    d = (0.1, 0.2, -1.0)
    assert dist(p_zero, (1.5, -2.25, -7.0), d) is None
    assert dist(p_zero, (1.5, -2.25, float(np.nextafter(-7.0, 0.0))), d) is not None
    assert dist(p_zero, (1.5, -2.25, float(np.nextafter(-7.0, -8.0))), d) is None
    rays += [((1.5, -2.25, z), d) for z in (-7.0, float(np.nextafter(-7.0, 0.0)), float(np.nextafter(-7.0, -8.0)))]
    # an oblique normal: (2, -1, 3) . (1, 2, 0) == 0 exactly
    d = (-1.0, -2.0, 0.5)
    on = (4.0, 1.0, 5.0)
    assert dist(p_exact, on, d) is None and dist(p_exact, (4.001, 1.002, 5.0), d) is not None
    lo, hi = flip_pair(lambda e: dist(p_exact, (4.0 + e, 1.0 + 2.0 * e, 5.0), d) is not None, -1e-3, 1e-3)
    rays += [(on, d)] + [((4.0 + e, 1.0 + 2.0 * e, 5.0), d) for e in (lo, hi)]
    # a direction exactly parallel: norm(2, -1, 5) . (1, 2, 0) == 0 exactly (2 / len - (1 / len) * 2)
    o = (3.0, 4.0, 2.0)
    assert dist(p_exact, o, (2.0, -1.0, 5.0)) is None
    lo, hi = flip_pair(lambda e: dist(p_exact, o, (2.0 + e, -1.0 + 2.0 * e, 5.0)) is not None, -1e-3, 1e-3)
    rays += [(o, (2.0, -1.0, 5.0))] + [(o, (2.0 + e, -1.0 + 2.0 * e, 5.0)) for e in (lo, hi)]
    return _family(dtype, "planes", shapes, rays)


# ---- triangles ------------------------------------------------------------------------------------------------------------------------------
def _oriented(v0, v1, v2, towards):
    """the triangle wound so that its normal has a positive component along `towards`"""
    v0, v1, v2 = (np.asarray(v, dtype=np.float64) for v in (v0, v1, v2))
    if float(np.cross(v1 - v0, v2 - v0) @ np.asarray(towards)) < 0.0:
        v1, v2 = v2, v1
    return (T, tuple(np.concatenate([v0, v1, v2])))


def triangle_cull(dtype):
    """triangle.rs:115 culls with n . (v0 - dir), the direction AS GIVEN: along one line of sight the same triangle is hit for a short
    direction and culled for a long one.  Lengths 0.01 ... 100 and the two neighbouring lengths at the threshold, for a triangle in
    x = 5 and an oblique one; triangle.rs:122 advances along the un-normalised direction, so the point `contains` tests is off the
    plane (its projection along the dropped row decides).  And the same line backwards: phantom hits behind the origin (:118)."""
    u = _unit((1.0, 0.02, 0.05))
    o = (0.0, 0.0, 0.0)
    tris = [(T, (5.0, -10.0, -10.0, 5.0, 10.0, -10.0, 5.0, 0.0, 10.0)),
            _oriented((-20.0, -20.0, 25.0), (60.0, -20.0, -55.0), (5.0, 40.0, 0.0), u)]      # in x + z = 5
    rays = []
    for tri in tris:
        lo, hi = flip_pair(lambda k: dist(tri, o, u * k) is not None, 0.01, 100.0)
        assert kept(dist(tri, o, u * lo)) and dist(tri, o, u * hi) is None and 1.0 < lo < 100.0
        rays += [(o, u * lo), (o, u * hi)]
        assert kept(dist(tri, o, -u)) and kept(dist(tri, o, -u * 2.0))        # phantom hits
    for k in np.geomspace(0.01, 100.0, 25):
        rays += [(o, u * k), (o, -u * k)]
    rng = np.random.default_rng(53)
    for j in range(60):                                             # non-unit directions from anywhere
        oo = rng.uniform(-3.0, 3.0, 3)
        rays.append((oo, (rng.uniform(-9.0, 9.0, 3) + (5.0, 0.0, 0.0) - oo) * rng.uniform(0.05, 3.0)))
    return _family(dtype, "triangles: the cull by direction, non-unit directions, phantom hits", tris, rays)


def triangle_row_swaps(dtype):
    """every branch of Triangle::contains' row handling (triangle.rs:60-71, :81-87), with r = v1 - v0, s = v2 - v0:
    0 no swap; 1 r.x == 0; 2 r.x == r.y == 0; 3 r == 0 ("can't handle LGS", never hit); 4 the second pivot 0 with a usable third
    row; 5 the second pivot 0 and no third row (s = 2 r: "can't handle LGS"; the normal is 0 / 0); 6 r.x == -0.0."""
    tris = [(T, (1.0, 1.0, 4.0, 2.5, 1.5, 4.5, 1.5, 3.0, 5.0)),
            (T, (3.0, 0.0, 0.0, 3.0, 2.0, 0.5, 4.0, 0.5, 2.0)),
            (T, (-3.0, 0.0, 0.0, -3.0, 0.0, 2.0, -4.0, 1.5, 0.5)),
            (T, (0.0, 5.0, 0.0, 0.0, 5.0, 0.0, 1.0, 5.0, 1.0)),
            (T, (0.0, -5.0, 0.0, 1.0, -4.0, 0.0, 2.0, -3.0, 3.0)),
            (T, (0.0, 0.0, 6.0, 1.0, 1.0, 7.0, 2.0, 2.0, 8.0)),
            (T, (0.0, 0.0, -5.0, -0.0, 2.0, -5.5, 1.0, 0.5, -7.0))]
    g = np.array(tris[6][1])
    assert math.copysign(1.0, g[3] - g[0]) < 0.0 and g[3] - g[0] == 0.0
    rays = []
    hit = [set() for _ in tris]
    rng = np.random.default_rng(59)
    for k, tri in enumerate(tris):
        v = np.array(tri[1]).reshape(3, 3)
        r, s = v[1] - v[0], v[2] - v[0]
        if k in (3, 5):
            s = s + (0.3, -0.2, 0.1)                              # (aim somewhere: the shape itself is degenerate)
        for a, b in ((0.3, 0.3), (0.1, 0.8), (0.6, 0.1), (-0.2, 0.5), (0.5, -0.2), (0.7, 0.6), (1.2, 0.1), (0.02, 0.02)):
            target = v[0] + a * r + b * s
            for j in range(4):
                o = rng.uniform(-0.5, 0.5, 3) + (0.1, 0.2, 0.3)
                if j == 1:
                    o = 2.0 * target - o                          # from the other side
                d = _unit(target - o) if j != 2 else (target - o) * 0.7
                if j == 3:
                    d = -d
                rays.append((o, d))
                hit[k].add(kept(dist(tri, o, d)))
    for k in (0, 1, 2, 4, 6):
        assert hit[k] == {True, False}, (k, hit[k])
    assert hit[3] == {False} and hit[5] == {False}
    return _family(dtype, "triangles: the row swaps of contains", tris, rays)


def triangle_edges(dtype):
    """triangle.rs:100: a = 0, b = 0 and a + b = 1 are INSIDE.  A triangle in x = 5 with dyadic vertices, rays along +x: the hit point
    and (a, b) are exact.  The three vertices, a point of every edge, and for each its neighbour one place outside; dir . n == 0
    exactly (triangle.rs:31: no distance)."""
    tri = (T, (5.0, -1.0, -1.0, 5.0, 1.0, -1.0, 5.0, 0.0, 1.0))
    d = (1.0, 0.0, 0.0)
    rays = []
    # (y, z) on the border, and the coordinate + direction to step outside
    border = [((-1.0, -1.0), (0, -2.0)), ((-1.0, -1.0), (1, -2.0)), ((1.0, -1.0), (0, 2.0)), ((1.0, -1.0), (1, -2.0)),
              ((0.0, 1.0), (1, 2.0)), ((-0.5, 0.0), (0, -2.0)), ((0.0, -1.0), (1, -2.0)), ((0.5, 0.0), (0, 2.0)), ((0.25, 0.5), (1, 2.0))]
    for (y, z), (axis, to) in border:
        on = [0.0, y, z]
        assert dist(tri, on, d) == 5.0, on
        rays.append((tuple(on), d))
        for _ in range(64):                                         # (p = point - v0 rounds: the first places outside may still be "on")
            out = list(on)
            out[1 + axis] = float(np.nextafter(on[1 + axis], to))
            if dist(tri, out, d) is None:
                break
            on = out
        assert dist(tri, on, d) == 5.0 and dist(tri, out, d) is None, (on, out)
        rays += [(tuple(on), d), (tuple(out), d)]
    for dd in ((0.0, 1.0, 0.0), (0.0, 0.0, -3.0), (0.0, 0.6, 0.8)):
        assert dist(tri, (0.0, 0.0, 0.0), dd) is None
        rays.append(((0.0, 0.0, 0.0), dd))
    return _family(dtype, "triangles: edges, vertices, parallel directions", [tri], rays)


def triangle_subnormal(dtype):
    """scene.rs:249 is is_normal(), not > 0: a triangle 1e-310 in front of the origin reports a SUBNORMAL distance, is dropped, and the
    sphere behind it wins; at 3e-308 (normal) the triangle wins.  Both sides of f64::MIN_POSITIVE as well.  Only Triangle::distance
    can return a positive subnormal."""
    tri = (T, (0.0, -1.0, -1.0, 0.0, 0.0, 1.0, 0.0, 1.0, -1.0))   # n = (-1, 0, 0)
    sph = (S, (3.0, 0.0, 0.0, 1.0))
    d = (1.0, 0.0, 0.0)
    rays, won = [], []
    for x in (1e-310, 3e-308, MIN_NORMAL, float(np.nextafter(MIN_NORMAL, 0.0)), 5e-324, 1e-300):
        o = (-x, 0.0, 0.0)
        assert dist(tri, o, d) == x
        rays.append((o, d))
        won.append(winner([tri, sph], o, d)[0])
    assert won == [1, 0, 0, 1, 1, 0], won
    return _family(dtype, "triangles: a subnormal distance", [tri, sph], rays)


# ---- ties across kinds ----------------------------------------------------------------------------------------------------------------------
def _tie_shapes(nearer=None):
    """a plane, a sphere and a triangle that the ray from the origin along +x meets at exactly 4.0 -- or, for `nearer` (a kind), that one
    one place nearer than the other two"""
    x = float(np.nextafter(4.0, 0.0))
    up = float(np.nextafter(4.0, 5.0))
    o, d = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    px = x if nearer == P else (up if nearer == S else 4.0)       # (the sphere's root moves in coarser steps: the other two step back)
    tx = x if nearer == T else (up if nearer == S else 4.0)
    plane = (P, (px, 0.0, 0.0, -1.0, 0.0, 0.0))
    tri = (T, (tx, -1.0, -1.0, tx, 1.0, -1.0, tx, 0.0, 1.0))
    sph = (S, (5.0, 0.0, 0.0, 1.0))
    want = {P: px, S: 4.0, T: tx}
    for sh in (plane, sph, tri):
        assert dist(sh, o, d) == want[sh[0]], (sh, dist(sh, o, d))
    return {P: plane, S: sph, T: tri}


def tie_scenes(dtype):
    """closest_object keeps the FIRST minimum in scene order (scene.rs:250), across kinds -- the device keeps spheres, planes and
    triangles in separate arrays.  All six orders of the three, all ordered pairs, and all six orders again with one of the three one
    place nearer (it wins wherever it stands); fillers before, between and after.  Yields (name, objects, origins, directions, index
    of the expected winner)."""
    fill = filler_shapes()
    blocks = [[fill[0], fill[6], fill[1]], [fill[7], fill[2], fill[8]], [fill[3], fill[9], fill[4]], [fill[10], fill[5], fill[11]]]
    names = {P: "plane", S: "sphere", T: "triangle"}
    o, d = np.zeros((1, 3)), np.array([[1.0, 0.0, 0.0]])
    for nearer in (None, S, P, T):
        shapes = _tie_shapes(nearer)
        orders = list(itertools.permutations((S, P, T)))
        if nearer is None:
            orders += list(itertools.permutations((S, P, T), 2))
        for order in orders:
            scene, at = [], {}
            for k, kind in enumerate(order):
                scene += blocks[k]
                at[kind] = len(scene)
                scene.append(shapes[kind])
            scene += blocks[len(order)]
            for blk in blocks[len(order) + 1:]:
                scene += blk
            first = at[order[0]] if nearer is None else at[nearer]
            assert winner(scene, o[0], d[0]) == (first, float(np.nextafter(4.0, 0.0)) if nearer in (P, T) else 4.0)
            name = "tie: " + ", ".join(names[k] for k in order) + ("" if nearer is None else "; the %s one place nearer" % names[nearer])
            yield name, pack(dtype, scene), o, d, first


def families(dtype):
    for build in (sphere_origins, sphere_grazing, sphere_radii, sphere_direction_lengths, planes, triangle_cull, triangle_row_swaps,
                  triangle_edges, triangle_subnormal):
        yield build(dtype)


# ---- the fuzz ---------------------------------------------------------------------------------------------------------------------------------
FUZZ_SCENES, FUZZ_RAYS, AIMED_RAYS = 150, 160, 320


def fuzz_cases(dtype, n_scenes=FUZZ_SCENES):
    """The scenes and rays of test_queries_equal_the_oracle_on_fuzzed_scenes (the same generator calls on the same seed), the first
    FUZZ_RAYS rays of each scene -- 24 000 in all, the zero and NaN directions among them -- and AIMED_RAYS more per scene from the
    next origins of the same batch TOWARDS a point of a sphere's surface or of a triangle (seven in ten unit length, so that the
    tree walk takes them; a generator of their own, so that the scenes stay the same).  fuzz_rays alone hits something with one
    ray in three; with the aimed ones more than half of all rays do.  Yields (index, objects, camera, origins, directions)."""
    rng = np.random.default_rng(2024)
    shim = types.SimpleNamespace(OBJECT_DTYPE=dtype)
    for s in range(n_scenes):
        objs, cam = fuzz_scene(shim, rng)
        o, d = fuzz_rays(rng, objs, 2048)
        o, d = o[:FUZZ_RAYS + AIMED_RAYS].copy(), d[:FUZZ_RAYS + AIMED_RAYS].copy()
        rng2 = np.random.default_rng(7700 + s)
        g = objs["geom"]
        sph = g[(objs["kind"] == 0) & (g[:, 3] != 0.0)]
        tri = g[objs["kind"] == 2]
        for k in range(FUZZ_RAYS, len(o)):
            if len(sph) + len(tri) == 0:
                break
            j = int(rng2.integers(0, len(sph) + len(tri)))
            if j < len(sph):
                target = sph[j, :3] + abs(sph[j, 3]) * _unit(rng2.normal(size=3))
            else:
                w = rng2.dirichlet((1.0, 1.0, 1.0))
                v = tri[j - len(sph)].reshape(3, 3)
                target = v[0] * w[0] + v[1] * w[1] + v[2] * w[2]
            t = target - o[k]
            if not np.isfinite(t).all() or not t.any():
                continue
            d[k] = _unit(t) if rng2.random() < 0.7 else t * rng2.uniform(0.1, 3.0)
        yield s, objs, cam, np.ascontiguousarray(o), np.ascontiguousarray(d)
