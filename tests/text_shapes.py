"""The reference's intersection arithmetic, closest_object, the two colour updates of ray_hit and avg -- restated ONCE, from the text,
in plain scalar Python over a number namespace, so that the same lines run
  * on np.float64 scalars (F64: IEEE semantics under np.errstate(all="ignore") -- x / 0 and 0 / 0 do not raise, np.sqrt is correctly
    rounded, nothing is contracted): the BITS the text determines; and
  * on mpmath numbers: mp.mpf at 400 bits (MPF: the value the text means) and mp.iv at 53 bits (IV: outward rounding -- an enclosure of
    the real value AND of any round-to-nearest f64 evaluation of the same expression, as long as nothing under- or overflows).
This module imports neither the oracle nor the product package: it is a second reading of the text, independent of both.

Restated (file:line of the reference):
  vector.rs:85-107            dot and len sum left to right; norm divides each component by len
  sphere.rs:19-33             Sphere::distance (the NEAR root, no sign test) and normal
  plane.rs:20-35              Plane::distance (the two decisions use the RAW normal, the distance normal.norm()) and normal
  triangle.rs:26-35, :37-101, :104-127   plane_distance, contains (three whole rows and the row swaps, nothing hoisted), normal, distance
  object.rs:37-39             Object::normal_at's second norm
  scene.rs:243-251            closest_object: is_normal() && is_sign_positive(), total_cmp, the first minimum wins
  scene.rs:234                the hit point position + direction * dst (the direction AS GIVEN)
  scene.rs:276-277            resulting_color += light_color * emission; light_color *= base_color
  scene.rs:253-259 with iter_ops.rs:4-8 and div.rs:11-20   avg: fold(zeros, a + b), then each component / (len as f64)

Where the reference would PANIC -- the assert_eq! lines of triangle.rs:76-78 and :92-94, which fail on a non-finite pivot (r or s
non-finite, or s.x / r.x overflowing) -- `triangle_contains` returns None and `triangle_distance` raises ReferencePanics: there is
no value to compare.  Test inputs stay away from there.

A vector is a 3-tuple of numbers of the namespace; a shape is (kind, geom): kind 0 sphere (cx, cy, cz, radius), 1 plane (position,
normal), 2 triangle (v0, v1, v2)."""
import numpy as np

SPHERE, PLANE, TRIANGLE = 0, 1, 2
F64_MIN_NORMAL = 2.2250738585072014e-308                 # f64::MIN_POSITIVE: is_normal() is |x| >= this, finite


class Undecided(Exception):
    """an interval straddles one of the text's comparisons"""


class ReferencePanics(Exception):
    """triangle.rs:76-78 / :92-94: an assert_eq! of Triangle::contains fails"""


class F64:
    """np.float64 scalars.  Use inside `with np.errstate(all="ignore")`."""
    name = "f64"
    inf = np.float64(np.inf)

    @staticmethod
    def num(x):
        return np.float64(x)

    @staticmethod
    def sqrt(x):
        return np.sqrt(x)

    @staticmethod
    def abs(x):
        return np.abs(x)

    @staticmethod
    def lt(a, b):
        return bool(a < b)

    @staticmethod
    def le(a, b):
        return bool(a <= b)

    @staticmethod
    def eq(a, b):
        return bool(a == b)

    @staticmethod
    def asserted_eq(a, b):
        return bool(a == b)

    @staticmethod
    def is_normal_positive(x):                            # f64::is_normal() && f64::is_sign_positive()
        return bool(np.isfinite(x)) and bool(x >= F64_MIN_NORMAL)


class MPF:
    """mpmath.mpf at `prec` bits (a context of its own: the global mp.prec stays as it is)."""
    name = "mpf"

    def __init__(self, prec=400):
        import mpmath
        self.ctx = mpmath.MPContext()
        self.ctx.prec = prec
        self.inf = self.ctx.inf

    def num(self, x):
        return self.ctx.mpf(float(x)) if not isinstance(x, self.ctx.mpf) else x

    def sqrt(self, x):
        return self.ctx.sqrt(x)

    def abs(self, x):
        return abs(x)

    @staticmethod
    def lt(a, b):
        return bool(a < b)

    @staticmethod
    def le(a, b):
        return bool(a <= b)

    @staticmethod
    def eq(a, b):
        return bool(a == b)

    @staticmethod
    def asserted_eq(a, b):
        return bool(a == b)

    @staticmethod
    def is_normal_positive(x):                            # the f64 notion, applied to the value
        return bool(x >= F64_MIN_NORMAL) and bool(x < float("inf"))


class IV:
    """mpmath.iv at 53 bits: every operation rounds outward.  A comparison the interval does not decide raises Undecided; an
    assert_eq! holds when the interval CONTAINS the value (x / x is [1 - e, 1 + e] here: only IEEE decides a panic, the f64 run does)."""
    name = "iv"

    def __init__(self, prec=53):
        import mpmath
        self.ctx = mpmath.iv
        self.ctx.prec = prec
        self.inf = self.ctx.inf

    def num(self, x):
        return x if isinstance(x, self.ctx.mpf) else self.ctx.mpf(float(x))

    def sqrt(self, x):
        if x.a < 0:
            raise Undecided("sqrt of an interval that reaches below 0")
        return self.ctx.sqrt(x)

    def abs(self, x):
        return abs(x)

    def _iv(self, x):
        return self.num(x)

    def lt(self, a, b):
        a, b = self._iv(a), self._iv(b)
        if a.b < b.a:
            return True
        if a.a >= b.b:
            return False
        raise Undecided("<")

    def le(self, a, b):
        a, b = self._iv(a), self._iv(b)
        if a.b <= b.a:
            return True
        if a.a > b.b:
            return False
        raise Undecided("<=")

    def eq(self, a, b):
        a, b = self._iv(a), self._iv(b)
        if a.a == a.b == b.a == b.b:
            return True
        if a.b < b.a or b.b < a.a:
            return False
        raise Undecided("==")

    def asserted_eq(self, a, b):
        a, b = self._iv(a), self._iv(b)
        return bool(a.a <= b.b and b.a <= a.b)

    def is_normal_positive(self, x):
        return self.le(F64_MIN_NORMAL, x) and self.lt(x, self.inf)


# ---- Vector3 (vector.rs, vector/{add,sub,mul,div}.rs) ---------------------------------------------------------------------------------
def vec(ns, v):
    return (ns.num(v[0]), ns.num(v[1]), ns.num(v[2]))


def add(a, b):                                            # add.rs:16-24
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):                                            # sub.rs:16-24
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def muls(a, s):                                           # mul.rs:11-20
    return (a[0] * s, a[1] * s, a[2] * s)


def mulv(a, b):                                           # mul.rs:22-30: element-wise
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def divs(a, s):                                           # div.rs:11-20: three true divisions
    return (a[0] / s, a[1] / s, a[2] / s)


def dot(a, b):                                            # vector.rs:85-87: left to right
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):                                          # vector.rs:89-95
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def length(ns, a):                                        # vector.rs:97-103: (self * self).sum().sqrt(), sum = x + y + z
    sq = mulv(a, a)
    return ns.sqrt(sq[0] + sq[1] + sq[2])


def norm(ns, a):                                          # vector.rs:105-107
    return divs(a, length(ns, a))


# ---- Sphere (sphere.rs) -----------------------------------------------------------------------------------------------------------------
def sphere_distance(ns, g, ray_position, ray_direction):
    """sphere.rs:19-30.  None: the text's None."""
    position, radius = (g[0], g[1], g[2]), g[3]
    offset = sub(ray_position, position)
    ray_direction = norm(ns, ray_direction)
    a = dot(ray_direction, ray_direction)
    b = ns.num(2.0) * dot(offset, ray_direction)
    c = dot(offset, offset) - radius * radius
    discriminant = b * b - ns.num(4.0) * a * c
    if ns.le(discriminant, ns.num(1e-100)):               # (false for a NaN: the text goes on and returns a NaN)
        return None
    return (-b - ns.sqrt(discriminant)) / (ns.num(2.0) * a)


def sphere_normal(ns, g, world_position):                 # sphere.rs:31-33
    return norm(ns, sub(world_position, (g[0], g[1], g[2])))


# ---- Plane (plane.rs) -------------------------------------------------------------------------------------------------------------------
def plane_distance(ns, g, ray_pos, ray_dir):
    """plane.rs:20-31: the two decisions on the normal AS GIVEN, the distance with normal.norm()."""
    position, normal = (g[0], g[1], g[2]), (g[3], g[4], g[5])
    offset = sub(ray_pos, position)
    nhat = norm(ns, normal)
    d = norm(ns, ray_dir)
    zero = ns.num(0.0)
    if ns.le(zero, dot(d, normal)) or ns.le(dot(offset, normal), zero):       # >= 0. || <= 0.
        return None
    t = dot(offset, nhat) / dot(d, nhat)
    intersection_point = add(offset, muls(d, t))
    return length(ns, sub(offset, intersection_point))


def plane_normal(ns, g, relative_position):               # plane.rs:33-35
    return (g[3], g[4], g[5])


# ---- Triangle (triangle.rs) -------------------------------------------------------------------------------------------------------------
def _plane_vectors(g):                                    # triangle.rs:20-25
    basis = (g[0], g[1], g[2])
    return basis, sub((g[3], g[4], g[5]), basis), sub((g[6], g[7], g[8]), basis)


def triangle_normal(ns, g, world_position=None):          # triangle.rs:104-107
    _, a, b = _plane_vectors(g)
    return norm(ns, cross(a, b))


def _triangle_plane_distance(ns, g, ray_pos, d):          # triangle.rs:26-35
    d = norm(ns, d)
    normal = triangle_normal(ns, g)
    self_pos = (g[0], g[1], g[2])
    if ns.eq(dot(d, normal), ns.num(0.0)):
        return ns.inf
    return dot(normal, sub(self_pos, ray_pos)) / dot(d, normal)


def triangle_contains(ns, g, point, want_ab=False):
    """triangle.rs:37-101: Gauss-Jordan on the three rows (r.c, s.c, p.c), c = x, y, z, of a r + b s = p.  True / False; None where
    an assert_eq! would fail.  want_ab: ((a, b), answer) instead."""
    zero, one = ns.num(0.0), ns.num(1.0)
    pos, r, s = _plane_vectors(g)
    p = sub(point, pos)
    lgs1 = (r[0], s[0], p[0])
    lgs2 = (r[1], s[1], p[1])
    lgs3 = (r[2], s[2], p[2])
    if ns.eq(lgs1[0], zero):                              # :60-71
        if ns.eq(lgs2[0], zero):
            if ns.eq(lgs3[0], zero):
                return (None, False) if want_ab else False           # "can't handle LGS"
            lgs3, lgs1 = lgs1, lgs3
        else:
            lgs1, lgs2 = lgs2, lgs1
    lgs1 = divs(lgs1, lgs1[0])                            # :72
    lgs2 = sub(lgs2, muls(lgs1, lgs2[0] / lgs1[0]))       # :73
    lgs3 = sub(lgs3, muls(lgs1, lgs3[0] / lgs1[0]))       # :74
    if not (ns.asserted_eq(lgs1[0], one) and ns.asserted_eq(lgs2[0], zero) and ns.asserted_eq(lgs3[0], zero)):   # :76-78
        return (None, None) if want_ab else None
    if ns.eq(lgs2[1], zero):                              # :81-87
        if ns.eq(lgs3[1], zero):
            return (None, False) if want_ab else False               # "can't handle LGS"
        lgs2, lgs3 = lgs3, lgs2
    lgs2 = divs(lgs2, lgs2[1])                            # :88
    lgs1 = sub(lgs1, muls(lgs2, lgs1[1] / lgs2[1]))       # :89
    lgs3 = sub(lgs3, muls(lgs2, lgs3[1] / lgs2[1]))       # :90
    if not (ns.asserted_eq(lgs1[1], zero) and ns.asserted_eq(lgs2[1], one) and ns.asserted_eq(lgs3[1], zero)):   # :92-94
        return (None, None) if want_ab else None
    a, b = lgs1[2], lgs2[2]                               # :96
    inside = ns.le(zero, a) and ns.le(a, one) and ns.le(zero, b) and ns.le(b, one) and ns.le(a + b, one)      # :100
    return ((a, b), inside) if want_ab else inside


def triangle_distance(ns, g, pos, d):
    """triangle.rs:108-127: the cull by the direction AS GIVEN (:115), |plane distance| (:118: phantom hits behind the ray), the hit
    point along the direction AS GIVEN (:122)."""
    if ns.lt(dot(triangle_normal(ns, g), sub((g[0], g[1], g[2]), d)), ns.num(0.0)):       # :115
        return None
    distance = ns.abs(_triangle_plane_distance(ns, g, pos, d))                           # :118
    if ns.eq(distance, ns.inf):                                                          # :119
        return None
    hit_point = add(pos, muls(d, distance))                                              # :122
    inside = triangle_contains(ns, g, hit_point)
    if inside is None:
        raise ReferencePanics("Triangle::contains, an assert_eq! fails")
    if not inside:
        return None
    return distance


# ---- Object, Scene ----------------------------------------------------------------------------------------------------------------------
_DISTANCE = (sphere_distance, plane_distance, triangle_distance)
_NORMAL = (sphere_normal, plane_normal, triangle_normal)


def distance(ns, shape, pos, d):                          # object.rs:49-51
    return _DISTANCE[shape[0]](ns, shape[1], pos, d)


def normal_at(ns, shape, world_pos):                      # object.rs:37-39: the shape's normal, normalised AGAIN
    return norm(ns, _NORMAL[shape[0]](ns, shape[1], world_pos))


def closest_object(ns, shapes, pos, d):
    """scene.rs:243-251 -> (dst, index) or None.  Among the distances that pass the filter total_cmp is the order of the reals, and
    Iterator::min_by returns the FIRST minimum."""
    best = None
    for i, shape in enumerate(shapes):
        dst = distance(ns, shape, pos, d)
        if dst is None:
            continue
        if not ns.is_normal_positive(dst):                # :249 (a NaN, zero, a subnormal, a negative, an infinity: dropped)
            continue
        if best is None or ns.lt(dst, best[0]):           # :250
            best = (dst, i)
    return best


def hit_point(pos, d, dst):                               # scene.rs:234
    return add(pos, muls(d, dst))


def ray_hit_colours(resulting_color, light_color, emission_color, base_color):
    """scene.rs:276-277, one channel: (resulting_color + light_color * emission, light_color * base_color)"""
    return resulting_color + light_color * emission_color, light_color * base_color


def avg(ns, samples):
    """scene.rs:253-259, one channel: iter.sum() is fold(zeros, a + b) (iter_ops.rs:4-8), then / (len as f64) (div.rs:11-20)"""
    total = ns.num(0.0)
    for s in samples:
        total = total + s
    return total / ns.num(float(len(samples)))


# ---- packed scenes (the suite's object records) --------------------------------------------------------------------------------------
_GEOM_LEN = (4, 6, 9)


def shapes_of(ns, objs):
    """[(kind, geom)] in scene order from an array with fields kind and geom[9]"""
    return [(int(k), tuple(ns.num(x) for x in g[:_GEOM_LEN[int(k)]])) for k, g in zip(objs["kind"], objs["geom"])]


def answers(objs, origins, directions):
    """(distance, object, position, normal) arrays of the f64 reading for a batch of rays, as a closest-hit query reports them:
    +inf, -1, NaN, NaN where nothing is hit."""
    n = len(origins)
    dist = np.full(n, np.inf)
    obj = np.full(n, -1, dtype=np.int64)
    pos = np.full((n, 3), np.nan)
    nrm = np.full((n, 3), np.nan)
    with np.errstate(all="ignore"):
        shapes = shapes_of(F64, objs)
        for k in range(n):
            o, d = vec(F64, origins[k]), vec(F64, directions[k])
            best = closest_object(F64, shapes, o, d)
            if best is None:
                continue
            dist[k], obj[k] = best
            p = hit_point(o, d, best[0])
            pos[k] = p
            nrm[k] = normal_at(F64, shapes[best[1]], p)
    return dist, obj, pos, nrm
