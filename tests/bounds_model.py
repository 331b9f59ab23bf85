"""A model of the tree walks' f32 bound arithmetic (rtx_traverse.h box_entry32 / rect_entry32 / sphere_node_step_q3 / the sphere leaf
bounds, rtx_mesh_step.h qrect_entry / tri_bounds, rtx_device.h tri_filter_sign) and of the builder's boxes and records (rtx_bvh.h,
rtx_pack.hip pack_scene; refit() and deform(): what an update in place must leave, from its documented contract), in which every f32 operation is formed EXACTLY and rounded ONCE, and every margin is a knob.

How one rounding is kept.  All operands are f32 values held in f64.  A product of two of them is exact in f64 (48 bits).  A sum s + c
of two f64 values is formed exactly as hi + lo (Knuth's two-sum), hi is moved to the neighbour with an odd last bit when lo != 0
(round to odd: 53 >= 2 * 24 + 2 bits), and only then rounded to f32 -- the result is RN_f32 of the exact sum, so an fma is one
rounding, not two.  f32 division and the conversions from f64 go through one f64 operation, which is innocuous for the same reason.
`exact_fma32` does the same with fractions.Fraction, one number at a time; tests/test_walk_bounds.py holds the array form to it.
Everything is numpy over the batch of rays, so 10^5 pairs take a second.

What is NOT exact: the hardware square root of the sphere bounds (__builtin_amdgcn_sqrtf: 1 ulp).  It is an interval -- one f32
below the rounded-down root to one above the rounded-up root -- and the two bounds are evaluated at both ends (every later operation is
monotone).  f32 division (tri_bounds) is taken as correctly rounded; the gpu part of the test compares it with the device.

Margins (class Margins): each is a factor on the shipped constant, 1.0 as shipped; a test weakens one at a time.
  widen     the 2^-21 widening of the slab interval         abs_pad   the builder's absolute padding of every box
  abs_pad2  the 64-byte sphere nodes' second abs_pad        slack     Ray32S's slack for origins beyond origin_limit (both terms)
  K, G      the sphere bounds' K = 24uM and G = 128uMr + 8192u^2M^2
  e_nv, e_dn, e_ab   tri_bounds' 16uS, 8u and the (a, b) margins ea / eb
  E         the sweep's sphere filter: E = 64uM^2 of filter_from_ray (sweep_params)
  A         the triangle filter's allowance A = 64uS of tri_filter_from_ray (tri_params; tri_bounds takes its S from the same word)

The LDS sweep's filters (trace_mixed_kernel, rtx_kernels.hip): sweep_record() restates the sphere_f32 records of pack_scene /
derive_sphere, sweep_params() filter_from_ray, sweep_disc() filter_disc1 and filter_disc2 (one nesting), tri_filter_sxy()
tri_filter_sign; tests/test_sweep_filters.py holds them to the f64 text and to the device (rtx_debug_sweep_filter).
"""
from dataclasses import dataclass, replace
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
F32 = np.float32
INF32 = F32(np.inf)
RANGE64 = 134217728.0                                    # kBvhRange64
DIR_TOL = 9.094947017729282e-13                          # kQueryDirTol


@dataclass(frozen=True)
class Margins:
    widen: float = 1.0
    abs_pad: float = 1.0
    abs_pad2: float = 1.0
    slack: float = 1.0
    K: float = 1.0
    G: float = 1.0
    e_nv: float = 1.0
    e_dn: float = 1.0
    e_ab: float = 1.0
    E: float = 1.0
    A: float = 1.0


SHIPPED = Margins()
WEAKENED = {name: replace(SHIPPED, **{name: 0.0}) for name in ("widen", "abs_pad", "abs_pad2", "slack", "K", "G", "e_nv", "e_dn", "e_ab", "E", "A")}


# ---- f32 operations, one rounding each --------------------------------------------------------------------------------------------------
def _d(x):
    return np.asarray(x, dtype=np.float64)


def _sum32(s, c):
    """RN_f32(s + c), s and c f64 values whose exact sum is wanted"""
    s, c = np.broadcast_arrays(_d(s), _d(c))
    with np.errstate(all="ignore"):
        hi = s + c
        bb = hi - s
        lo = (s - (hi - bb)) + (c - bb)
        fix = np.isfinite(hi) & np.isfinite(lo) & (lo != 0.0)
        bits = hi.copy().view(np.int64)
        even = (bits & 1) == 0
        grow = (lo > 0.0) == (hi > 0.0)                    # the exact sum lies beyond hi, away from zero
        step = np.where(grow, 1, -1).astype(np.int64)
        bits = np.where(fix & even, bits + step, bits)
        return bits.view(np.float64).astype(F32)


def add32(a, b):
    return _sum32(a, b)


def sub32(a, b):
    return _sum32(a, -_d(b))


def mul32(a, b):
    with np.errstate(all="ignore"):
        return (_d(a) * _d(b)).astype(F32)


def fma32(a, b, c):
    with np.errstate(all="ignore"):
        return _sum32(_d(a) * _d(b), c)


def div32(a, b):
    with np.errstate(all="ignore"):
        return (_d(a) / _d(b)).astype(F32)


def ru32(x):
    """f64 -> f32 rounded up (__double2float_ru, round_up_f32)"""
    x = _d(x)
    with np.errstate(all="ignore"):
        f = x.astype(F32)
        return np.where(f.astype(np.float64) < x, np.nextafter(f, INF32), f).astype(F32)


def rd32(x):
    x = _d(x)
    with np.errstate(all="ignore"):
        f = x.astype(F32)
        return np.where(f.astype(np.float64) > x, np.nextafter(f, -INF32), f).astype(F32)


def rn32(x):
    with np.errstate(all="ignore"):
        return _d(x).astype(F32)


def sqrt32_interval(x):
    """[lo, hi] f32 that hold every value within 1 ulp of sqrt(x), x >= 0 an f32"""
    with np.errstate(all="ignore"):
        s = np.sqrt(_d(x))
    lo = np.nextafter(rd32(s), -INF32)
    hi = np.nextafter(ru32(s), INF32)
    return np.maximum(lo, F32(0.0)).astype(F32), hi.astype(F32)


def exact_fma32(a, b, c):
    """RN_f32(a * b + c) of three finite f32 values, through fractions.Fraction: the scalar check of fma32 / add32 / mul32"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return F32(0.0)
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    q = max(e, -126) - 23                                 # the exponent of the last place (gradual underflow below 2^-126)
    m = x / Fraction(2) ** q
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** q
    if v >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(v))


# ---- the ray as the walks prepare it ------------------------------------------------------------------------------------------------------
def vnorm(d):
    d = _d(d)
    with np.errstate(all="ignore"):
        ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return d / ln[:, None]


def ray_form(pos, dirs, limit32):
    """query_walkable: (form, in32) -- 0 Ray32, 1 beyond origin_limit (Ray32S's slack or Ray64), 3 no walk"""
    pos, dirs = _d(pos), _d(dirs)
    with np.errstate(all="ignore"):
        omax = np.max(np.abs(pos.astype(F32)), axis=1)    # (a NaN propagates: every comparison below is then false)
        omax = np.where(np.isnan(pos).any(axis=1), F32(np.nan), omax)
        in32 = omax <= F32(limit32)
        far = omax <= mul32(F32(limit32), F32(RANGE64))
        n2 = (dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2]
        dir_ok = np.abs(n2 - 1.0) <= DIR_TOL
    walk = dir_ok & (in32 | far)
    return np.where(walk, np.where(in32, 0, 1), 3), in32


def make_ray32(pos, dirs, inv_max32, in32, m=SHIPPED):
    """make_ray32 + ray32_slack: dict inv (n, 3), noi (n, 3), e (n,)"""
    pos, dn = _d(pos), vnorm(dirs)
    inv_max = float(F32(inv_max32))
    with np.errstate(all="ignore"):
        i = 1.0 / dn
        i = np.where(np.abs(i) <= inv_max, i, np.copysign(inv_max, dn))
        inv = i.astype(F32)
        noi = (-pos * inv.astype(np.float64)).astype(F32)
    c = F32(2.0 ** -23 * (1.0 + 2.0 ** -20))
    an, ai = np.abs(noi), np.abs(inv)
    with np.errstate(all="ignore"):                         # ray32_slack: noi's rounding + the reference's own roundings (rtx_traverse.h)
        om = np.max(div32(an, ai), axis=1)
        extra = np.minimum(mul32(mul32(om, np.max(ai, axis=1)), F32(2.0) * c), F32(1.0e38))
        e = np.where(in32, F32(0.0), add32(mul32(np.max(an, axis=1), c), extra))
    e = mul32(e, F32(m.slack))
    return {"inv": inv, "noi": noi, "e": e.astype(F32)}


def _finish(tn, tf, q, best_up, m):
    w = 2.0 ** -21 * m.widen
    tn_lo = fma32(tn, F32(1.0 - w), -q["e"])
    tf_hi = fma32(tf, F32(1.0 + w), q["e"])
    with np.errstate(all="ignore"):
        hit = (tn_lo <= tf_hi) & (tn_lo <= F32(best_up))
    return np.where(hit, tn_lo, INF32).astype(F32)


def box_entry32(lo, hi, q, best_up, m=SHIPPED):
    """lo, hi (n, 3) f32 -> the entry distance, +inf on a miss"""
    x0, x1 = fma32(lo, q["inv"], q["noi"]), fma32(hi, q["inv"], q["noi"])
    with np.errstate(all="ignore"):
        tn = np.maximum(np.max(np.minimum(x0, x1), axis=1), F32(0.0))
        tf = np.min(np.maximum(x0, x1), axis=1)
    return _finish(tn, tf, q, best_up, m)


def rect_entry32(r4, q, best_up, m=SHIPPED):
    """r4 (n, 4) = {lo.x, lo.y, hi.x, hi.y}"""
    inv, noi = q["inv"][:, :2], q["noi"][:, :2]
    x0, x1 = fma32(r4[:, 0:2], inv, noi), fma32(r4[:, 2:4], inv, noi)
    with np.errstate(all="ignore"):
        tn = np.maximum(np.max(np.minimum(x0, x1), axis=1), F32(0.0))
        tf = np.min(np.maximum(x0, x1), axis=1)
    return _finish(tn, tf, q, best_up, m)


def q3_entry(o, s, qlo, qhi, q, best_up, m=SHIPPED):
    """sphere_node_step_q3's test of one child: o, s (n, 3) f32, qlo, qhi (n, 3) integers 0..255 -> (entered, tn_lo)"""
    S = mul32(s, q["inv"])
    O = fma32(o, q["inv"], q["noi"])
    neg = q["inv"] < 0
    near, far = np.where(neg, qhi, qlo).astype(F32), np.where(neg, qlo, qhi).astype(F32)
    x0, x1 = fma32(near, S, O), fma32(far, S, O)
    with np.errstate(all="ignore"):
        tn = np.maximum(np.max(x0, axis=1), F32(0.0))
        tf = np.min(x1, axis=1)
    w = 2.0 ** -21 * m.widen
    tn_lo = fma32(tn, F32(1.0 - w), -q["e"])
    tf_hi = fma32(tf, F32(1.0 + w), q["e"])
    with np.errstate(all="ignore"):
        return tn_lo <= np.minimum(tf_hi, F32(best_up)), tn_lo


def qrect_entry(o, s, qx, qy, q, best_up, m=SHIPPED):
    """mesh_step<2>'s test of one child: o, s (n, 2) f32, qx, qy (n,) = lo | hi << 16"""
    inv, noi = q["inv"][:, :2], q["noi"][:, :2]
    A = mul32(s, inv)
    B = fma32(o, inv, noi)
    ql = np.stack([qx & 0xFFFF, qy & 0xFFFF], axis=1).astype(F32)
    qh = np.stack([qx >> 16, qy >> 16], axis=1).astype(F32)
    x0, x1 = fma32(ql, A, B), fma32(qh, A, B)
    with np.errstate(all="ignore"):
        tn = np.maximum(np.max(np.minimum(x0, x1), axis=1), F32(0.0))
        tf = np.min(np.maximum(x0, x1), axis=1)
    return _finish(tn, tf, q, best_up, m)


# ---- sphere bounds --------------------------------------------------------------------------------------------------------------------------
def sphere_ray(pos, dirs, centre, cmax, m=SHIPPED):
    pos, dirs = _d(pos), _d(dirs)
    with np.errstate(all="ignore"):
        p = pos - _d(centre)[None, :]
        M = cmax + np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        off = ~(M < 1.0e14) | ~(M > 1.0e-12)
        Kg = ru32(128.0 * U * M)
        c0 = ru32(8192.0 * U * U * M * M)
        K = ru32(24.0 * U * M)
    z = F32(0.0)
    sr = {"p": np.where(off[:, None], z, p.astype(F32)), "d": np.where(off[:, None], z, dirs.astype(F32)),
          "Kg": mul32(np.where(off, z, Kg), F32(m.G)), "c0": np.where(off, INF32, mul32(c0, F32(m.G))),
          "K": mul32(np.where(off, z, K), F32(m.K)), "off": off, "M": M}
    return sr


def sphere_leaf(rec, sr, best_up):
    """the leaf bounds of one record {c - centre, r} per ray -> dict: cand / certain (from best_up = +inf) as [worst, best] pairs over
    the sqrt interval, tlo and thi as (low end, high end)"""
    p, d = sr["p"], sr["d"]
    o = sub32(rec[:, :3], p)
    b = fma32(o[:, 0], d[:, 0], fma32(o[:, 1], d[:, 1], mul32(o[:, 2], d[:, 2])))
    l = fma32(-b[:, None], d, o)
    l2 = fma32(l[:, 0], l[:, 0], fma32(l[:, 1], l[:, 1], mul32(l[:, 2], l[:, 2])))
    r = rec[:, 3]
    Dl = fma32(r, r, -l2)
    G = fma32(sr["Kg"], r, sr["c0"])
    Dp, Dm = add32(Dl, G), sub32(Dl, G)
    with np.errstate(all="ignore"):
        pass0 = Dp >= 0
        sp_lo, sp_hi = sqrt32_interval(np.where(pass0, Dp, F32(0.0)))
        sm_lo, sm_hi = sqrt32_interval(np.where(Dm > 0, Dm, F32(0.0)))
        up, dn = F32(1.0 + 2.0 ** -21), F32(1.0 - 2.0 ** -21)
        tlo = [sub32(sub32(b, mul32(s, up)), sr["K"]) for s in (sp_hi, sp_lo)]          # (low end, high end)
        thi = [np.where(Dm > 0, add32(sub32(b, mul32(s, dn)), sr["K"]), INF32).astype(F32) for s in (sm_hi, sm_lo)]
        bu = F32(best_up) if np.ndim(best_up) == 0 else np.asarray(best_up, dtype=F32)
        out = {"tlo": tlo, "thi": thi, "Dp": Dp, "Dm": Dm, "b": b, "G": G, "Dl": Dl}
        for k, (tl, th) in enumerate(((tlo[1], thi[0]), (tlo[0], thi[1]))):                # k = 0: the end that hurts, 1: the kind one
            open_ = pass0 & ~(th < 0)
            out["cand%d" % k] = open_ & (tl <= bu)
        # certain: the +inf run lowers the bound.  worst for "unreported => not certain" is the end where tlo is largest
        out["certain_any"] = pass0 & ~(thi[1] < 0) & (tlo[1] > sr["K"]) & (thi[0] < INF32)
        out["certain_all"] = pass0 & ~(thi[0] < 0) & (tlo[0] > sr["K"]) & (thi[1] < INF32)
    return out


# ---- triangle bounds --------------------------------------------------------------------------------------------------------------------------
def tri_params(pos, dirs, centre, tri_extent, m=SHIPPED):
    """tri_filter_from_ray: d, np = -p, A = 64uS (times m.A), off: the pass-all filter (A = 1e30) of S >= 1e14 or a NaN origin"""
    pos, dirs = _d(pos), _d(dirs)
    with np.errstate(all="ignore"):
        p = pos - _d(centre)[None, :]
        S = tri_extent + np.abs(p[:, 0]) + np.abs(p[:, 1]) + np.abs(p[:, 2]) + 1.0
        off = ~(S < 1.0e14)
        z = F32(0.0)
        return {"d": np.where(off[:, None], z, dirs.astype(F32)), "np": np.where(off[:, None], z, (-p).astype(F32)),
                "A": np.where(off, F32(1.0e30), ((S * (64.0 / 16777216.0)) * m.A).astype(F32)), "off": off}


def _dn_nv(A, f):
    dn = fma32(A[:, 0], f["d"][:, 0], fma32(A[:, 1], f["d"][:, 1], mul32(A[:, 2], f["d"][:, 2])))
    nv = fma32(A[:, 0], f["np"][:, 0], fma32(A[:, 1], f["np"][:, 1], fma32(A[:, 2], f["np"][:, 2], A[:, 3])))
    return dn, nv


def tri_filter_sxy(A, B, f):
    """tri_filter_sign's two values: the record is a candidate <=> neither has its sign bit set"""
    dn, nv = _dn_nv(A, f)
    adn, anv = np.abs(dn), np.abs(nv)
    ax, ay = sub32(-f["np"][:, 0], B[:, 0]), sub32(-f["np"][:, 1], B[:, 1])
    ex = fma32(ax, adn, mul32(f["d"][:, 0], anv))
    ey = fma32(ay, adn, mul32(f["d"][:, 1], anv))
    sx = sub32(fma32(B[:, 2], adn, f["A"]), np.abs(ex))
    sy = sub32(fma32(B[:, 3], adn, f["A"]), np.abs(ey))
    return sx, sy


def tri_filter_pass(A, B, f):
    sx, sy = tri_filter_sxy(A, B, f)
    return ~(np.signbit(sx) | np.signbit(sy))


def tri_bounds(A, g0, g1, f, m=SHIPPED):
    """-> (tlo, thi): tlo +inf = certainly no hit, thi +inf = not certain"""
    u = F32(U)
    one4 = F32(1.0 + 4.0 * U)
    with np.errstate(all="ignore"):
        S = mul32(mul32(f["A"], F32(262144.0)), one4)
        dn, nv = _dn_nv(A, f)
        N, D = np.abs(nv), np.abs(dn)
        e_nv = mul32(mul32(F32(16.0 * U), S), F32(m.e_nv))
        e_dn = F32(8.0 * U * m.e_dn)
        tlo = mul32(div32(np.maximum(sub32(N, e_nv), F32(0.0)), add32(D, e_dn)), F32(1.0 - 4.0 * U))
        deep = (D > F32(4.0) * e_dn) & (tlo > 0)
        th = mul32(div32(add32(N, e_nv), sub32(D, e_dn)), one4)
        cm = add32(mul32(F32(2.0 * U), np.abs(g1[:, 2])), F32(2.0) * e_dn)
        gd = sub32(g1[:, 2], dn)
        cull_ok, culled = gd > cm, gd < -cm
        tm = mul32(F32(0.5), add32(tlo, th))
        ht = add32(mul32(mul32(F32(0.5), sub32(th, tlo)), one4), mul32(u, th))
        pl = g1[:, 3]
        du = np.where(pl == 2.0, f["d"][:, 1], f["d"][:, 0]); pu = np.where(pl == 2.0, f["np"][:, 1], f["np"][:, 0])
        dv = np.where(pl == 0.0, f["d"][:, 1], f["d"][:, 2]); pv = np.where(pl == 0.0, f["np"][:, 1], f["np"][:, 2])
        qx, qy = fma32(du, tm, -pu), fma32(dv, tm, -pv)
        eq0 = add32(mul32(F32(6.0 * U), add32(S, th)), mul32(F32(2.0 * U), S))
        ewx, ewy = fma32(np.abs(du), ht, eq0), fma32(np.abs(dv), ht, eq0)
        wx, wy = sub32(qx, g0[:, 0]), sub32(qy, g0[:, 1])
        a = fma32(g0[:, 2], wx, mul32(g0[:, 3], wy))
        b = fma32(g1[:, 0], wx, mul32(g1[:, 1], wy))

        def err(m0, m1):
            lead = mul32(add32(mul32(np.abs(m0), ewx), mul32(np.abs(m1), ewy)), one4)
            return mul32(add32(lead, mul32(F32(4.0 * U), add32(np.abs(mul32(m0, wx)), np.abs(mul32(m1, wy))))), F32(m.e_ab))
        ea, eb = err(g0[:, 2], g0[:, 3]), err(g1[:, 0], g1[:, 1])
        four_u = F32(4.0 * U)
        inside = (sub32(a, ea) >= 0) & (sub32(b, eb) >= 0) & (add32(add32(add32(add32(a, b), ea), eb), four_u) <= 1)
        outside = (add32(a, ea) < 0) | (add32(b, eb) < 0) | (sub32(sub32(sub32(add32(a, b), ea), eb), four_u) > 1)
        thi = np.where(deep & cull_ok & inside & (th < INF32), th, INF32).astype(F32)
        tlo = np.where(deep & (outside | culled), INF32, tlo).astype(F32)
    return tlo, thi, {"dn": dn, "nv": nv, "a": a, "b": b, "ea": ea, "eb": eb, "S": S, "th": th}


# ---- the builder's boxes and records (rtx_bvh.h, rtx_pack.hip pack_scene), restated ---------------------------------------------------------------
def _tri_rows(v):
    """make_triangle's pivots (triangle.rs:60-71, 81-87): (i, j) the rows Triangle::contains solves in, or None (degenerate)"""
    r, s = v[1] - v[0], v[2] - v[0]
    ax, ay, idx = list(r), list(s), [0, 1, 2]

    def swap(a, b):
        ax[a], ax[b] = ax[b], ax[a]; ay[a], ay[b] = ay[b], ay[a]; idx[a], idx[b] = idx[b], idx[a]
    if ax[0] == 0.0:
        if ax[1] == 0.0:
            if ax[2] == 0.0:
                return None
            swap(2, 0)
        else:
            swap(0, 1)
    l1y = ay[0] / ax[0]
    l2y, l3y = ay[1] - l1y * ax[1], ay[2] - l1y * ax[2]
    jrow = 1
    if l2y == 0.0:
        if l3y == 0.0:
            return None
        jrow = 2
    return idx[0], idx[jrow]


def tri_record(vabs, centre):
    """One triangle as the upload and a deform write it (pack_scene's expressions in pack_scene's order; the ONE text pack() and
    deform() share): vabs (3, 3) the vertices, centre (3,) the point the f32 records are offsets from -- the pack's own, or the KEPT
    one.  -> None when the triangle is not QUALIFIED (no record in the model), else (f, rec (16,) f32 = A, B, g0, g1 -- B pass-all,
    or the grown rectangle for f = 2 --, blo, bhi (3,) f64: the footprint with its relative padding, -inf / +inf along f, BEFORE
    abs_pad and the outward rounding, reach = the largest |v - centre| component)"""
    rows = _tri_rows(vabs)
    if rows is None:
        return None
    r_, s_ = vabs[1] - vabs[0], vabs[2] - vabs[0]
    cr = np.array([r_[1] * s_[2] - r_[2] * s_[1], r_[2] * s_[0] - r_[0] * s_[2], r_[0] * s_[1] - r_[1] * s_[0]])
    nrm = cr / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
    kabs = (nrm[0] * vabs[0, 0] + nrm[1] * vabs[0, 1]) + nrm[2] * vabs[0, 2]
    if not (np.isfinite(kabs) and np.isfinite(nrm).all()) or kabs < -(1.0 + 1e-9):
        return None
    v = vabs - centre
    fa = 3 - rows[0] - rows[1]
    a0, a1 = (1 if fa == 0 else 0), (1 if fa == 2 else 2)
    r0, r1, s0, s1 = v[1, a0] - v[0, a0], v[1, a1] - v[0, a1], v[2, a0] - v[0, a0], v[2, a1] - v[0, a1]
    det = r0 * s1 - r1 * s0
    if not (np.isfinite(vabs).all() and rows[0] != rows[1] and abs(det) > 1e-6 * np.hypot(r0, r1) * np.hypot(s0, s1)):
        return None
    blo, bhi = np.full(3, np.nan), np.full(3, np.nan)
    for a in range(3):
        if a == fa:
            blo[a], bhi[a] = -np.inf, np.inf
            continue
        l, h = vabs[:, a].min(), vabs[:, a].max()
        pad = max(abs(l), abs(h)) * (1.0 / 1048576.0) + 1e-300
        blo[a], bhi[a] = l - pad, h + pad
    rec = np.zeros(16, dtype=F32)
    kc = (nrm[0] * v[0, 0] + nrm[1] * v[0, 1]) + nrm[2] * v[0, 2]
    rec[0:4] = np.array([nrm[0], nrm[1], nrm[2], kc]).astype(F32)
    rec[4:8] = np.array([0.0, 0.0, 1.0e30, 1.0e30]).astype(F32)
    rec[8:12] = np.array([v[0, a0], v[0, a1], s1 / det, -s0 / det]).astype(F32)
    rec[12:16] = np.array([-r1 / det, r0 / det, kabs, 2 - fa]).astype(F32)
    if fa == 2:
        xl, xh, yl, yh = v[:, 0].min(), v[:, 0].max(), v[:, 1].min(), v[:, 1].max()
        grow = 1.0 + 1.0 / 1048576.0
        rec[4:6] = np.array([0.5 * (xl + xh), 0.5 * (yl + yh)]).astype(F32)
        rec[6] = ru32(0.5 * (xh - xl) * grow + 1e-30)
        rec[7] = ru32(0.5 * (yh - yl) * grow + 1e-30)
    return fa, rec, blo, bhi, float(np.abs(v).max())


def pack(objs, m=SHIPPED):
    """What the walks' bound functions read for every object of the tree: dict with centre, cmax, limit32 (origin_limit), inv_max32,
    tri_extent, in_tree (bool per object), kind, rec (n_objects, 16) f32 -- a sphere's {c - centre, r} or a triangle's A, B, g0, g1 --,
    lo / hi (n_objects, 3) f32: the object's own padded box (a triangle: unbounded along its free axis), free (the free axis, -1: a
    sphere).  With np.float64 operations in the builder's order."""
    kind = np.asarray(objs["kind"]).astype(int)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    n = len(kind)
    with np.errstate(all="ignore"):
        pts = [geom[k, :3].reshape(1, 3) if kind[k] == 0 else geom[k, :9].reshape(3, 3) for k in range(n) if kind[k] in (0, 2)]
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for p in pts:
            for c in range(3):
                fin = p[:, c][np.isfinite(p[:, c])]
                if len(fin):
                    lo[c], hi[c] = min(lo[c], fin.min()), max(hi[c], fin.max())
        centre = np.where(lo <= hi, 0.5 * (lo + hi), 0.0)
        sph = [k for k in range(n) if kind[k] == 0]
        cmax = 0.0
        for k in sph:
            c = geom[k, :3] - centre
            reach = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + abs(geom[k, 3])
            if not reach <= cmax:
                cmax = reach
        blo, bhi = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
        free = np.full(n, -1)
        in_tree = np.zeros(n, dtype=bool)
        rec = np.zeros((n, 16), dtype=F32)
        sph_ok = len(sph) > 4 and all(np.isfinite(geom[k, :4]).all() for k in sph)
        for k in sph:
            s, r = geom[k, :3], abs(geom[k, 3])
            pad = (np.abs(s) + r) * (1.0 / 1048576.0) + 1e-300
            blo[k], bhi[k] = s - r - pad, s + r + pad
            in_tree[k] = sph_ok
            rec[k, :3] = (s - centre).astype(F32)
            rec[k, 3] = ru32(r)
        tri_extent = 0.0
        classes = {0: [], 1: [], 2: []}
        for k in range(n):
            if kind[k] != 2:
                continue
            t = tri_record(geom[k, :9].reshape(3, 3), centre)
            if t is None:
                continue
            fa, rec[k], blo[k], bhi[k], reach = t
            tri_extent = max(tri_extent, reach)
            free[k] = fa
            classes[fa].append(k)
        for fa, ks in classes.items():
            for k in ks:
                in_tree[k] = len(ks) > 4
        used = in_tree
        fin = np.concatenate([blo[used].ravel(), bhi[used].ravel()]) if used.any() else np.zeros(0)
        fin = fin[np.isfinite(fin)]
        scale = float(np.abs(fin).max()) if len(fin) else 0.0
        limit = 4.0 * scale + 1.0
        abs_pad = limit * (1.0 / 4194304.0)
        lo32, hi32 = rd32(blo - abs_pad * m.abs_pad), ru32(bhi + abs_pad * m.abs_pad)
    return {"centre": centre, "cmax": cmax, "limit32": F32(limit), "limit": limit, "abs_pad": abs_pad,
            "inv_max32": F32(min(1.0e30, 1.0e37 / max(limit, 1.0))), "tri_extent": tri_extent, "in_tree": in_tree, "kind": kind,
            "rec": rec, "lo": lo32, "hi": hi32, "free": free}


def q3_node(lo, hi, abs_pad, m=SHIPPED):
    """build_q3nodes for ONE node whose children are the f32 boxes lo, hi (c, 3): (o, s) f32 (3,), qlo, qhi (c, 3) ints, or None when
    the node has no 64-byte form"""
    pad = abs_pad * m.abs_pad2
    l, h = _d(lo) - pad, _d(hi) + pad
    nlo, nhi = l.min(axis=0), h.max(axis=0)
    o, sc = np.zeros(3), np.ones(3)
    for a in range(3):
        ext = nhi[a] - nlo[a]
        sc[a] = np.exp2(np.ceil(np.log2(ext / 254.0))) if ext > 0 else 1.0
        if not (1.1754944e-38 <= sc[a] <= 1.0e30):
            return None
        o[a] = np.floor(nlo[a] / sc[a]) * sc[a]
        while (nhi[a] - o[a]) / sc[a] > 255.0:
            sc[a] *= 2.0
            o[a] = np.floor(nlo[a] / sc[a]) * sc[a]
        if not abs(o[a] / sc[a]) + 256.0 < 16777216.0 or float(F32(o[a])) != o[a]:
            return None
    ql, qh = np.floor((l - o) / sc), np.ceil((h - o) / sc)
    if (ql < 0).any() or (qh > 255).any() or (ql > qh).any():
        return None
    return o.astype(F32), sc.astype(F32), ql.astype(np.int64), qh.astype(np.int64)


def q_node(r4):
    """build_qnodes for ONE footprint node whose children are the f32 rectangles r4 (c, 4): (o, s) f32 (2,), qx, qy (c,) words"""
    r4 = _d(r4)
    lo, hi = r4[:, 0:2].min(axis=0), r4[:, 2:4].max(axis=0)
    sc = np.ones(2)
    for a in range(2):
        ext = hi[a] - lo[a]
        sc[a] = np.exp2(np.ceil(np.log2(ext / 65535.0))) if ext > 0 else 1.0
        while ext / sc[a] > 65535.0:
            sc[a] *= 2.0
    l = np.floor((r4[:, 0:2] - lo) / sc).astype(np.int64)
    h = np.ceil((r4[:, 2:4] - lo) / sc).astype(np.int64)
    if (l < 0).any() or (h > 65535).any():
        return None
    return lo.astype(F32), sc.astype(F32), l[:, 0] | (h[:, 0] << 16), l[:, 1] | (h[:, 1] << 16)


# ---- the LDS sweep's sphere filter (rtx_device.h filter_from_ray / filter_disc1, rtx_kernels.hip filter_disc2) ---------------------------
def sweep_cmax(objs, centre, hidden=None):
    """pack_scene's sphere_cmax against `centre`: max of |c - centre| + |r| in scene order, a NaN reach propagating (`!(reach <=
    cmax)`); a hidden sphere's reach is 0 (hide_record)"""
    geom = np.asarray(objs["geom"], dtype=np.float64)
    cmax = 0.0
    with np.errstate(all="ignore"):
        for k in np.nonzero(np.asarray(objs["kind"]).astype(int) == 0)[0]:
            c = geom[k, :3] - _d(centre)
            reach = 0.0 if hidden is not None and hidden[k] else np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + abs(geom[k, 3])
            if not reach <= cmax:
                cmax = reach
    return float(cmax)


def sweep_record(objs, centre, hidden=None):
    """The sphere_f32 record of every sphere in scene order, UN-interleaved: (ns4, 4) f32 rows {c - centre, f32(|c - centre|^2 - r^2)},
    ns4 = the sphere count rounded up to a multiple of 4.  f64 in pack_scene's operation order (cc = (cx cx + cy cy) + cz cz, rr = r r,
    each value rounded once to f32).  Rows behind the last sphere and the rows of hidden spheres (`hidden`: a bool per object) are the
    sentinel (0, 0, 0, 1e30); a pack whose cmax is not below 1e14 holds (0, 0, 0, -1e30) in EVERY row.  The device holds rows 2k and
    2k + 1 as the pair {x0, x1, y0, y1} {z0, z1, w0, w1}."""
    kind = np.asarray(objs["kind"]).astype(int)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    sph = np.nonzero(kind == 0)[0]
    ns4 = (len(sph) + 3) & ~3
    rec = np.zeros((ns4, 4), dtype=F32)
    rec[:, 3] = F32(1.0e30)
    if not sweep_cmax(objs, centre, hidden) < 1.0e14:
        rec[:, 3] = F32(-1.0e30)
        return rec
    with np.errstate(all="ignore"):
        c = geom[sph, :3] - _d(centre)[None, :]
        cc = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        rows = np.concatenate([c, (cc - geom[sph, 3] * geom[sph, 3])[:, None]], axis=1).astype(F32)
    keep = np.ones(len(sph), dtype=bool) if hidden is None else ~np.asarray(hidden, dtype=bool)[sph]
    rec[:len(sph)][keep] = rows[keep]
    return rec


def sweep_params(pos, dirs, centre, cmax, m=SHIPPED):
    """filter_from_ray: -> (words (n, 8) f32 = {d.xyz, -p.d, 2p.xyz, E - p.p}, pass_all (n,) bool, M (n,) f64).  All in f64 in the
    function's order, one rounding to f32 each; E = 64uM^2 times m.E.  pass_all = !(M < 1e14) || !(M > 1e-12), M = cmax + |p| -- true
    for a NaN origin and a NaN cmax too --: the words are then (0, ..., 0, 1e30)."""
    pos, dirs = _d(pos), _d(dirs)
    with np.errstate(all="ignore"):
        p = pos - _d(centre)[None, :]
        pp = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        pd = (p[:, 0] * dirs[:, 0] + p[:, 1] * dirs[:, 1]) + p[:, 2] * dirs[:, 2]
        M = cmax + np.sqrt(pp)
        off = ~(M < 1.0e14) | ~(M > 1.0e-12)
        E = (M * M * (64.0 / 16777216.0)) * m.E
        w = np.concatenate([dirs, (-pd)[:, None], 2.0 * p, (E - pp)[:, None]], axis=1).astype(F32)
    w = np.where(off[:, None], F32(0.0), w)
    w[:, 7] = np.where(off, F32(1.0e30), w[:, 7])
    return w.astype(F32), off, M


def sweep_disc(rec, f):
    """D of one record per ray, rec (n, 4) f32 and f (n, 8) the FilterParams words, in the kernel's fma order:
        b = fma(x, dx, fma(y, dy, fma(z, dz, npd)));  q = fma(x, p2x, fma(y, p2y, fma(z, p2z, nppE)));  D = fma(b, b, q - w).
    filter_disc1 and filter_disc2 nest their fmas the SAME way (z innermost, then y, then x; q - w one rounded subtraction), so one
    function stands for both; the device returns both values and the gpu part holds each to this one.  The record is a candidate <=>
    D's sign bit is clear."""
    b = fma32(rec[:, 0], f[:, 0], fma32(rec[:, 1], f[:, 1], fma32(rec[:, 2], f[:, 2], f[:, 3])))
    q = fma32(rec[:, 0], f[:, 4], fma32(rec[:, 1], f[:, 5], fma32(rec[:, 2], f[:, 6], f[:, 7])))
    return fma32(b, b, sub32(q, rec[:, 3]))


# ---- one case through the model ------------------------------------------------------------------------------------------------------------
def own_steps(pk, target, node_form, m=SHIPPED):
    """The tightest path the builder can give an object: ONE node visit whose child is the object's own padded box (a leaf of one
    record).  node_form 0: the 128-byte child (a footprint rectangle for an (x, y) triangle); 2: the 64-byte forms, the node's grid
    spanned by the object's box and the box of the next object of its kind (build_q3nodes / build_qnodes on those two children;
    m.abs_pad2 is the factor on build_q3nodes' second padding).
    -> a list with one step (layout, arrays), or None where the form does not exist for the scene."""
    lo, hi, free = pk["lo"][target], pk["hi"][target], pk["free"][target]
    flat = (pk["free"][pk["in_tree"]] == 2).all()          # a pure (x, y)-footprint tree: every node is a footprint node
    if node_form == 0:
        return [("mixed", lo, hi, (free == 2))]
    ids = np.nonzero(pk["in_tree"])[0]
    if (pk["kind"][ids] == 0).all():
        o = np.zeros((len(target), 3), dtype=F32); s = np.ones((len(target), 3), dtype=F32)
        ql = np.zeros((len(target), 3), dtype=np.int64); qh = np.zeros((len(target), 3), dtype=np.int64)
        ok = np.zeros(len(target), dtype=bool)
        cache = {}
        for i, j in enumerate(target):
            if j not in cache:
                nb = ids[(np.nonzero(ids == j)[0][0] + 1) % len(ids)]
                cache[j] = q3_node(pk["lo128"][[j, nb]], pk["hi128"][[j, nb]], pk["abs_pad"], m)
            g = cache[j]
            if g is not None:
                o[i], s[i], ql[i], qh[i], ok[i] = g[0], g[1], g[2][0], g[3][0], True
        return [("q3", o, s, ql, qh, ok)]
    if flat:
        o = np.zeros((len(target), 2), dtype=F32); s = np.ones((len(target), 2), dtype=F32)
        qx = np.zeros(len(target), dtype=np.int64); qy = np.zeros(len(target), dtype=np.int64)
        ok = np.zeros(len(target), dtype=bool)
        cache = {}
        for i, j in enumerate(target):
            if j not in cache:
                nb = ids[(np.nonzero(ids == j)[0][0] + 1) % len(ids)]
                r4 = np.stack([np.concatenate([pk["lo"][k][:2], pk["hi"][k][:2]]) for k in (j, nb)])
                cache[j] = q_node(r4)
            g = cache[j]
            if g is not None:
                o[i], s[i], qx[i], qy[i], ok[i] = g[0], g[1], g[2][0], g[3][0], True
        return [("qrect", o, s, qx, qy, ok)]
    return None


def pack_for(objs, m=SHIPPED):
    """pack() with the margins m; lo128 / hi128 are the boxes the 64-byte sphere nodes are built FROM (always with the shipped first
    abs_pad baked in by m.abs_pad, as build_q3nodes reads the 128-byte nodes)"""
    pk = pack(objs, m)
    pk["lo128"], pk["hi128"] = pk["lo"], pk["hi"]
    return pk


def _updated(base_objs, indices, new, m):
    """(the base pack, the updated list: entries in order, the last entry of a repeated index wins)"""
    pk = pack_for(base_objs, m)
    now = np.array(base_objs, copy=True)
    for i, o in zip(np.asarray(indices).astype(np.int64), new):
        now[int(i)] = o
    assert np.array_equal(np.asarray(now["kind"]).astype(int), pk["kind"]), "an update in place keeps every object's kind"
    return pk, now


def _refit_spheres(pk, now, m):
    """refit()'s and deform()'s common part: the base pack with every sphere of the updated list written against the KEPT centre"""
    geom = np.asarray(now["geom"], dtype=np.float64)
    sph = pk["kind"] == 0
    out = dict(pk)
    rec, lo, hi = pk["rec"].copy(), pk["lo"].copy(), pk["hi"].copy()
    with np.errstate(all="ignore"):
        s, r = geom[sph, :3], np.abs(geom[sph, 3])
        c = s - pk["centre"][None, :]
        cc = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        reach = np.sqrt(cc) + r
        rec[sph, :3] = c.astype(F32)
        rec[sph, 3] = ru32(r)
        fw = np.zeros(len(now), dtype=F32)
        fw[sph] = (cc - r * r).astype(F32)
        filt = np.zeros((len(now), 4), dtype=F32)
        filt[sph, :3] = c.astype(F32)
        filt[sph, 3] = fw[sph]
        pad = (np.abs(s) + r[:, None]) * (1.0 / 1048576.0) + 1e-300
        lo[sph] = rd32(((s - r[:, None]) - pad) - pk["abs_pad"] * m.abs_pad)
        hi[sph] = ru32(((s + r[:, None]) + pad) + pk["abs_pad"] * m.abs_pad)
    out.update(rec=rec, lo=lo, hi=hi, lo128=lo, hi128=hi, fw=fw, filt=filt, cmax=float(reach.max()) if sph.any() else 0.0, objs=now)
    out["sweep"] = sweep_record(now, pk["centre"])          # the sweep's records of the updated list against the KEPT centre
    return out


def refit(base_objs, indices, new, m=SHIPPED):
    """What rtx_scene_update_objects' REFIT of the tree of `base_objs` by objects[indices[i]] = new[i] (in order: the last entry of a
    repeated index wins) must leave when NO TRIANGLE GETS NEW VERTICES (the REFIT of RTX_UPDATE_AUTO; a triangle that moves under
    RTX_UPDATE_DEFORM is deform()'s), from its contract (include/rtx_hip.h) and not from the kernel's text: a dict as
    pack_for() returns it.  KEPT from the base pack: centre, limit32 / limit (origin_limit), abs_pad, inv_max32, in_tree, kind, free
    and -- because no triangle moves -- tri_extent and every triangle's record and box.  NEW, for every sphere of the updated list
    against the KEPT centre: rec[:, :3] = f32(c - centre), rec[:, 3] = |r| rounded up (the leaf record), fw = f32(|c - centre|^2 -
    r^2) (the filter record's fourth scalar; `filt` is the whole filter record {f32(c - centre), fw}), lo / hi = sphere_box() widened
    by the base abs_pad and rounded outward, and scene-wide cmax = max(sqrt(cc) + |r|).  `sweep`: sweep_record() of the updated list
    against the kept centre, the LDS sweep's records with their padding (deform() yields it too, next to its tri_extent).
    A sphere the update does not name keeps the bits pack() gave it (the expressions are pack()'s).  numpy f64, one rounding per
    operation, sums left to right."""
    pk, now = _updated(base_objs, indices, new, m)
    tri = pk["kind"] == 2
    assert np.asarray(now["geom"])[tri].tobytes() == np.asarray(base_objs["geom"])[tri].tobytes(), "a triangle with new vertices: deform()"
    return _refit_spheres(pk, now, m)


def deform(base_objs, indices, new, m=SHIPPED):
    """What a REFIT under RTX_UPDATE_DEFORM must leave (DESIGN.md 3.13 "Moving triangles", include/rtx_hip.h "Triangles"; not from the
    kernel's text): a dict as pack_for() returns it.  KEPT from the base pack: centre, limit32 / limit, abs_pad, inv_max32, in_tree,
    kind, free.  NEW, for every QUALIFIED triangle the update names, tri_record() against the KEPT centre -- pack()'s expressions in
    pack()'s order, v = vabs - kept centre: rec[:, 0:16] = A, B (pass-all, or the grown rectangle for f = 2), g0, g1; lo / hi = the
    footprint with its relative padding, widened by the BASE abs_pad, rounded outward, -inf / +inf along f.  Scene-wide: tri_extent =
    the largest |v| component over ALL qualified triangles of the updated list against the kept centre.  The spheres named in the same
    call get what refit() gives them (cmax included).  A triangle the update does not name keeps pack()'s bits.
    The premise -- class and free axis of every triangle are the resident ones, or the library rebuilds -- is asserted."""
    pk, now = _updated(base_objs, indices, new, m)
    out = _refit_spheres(pk, now, m)
    named = {int(i) for i in np.asarray(indices).astype(np.int64)}
    geom = np.asarray(now["geom"], dtype=np.float64)
    rec, lo, hi = out["rec"], out["lo"].copy(), out["hi"].copy()
    tri_extent = 0.0
    with np.errstate(all="ignore"):
        for k in np.nonzero(pk["kind"] == 2)[0]:
            t = tri_record(geom[k, :9].reshape(3, 3), pk["centre"])
            assert (-1 if t is None else t[0]) == pk["free"][k], "triangle %d: class / free axis %s is not the resident %d" % (k, t and t[0], pk["free"][k])
            if t is None:
                continue
            tri_extent = max(tri_extent, t[4])
            if k in named:
                rec[k] = t[1]
                lo[k], hi[k] = rd32(t[2] - pk["abs_pad"] * m.abs_pad), ru32(t[3] + pk["abs_pad"] * m.abs_pad)
    out.update(rec=rec, lo=lo, hi=hi, lo128=lo, hi128=hi, tri_extent=tri_extent)
    return out


def device_steps(path, lens):
    """the hook's path_data (n, steps, 16) uint32 -> steps as own_steps lists them; `lens` (n,): steps beyond a row's length are
    entered by definition"""
    out = []
    for k in range(path.shape[1]):
        w = np.ascontiguousarray(path[:, k, :])
        f = w.view(F32)
        live = k < lens
        lay = w[:, 0]
        if (lay[live] == 2).all() and live.any():
            out.append(("q3", f[:, 1:4], f[:, 4:7], w[:, 7:10].astype(np.int64), w[:, 10:13].astype(np.int64), live))
        elif (lay[live] == 3).all() and live.any():
            out.append(("qrect", f[:, 1:3], f[:, 3:5], w[:, 5].astype(np.int64), w[:, 6].astype(np.int64), live))
        elif live.any():
            flat = lay == 1
            lo = np.where(flat[:, None], np.stack([f[:, 1], f[:, 2], np.full(len(f), -INF32)], axis=1), f[:, 1:4])
            hi = np.where(flat[:, None], np.stack([f[:, 3], f[:, 4], np.full(len(f), INF32)], axis=1), f[:, 4:7])
            out.append(("mixed", lo.astype(F32), hi.astype(F32), flat, live))
    return out


def walk_steps(steps, q, best_up, m=SHIPPED):
    """-> (entered_all (n,), bound (n,) f32: the largest entry distance returned, -inf where the form returns none).  A step's last
    array says for which rows the step exists (own_steps: for which the one-node form exists); other rows pass it."""
    n = len(q["e"])
    entered = np.ones(n, dtype=bool)
    bound = np.full(n, -INF32, dtype=F32)
    for st in steps:
        if st[0] == "mixed":
            lo, hi, flat = st[1], st[2], st[3]
            live = st[4] if len(st) > 4 else np.ones(n, dtype=bool)
            t3 = box_entry32(lo, hi, q, best_up, m)
            t2 = rect_entry32(np.concatenate([lo[:, :2], hi[:, :2]], axis=1), q, best_up, m)
            tc = np.where(flat, t2, t3)
        elif st[0] == "q3":
            live = st[5]
            ent, _ = q3_entry(st[1], st[2], st[3], st[4], q, best_up, m)
            tc = np.where(ent, -INF32, INF32)
        else:
            live = st[5]
            tc = qrect_entry(st[1], st[2], st[3], st[4], q, best_up, m)
        with np.errstate(all="ignore"):
            ok = tc < INF32
            entered &= ok | ~live
            bound = np.where(live & ok, np.maximum(bound, tc), bound).astype(F32)
    return entered, bound


def leaf_bounds(kind, rec, o, d, centre, cmax, tri_extent, best_up, m=SHIPPED):
    """-> dict of (n,) arrays: cand (the end of the sqrt interval that hurts), tlo_hi / tlo_lo, certain_any / certain_all, thi_lo / thi_hi"""
    n = len(o)
    sph = sphere_leaf(rec[:, :4], sphere_ray(o, d, centre, cmax, m), best_up)
    f = tri_params(o, d, centre, tri_extent, m)
    ok = tri_filter_pass(rec[:, 0:4], rec[:, 4:8], f)
    tlo, thi, dbg = tri_bounds(rec[:, 0:4], rec[:, 8:12], rec[:, 12:16], f, m)
    off = f["off"]                                          # the pass-all filter: A = 1e30, S = inf -- every bound is then vacuous
    with np.errstate(all="ignore"):
        bu = np.broadcast_to(np.asarray(best_up, dtype=F32), (n,))
        tcand = ok & (tlo <= bu) & (tlo < INF32)
    tri = kind == 2
    pick = lambda a, b: np.where(tri, b, a)
    return {"cand": pick(sph["cand0"], tcand), "cand_best": pick(sph["cand1"], tcand),
            "tlo_hi": pick(sph["tlo"][1], tlo).astype(F32), "tlo_lo": pick(sph["tlo"][0], tlo).astype(F32),
            "certain_any": pick(sph["certain_any"], ok & (tlo < INF32) & (thi < INF32)),
            "certain_all": pick(sph["certain_all"], ok & (tlo < INF32) & (thi < INF32)),
            "thi_lo": pick(sph["thi"][0], thi).astype(F32), "thi_hi": pick(sph["thi"][1], thi).astype(F32), "tri_off": off}


def round_up32(t):
    return ru32(t)


def check(t, reported, entered, bound, leaf, active):
    """section 2's properties on the pairs `active` (walked, in the tree, the form exists).  -> {name: (n,) bool, True = VIOLATED}.
    f32 bounds are compared with the f64 distance exactly (both are f64 values)."""
    rep, un = active & reported, active & ~reported
    with np.errstate(all="ignore"):
        t = _d(t)
        return {"path not entered": rep & ~entered,
                "entry bound above t": rep & (_d(bound) > t),
                "not a candidate": rep & ~leaf["cand"],
                "t_lo above t": rep & leaf["cand"] & (_d(leaf["tlo_hi"]) > t),
                "t_hi below t": rep & leaf["certain_any"] & (t > _d(leaf["thi_lo"])),
                "certain but unreported": un & leaf["certain_any"]}
