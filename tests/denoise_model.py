"""The denoiser of include/rtx_hip.h ("Denoising", the comment above RtxDenoiseParams) in plain numpy, written from that text: every
operation one rounded f64 operation in the header's order, accumulation written out left to right (never np.sum).  Two readings:

  denoise(...)         whole-array arithmetic on shifted slices: a tap (dx, dy) of a pass is one slice of centres and one of neighbours
  denoise_scalar(...)  one pixel at a time over Python floats, the loops as the header writes them

Both return (out, var_out) -- var_out None without a variance.  Neither shares code with the other beyond the parameter record, and
neither runs anything of the library.  tests/test_denoise.py holds them to each other bit for bit; tests/test_denoise_gpu.py holds the
device to the array reading.
"""
import math

import numpy as np

NO_NORMAL = 0xFFFFFFFF
DEMODULATE = 1
B3 = (0.0625, 0.25, 0.375, 0.25, 0.0625)
INF = float("inf")


class Params:
    """RtxDenoiseParams; the defaults here are only this file's (the library's come from rtx_denoise_default_params)"""

    def __init__(self, passes=1, flags=DEMODULATE, normal_power_log2=5, sigma_color=4.0, sigma_depth=0.05, sigma_albedo=0.1,
                 epsilon=1e-10, albedo_min=1e-3):
        self.passes, self.flags, self.normal_power_log2 = int(passes), int(flags), int(normal_power_log2)
        self.sigma_color, self.sigma_depth, self.sigma_albedo = float(sigma_color), float(sigma_depth), float(sigma_albedo)
        self.epsilon, self.albedo_min = float(epsilon), float(albedo_min)

    def replace(self, **kw):
        p = Params(**self.__dict__)
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, type(getattr(p, k))(v))
        return p


# ---- the array reading ----------------------------------------------------------------------------------------------------------
def _finite3(u):
    return np.isfinite(u[..., 0]) & np.isfinite(u[..., 1]) & np.isfinite(u[..., 2])


def _window(n, shift):
    """centres c in [0, n) whose neighbour c + shift lies in [0, n): (slice of centres, slice of neighbours), or None"""
    lo, hi = max(0, -shift), min(n, n - shift)
    if lo >= hi:
        return None
    return slice(lo, hi), slice(lo + shift, hi + shift)


def _prepare(rgb, var, albedo, emission, p):
    if p.flags & DEMODULATE:
        div = albedo > p.albedo_min
        t = rgb - emission
        u = np.where(div, t / np.where(div, albedo, 1.0), t)
        v = None if var is None else np.where(div, var / np.where(div, albedo * albedo, 1.0), var)
    else:
        u, v = rgb.copy(), (None if var is None else var.copy())
    return u, v


def _pass(u, v, normal, depth, albedo, s, p):
    h_, w_ = depth.shape
    has_var = v is not None
    color = has_var and not math.isinf(p.sigma_color)
    fin_p = _finite3(u)
    if color:
        nv = (v[..., 0] + v[..., 1]) + v[..., 2]
        g, gw = np.zeros((h_, w_)), np.zeros((h_, w_))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                wy, wx = _window(h_, dy), _window(w_, dx)
                if wy is None or wx is None:
                    continue
                m = float((2 if dx == 0 else 1) * (2 if dy == 0 else 1))
                g[wy[0], wx[0]] = g[wy[0], wx[0]] + m * nv[wy[1], wx[1]]
                gw[wy[0], wx[0]] = gw[wy[0], wx[0]] + m
        cden = (p.sigma_color * p.sigma_color) * (g / gw) + p.epsilon
    sc, sw = np.zeros((h_, w_, 3)), np.zeros((h_, w_))
    sv = np.zeros((h_, w_, 3)) if has_var else None
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            wy, wx = _window(h_, dy * s), _window(w_, dx * s)
            if wy is None or wx is None:
                continue
            P, Q = (wy[0], wx[0]), (wy[1], wx[1])
            hh = B3[dx + 2] * B3[dy + 2]
            uq = u[Q]
            if dx == 0 and dy == 0:
                w = np.full(uq.shape[:2], hh)
                keep = np.ones(uq.shape[:2], dtype=bool)
            else:
                shape = uq.shape[:2]
                wn = wz = wa = wc = np.ones(shape)
                if p.normal_power_log2 != NO_NORMAL:
                    a, b = normal[P], normal[Q]
                    t = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
                    t = np.where(t > 0.0, t, 0.0)
                    for _ in range(p.normal_power_log2):
                        t = t * t
                    wn = t
                if not math.isinf(p.sigma_depth):
                    zp, zq = depth[P], depth[Q]
                    fp, fq = np.isfinite(zp), np.isfinite(zq)
                    r = (zp - zq) / (p.sigma_depth * (zp + zq))
                    wz = np.where(fp & fq, 1.0 / (1.0 + r * r), np.where(fp == fq, 1.0, 0.0))
                if not math.isinf(p.sigma_albedo):
                    d = albedo[P] - albedo[Q]
                    da = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wa = 1.0 / (1.0 + da / (p.sigma_albedo * p.sigma_albedo))
                if color:
                    d = u[P] - uq
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wc = 1.0 / (1.0 + d2 / cden[P])
                w = (((hh * wn) * wz) * wa) * wc
                keep = w > 0.0
            keep = keep & _finite3(uq)
            sc[P] = np.where(keep[..., None], sc[P] + w[..., None] * uq, sc[P])
            sw[P] = np.where(keep, sw[P] + w, sw[P])
            if has_var:
                sv[P] = np.where(keep[..., None], sv[P] + (w * w)[..., None] * v[Q], sv[P])
    un = np.where(fin_p[..., None], sc / sw[..., None], u)
    vn = np.where(fin_p[..., None], sv / (sw * sw)[..., None], v) if has_var else None
    return un, vn


def _finish(u, v, albedo, emission, p):
    if p.flags & DEMODULATE:
        div = albedo > p.albedo_min
        return np.where(div, u * albedo + emission, u + emission), (None if v is None else np.where(div, v * (albedo * albedo), v))
    return u, v


def denoise_each(rgb, var, albedo, emission, normal, depth, p):
    """yields (passes, out, var_out) for passes = 1 .. p.passes: the first k passes of a run are the run with passes = k, so one sweep
    gives every pass count"""
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    var = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
    with np.errstate(all="ignore"):
        u, v = _prepare(rgb, var, albedo, emission, p)
        for i in range(p.passes):
            u, v = _pass(u, v, normal, depth, albedo, 1 << i, p)
            yield (i + 1,) + _finish(u, v, albedo, emission, p)


def denoise(rgb, var, albedo, emission, normal, depth, p):
    """rgb, albedo, emission, normal [h][w][3], depth [h][w], var [h][w][3] or None -> (out, var_out or None)"""
    if p.passes == 0:
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
        return rgb.copy(), (None if var is None else np.ascontiguousarray(var, dtype=np.float64).copy())
    for _, out, vout in denoise_each(rgb, var, albedo, emission, normal, depth, p):
        pass
    return out, vout


# ---- the scalar reading ---------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE a / b on Python floats (Python raises on a zero divisor)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _fin(x):
    return not (math.isinf(x) or math.isnan(x))


def denoise_scalar(rgb, var, albedo, emission, normal, depth, p):
    h_, w_ = np.asarray(depth).shape
    rgb_l, alb, emi, nor, dep = (np.asarray(a, dtype=np.float64).tolist() for a in (rgb, albedo, emission, normal, depth))
    var_l = None if var is None else np.asarray(var, dtype=np.float64).tolist()
    has_var = var_l is not None
    if p.passes == 0:
        return np.array(rgb_l, dtype=np.float64).reshape(h_, w_, 3), (np.array(var_l, dtype=np.float64).reshape(h_, w_, 3) if has_var else None)
    demod = bool(p.flags & DEMODULATE)
    u = [[[0.0] * 3 for _ in range(w_)] for _ in range(h_)]
    v = [[[0.0] * 3 for _ in range(w_)] for _ in range(h_)]
    for y in range(h_):
        for x in range(w_):
            for k in range(3):
                c, a = rgb_l[y][x][k], alb[y][x][k]
                if demod:
                    t = c - emi[y][x][k]
                    u[y][x][k] = _div(t, a) if a > p.albedo_min else t
                    if has_var:
                        v[y][x][k] = _div(var_l[y][x][k], a * a) if a > p.albedo_min else var_l[y][x][k]
                else:
                    u[y][x][k] = c
                    if has_var:
                        v[y][x][k] = var_l[y][x][k]
    color = has_var and not math.isinf(p.sigma_color)
    for i in range(p.passes):
        s = 1 << i
        nv = [[(v[y][x][0] + v[y][x][1]) + v[y][x][2] for x in range(w_)] for y in range(h_)]
        un = [[None] * w_ for _ in range(h_)]
        vn = [[None] * w_ for _ in range(h_)]
        for y in range(h_):
            for x in range(w_):
                up = u[y][x]
                if not (_fin(up[0]) and _fin(up[1]) and _fin(up[2])):
                    un[y][x], vn[y][x] = list(up), list(v[y][x])
                    continue
                cden = 0.0
                if color:
                    g = gw = 0.0
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            qx, qy = x + dx, y + dy
                            if 0 <= qx < w_ and 0 <= qy < h_:
                                m = float((2 if dx == 0 else 1) * (2 if dy == 0 else 1))
                                g = g + m * nv[qy][qx]
                                gw = gw + m
                    cden = (p.sigma_color * p.sigma_color) * _div(g, gw) + p.epsilon
                sc, sv, sw = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], 0.0
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        hh = B3[dx + 2] * B3[dy + 2]
                        qx, qy = x + s * dx, y + s * dy
                        if dx == 0 and dy == 0:
                            w = hh
                        else:
                            if not (0 <= qx < w_ and 0 <= qy < h_):
                                continue
                            wn = wz = wa = wc = 1.0
                            if p.normal_power_log2 != NO_NORMAL:
                                a, b = nor[y][x], nor[qy][qx]
                                t = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
                                t = t if t > 0.0 else 0.0
                                for _ in range(p.normal_power_log2):
                                    t = t * t
                                wn = t
                            if not math.isinf(p.sigma_depth):
                                zp, zq = dep[y][x], dep[qy][qx]
                                if _fin(zp) and _fin(zq):
                                    r = _div(zp - zq, p.sigma_depth * (zp + zq))
                                    wz = _div(1.0, 1.0 + r * r)
                                else:
                                    wz = 1.0 if _fin(zp) == _fin(zq) else 0.0
                            if not math.isinf(p.sigma_albedo):
                                d = [alb[y][x][k] - alb[qy][qx][k] for k in range(3)]
                                da = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                                wa = _div(1.0, 1.0 + _div(da, p.sigma_albedo * p.sigma_albedo))
                            if color:
                                d = [up[k] - u[qy][qx][k] for k in range(3)]
                                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                                wc = _div(1.0, 1.0 + _div(d2, cden))
                            w = (((hh * wn) * wz) * wa) * wc
                            if not (w > 0.0):
                                continue
                        uq = u[qy][qx]
                        if not (_fin(uq[0]) and _fin(uq[1]) and _fin(uq[2])):
                            continue
                        for k in range(3):
                            sc[k] = sc[k] + w * uq[k]
                        sw = sw + w
                        if has_var:
                            for k in range(3):
                                sv[k] = sv[k] + (w * w) * v[qy][qx][k]
                un[y][x] = [_div(sc[k], sw) for k in range(3)]
                vn[y][x] = [_div(sv[k], sw * sw) for k in range(3)] if has_var else [0.0, 0.0, 0.0]
        u, v = un, vn
    out = np.zeros((h_, w_, 3))
    vout = np.zeros((h_, w_, 3)) if has_var else None
    for y in range(h_):
        for x in range(w_):
            for k in range(3):
                a = alb[y][x][k]
                o, vo = u[y][x][k], v[y][x][k]
                if demod:
                    if a > p.albedo_min:
                        o, vo = o * a + emi[y][x][k], vo * (a * a)
                    else:
                        o = o + emi[y][x][k]
                out[y, x, k] = o
                if has_var:
                    vout[y, x, k] = vo
    return out, vout
