"""The guided upsampler of include/rtx_hip.h ("Guided upsampling", the comment above RtxUpsampleParams) in plain numpy, written from
that text: every operation one rounded f64 operation in the header's order, the sums written out tap by tap (never np.sum).  Two
readings:

  upsample(...)         whole-array arithmetic: each of the four taps is one gather of the low frame for every output pixel at once
  upsample_scalar(...)  one output pixel at a time over Python floats, the loops as the header writes them

Both take the low frame (rgb, var or None, albedo, emission, normal, depth: dict `lo`), the output frame's guides (dict `hi`: albedo,
emission, normal, depth) and a Params, and return (out, var_out) -- var_out None without a variance.  Neither shares code with the other
beyond the parameter record, and neither runs anything of the library.  tests/test_upsample.py holds them to each other bit for bit;
tests/test_upsample_gpu.py holds the device to the array reading.
"""
import math

import numpy as np

NO_NORMAL = 0xFFFFFFFF
DEMODULATE = 1
INF = float("inf")


class Params:
    """RtxUpsampleParams; the defaults here are only this file's (the library's come from rtx_upsample_default_params)"""

    def __init__(self, factor=2, flags=DEMODULATE, normal_power_log2=0, sigma_depth=0.1, sigma_albedo=0.5, albedo_min=1e-3,
                 min_weight=0.0):
        self.factor, self.flags, self.normal_power_log2 = int(factor), int(flags), int(normal_power_log2)
        self.sigma_depth, self.sigma_albedo = float(sigma_depth), float(sigma_albedo)
        self.albedo_min, self.min_weight = float(albedo_min), float(min_weight)

    def replace(self, **kw):
        p = Params(**self.__dict__)
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, type(getattr(p, k))(v))
        return p


# ---- the array reading ----------------------------------------------------------------------------------------------------------
def tap_values(lo, p):
    """(u, v or None, usable) of every low pixel and channel"""
    rgb = np.ascontiguousarray(lo["rgb"], dtype=np.float64)
    var = None if lo.get("var") is None else np.ascontiguousarray(lo["var"], dtype=np.float64)
    with np.errstate(all="ignore"):
        if p.flags & DEMODULATE:
            div = lo["albedo"] > p.albedo_min
            t = rgb - lo["emission"]
            u = np.where(div, t / np.where(div, lo["albedo"], 1.0), t)
            v = None if var is None else np.where(div, var / np.where(div, lo["albedo"] * lo["albedo"], 1.0), var)
            usable = np.isfinite(u) & div
        else:
            u, v = rgb.copy(), (None if var is None else var.copy())
            usable = np.isfinite(u)
    return u, v, usable


def upsample(lo, hi, p, trace=None):
    """-> (out [h][w][3], var_out or None).  trace: a dict that receives, per output pixel (and channel), which arm of the text ran --
    the masks tests/upsample_cases.py checks its cases with"""
    s = p.factor
    hl, wl = np.asarray(lo["depth"]).shape
    H, W = hl * s, wl * s
    assert np.asarray(hi["depth"]).shape == (H, W)
    has_var = lo.get("var") is not None
    demod = bool(p.flags & DEMODULATE)
    with np.errstate(all="ignore"):
        ul, vl, usable_l = tap_values(lo, p)
        x, y = np.meshgrid(np.arange(W), np.arange(H))
        X0, Y0 = x // s, y // s
        rx, ry = x - s * X0, y - s * Y0
        fx, fy = rx.astype(np.float64) / float(s), ry.astype(np.float64) / float(s)
        lattice = (rx == 0) & (ry == 0)
        zeros3 = lambda: np.zeros((H, W, 3))
        tc, tw, tv, sc, sw, sv = zeros3(), zeros3(), zeros3(), zeros3(), zeros3(), zeros3()
        outside_seen, h_zero_seen = np.zeros((H, W), bool), np.zeros((H, W), bool)
        for j in (0, 1):
            for i in (0, 1):
                X, Y = X0 + i, Y0 + j
                inside = (X < wl) & (Y < hl)
                Xc, Yc = np.minimum(X, wl - 1), np.minimum(Y, hl - 1)
                hh = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
                taken = inside & (hh != 0.0) & ~lattice
                outside_seen |= ~inside & ~lattice
                h_zero_seen |= inside & (hh == 0.0) & ~lattice
                wn = wz = wa = np.ones((H, W))
                if p.normal_power_log2 != NO_NORMAL:
                    a, b = hi["normal"], lo["normal"][Yc, Xc]
                    t = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
                    t = np.where(t > 0.0, t, 0.0)
                    for _ in range(p.normal_power_log2):
                        t = t * t
                    wn = t
                if not math.isinf(p.sigma_depth):
                    zp, zq = hi["depth"], lo["depth"][Yc, Xc]
                    fp, fq = np.isfinite(zp), np.isfinite(zq)
                    r = (zp - zq) / (p.sigma_depth * (zp + zq))
                    wz = np.where(fp & fq, 1.0 / (1.0 + r * r), np.where(fp == fq, 1.0, 0.0))
                if not math.isinf(p.sigma_albedo):
                    d = hi["albedo"] - lo["albedo"][Yc, Xc]
                    da = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wa = 1.0 / (1.0 + da / (p.sigma_albedo * p.sigma_albedo))
                w = ((hh * wn) * wz) * wa
                uq, ok = ul[Yc, Xc], usable_l[Yc, Xc] & taken[..., None]
                okg = ok & (w > 0.0)[..., None]
                tc = np.where(ok, tc + hh[..., None] * uq, tc)
                tw = np.where(ok, tw + hh[..., None], tw)
                sc = np.where(okg, sc + w[..., None] * uq, sc)
                sw = np.where(okg, sw + w[..., None], sw)
                if has_var:
                    vq = vl[Yc, Xc]
                    tv = np.where(ok, tv + (hh * hh)[..., None] * vq, tv)
                    sv = np.where(okg, sv + (w * w)[..., None] * vq, sv)
        guided = sw > p.min_weight * tw
        tent = ~guided & (tw > 0.0)
        u = np.where(guided, sc / sw, np.where(tent, tc / tw, 0.0))
        v = np.where(guided, sv / (sw * sw), np.where(tent, tv / (tw * tw), 0.0)) if has_var else None
        # lattice pixels: the low pixel itself, moved
        lat_u, lat_ok = ul[Y0, X0], usable_l[Y0, X0]
        u = np.where(lattice[..., None], np.where(lat_ok, lat_u, 0.0), u)
        if has_var:
            v = np.where(lattice[..., None], np.where(lat_ok, vl[Y0, X0], 0.0), v)
        if demod:
            div = hi["albedo"] > p.albedo_min
            out = np.where(div, u * hi["albedo"] + hi["emission"], hi["emission"])
            vout = np.where(div, v * (hi["albedo"] * hi["albedo"]), 0.0) if has_var else None
        else:
            out, vout = u, v
    if trace is not None:
        nl = ~lattice[..., None]
        trace.update(lattice=lattice, outside=outside_seen, h_zero=h_zero_seen, guided=guided & nl, tent=tent & nl,
                     none=~guided & ~tent & nl, X0=X0, Y0=Y0)
    return np.ascontiguousarray(out, dtype=np.float64), (None if vout is None else np.ascontiguousarray(vout, dtype=np.float64))


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


def upsample_scalar(lo, hi, p):
    s = p.factor
    hl, wl = np.asarray(lo["depth"]).shape
    H, W = hl * s, wl * s
    L = {k: np.asarray(lo[k], dtype=np.float64).tolist() for k in ("rgb", "albedo", "emission", "normal", "depth")}
    G = {k: np.asarray(hi[k], dtype=np.float64).tolist() for k in ("albedo", "emission", "normal", "depth")}
    has_var = lo.get("var") is not None
    lvar = np.asarray(lo["var"], dtype=np.float64).tolist() if has_var else None
    demod = bool(p.flags & DEMODULATE)

    def tap(X, Y, k):
        """(u, v, usable) of channel k of low pixel (X, Y)"""
        c, a = L["rgb"][Y][X][k], L["albedo"][Y][X][k]
        var = lvar[Y][X][k] if has_var else 0.0
        if demod:
            t = c - L["emission"][Y][X][k]
            if a > p.albedo_min:
                u = _div(t, a)
                v = _div(var, a * a) if has_var else 0.0
                return u, v, _fin(u)
            return t, var, False
        return c, var, _fin(c)

    out = np.zeros((H, W, 3))
    vout = np.zeros((H, W, 3)) if has_var else None
    for y in range(H):
        for x in range(W):
            X0, Y0 = x // s, y // s
            rx, ry = x - s * X0, y - s * Y0
            u, v = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            if rx == 0 and ry == 0:
                for k in range(3):
                    uq, vq, ok = tap(X0, Y0, k)
                    if ok:
                        u[k], v[k] = uq, vq
            else:
                fx, fy = float(rx) / float(s), float(ry) / float(s)
                tc, tw, tv = [0.0] * 3, [0.0] * 3, [0.0] * 3
                sc, sw, sv = [0.0] * 3, [0.0] * 3, [0.0] * 3
                n, z, a = G["normal"][y][x], G["depth"][y][x], G["albedo"][y][x]
                for j in (0, 1):
                    for i in (0, 1):
                        X, Y = X0 + i, Y0 + j
                        hh = (fx if i else 1.0 - fx) * (fy if j else 1.0 - fy)
                        if X >= wl or Y >= hl or hh == 0.0:
                            continue
                        wn = wz = wa = 1.0
                        if p.normal_power_log2 != NO_NORMAL:
                            b = L["normal"][Y][X]
                            t = (n[0] * b[0] + n[1] * b[1]) + n[2] * b[2]
                            t = t if t > 0.0 else 0.0
                            for _ in range(p.normal_power_log2):
                                t = t * t
                            wn = t
                        if not math.isinf(p.sigma_depth):
                            zq = L["depth"][Y][X]
                            if _fin(z) and _fin(zq):
                                r = _div(z - zq, p.sigma_depth * (z + zq))
                                wz = _div(1.0, 1.0 + r * r)
                            else:
                                wz = 1.0 if _fin(z) == _fin(zq) else 0.0
                        if not math.isinf(p.sigma_albedo):
                            d = [a[k] - L["albedo"][Y][X][k] for k in range(3)]
                            da = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                            wa = _div(1.0, 1.0 + _div(da, p.sigma_albedo * p.sigma_albedo))
                        w = ((hh * wn) * wz) * wa
                        for k in range(3):
                            uq, vq, ok = tap(X, Y, k)
                            if not ok:
                                continue
                            tc[k] = tc[k] + hh * uq
                            tw[k] = tw[k] + hh
                            if has_var:
                                tv[k] = tv[k] + (hh * hh) * vq
                            if w > 0.0:
                                sc[k] = sc[k] + w * uq
                                sw[k] = sw[k] + w
                                if has_var:
                                    sv[k] = sv[k] + (w * w) * vq
                for k in range(3):
                    if sw[k] > p.min_weight * tw[k]:
                        u[k] = _div(sc[k], sw[k])
                        v[k] = _div(sv[k], sw[k] * sw[k]) if has_var else 0.0
                    elif tw[k] > 0.0:
                        u[k] = _div(tc[k], tw[k])
                        v[k] = _div(tv[k], tw[k] * tw[k]) if has_var else 0.0
            for k in range(3):
                o, vo = u[k], v[k]
                if demod:
                    ak, ek = G["albedo"][y][x][k], G["emission"][y][x][k]
                    if ak > p.albedo_min:
                        o, vo = o * ak + ek, vo * (ak * ak)
                    else:
                        o, vo = ek, 0.0
                out[y, x, k] = o
                if has_var:
                    vout[y, x, k] = vo
    return out, vout
