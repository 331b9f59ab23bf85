"""Temporal accumulation of include/rtx_hip.h ("Temporal accumulation", the comment above RtxTemporalParams) in plain Python, written
from that text: every operation one rounded f64 operation in the header's order.  Two readings:

  accumulate(...)         whole-array numpy arithmetic over all pixels at once; the table search is the header's loop, run on arrays
  accumulate_scalar(...)  one pixel at a time over Python floats, the loops as the header writes them

A frame is a dict: "rgb" (h, w, 3), "var" (h, w, 3) or None, "position", "normal" (h, w, 3) and "object" (h, w) int64 of the pick
buffer; a history is a dict with "rgb", "var" (or None), "len" (h, w), "position", "normal", "object", and "cam_pos" (3,), "to_cam" (9,)
and "tables" ((w + 1) + (h + 1),) of the previous camera; None: the first frame.  Both return (out_rgb, out_var or None, out_len,
motion); accumulate(..., info=True) adds what happened to every pixel (the cases are checked with it).  Neither shares code with the
other beyond the parameter record, and neither runs anything of the library.  tests/test_temporal.py holds them to each other bit for
bit; tests/test_temporal_gpu.py holds the device to the array reading.
"""
import math

import numpy as np

NAN = float("nan")
INF = float("inf")
# what happened to a pixel (info["why"], one value) and to its taps (info["taps"], a bit set over the taps inside the frame with w > 0)
FIRST, MISS, BEHIND, LEFT, RIGHT, ABOVE, BELOW, LOW_WEIGHT, BLENDED = range(9)
TAP_OBJECT, TAP_LEN, TAP_NOT_FINITE, TAP_NORMAL, TAP_PLANE = 1, 2, 4, 8, 16


class Params:
    """RtxTemporalParams; the defaults here are only this file's (the library's come from rtx_temporal_default_params)"""

    def __init__(self, alpha_min=0.05, max_history=32.0, plane_tolerance=0.02, normal_min=0.9, min_weight=0.01):
        self.alpha_min, self.max_history, self.plane_tolerance = float(alpha_min), float(max_history), float(plane_tolerance)
        self.normal_min, self.min_weight = float(normal_min), float(min_weight)

    def replace(self, **kw):
        p = Params(**self.__dict__)
        for k, v in kw.items():
            assert hasattr(p, k), k
            setattr(p, k, float(v))
        return p


def tables(fov, width, height):
    """the header's tables with math.sin: Tx[width + 1] then Ty[height + 1]"""
    vfov = height / width * fov
    return np.array([math.sin(fov * (i / width - 0.5)) for i in range(width + 1)] +
                    [math.sin(vfov * (j / height - 0.5)) for j in range(height + 1)], dtype=np.float64)


# ---- the array reading ----------------------------------------------------------------------------------------------------------
def _finite3(u):
    return np.isfinite(u[..., 0]) & np.isfinite(u[..., 1]) & np.isfinite(u[..., 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unmap(T, n, s):
    lo = np.zeros(s.shape, dtype=np.int64)
    hi = np.full(s.shape, n, dtype=np.int64)
    while True:
        active = hi - lo > 1
        if not active.any():
            break
        mid = (lo + hi) >> 1
        le = T[mid] <= s
        lo = np.where(active & le, mid, lo)
        hi = np.where(active & ~le, mid, hi)
    t0 = T[lo]
    den = T[lo + 1] - t0
    pos = den > 0
    return lo.astype(np.float64) + np.where(pos, (s - t0) / np.where(pos, den, 1.0), 0.0)


def accumulate(cur, hist, p, info=False):
    c, v = cur["rgb"], cur.get("var")
    h, w = cur["object"].shape
    out, out_var = c.copy(), (None if v is None else v.copy())
    out_len, motion = np.ones((h, w)), np.full((h, w, 2), NAN)
    why, taps, kept = np.full((h, w), FIRST), np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    if hist is not None:
        with np.errstate(all="ignore"):
            P, n, o = cur["position"], cur["normal"], cur["object"]
            cam, M, T = np.asarray(hist["cam_pos"], dtype=np.float64), np.asarray(hist["to_cam"], dtype=np.float64), hist["tables"]
            Tx, Ty = T[:w + 1], T[w + 1:]
            seen = (o >= 0) & _finite3(P)
            e = P - cam
            ccx, ccy, ccz = _dot(e, M[0:3]), _dot(e, M[3:6]), _dot(e, M[6:9])
            front = seen & (ccz > 0)
            a, b = ccx * ccx, ccy * ccy
            L = (a + b) + ccz * ccz
            q = L * L - 4.0 * (a * b)
            q = np.where(q > 0, q, 0.0)
            m = 2.0 / (L + np.sqrt(q))
            k = np.sqrt(m)
            sx, sy = ccx * k, ccy * k
            fx, fy = _unmap(Tx, w, sx), _unmap(Ty, h, sy)
            in_x, in_y = (fx >= -0.5) & (fx <= w - 0.5), (fy >= -0.5) & (fy <= h - 0.5)
            proj = front & in_x & in_y
            why[:] = np.where(~seen, MISS, np.where(~front, BEHIND, np.where(fx < -0.5, LEFT, np.where(fx > w - 0.5, RIGHT,
                              np.where(fy < -0.5, ABOVE, np.where(fy > h - 0.5, BELOW, np.where(~proj, BEHIND, LOW_WEIGHT)))))))   # (a NaN projection: filed under BEHIND)
            motion[proj] = np.stack([fx, fy], axis=-1)[proj]
            gx, gy = np.where(proj, fx, 0.0), np.where(proj, fy, 0.0)
            fi, fj = np.floor(gx), np.floor(gy)
            tx, ty = gx - fi, gy - fj
            i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
            nn, ee = _dot(n, n), _dot(e, e)
            rhs = ((p.plane_tolerance * p.plane_tolerance) * ee) * nn
            nmin2 = p.normal_min * p.normal_min
            sw, hn = np.zeros((h, w)), np.zeros((h, w))
            hs, hv = np.zeros((h, w, 3)), np.zeros((h, w, 3))
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = i0 + dx, j0 + dy
                    wt = (tx if dx else 1.0 - tx) * (ty if dy else 1.0 - ty)
                    live = proj & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wt > 0)
                    cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    ql, hc = hist["len"][cy, cx], hist["rgb"][cy, cx]
                    fin = _finite3(hc)
                    if v is not None:
                        hq = hist["var"][cy, cx]
                        fin = fin & _finite3(hq)
                    nq, Q = hist["normal"][cy, cx], hist["position"][cy, cx]
                    t = _dot(n, nq)
                    ok_n = (t > 0) & (t * t >= nmin2 * (nn * _dot(nq, nq)))
                    d = _dot(Q - P, n)
                    ok_p = d * d <= rhs
                    ok_o, ok_l = hist["object"][cy, cx] == o, ql >= 1
                    keep = live & ok_o & ok_l & fin & ok_n & ok_p
                    taps |= np.where(live, (~ok_o) * TAP_OBJECT | (~ok_l) * TAP_LEN | (~fin) * TAP_NOT_FINITE | (~ok_n) * TAP_NORMAL |
                                     (~ok_p) * TAP_PLANE, 0)
                    kept += keep
                    sw = np.where(keep, sw + wt, sw)
                    hs = np.where(keep[..., None], hs + wt[..., None] * hc, hs)
                    if v is not None:
                        hv = np.where(keep[..., None], hv + wt[..., None] * hq, hv)
                    hn = np.where(keep, hn + wt * ql, hn)
            blend = proj & (sw > p.min_weight)
            why[blend] = BLENDED
            sws = np.where(blend, sw, 1.0)
            N = hn / sws
            alpha = 1.0 / (N + 1.0)
            alpha = np.where(alpha > p.alpha_min, alpha, p.alpha_min)
            beta = 1.0 - alpha
            out = np.where(blend[..., None], beta[..., None] * (hs / sws[..., None]) + alpha[..., None] * c, c)
            if v is not None:
                out_var = np.where(blend[..., None], (beta * beta)[..., None] * (hv / sws[..., None]) + (alpha * alpha)[..., None] * v, v)
            ln = N + 1.0
            out_len = np.where(blend, np.where(ln < p.max_history, ln, p.max_history), 1.0)
    if info:
        return out, out_var, out_len, motion, dict(why=why, taps=taps, kept=kept)
    return out, out_var, out_len, motion


# ---- the scalar reading ---------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE a / b on Python floats (which raise on a zero divisor)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _fin(x):
    return x == x and x not in (INF, -INF)


def _dots(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unmap_scalar(T, n, s):
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if T[mid] <= s:
            lo = mid
        else:
            hi = mid
    den = T[lo + 1] - T[lo]
    return lo + (_div(s - T[lo], den) if den > 0 else 0.0)


def accumulate_scalar(cur, hist, p):
    h, w = cur["object"].shape
    has_var = cur.get("var") is not None
    out, out_var = cur["rgb"].copy(), (cur["var"].copy() if has_var else None)              # byte copies
    out_len, motion = np.ones((h, w)), np.full((h, w, 2), NAN)
    if hist is None:
        return out, out_var, out_len, motion
    cam, M = [float(x) for x in hist["cam_pos"]], [float(x) for x in hist["to_cam"]]
    Tx, Ty = [float(x) for x in hist["tables"][:w + 1]], [float(x) for x in hist["tables"][w + 1:]]
    pt2, nm2 = p.plane_tolerance * p.plane_tolerance, p.normal_min * p.normal_min
    for y in range(h):
        for x in range(w):
            o = int(cur["object"][y, x])
            P = [float(t) for t in cur["position"][y, x]]
            if o < 0 or not (_fin(P[0]) and _fin(P[1]) and _fin(P[2])):
                continue
            n = [float(t) for t in cur["normal"][y, x]]
            c = [float(t) for t in cur["rgb"][y, x]]
            v = [float(t) for t in cur["var"][y, x]] if has_var else None
            e = [P[0] - cam[0], P[1] - cam[1], P[2] - cam[2]]
            ccx, ccy, ccz = _dots(e, M[0:3]), _dots(e, M[3:6]), _dots(e, M[6:9])
            if not ccz > 0.0:
                continue
            a, b = ccx * ccx, ccy * ccy
            L = (a + b) + ccz * ccz
            q = L * L - 4.0 * (a * b)
            q = q if q > 0.0 else 0.0
            m = _div(2.0, L + math.sqrt(q))
            k = math.sqrt(m)
            sx, sy = ccx * k, ccy * k
            fx, fy = _unmap_scalar(Tx, w, sx), _unmap_scalar(Ty, h, sy)
            if not (fx >= -0.5 and fx <= w - 0.5) or not (fy >= -0.5 and fy <= h - 0.5):
                continue
            motion[y, x, 0], motion[y, x, 1] = fx, fy
            i0, j0 = math.floor(fx), math.floor(fy)
            tx, ty = fx - i0, fy - j0
            nn, ee = _dots(n, n), _dots(e, e)
            sw, hn, hs, hv = 0.0, 0.0, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = i0 + dx, j0 + dy
                    if qx < 0 or qx >= w or qy < 0 or qy >= h:
                        continue
                    wt = (tx if dx else 1.0 - tx) * (ty if dy else 1.0 - ty)
                    if not wt > 0.0:
                        continue
                    if int(hist["object"][qy, qx]) != o:
                        continue
                    ql = float(hist["len"][qy, qx])
                    if not ql >= 1.0:
                        continue
                    hc = [float(t) for t in hist["rgb"][qy, qx]]
                    if not (_fin(hc[0]) and _fin(hc[1]) and _fin(hc[2])):
                        continue
                    if has_var:
                        hq = [float(t) for t in hist["var"][qy, qx]]
                        if not (_fin(hq[0]) and _fin(hq[1]) and _fin(hq[2])):
                            continue
                    nq = [float(t) for t in hist["normal"][qy, qx]]
                    t = _dots(n, nq)
                    if not t > 0.0:
                        continue
                    if not t * t >= nm2 * (nn * _dots(nq, nq)):
                        continue
                    Q = [float(t_) for t_ in hist["position"][qy, qx]]
                    d = _dots([Q[0] - P[0], Q[1] - P[1], Q[2] - P[2]], n)
                    if not d * d <= (pt2 * ee) * nn:
                        continue
                    sw = sw + wt
                    for j in range(3):
                        hs[j] = hs[j] + wt * hc[j]
                        if has_var:
                            hv[j] = hv[j] + wt * hq[j]
                    hn = hn + wt * ql
            if not sw > p.min_weight:
                continue
            N = hn / sw
            alpha = _div(1.0, N + 1.0)
            alpha = alpha if alpha > p.alpha_min else p.alpha_min
            beta = 1.0 - alpha
            for j in range(3):
                out[y, x, j] = beta * (hs[j] / sw) + alpha * c[j]
                if has_var:
                    out_var[y, x, j] = (beta * beta) * (hv[j] / sw) + (alpha * alpha) * v[j]
            ln = N + 1.0
            out_len[y, x] = ln if ln < p.max_history else p.max_history
    return out, out_var, out_len, motion
