"""Rewinding a pick buffer (include/rtx_hip.h, "Rewinding a pick buffer", the comment above RtxObjectMotion) in plain Python, written
from that text: every operation one rounded f64 operation in the header's order.  Two readings:

  rewind(...)         whole-array numpy arithmetic over all hits at once; the list search is the header's loop, run on arrays
  rewind_scalar(...)  one hit at a time over Python floats, the branches as the header writes them

hits: a dict of "position", "normal" (n, 3) float64, "distance" (n,) float64 and "object" (n,) int64; objects: (m,) int64, ascending;
motions: a dict of "kind" (m,) int64 (LOST: no previous geometry), "now" and "before" (m, 9) float64.  Both return a dict like hits;
rewind(..., info=True) adds what happened to every hit (the cases are checked with it).  Neither shares code with the other, and
neither runs anything of the library.  tests/test_rewind.py holds them to each other bit for bit; tests/test_rewind_gpu.py holds the
device to the array reading.  object_motions() is the ten-line restatement of rtx_object_motions.
"""
import math

import numpy as np

NAN, INF = float("nan"), float("inf")
SPHERE, PLANE, TRIANGLE, LOST = 0, 1, 2, 0xFFFFFFFF
WORDS = {SPHERE: 4, PLANE: 6, TRIANGLE: 9}
# what happened to a hit (info["why"])
NO_LIST, NO_OBJECT, NOT_LISTED, LOST_KIND, LOST_POSITION, LOST_SHAPE, LOST_RESULT, REWOUND = range(8)


# ---- the array reading ----------------------------------------------------------------------------------------------------------
def _finite3(u):
    return np.isfinite(u[..., 0]) & np.isfinite(u[..., 1]) & np.isfinite(u[..., 2])


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _norm(a):
    ln = np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
    return a / ln[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _find(L, o):
    """the header's search of the ascending list L (m >= 1) for every o -> lo"""
    lo = np.zeros(o.shape, dtype=np.int64)
    hi = np.full(o.shape, len(L), dtype=np.int64)
    while True:
        active = hi - lo > 1
        if not active.any():
            return lo
        mid = (lo + hi) >> 1
        le = L[mid] <= o
        lo = np.where(active & le, mid, lo)
        hi = np.where(active & ~le, mid, hi)


def rewind(hits, objects, motions, info=False):
    P, o = hits["position"], hits["object"]
    n = len(o)
    out = dict(position=P.copy(), normal=hits["normal"].copy(), distance=hits["distance"].copy(), object=o.copy())
    why = np.full(n, NO_LIST)
    m = len(objects)
    if m:
        with np.errstate(all="ignore"):
            L = np.asarray(objects, dtype=np.int64)
            lo = _find(L, o)
            listed = (o >= 0) & (L[lo] == o)
            kind = np.asarray(motions["kind"], dtype=np.int64)[lo]
            now, was = np.asarray(motions["now"], dtype=np.float64)[lo], np.asarray(motions["before"], dtype=np.float64)[lo]
            is_s, is_p, is_t = kind == SPHERE, kind == PLANE, kind == TRIANGLE
            known = is_s | is_p | is_t
            finite = _finite3(P)
            # sphere
            s = was[:, 3] / now[:, 3]
            ok_s = (s > 0) & (s < INF)
            Qs = was[:, 0:3] + (P - now[:, 0:3]) * s[:, None]
            Ns = _norm(_norm(Qs - was[:, 0:3]))
            # plane
            Qp = P + (was[:, 0:3] - now[:, 0:3])
            Np = _norm(was[:, 3:6])
            # triangle
            e1, e2, w = now[:, 3:6] - now[:, 0:3], now[:, 6:9] - now[:, 0:3], P - now[:, 0:3]
            d11, d12, d22, w1, w2 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2), _dot(w, e1), _dot(w, e2)
            det = d11 * d22 - d12 * d12
            ok_t = (det > 0) & (det < INF)
            u = (d22 * w1 - d12 * w2) / det
            v = (d11 * w2 - d12 * w1) / det
            f1, f2 = was[:, 3:6] - was[:, 0:3], was[:, 6:9] - was[:, 0:3]
            Qt = (was[:, 0:3] + u[:, None] * f1) + v[:, None] * f2
            Nt = _norm(_norm(_cross(f1, f2)))
            Q = np.where(is_s[:, None], Qs, np.where(is_p[:, None], Qp, Qt))
            N = np.where(is_s[:, None], Ns, np.where(is_p[:, None], Np, Nt))
            shape_ok = np.where(is_s, ok_s, np.where(is_t, ok_t, True))
            good = listed & known & finite & shape_ok & _finite3(Q)
            lost = listed & ~good
            why = np.where(o < 0, NO_OBJECT, np.where(~listed, NOT_LISTED, np.where(~known, LOST_KIND, np.where(~finite, LOST_POSITION,
                           np.where(~shape_ok, LOST_SHAPE, np.where(~_finite3(Q), LOST_RESULT, REWOUND))))))
            out["position"] = np.where(good[:, None], Q, P)
            out["normal"] = np.where(good[:, None], N, hits["normal"])
            out["object"] = np.where(lost, -1, o)
    if info:
        return out, why
    return out


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


def _sqrt(x):
    return math.sqrt(x) if x >= 0.0 else NAN               # (a sum of squares is never negative; a NaN stays one)


def _norms(a):
    ln = _sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    return [_div(a[0], ln), _div(a[1], ln), _div(a[2], ln)]


def rewind_scalar(hits, objects, motions):
    out = dict(position=hits["position"].copy(), normal=hits["normal"].copy(), distance=hits["distance"].copy(),
               object=hits["object"].copy())                # byte copies
    m = len(objects)
    L = [int(x) for x in objects]
    for p in range(len(hits["object"])):
        o = int(hits["object"][p])
        if m == 0 or o < 0:
            continue
        lo, hi = 0, m
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if L[mid] <= o:
                lo = mid
            else:
                hi = mid
        if L[lo] != o:
            continue
        kind = int(motions["kind"][lo])
        now, was = [float(x) for x in motions["now"][lo]], [float(x) for x in motions["before"][lo]]
        P = [float(x) for x in hits["position"][p]]
        Q = N = None
        if _fin(P[0]) and _fin(P[1]) and _fin(P[2]):
            if kind == SPHERE:
                s = _div(was[3], now[3])
                if s > 0.0 and s != INF:
                    Q = [was[k] + (P[k] - now[k]) * s for k in range(3)]
                    N = _norms(_norms([Q[k] - was[k] for k in range(3)]))
            elif kind == PLANE:
                Q = [P[k] + (was[k] - now[k]) for k in range(3)]
                N = _norms(was[3:6])
            elif kind == TRIANGLE:
                e1, e2, w = [now[3 + k] - now[k] for k in range(3)], [now[6 + k] - now[k] for k in range(3)], [P[k] - now[k] for k in range(3)]
                d11, d12, d22, w1, w2 = _dots(e1, e1), _dots(e1, e2), _dots(e2, e2), _dots(w, e1), _dots(w, e2)
                det = d11 * d22 - d12 * d12
                if det > 0.0 and det != INF:
                    u = (d22 * w1 - d12 * w2) / det
                    v = (d11 * w2 - d12 * w1) / det
                    f1, f2 = [was[3 + k] - was[k] for k in range(3)], [was[6 + k] - was[k] for k in range(3)]
                    Q = [(was[k] + u * f1[k]) + v * f2[k] for k in range(3)]
                    c = [f1[1] * f2[2] - f1[2] * f2[1], f1[2] * f2[0] - f1[0] * f2[2], f1[0] * f2[1] - f1[1] * f2[0]]
                    N = _norms(_norms(c))
        if Q is None or not (_fin(Q[0]) and _fin(Q[1]) and _fin(Q[2])):
            out["object"][p] = -1
            continue
        out["position"][p] = Q
        out["normal"][p] = N
    return out


# ---- rtx_object_motions, restated -----------------------------------------------------------------------------------------------
def object_motions(indices, before, now):
    """before / now: lists of (kind, geom[9]) -> (ascending indices, [(kind, now[9], before[9])])"""
    first, last = {}, {}
    for i, b, a in zip(indices, before, now):
        first.setdefault(int(i), b)
        last[int(i)] = a
    objects, motions = [], []
    for i in sorted(first):
        (kb, gb), (ka, ga) = first[i], last[i]
        if kb != ka:                                         # a changed kind; LOST in `before` is no shape kind
            objects.append(i), motions.append((LOST, [0.0] * 9, [0.0] * 9))
        elif np.asarray(gb[:WORDS[ka]], dtype=np.float64).tobytes() != np.asarray(ga[:WORDS[ka]], dtype=np.float64).tobytes():
            objects.append(i), motions.append((ka, list(ga), list(gb)))
    return objects, motions
