"""Fuzzed inputs for the rewind tests (CPU and GPU): a sorted list of moved objects of all three kinds with random previous geometry,
hits that lie on the objects' CURRENT surfaces, and -- planted on chosen list entries and hits -- every way of being unmoved, every
way of being lost, and hostile values in P, in `now` and in `before`.  Every case is checked on the CPU when it is made (check_case),
so a generator that stops producing a branch fails loudly and no case is vacuous."""
import numpy as np

import rewind_model as rm
from temporal_cases import bits_equal                        # noqa: F401  (re-exported: the tests compare with it)

NAN, INF = float("nan"), float("inf")
PLANT_M, PLANT_N = 32, 200                                   # the least list and buffer that hold every planted entry and hit


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _geometry(rng, kind):
    """one random well-formed geometry of a kind: 9 words"""
    g = np.zeros(9)
    if kind == rm.SPHERE:
        g[0:3], g[3] = rng.normal(0, 3, 3), rng.uniform(0.3, 2.0)
    elif kind == rm.PLANE:
        g[0:3], g[3:6] = rng.normal(0, 3, 3), _unit(rng, 1)[0] * rng.choice([1.0, 0.5, 3.0])
    else:
        while True:
            g[:] = rng.normal(0, 3, 9)
            e1, e2 = g[3:6] - g[0:3], g[6:9] - g[0:3]
            if np.linalg.norm(np.cross(e1, e2)) > 0.2 * np.linalg.norm(e1) * np.linalg.norm(e2):
                break
    return g


def surface_point(rng, kind, g, outside=False):
    """a point of the shape's surface (a triangle's: inside it, or -- outside -- in its plane beyond an edge)"""
    if kind == rm.SPHERE:
        return g[0:3] + g[3] * _unit(rng, 1)[0]
    if kind == rm.PLANE:
        n = g[3:6] / np.linalg.norm(g[3:6])
        t = np.cross(n, _unit(rng, 1)[0])
        return g[0:3] + 4.0 * rng.uniform(-1, 1) * t
    u, v = (1.5, 0.7) if outside else sorted(rng.uniform(0, 1, 2))
    if not outside:
        u, v = u, v - u                                      # u, v >= 0, u + v <= 1
    return g[0:3] + u * (g[3:6] - g[0:3]) + v * (g[6:9] - g[0:3])


def fuzz_case(seed, n, m, planted=None):
    """-> dict(hits, objects, motions, n, m, planted, plants).  planted (default: when the sizes allow): every branch is present"""
    rng = np.random.default_rng(seed)
    if planted is None:
        planted = n >= PLANT_N and m >= PLANT_M
    assert not planted or (n >= PLANT_N and m >= PLANT_M), "planted cases need room"
    # the list: ascending indices from 3 upwards with gaps (so that a hit can fall below, between and above)
    objects = 3 + np.cumsum(rng.integers(2, 5, m)).astype(np.int64) if m else np.zeros(0, dtype=np.int64)
    kind = rng.integers(0, 3, m).astype(np.int64)
    now, was = np.zeros((m, 9)), np.zeros((m, 9))
    if m:
        kind[0], kind[-1] = rm.SPHERE, rm.TRIANGLE
    for k in range(m):
        now[k], was[k] = _geometry(rng, int(kind[k])), _geometry(rng, int(kind[k]))
        if rng.random() < 0.3:                               # a plain translation
            d = rng.normal(0, 1, 3)
            was[k] = now[k]
            for a in range(0, {0: 3, 1: 3, 2: 9}[int(kind[k])], 3):
                was[k, a:a + 3] = now[k, a:a + 3] + d
    hits = dict(position=np.zeros((n, 3)), normal=_unit(rng, n) * rng.choice([1.0, 0.5, 2.0], (n, 1)), distance=rng.uniform(0.5, 30.0, n),
                object=np.zeros(n, dtype=np.int64))
    plants = {}
    free_k = iter(rng.permutation(np.arange(1, max(m - 1, 1))))
    free_p = iter(rng.permutation(n))
    special = set()

    def entry(kd, g_now, g_was):
        k = int(next(free_k))
        special.add(k)
        kind[k], now[k], was[k] = kd, g_now, g_was
        return k

    def hit(name, k, P=None, outside=False, obj=None):
        p = int(next(free_p))
        plants[name] = p
        if k is not None:
            hits["object"][p] = objects[k]
            hits["position"][p] = surface_point(rng, int(kind[k]), now[k], outside) if P is None else P
        else:
            hits["object"][p] = obj
            hits["position"][p] = rng.normal(0, 3, 3) if P is None else P
        return p

    if planted:
        G = lambda kd: _geometry(rng, kd)
        # -- unmoved
        hit("miss", None, P=[NAN, NAN, NAN], obj=-1)
        hit("below the list", None, obj=int(objects[0]) - 1)
        hit("above the list", None, obj=int(objects[-1]) + 5)
        hit("between two entries", None, obj=int(objects[m // 2]) + 1)
        assert int(objects[m // 2]) + 1 < int(objects[m // 2 + 1])
        # -- rewound: the first and the last entry, a hit outside its triangle, a turned plane, -0.0 in P, now and before
        hit("first entry", 0)
        hit("last entry", m - 1)
        hit("outside the triangle", m - 1, outside=True)
        g = G(rm.PLANE); g2 = G(rm.PLANE)
        hit("turned plane", entry(rm.PLANE, g, g2))
        g = G(rm.SPHERE); g[0] = 0.0
        hit("-0.0 in P", entry(rm.SPHERE, g, G(rm.SPHERE)), P=[-0.0, g[1] + g[3], g[2]])
        g = G(rm.PLANE); g[1] = -0.0; g2 = g.copy(); g2[2] += 1.0
        hit("-0.0 in now", entry(rm.PLANE, g, g2))
        g = G(rm.TRIANGLE); g2 = G(rm.TRIANGLE); g2[4] = -0.0
        hit("-0.0 in before", entry(rm.TRIANGLE, g, g2))
        # -- lost: the record's kind
        hit("kind LOST", entry(rm.LOST, np.zeros(9), np.zeros(9)), P=rng.normal(0, 3, 3))
        hit("unknown kind", entry(7, G(rm.SPHERE), G(rm.SPHERE)), P=rng.normal(0, 3, 3))
        # -- lost: the shape says so
        g = G(rm.SPHERE); g[3] = 0.0
        hit("r = 0", entry(rm.SPHERE, g, G(rm.SPHERE)), P=g[0:3] + 1.0)
        g = G(rm.SPHERE); g[3] = 0.0
        hit("r' = 0", entry(rm.SPHERE, G(rm.SPHERE), g))
        g = G(rm.SPHERE); g[3] = -g[3]
        hit("negative radius", entry(rm.SPHERE, g, G(rm.SPHERE)), P=g[0:3] + 1.0)
        g = G(rm.SPHERE); g[3] = 1e-300; g2 = G(rm.SPHERE); g2[3] = 1e300
        hit("radius ratio overflows", entry(rm.SPHERE, g, g2))
        g = G(rm.SPHERE); g[3] = NAN
        hit("NaN radius", entry(rm.SPHERE, g, G(rm.SPHERE)), P=g[0:3] + 1.0)
        g = np.array([1.0, 2.0, 3.0, 2.0, 4.0, 3.0, 3.0, 6.0, 3.0])           # C - A = 2 (B - A): det == 0 exactly
        hit("degenerate triangle", entry(rm.TRIANGLE, g, G(rm.TRIANGLE)), P=[1.5, 3.0, 3.0])
        g = np.array([0.0, 0.0, 0.0, 1e80, 0.0, 0.0, 0.0, 1e80, 0.0])         # d11 * d22 overflows, d12 == 0: det == +inf
        hit("infinite det", entry(rm.TRIANGLE, g, G(rm.TRIANGLE)), P=[1e79, 1e79, 0.0])
        # -- lost: P' is not finite (hostile words in now and in before; an overflow)
        g = G(rm.SPHERE); g[1] = NAN
        hit("NaN in now", entry(rm.SPHERE, g, G(rm.SPHERE)), P=rng.normal(0, 3, 3))
        g = G(rm.PLANE); g[0] = -INF
        hit("-inf in now", entry(rm.PLANE, g, G(rm.PLANE)), P=rng.normal(0, 3, 3))
        g = G(rm.SPHERE); g[0] = INF
        hit("+inf in now", entry(rm.SPHERE, g, G(rm.SPHERE)), P=rng.normal(0, 3, 3))
        g = G(rm.SPHERE); g[2] = INF
        hit("+inf in before", entry(rm.SPHERE, G(rm.SPHERE), g))
        g = G(rm.PLANE); g[1] = NAN
        hit("NaN in before", entry(rm.PLANE, G(rm.PLANE), g))
        g = G(rm.TRIANGLE); g[7] = -INF
        hit("-inf in before", entry(rm.TRIANGLE, G(rm.TRIANGLE), g))
        g = G(rm.SPHERE); g2 = G(rm.SPHERE); g2[3] = 1e200 * g[3]
        hit("P' overflows", entry(rm.SPHERE, g, g2), P=g[0:3] + np.array([1e150, 0.0, 0.0]))
        # -- rewound with a normal that is not finite: a plane whose previous normal is zero
        g = G(rm.PLANE); g[3:6] = 0.0
        hit("zero normal before", entry(rm.PLANE, G(rm.PLANE), g))
        # -- lost: P (on entries that are none of the planted ones)
        for name, bad in (("NaN in P", NAN), ("+inf in P", INF), ("-inf in P", -INF)):
            k = int(rng.choice([k for k in range(m) if k not in special]))
            P = surface_point(rng, int(kind[k]), now[k])
            P[int(rng.integers(3))] = bad
            hit(name, k, P=P)
    taken = set(plants.values())
    regular = [k for k in range(m) if k not in special]
    for p in range(n):
        if p in taken:
            continue
        r = rng.random()
        if m == 0 or r < 0.1 or not regular:
            hits["object"][p], hits["position"][p] = -1, NAN
            hits["normal"][p] = NAN
        elif r < 0.5:                                        # most hits of a frame are on objects that did not move
            hits["object"][p] = int(objects[int(rng.integers(0, m))]) + 1 if rng.random() < 0.5 else int(rng.integers(0, 3))
            hits["position"][p] = rng.normal(0, 3, 3)
        else:
            k = regular[int(rng.integers(0, len(regular)))]
            hits["object"][p] = objects[k]
            hits["position"][p] = surface_point(rng, int(kind[k]), now[k])
    case = dict(hits=hits, objects=objects, motions=dict(kind=kind, now=now, before=was), n=n, m=m, planted=planted, plants=plants)
    check_case(case)
    return case


EXPECT = {"miss": rm.NO_OBJECT, "below the list": rm.NOT_LISTED, "above the list": rm.NOT_LISTED, "between two entries": rm.NOT_LISTED,
          "first entry": rm.REWOUND, "last entry": rm.REWOUND, "outside the triangle": rm.REWOUND, "turned plane": rm.REWOUND,
          "-0.0 in P": rm.REWOUND, "-0.0 in now": rm.REWOUND, "-0.0 in before": rm.REWOUND, "kind LOST": rm.LOST_KIND,
          "unknown kind": rm.LOST_KIND, "NaN in P": rm.LOST_POSITION, "+inf in P": rm.LOST_POSITION, "-inf in P": rm.LOST_POSITION,
          "r = 0": rm.LOST_SHAPE, "r' = 0": rm.LOST_SHAPE, "negative radius": rm.LOST_SHAPE, "radius ratio overflows": rm.LOST_SHAPE,
          "NaN radius": rm.LOST_SHAPE, "degenerate triangle": rm.LOST_SHAPE, "infinite det": rm.LOST_SHAPE, "NaN in now": rm.LOST_RESULT,
          "-inf in now": rm.LOST_RESULT, "+inf in now": rm.LOST_RESULT, "+inf in before": rm.LOST_RESULT, "NaN in before": rm.LOST_RESULT, "-inf in before": rm.LOST_RESULT,
          "P' overflows": rm.LOST_RESULT, "zero normal before": rm.REWOUND}


def check_case(case):
    """no case is vacuous: every planted hit took the branch it was planted for, all three kinds are rewound, and without a list the
    call is a copy"""
    hits, objects, motions = case["hits"], case["objects"], case["motions"]
    out, why = rm.rewind(hits, objects, motions, info=True)
    assert (np.diff(objects) > 0).all()
    none, why0 = rm.rewind(hits, objects[:0], dict(kind=motions["kind"][:0], now=motions["now"][:0], before=motions["before"][:0]), info=True)
    assert (why0 == rm.NO_LIST).all() and all(none[k].tobytes() == hits[k].tobytes() for k in hits)       # UNMOVED: m == 0
    if case["m"] == 0:
        assert all(out[k].tobytes() == hits[k].tobytes() for k in hits)
    if not case["planted"]:
        return
    assert set(case["plants"]) == set(EXPECT)
    for name, p in case["plants"].items():
        assert why[p] == EXPECT[name], (name, int(why[p]))
    done = why == rm.REWOUND
    assert done.sum() * 4 >= case["n"], "fewer than a quarter of the hits are rewound"
    lo = np.searchsorted(objects, hits["object"].clip(objects[0], objects[-1]))
    for kd in (rm.SPHERE, rm.PLANE, rm.TRIANGLE):
        assert (done & (motions["kind"][lo] == kd)).any(), kd
    unmoved = (why == rm.NO_OBJECT) | (why == rm.NOT_LISTED)
    for k in hits:
        assert out[k][unmoved].tobytes() == hits[k][unmoved].tobytes(), k
    lost = (why >= rm.LOST_KIND) & (why <= rm.LOST_RESULT)
    assert (out["object"][lost] == -1).all() and (out["object"][~lost] == hits["object"][~lost]).all()
    for k in ("position", "normal", "distance"):
        assert out[k][lost].tobytes() == hits[k][lost].tobytes(), k
    assert out["distance"].tobytes() == hits["distance"].tobytes()
    p = case["plants"]["zero normal before"]
    assert np.isnan(out["normal"][p]).all() and np.isfinite(out["position"][p]).all()
    p = case["plants"]["turned plane"]
    assert np.isfinite(out["normal"][p]).all()


def hit_records(dtype, hits):
    """RtxHit records of a hits dict"""
    r = np.zeros(len(hits["object"]), dtype=dtype)
    for k in ("position", "normal", "distance", "object"):
        r[k] = hits[k]
    return r


def hits_of(records):
    """a hits dict of RtxHit records"""
    r = np.asarray(records).reshape(-1)
    return dict(position=r["position"].copy(), normal=r["normal"].copy(), distance=r["distance"].copy(), object=r["object"].copy())


def motion_records(dtype, motions):
    """RtxObjectMotion records of a motions dict (kind LOST = 0xFFFFFFFF, the header's RTX_MOTION_LOST)"""
    r = np.zeros(len(motions["kind"]), dtype=dtype)
    r["kind"], r["now"], r["before"] = motions["kind"], motions["now"], motions["before"]
    return r


def motions_of(records):
    r = np.asarray(records).reshape(-1)
    return dict(kind=r["kind"].astype(np.int64), now=r["now"].copy(), before=r["before"].copy())


def same_hits(a, b):
    """two hits dicts hold the same patterns (every NaN one pattern)"""
    return (np.array_equal(a["object"], b["object"]) and bits_equal(a["position"], b["position"]) and bits_equal(a["normal"], b["normal"])
            and bits_equal(a["distance"], b["distance"]))


def four_tap_pixels(motion, prev_object, now_object, index):
    """the pixels of object `index` whose four reprojection taps all lie on it in the previous pick"""
    h, w = now_object.shape
    ok = (now_object == index) & np.isfinite(motion).all(axis=-1)
    i0, j0 = np.floor(np.where(ok, motion[..., 0], 0)).astype(int), np.floor(np.where(ok, motion[..., 1], 0)).astype(int)
    for dy in (0, 1):
        for dx in (0, 1):
            qx, qy = i0 + dx, j0 + dy
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            ok &= inside & (prev_object[qy.clip(0, h - 1), qx.clip(0, w - 1)] == index)
    return ok
