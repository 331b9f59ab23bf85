"""Rewinding a pick buffer without a GPU: the model's two readings (tests/rewind_model.py) against each other on every fuzzed case, the
rewound normal against tests/text_shapes.py, the rewound position against exact rationals, what before == now leaves unchanged,
rtx_object_motions against its restatement, the C ABI's refusals and layout, the scenes of the end-to-end GPU test, and the one
quality condition on oracle frames."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

import rewind_model as rm
import temporal_model as tm
import text_shapes as ts
from helpers import DEFAULT_CAM
from rewind_cases import PLANT_M, PLANT_N, bits_equal, fuzz_case, hit_records, hits_of, motion_records, same_hits, surface_point, four_tap_pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [(221, 37), (2345, 37), (PLANT_N, PLANT_M), (2345, 4097), (1, 0), (1, 1), (6, 1), (6, 2), (221, 0), (221, 1), (221, 2), (67, 37)]
U = Fr(1, 2 ** 53)                                            # the unit roundoff of f64


@pytest.mark.parametrize("n,m", CASES)
def test_the_two_readings_agree_bit_for_bit(n, m):
    case = fuzz_case(n * 131 + m, n, m)                       # (checked when made: rewind_cases.check_case)
    assert case["planted"] == (n >= PLANT_N and m >= PLANT_M)
    a = rm.rewind(case["hits"], case["objects"], case["motions"])
    b = rm.rewind_scalar(case["hits"], case["objects"], case["motions"])
    assert same_hits(a, b)


def _shape(kind, g):
    return (int(kind), tuple(np.float64(x) for x in g[:rm.WORDS[int(kind)]]))


@pytest.mark.parametrize("n,m", [(221, 37), (2345, 4097)])
def test_the_rewound_normal_is_normal_at_of_the_previous_shape(n, m):
    """independent of the model's arithmetic: tests/text_shapes.py normal_at (object.rs:37-39 over the three shapes) of the shape
    with geometry `before`, at the rewound position, bit for bit on every rewound hit"""
    case = fuzz_case(n + m, n, m)
    out, why = rm.rewind(case["hits"], case["objects"], case["motions"], info=True)
    idx = np.flatnonzero(why == rm.REWOUND)
    assert len(idx) * 4 >= n
    seen = set()
    with np.errstate(all="ignore"):
        for p in idx:
            k = int(np.searchsorted(case["objects"], case["hits"]["object"][p]))
            kind = int(case["motions"]["kind"][k])
            want = ts.normal_at(ts.F64, _shape(kind, case["motions"]["before"][k]), ts.vec(ts.F64, out["position"][p]))
            assert bits_equal(out["normal"][p], np.array(want, dtype=np.float64)), (p, kind)
            seen.add(kind)
    assert seen == {rm.SPHERE, rm.PLANE, rm.TRIANGLE}


# ---- positions against exact rationals ------------------------------------------------------------------------------------------------
def _fr(v):
    return [Fr(float(x)) for x in v]


def _sqrt_up(q, bits=160):
    """a rational >= sqrt(q), within 2^-bits relative"""
    if q == 0:
        return Fr(0)
    s = 2 * bits + max(0, q.denominator.bit_length() - q.numerator.bit_length()) * 2
    return Fr(math.isqrt((q.numerator << (2 * s)) // q.denominator) + 1, 1 << s)


def _sqrt_down(q, bits=160):
    if q == 0:
        return Fr(0)
    s = 2 * bits + max(0, q.denominator.bit_length() - q.numerator.bit_length()) * 2
    return Fr(math.isqrt((q.numerator << (2 * s)) // q.denominator), 1 << s)


def _dotq(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def test_a_rewound_sphere_hit_lies_on_the_previous_sphere():
    """Exact: P'* = c' + (P - c) r'/r, so | |P'* - c'| - r' | = s* | |P - c| - r |, s* = r'/r: the residual P had on the current sphere,
    scaled.  Computed, every operation within u = 2^-53 relative: s = s*(1 + d1); g_k = (P_k - c_k)(1 + d2); the product (1 + d3); the
    sum (c'_k + ...)(1 + d4).  So P'_k - c'_k = (P_k - c_k) s* (1 + d1)(1 + d2)(1 + d3)(1 + d4) + c'_k d4 (1 + ...), and by the triangle
    inequality
        | |P' - c'| - r' |  <=  s* resid  +  s* |P - c| ((1 + u)^4 - 1)  +  (|c'| + s* |P - c| (1 + u)^3) u,
    the four operations' rounding.  Checked with exact rationals (square roots bracketed to 2^-160), not with the model's floats."""
    rng = np.random.default_rng(5)
    worst = Fr(0)
    for trial in range(300):
        c, r = rng.normal(0, 30, 3), rng.uniform(0.01, 50)
        c2, r2 = rng.normal(0, 30, 3), rng.uniform(0.01, 50)
        P = surface_point(rng, rm.SPHERE, np.array([*c, r, 0, 0, 0, 0, 0]))
        hits = dict(position=P[None], normal=np.ones((1, 3)), distance=np.ones(1), object=np.zeros(1, dtype=np.int64))
        mot = dict(kind=np.array([rm.SPHERE]), now=np.array([[*c, r, 0, 0, 0, 0, 0]]), before=np.array([[*c2, r2, 0, 0, 0, 0, 0]]))
        out = rm.rewind(hits, np.zeros(1, dtype=np.int64), mot)
        Q = _fr(out["position"][0])
        cq, c2q, Pq, rq, r2q = _fr(c), _fr(c2), _fr(P), Fr(float(r)), Fr(float(r2))
        s = r2q / rq
        g2 = _dotq([Pq[k] - cq[k] for k in range(3)], [Pq[k] - cq[k] for k in range(3)])
        resid = max(_sqrt_up(g2) - rq, rq - _sqrt_down(g2))
        bound = s * resid + s * _sqrt_up(g2) * ((1 + U) ** 4 - 1) + (_sqrt_up(_dotq(c2q, c2q)) + s * _sqrt_up(g2) * (1 + U) ** 3) * U
        d2 = _dotq([Q[k] - c2q[k] for k in range(3)], [Q[k] - c2q[k] for k in range(3)])
        off = max(_sqrt_up(d2) - r2q, r2q - _sqrt_down(d2))
        assert off <= bound, (trial, float(off), float(bound))
        worst = max(worst, off / bound)
    print("sphere: the worst residual is %.3f of its bound" % float(worst))


def _min_angle_ok(g, degrees=20.0):
    A, B, Cc = g[0:3], g[3:6], g[6:9]
    for a, b, c in ((A, B, Cc), (B, Cc, A), (Cc, A, B)):
        e, f = b - a, c - a
        if np.dot(e, f) / (np.linalg.norm(e) * np.linalg.norm(f)) > math.cos(math.radians(degrees)):
            return False
    return True


def test_a_rewound_triangle_hit_is_the_affine_image():
    """The exact image: (u*, v*) solve the Gram system d11 u + d12 v = w1, d12 u + d22 v = w2 in rationals (P's affine coordinates, the
    least-squares ones where P's own rounding left it off the plane), P'* = A' + u* e1' + v* e2'.  The bound, with u = 2^-53,
    kappa = d11 d22 / det = 1 / sin^2 of the angle at A (the Gram determinant's conditioning; at most 8.55 when every angle is >= 20
    degrees, the angle at A then being in [20, 140] degrees):
      * a numerator d22 w1 - d12 w2 goes through 7 roundings (a subtraction, the dot's product and two sums, a product, the
        difference -- and the other term's as many), each on terms of size <= |e2|^2 |w| |e1|: absolute error <= 14 u |e2|^2 |w| |e1|,
        which over det = |e1|^2 |e2|^2 / kappa is 14 u kappa |w| / |e1| in u;
      * det goes through 6 roundings on terms <= d11 d22: relative error <= 12 u kappa; |u*| <= 2 kappa |w| / |e1|; the division adds u.
      So |u - u*| <= (16 + 24 kappa) kappa u |w| / |e1| =: Eu, |v - v*| <= (16 + 24 kappa) kappa u |w| / |e2| =: Ev, to first order;
      * P'_k = (A'_k + u e1'_k) + v e2'_k adds a subtraction, a product and a sum per term: <= 4 u (|A'_k| + |u*| |e1'_k| + |v*| |e2'_k|).
    B_k = 1.01 (Eu |e1'_k| + Ev |e2'_k| + 4 u (|A'_k| + |u*| |e1'_k| + |v*| |e2'_k|)); the 1.01 covers the second-order terms
    (kappa u < 1e-14).  Triangles whose smallest angle is at least 20 degrees; hits inside and outside them."""
    rng = np.random.default_rng(9)
    worst, done = Fr(0), 0
    while done < 200:
        g, g2 = rng.normal(0, 10, 9), rng.normal(0, 10, 9)
        if not _min_angle_ok(g):
            continue
        done += 1
        P = surface_point(rng, rm.TRIANGLE, g, outside=(done % 4 == 0))
        hits = dict(position=P[None], normal=np.ones((1, 3)), distance=np.ones(1), object=np.zeros(1, dtype=np.int64))
        out, why = rm.rewind(hits, np.zeros(1, dtype=np.int64), dict(kind=np.array([rm.TRIANGLE]), now=g[None], before=g2[None]), info=True)
        assert why[0] == rm.REWOUND
        A, B, Cc, A2, B2, C2, Pq = _fr(g[0:3]), _fr(g[3:6]), _fr(g[6:9]), _fr(g2[0:3]), _fr(g2[3:6]), _fr(g2[6:9]), _fr(P)
        e1, e2, w = [B[k] - A[k] for k in range(3)], [Cc[k] - A[k] for k in range(3)], [Pq[k] - A[k] for k in range(3)]
        d11, d12, d22, w1, w2 = _dotq(e1, e1), _dotq(e1, e2), _dotq(e2, e2), _dotq(w, e1), _dotq(w, e2)
        det = d11 * d22 - d12 * d12
        us, vs = (d22 * w1 - d12 * w2) / det, (d11 * w2 - d12 * w1) / det
        kappa = d11 * d22 / det
        assert kappa <= Fr(855, 100)
        f1, f2 = [B2[k] - A2[k] for k in range(3)], [C2[k] - A2[k] for k in range(3)]
        lw = _sqrt_up(_dotq(w, w))
        Eu = (16 + 24 * kappa) * kappa * U * lw / _sqrt_down(d11)
        Ev = (16 + 24 * kappa) * kappa * U * lw / _sqrt_down(d22)
        Q = _fr(out["position"][0])
        for k in range(3):
            exact = A2[k] + us * f1[k] + vs * f2[k]
            bound = Fr(101, 100) * (Eu * abs(f1[k]) + Ev * abs(f2[k]) + 4 * U * (abs(A2[k]) + abs(us) * abs(f1[k]) + abs(vs) * abs(f2[k])))
            assert abs(Q[k] - exact) <= bound, (done, k, float(abs(Q[k] - exact)), float(bound))
            worst = max(worst, abs(Q[k] - exact) / bound)
    print("triangle: the worst error is %.4f of its bound" % float(worst))


def test_unchanged_geometry_leaves_positions_where_the_header_says():
    """before == now bitwise: a plane's P' == P (the bits too, but for a -0.0 component, which comes back +0.0); a sphere's P'_k is within
    2^-53 (|P_k - c_k| + |P'_k|) of P_k (s == 1; the subtraction and the sum round once each)"""
    case = fuzz_case(77, 600, 40)
    mot = dict(case["motions"], before=case["motions"]["now"].copy())
    hits = case["hits"]
    out, why = rm.rewind(hits, case["objects"], mot, info=True)
    k = np.searchsorted(case["objects"], hits["object"].clip(case["objects"][0], case["objects"][-1]))
    done = why == rm.REWOUND
    planes, spheres = done & (mot["kind"][k] == rm.PLANE), done & (mot["kind"][k] == rm.SPHERE)
    assert planes.sum() >= 20 and spheres.sum() >= 20
    P, Q = hits["position"], out["position"]
    assert (Q[planes] == P[planes]).all()
    nz = ~((P == 0) & np.signbit(P))
    assert np.array_equal(Q[planes][nz[planes]].view(np.uint64), P[planes][nz[planes]].view(np.uint64))
    assert not np.signbit(Q[planes][~nz[planes]]).any()
    c = mot["now"][k][:, 0:3]
    for p in np.flatnonzero(spheres):
        for j in range(3):
            assert abs(Fr(float(Q[p, j])) - Fr(float(P[p, j]))) <= U * (abs(Fr(float(P[p, j])) - Fr(float(c[p, j]))) + abs(Fr(float(Q[p, j]))))


# ---- rtx_object_motions ---------------------------------------------------------------------------------------------------------------
def _records(rtx, entries):
    a = np.zeros(len(entries), dtype=rtx.OBJECT_DTYPE)
    for r, (kind, g) in zip(a, entries):
        r["kind"] = kind
        r["geom"] = g
        r["roughness"] = 0.5
    return a


def test_object_motions_equal_the_restatement(rtx):
    rng = np.random.default_rng(3)
    geo = lambda: [float(x) for x in rng.normal(0, 3, 9)]
    g_same = geo()
    g_tail = list(g_same[:4]) + geo()[4:]                     # a sphere reads 4 words: the rest may differ
    idx = [9, 4, 9, 30, 4, 17, 2, 11, 9, 25, 26]
    before = [(0, geo()), (1, geo()), (0, geo()), (2, geo()), (1, geo()), (0, g_same), (rm.LOST, [0.0] * 9), (1, geo()), (0, geo()), (2, g_same),
              (1, g_same)]
    now = [(0, geo()), (1, geo()), (0, geo()), (0, geo()), (1, geo()), (0, g_tail), (2, geo()), (1, geo()), (0, geo()), (2, g_same),
           (1, list(g_same[:6]) + geo()[6:])]
    now[7] = (1, list(before[7][1][:5]) + [before[7][1][5] + 1.0] + geo()[6:])        # a plane whose sixth word changed: kept
    want_o, want_m = rm.object_motions(idx, before, now)
    assert want_o == [2, 4, 9, 11, 30] and [m[0] for m in want_m] == [rm.LOST, 1, 0, 1, rm.LOST]
    got_o, got_m = rtx.object_motions(idx, _records(rtx, before), _records(rtx, now))
    assert got_o.dtype == np.int64 and got_m.dtype == rtx.OBJECT_MOTION_DTYPE
    assert got_o.tolist() == want_o and (np.diff(got_o) > 0).all()
    for r, (kind, g_now, g_was) in zip(got_m, want_m):
        assert int(r["kind"]) == kind and int(r["reserved"]) == 0
        assert r["now"].tobytes() == np.array(g_now).tobytes() and r["before"].tobytes() == np.array(g_was).tobytes()
    # of index 9 the first `before` and the last `now` were kept; 4 likewise
    assert got_m[2]["before"].tolist() == before[0][1] and got_m[2]["now"].tolist() == now[8][1]
    assert got_m[1]["before"].tolist() == before[1][1] and got_m[1]["now"].tolist() == now[4][1]
    o, m = rtx.object_motions([], _records(rtx, []), _records(rtx, []))
    assert len(o) == 0 and len(m) == 0
    assert rtx.RTX_MOTION_LOST == rm.LOST and rtx.RTX_MOTION_LOST not in (rtx.RTX_SPHERE, rtx.RTX_PLANE, rtx.RTX_TRIANGLE)
    lib = rtx.load_library()
    INVALID = rtx.abi.RTX_ERR_INVALID_ARGUMENT
    i1, b1, n1 = np.array([3], dtype=np.uint64), _records(rtx, [(0, geo())]), _records(rtx, [(0, geo())])
    oo, mm, cnt = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=rtx.OBJECT_MOTION_DTYPE), C.c_uint64(7)
    call = lambda i, b, n, k, o_, m_, c_: lib.rtx_object_motions(i, b, n, k, o_, m_, c_)
    good = (i1.ctypes.data, b1.ctypes.data, n1.ctypes.data, 1, oo.ctypes.data, mm.ctypes.data, C.byref(cnt))
    assert call(*good) == rtx.abi.RTX_OK and cnt.value == 1 and oo[0] == 3
    for k in (0, 1, 2, 4, 5):
        a = list(good)
        a[k] = None
        assert call(*a) == INVALID, k
    assert call(*good[:6], None) == INVALID
    assert call(*good[:3], 1 << 31, *good[4:]) == INVALID
    big = np.array([1 << 63], dtype=np.uint64)
    assert call(big.ctypes.data, *good[1:]) == INVALID
    bad = _records(rtx, [(5, geo())])
    assert call(good[0], good[1], bad.ctypes.data, *good[3:]) == INVALID and call(good[0], bad.ctypes.data, *good[2:]) == INVALID
    lost_now = _records(rtx, [(rm.LOST, geo())])
    assert call(good[0], good[1], lost_now.ctypes.data, *good[3:]) == INVALID


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_struct_layout_matches_the_dtype(rtx, tmp_path):
    names = rtx.OBJECT_MOTION_DTYPE.names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rtx_hip.h"\nint main(void){ printf("%zu", sizeof(RtxObjectMotion));\n' +
                   "".join('printf(" %%zu", offsetof(RtxObjectMotion, %s));\n' % n for n in names) +
                   'printf(" %u", (unsigned)(RTX_MOTION_LOST != RTX_SPHERE && RTX_MOTION_LOST != RTX_PLANE && RTX_MOTION_LOST != RTX_TRIANGLE));\n'
                   'printf(" %lu", (unsigned long)RTX_MOTION_LOST);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    dt = rtx.OBJECT_MOTION_DTYPE
    assert got[0] == dt.itemsize == C.sizeof(rtx.abi.RtxObjectMotion) == 152
    assert got[1:5] == [dt.fields[n][1] for n in names] == [getattr(rtx.abi.RtxObjectMotion, n).offset for n in names] == [0, 4, 8, 80]
    assert got[5] == 1 and got[6] == rtx.RTX_MOTION_LOST
    hdr = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"RTX_STATIC_ASSERT\(sizeof\(RtxObjectMotion\) == 152", hdr)
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")).read()
    for fn in ("rtx_rewind_hits_device", "rtx_rewind_hits", "rtx_object_motions"):       # declared, bound in Python and in Rust alike
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % fn, plain)
        assert m and fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        n_args = m.group(1).count(",") + 1
        assert len([s for s in rtx.abi.SYMBOLS if s[0] == fn][0][2]) == n_args, fn
        r = re.search(r"pub fn %s\s*\(([^;]*)\)" % fn, rs)
        assert r and r.group(1).count(":") == n_args, fn
    assert "pub struct RtxObjectMotion" in rs and "RTX_MOTION_LOST" in rs


def _aligned(nbytes, off=0):
    raw = np.zeros(nbytes + 32, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + off
    return raw[start:start + nbytes]


def test_invalid_arguments_are_refused_without_a_device(rtx):
    lib = rtx.load_library()
    INVALID, OK, NO_DEVICE = rtx.abi.RTX_ERR_INVALID_ARGUMENT, rtx.abi.RTX_OK, rtx.abi.RTX_ERR_NO_DEVICE
    n, m = 8, 3
    case = fuzz_case(1, n, m)
    hits, out = _aligned(64 * n), _aligned(64 * n)
    hits[:] = hit_records(rtx.HIT_DTYPE, case["hits"]).view(np.uint8)
    objects = case["objects"].copy()
    motions = motion_records(rtx.OBJECT_MOTION_DTYPE, case["motions"])
    dev = lambda h=hits.ctypes.data, n_=n, o=objects.ctypes.data, mo=motions.ctypes.data, m_=m, flags=0, out_=out.ctypes.data: \
        lib.rtx_rewind_hits_device(h, n_, o, mo, m_, flags, out_, 0, None)
    host = lambda h=hits.ctypes.data, n_=n, o=objects.ctypes.data, mo=motions.ctypes.data, m_=m, out_=out.ctypes.data: \
        lib.rtx_rewind_hits(h, n_, o, mo, m_, out_)
    have = rtx.device_count() > 0
    # the baseline is acceptable: the host form takes the same arguments past the check (and then finds a device, or reports none)
    assert host() == (OK if have else NO_DEVICE)
    assert host(o=None, mo=None, m_=0) == (OK if have else NO_DEVICE)
    for f in (dev, host):
        assert f(h=None) == INVALID and f(out_=None) == INVALID
        assert f(o=None) == INVALID and f(mo=None) == INVALID
        assert f(n_=0) == INVALID and f(n_=(1 << 32) - 16) == INVALID and f(n_=1 << 40) == INVALID
        assert f(m_=1 << 31) == INVALID
        assert f(out_=hits.ctypes.data) == INVALID                                   # no in-place form
        assert f(out_=hits.ctypes.data + 64 * (n - 1)) == INVALID                    # any overlap
        assert f(o=hits.ctypes.data) == INVALID and f(mo=out.ctypes.data) == INVALID
    assert dev(flags=1) == INVALID
    odd_in, odd_out = _aligned(64 * n, 8), _aligned(64 * n, 8)
    assert dev(h=odd_in.ctypes.data) == INVALID and dev(out_=odd_out.ctypes.data) == INVALID        # the device form's 16-byte rule
    assert host(h=odd_in.ctypes.data, out_=odd_out.ctypes.data) == (OK if have else NO_DEVICE)
    # the host form's own refusals
    for bad in ([5, 5, 9], [9, 7, 12], [5, 9, 9]):
        o2 = np.array(bad, dtype=np.int64)
        assert host(o=o2.ctypes.data) == INVALID, bad
    mo2 = motions.copy(); mo2["kind"][1] = 3
    assert host(mo=mo2.ctypes.data) == INVALID
    mo2 = motions.copy(); mo2["reserved"][2] = 1
    assert host(mo=mo2.ctypes.data) == INVALID
    mo2 = motions.copy(); mo2["kind"][1] = rtx.RTX_MOTION_LOST
    assert host(mo=mo2.ctypes.data) == (OK if have else NO_DEVICE)
    with pytest.raises(ValueError):
        rtx.rewind_hits(hit_records(rtx.HIT_DTYPE, case["hits"]), objects, motions[:2])
    if not have:
        with pytest.raises(rtx.RtxError):
            rtx.rewind_hits(hit_records(rtx.HIT_DTYPE, case["hits"]), objects, motions)
    assert same_hits(hits_of(hit_records(rtx.HIT_DTYPE, case["hits"])), case["hits"])


# ---- golden scenes: the end-to-end test's preconditions and the quality condition -------------------------------------------------------
def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    import json
    return z["objects"], int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def _oracle_pick(oracle, rtx, objs_raw, cam, w, h, **cfg):
    """the pick buffer from the oracle's closest_object on every pixel's zero-offset ray, the normal from tests/text_shapes.py"""
    objs = np.frombuffer(objs_raw.tobytes(), dtype=rtx.OBJECT_DTYPE)
    sc = oracle.make_scene(np.frombuffer(objs_raw.tobytes(), dtype=oracle.OBJECT_DTYPE), cam, **cfg)
    L = oracle.lib()
    vfov = h / w * cam[2]
    pos, nrm, obj = np.full((h, w, 3), np.nan), np.full((h, w, 3), np.nan), np.full((h, w), -1, dtype=np.int64)
    o = np.array(cam[0], dtype=np.float64)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                rd = np.array(L.rtxo_get_ray_dir(C.byref(sc), x / w, y / h, vfov).tuple())
                i, dist = oracle.closest_object(sc, cam[0], tuple(rd))
                if i < 0:
                    continue
                P = o + rd * dist
                pos[y, x], obj[y, x] = P, i
                nrm[y, x] = ts.normal_at(ts.F64, _shape(objs[i]["kind"], objs[i]["geom"]), ts.vec(ts.F64, P))
    return dict(position=pos, normal=nrm, object=obj)


def _cam_hist(rtx, cam, w, h):
    c = rtx.Camera(*cam).to_c()
    return dict(cam_pos=np.array(c.position[:]), to_cam=np.array(c.to_cam_space[:]), tables=rtx.temporal_tables(c.fov, w, h))


def _rewound_pick(pick, index, now_geom, was_geom, kind=rm.SPHERE):
    """a (h, w) pick through the rewind model for one moved object"""
    h, w = pick["object"].shape
    flat = dict(position=pick["position"].reshape(-1, 3), normal=pick["normal"].reshape(-1, 3), distance=np.ones(h * w),
                object=pick["object"].reshape(-1))
    out = rm.rewind(flat, np.array([index], dtype=np.int64), dict(kind=np.array([kind]), now=now_geom[None], before=was_geom[None]))
    return dict(position=out["position"].reshape(h, w, 3), normal=out["normal"].reshape(h, w, 3), object=out["object"].reshape(h, w))


def most_seen_sphere(rtx, objs, pick):
    seen = np.bincount(pick["object"][pick["object"] >= 0].ravel(), minlength=len(objs))
    return [int(i) for i in np.argsort(-seen) if objs[i]["kind"] == rtx.RTX_SPHERE and seen[i] > 0][0]


def _nudged(k):
    a = 0.004 * k
    return ((0.0, 0.02 * k, 0.0), (math.cos(a), math.sin(a), 0.0), DEFAULT_CAM[2])


@pytest.mark.parametrize("name", ["c1_three_spheres_32x32", "mixed_40x24"])
def test_the_end_to_end_scenes_keep_the_moved_spheres_history(oracle, rtx, name):
    """what tests/test_rewind_gpu.py's sequence relies on, from the oracle's picks and the two models alone: after the shipped move
    (0.8 of its radius along y, the camera held) the sphere most pixels see has at least four pixels whose four taps all lie on it in
    the previous pick, and unrewound strictly fewer of the sphere's pixels take history than rewound.  (That EVERY four-tap pixel takes
    history is asserted on the device's own picks, in tests/test_rewind_gpu.py.)"""
    objs_raw, w, h, cfg = _golden(name)
    objs = np.frombuffer(objs_raw.tobytes(), dtype=rtx.OBJECT_DTYPE).copy()
    cam = _nudged(2)
    prev = _oracle_pick(oracle, rtx, objs_raw, cam, w, h, **cfg)
    s = most_seen_sphere(rtx, objs, prev)
    moved = objs.copy()
    moved["geom"][s, 1] += 0.8 * moved["geom"][s, 3]
    cur = _oracle_pick(oracle, rtx, moved, cam, w, h, **cfg)
    d = rtx.temporal_params()
    p = tm.Params(**{k: d[k].item() for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")})
    hist = dict(prev, rgb=np.ones((h, w, 3)), var=None, len=np.full((h, w), 3.0), **_cam_hist(rtx, cam, w, h))
    back = _rewound_pick(cur, s, moved["geom"][s], objs["geom"][s])
    *_, ln_with, motion = tm.accumulate(dict(back, rgb=np.ones((h, w, 3)), var=None), hist, p)
    *_, ln_without, _ = tm.accumulate(dict(cur, rgb=np.ones((h, w, 3)), var=None), hist, p)
    on = cur["object"] == s
    four = four_tap_pixels(motion, prev["object"], cur["object"], s)
    print("%s: sphere %d on %d pixels, %d with four taps; len > 1 on %d rewound, %d unrewound" %
          (name, s, on.sum(), four.sum(), (ln_with[on] > 1).sum(), (ln_without[on] > 1).sum()))
    assert four.sum() >= 4
    assert (ln_without[on] > 1).sum() < (ln_with[on] > 1).sum()


def _frames(oracle, objs_list, cam, w, h, spp, cfg, seed0):
    return [oracle.render(oracle.make_scene(np.frombuffer(o.tobytes(), dtype=oracle.OBJECT_DTYPE), cam, **dict(cfg, rays_per_pixel=spp, seed=seed0 + k)), w, h)
            for k, o in enumerate(objs_list)]


def _rmse(a, b):
    d = a - b
    return float(np.sqrt(np.mean(d * d)))


# the step: this share of the sphere's radius along y, per frame (away from the other sphere).  Of -0.2, -0.3, -0.5 and -0.8 the two
# smaller ones leave history on some of the sphere's pixels unrewound (the plane test passes near the limb); -0.5 is the least that
# does not, on the oracle's picks alone
QUALITY_SCENE, QUALITY_STEP = "c1_three_spheres_32x32", -0.5


def quality_numbers(oracle, rtx, name=QUALITY_SCENE, step=QUALITY_STEP, n_frames=6):
    """(rmse with rewinding, without, of the last frame alone, whether every unrewound frame left all the sphere's pixels at len 1,
    the number of pixels) over the pixels that show the moved sphere in the last frame, against 256 spp of the last frame"""
    objs_raw, w, h, cfg = _golden(name)
    objs = np.frombuffer(objs_raw.tobytes(), dtype=rtx.OBJECT_DTYPE).copy()
    cam = DEFAULT_CAM
    first = _oracle_pick(oracle, rtx, objs_raw, cam, w, h, **cfg)
    seen = np.bincount(first["object"][first["object"] >= 0].ravel(), minlength=len(objs))
    s = [int(i) for i in np.argsort(-seen, kind="stable") if objs[i]["kind"] == rtx.RTX_SPHERE and objs[i]["roughness"] >= 0.9 and
         not objs[i]["emission_color"].any()][0]             # the lit, rough sphere most pixels see directly
    lists = []
    for k in range(n_frames):
        o = objs.copy()
        o["geom"][s, 1] += k * step * objs["geom"][s, 3]
        lists.append(o)
    frames = _frames(oracle, lists, cam, w, h, 4, cfg, 31)
    ref = _frames(oracle, lists[-1:], cam, w, h, 256, cfg, 999)[0]
    d = rtx.temporal_params()
    p = tm.Params(**{k: d[k].item() for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")})
    ch = _cam_hist(rtx, cam, w, h)
    hist_w = hist_o = None
    all_lost = True
    for k, (o, f) in enumerate(zip(lists, frames)):
        pick = _oracle_pick(oracle, rtx, o, cam, w, h, **cfg)
        back = pick if k == 0 else _rewound_pick(pick, s, o["geom"][s], lists[k - 1]["geom"][s])
        out_w, _, ln_w, _ = tm.accumulate(dict(back, rgb=f, var=None), hist_w, p)
        out_o, _, ln_o, _ = tm.accumulate(dict(pick, rgb=f, var=None), hist_o, p)
        hist_w = dict(pick, rgb=out_w, var=None, len=ln_w, **ch)                 # the UNREWOUND pick is the next frame's history
        hist_o = dict(pick, rgb=out_o, var=None, len=ln_o, **ch)
        on = pick["object"] == s
        if k > 0:
            all_lost = all_lost and bool((ln_o[on] == 1).all())
    return _rmse(out_w[on], ref[on]), _rmse(out_o[on], ref[on]), _rmse(frames[-1][on], ref[on]), all_lost, int(on.sum()), float(ln_w[on].mean())


def test_rewinding_brings_the_moved_sphere_nearer_the_converged_frame(oracle, rtx):
    """the one quality condition, with both models on oracle frames and the library's default RtxTemporalParams: six 4-spp frames, the
    camera static, the lit rough sphere most pixels see directly (the red one) moved by QUALITY_STEP of its radius per frame (so far that, unrewound, every one
    of its pixels starts again at len == 1 in every frame), distinct seeds -- over the pixels that show the sphere in the last frame,
    RMSE against 256 spp of the last frame: with rewinding < without.  A condition, not a tuned number; the last frame alone is
    reported."""
    with_, without, alone, all_lost, npix, mean_len = quality_numbers(oracle, rtx)
    print("%s, step %.2f r: RMSE over the sphere's %d pixels against 256 spp: rewound %.6f, unrewound %.6f, the last frame alone %.6f; "
          "mean history length rewound %.2f" % (QUALITY_SCENE, QUALITY_STEP, npix, with_, without, alone, mean_len))
    assert all_lost, "the step is too small: an unrewound frame kept history on the moved sphere"
    assert npix >= 16
    assert with_ < without
