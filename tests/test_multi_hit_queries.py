"""Multi-hit ray queries: the k nearest objects along each ray (rtx_scene_multi_hits, rtx_scene_primary_multi_hits, rtx_multi_hits).

The contract: ray i's list is every object of Scene.objects whose Object::distance passes closest_object's filter (scene.rs:249) and
lies before t_max[i], sorted by (distance, index) -- entry j is what closest_object returns once the winners of entries 0 .. j-1 have
been retained out of the scene (test_sorted_distance_lists_equal_repeated_closest_object_on_the_oracle pins that identity on the oracle
alone).  Every comparison is exact: bytes, or f64 bit patterns with every NaN made one pattern."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import DEFAULT_CAM, fuzz_rays, fuzz_scene, hip_scene, same
from test_any_hit_queries import HIT, incoherent_rays, ladder, run_any

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
MULTI_FNS = ("rtx_scene_multi_hits", "rtx_scene_primary_multi_hits", "rtx_multi_hits")
INF, NAN = np.inf, np.nan
TINY = np.finfo(np.float64).tiny
KMAX = 8                                     # the longest list the oracle fixtures keep


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


# ---------------------------------------------------------------------------------------------------------------- rays and scenes
def scene_box(objs):
    g = objs["geom"]
    pts = np.concatenate([np.zeros((0, 3)), g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3)])
    if not len(pts):
        pts = np.zeros((1, 3))
    return pts.min(axis=0), pts.max(axis=0)


def pierce_rays(rng, objs, n):
    """origins on the sphere of radius |box diagonal| around the box centre, each aimed at a uniform point of the box: rays that cross
    the whole scene (a box without extent: radius 1, aimed at the centre's neighbourhood)"""
    lo, hi = scene_box(objs)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o = c + u * (diag if diag > 0.0 else 1.0)
    target = lo + (hi - lo) * rng.random((n, 3)) if diag > 0.0 else c + 0.1 * rng.normal(size=(n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def dense_scene(name):
    from rust_raytracing_amd import scenes
    if name == "S":
        return scenes.compact(scenes.random_spheres(2000, 1))
    if name == "T":
        return scenes.compact(scenes.random_triangles(20000, 2))
    return np.concatenate([scenes.compact(scenes.random_spheres(1000, 4)), scenes.compact(scenes.random_triangles(10000, 5))])


def dense_rays(rtx, objs, half, seed=11):
    rng = np.random.default_rng(seed)
    oi, di = incoherent_rays(rng, objs, half)
    op, dp = pierce_rays(rng, objs, half)
    return np.concatenate([oi, op]), np.concatenate([di, dp])


def doubled(objs, seed):
    """every object twice, shuffled; returns (objects, twin): twin[i] = the index of object i's copy"""
    n = len(objs)
    perm = np.random.default_rng(seed).permutation(2 * n)
    both = np.concatenate([objs, objs])[perm]
    where = np.argsort(perm)                                        # where[j] = the new index of old entry j
    twin = np.empty(2 * n, dtype=np.int64)
    twin[where[:n]] = where[n:]
    twin[where[n:]] = where[:n]
    assert np.array_equal(both["geom"][twin], both["geom"])
    return both, twin


# ---------------------------------------------------------------------------------------------------------------- the oracle's lists
def _oracle_fns(oracle):
    L = oracle.lib()
    L.rtxo_object_distance.restype = C.c_int
    L.rtxo_object_distance.argtypes = [C.c_void_p, oracle.Vec3, oracle.Vec3, C.POINTER(C.c_double)]
    L.rtxo_object_normal_at.restype = oracle.Vec3
    L.rtxo_object_normal_at.argtypes = [C.c_void_p, oracle.Vec3]
    return L


def oracle_lists(oracle, objs, o, d):
    """per ray the (t, index) pairs of the objects whose Object::distance is normal and positive, sorted"""
    L = _oracle_fns(oracle)
    objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
    base, size, t = objs.ctypes.data, objs.itemsize, C.c_double()
    out = []
    for r in range(len(o)):
        po, di, ts = oracle.vec(o[r]), oracle.vec(d[r]), []
        for j in range(len(objs)):
            if L.rtxo_object_distance(base + j * size, po, di, C.byref(t)) and TINY <= t.value < INF:     # is_normal && is_sign_positive
                ts.append((t.value, j))
        ts.sort()                                                    # (t, index): min_by's first minimal element, applied repeatedly
        out.append(ts)
    return out


def expected_records(oracle, objs, o, d, lists, k, t_max=None):
    """(records (n, k) of HIT, counts (n,)) the contract asks for: position = o + d * t, multiply then add; the oracle's normal_at"""
    L = _oracle_fns(oracle)
    objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
    n = len(o)
    rec = np.zeros((n, k), dtype=HIT)
    rec["position"], rec["normal"], rec["distance"], rec["object"] = NAN, NAN, INF, -1
    cnt = np.zeros(n, dtype=np.uint32)
    for r in range(n):
        lim = INF if t_max is None else t_max[r]
        keep = [e for e in lists[r] if e[0] < lim][:k]               # (a NaN limit: nothing)
        cnt[r] = len(keep)
        for j, (t, idx) in enumerate(keep):
            p = o[r] + d[r] * t
            nrm = L.rtxo_object_normal_at(objs.ctypes.data + idx * objs.itemsize, oracle.vec(p)).tuple()
            rec[r, j] = (p, nrm, t, idx)
    return rec, cnt


def check_records(got, got_cnt, want, want_cnt, what):
    for f in ("distance", "object", "position", "normal"):
        if not same(got[f].astype(np.float64), want[f].astype(np.float64)):
            g, w = got[f].astype(np.float64).reshape(len(got), -1), want[f].astype(np.float64).reshape(len(want), -1)
            bad = np.nonzero(~(((g == w) | (np.isnan(g) & np.isnan(w))).all(axis=1)))[0]
            raise AssertionError("%s: %s differs on %d rays, first %s: got %r want %r" % (what, f, len(bad), bad[:5], got[f][bad[0]], want[f][bad[0]]))
    if got_cnt is not None:
        assert np.array_equal(got_cnt, want_cnt), (what, np.nonzero(got_cnt != want_cnt)[0][:5])
    # behind the count: the nothing record, bit for bit the closest-hit miss
    k = got.shape[1]
    tail = np.arange(k)[None, :] >= np.asarray(want_cnt)[:, None]
    assert (got["object"][tail] == -1).all() and np.isposinf(got["distance"][tail]).all(), what
    assert np.isnan(got["position"][tail]).all() and np.isnan(got["normal"][tail]).all(), what


@pytest.fixture(scope="module")
def fuzz_cases(rtx, oracle):
    """20 fuzzed scenes x (512 fuzz_rays + 128 pierce rays) with the oracle's lists: computed once, shared, never changed"""
    rng = np.random.default_rng(777)
    cases = []
    for s in range(20):
        objs, cam = fuzz_scene(rtx, rng)
        of, df = fuzz_rays(rng, objs, 512)
        op, dp = pierce_rays(rng, objs, 128)
        o, d = np.concatenate([of, op]), np.concatenate([df, dp])
        lists = oracle_lists(oracle, objs, o, d)
        rec, cnt = expected_records(oracle, objs, o, d, lists, KMAX)
        cases.append(dict(objs=objs, cam=cam, o=o, d=d, lists=lists, rec=rec, cnt=cnt))
    return cases


def run_multi(hnd, rays, t_max, k, torch, counts=True, **kw):
    """(records (n, k), counts (n,) or None, stats) of rtx_scene_multi_hits on device buffers; t_max None = a null d_t_max"""
    dev = torch.device("cuda", hnd.device)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_lim = torch.from_numpy(np.ascontiguousarray(t_max, dtype=np.float64)).to(dev) if t_max is not None else None
    d_hits = torch.full((max(n * k, 1) * 64,), 0x5A, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev) if counts else None
    torch.cuda.synchronize(dev)
    st = hnd.multi_hits(d_rays.data_ptr(), d_lim.data_ptr() if d_lim is not None else None, n, k, d_hits.data_ptr(),
                        d_cnt.data_ptr() if counts else None, **kw)
    rec = d_hits[:n * k * 64].cpu().numpy().view(HIT).reshape(n, k)
    return rec, (d_cnt[:n].cpu().numpy().view(np.uint32) if counts else None), st


def run_closest_records(hnd, rays, torch):
    dev = torch.device("cuda", hnd.device)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    hnd.closest_hits(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
    return d_hits.cpu().numpy().view(HIT)


def shares(cnt, k):
    cnt = np.asarray(cnt)
    return float((cnt == k).mean()), float(((cnt > 0) & (cnt < k)).mean()), float((cnt == 0).mean())


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_abi_and_libraries_carry_the_multi_hit_entry_points(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+RTX_MULTI_HIT_MAX\s+32\b", hdr) and rtx.abi.RTX_MULTI_HIT_MAX == 32
    for fn in MULTI_FNS:
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
        assert fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        for lab in (False, True):
            assert getattr(rtx.load_library(lab), fn) is not None, (fn, lab)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    names = kernel_instances.kernel_names(rtx.abi.LIB_PATH)
    assert len(names) <= 25, names                                      # the mode lives inside the two existing instances
    assert "query_closest_kernel<false>" in names and "query_closest_kernel<true>" in names, names
    rows = [r for r in kernel_instances.kernels(rtx.abi.LIB_PATH) if r["name"] == "query_closest_kernel<false>"]
    assert len(rows) == 1, rows
    print("query_closest_kernel<false>:", rows[0])
    assert rows[0]["vgpr_spill"] == 0 and rows[0]["vgpr"] <= 128, rows[0]


def test_multi_hit_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    bad, ok = rtx.abi.RTX_ERR_INVALID_ARGUMENT, rtx.abi.RTX_OK
    sc = rtx.abi.RtxScene()
    sc.config.rays_per_pixel = 1
    rays = rtx.make_rays(np.zeros((3, 3)), np.ones((3, 3)))
    hits = np.zeros((3, 4), dtype=HIT)
    cnt = np.zeros(3, dtype=np.uint32)
    assert lib.rtx_multi_hits(None, rays.ctypes.data, None, 3, 4, hits.ctypes.data, cnt.ctypes.data) == bad          # null scene
    assert lib.rtx_multi_hits(C.byref(sc), rays.ctypes.data, None, 3, 0, hits.ctypes.data, cnt.ctypes.data) == bad   # k = 0
    assert lib.rtx_multi_hits(C.byref(sc), rays.ctypes.data, None, 3, rtx.abi.RTX_MULTI_HIT_MAX + 1, hits.ctypes.data, None) == bad
    assert lib.rtx_multi_hits(C.byref(sc), rays.ctypes.data, None, 0, 0, hits.ctypes.data, None) == bad              # k is checked before n
    assert lib.rtx_multi_hits(C.byref(sc), None, None, 3, 4, hits.ctypes.data, None) == bad                          # null rays
    assert lib.rtx_multi_hits(C.byref(sc), rays.ctypes.data, None, 3, 4, None, cnt.ctypes.data) == bad               # null hits
    assert lib.rtx_multi_hits(C.byref(sc), None, None, 0, 4, None, None) == ok                                       # n = 0
    assert lib.rtx_multi_hits(C.byref(sc), None, None, 0, rtx.abi.RTX_MULTI_HIT_MAX, None, None) == ok
    assert lib.rtx_scene_multi_hits(None, None, None, 1, 1, None, None, None, None) == bad                           # null handle
    assert lib.rtx_scene_primary_multi_hits(None, 4, 4, 1, None, None, None, None) == bad


def test_sorted_distance_lists_equal_repeated_closest_object_on_the_oracle(rtx, oracle, fuzz_cases):
    """the identity the GPU tests lean on: the per-object Object::distance list, filtered and sorted by (t, index), is -- entry by
    entry -- closest_object applied again and again to the scene with the previous winners removed, and ends where it returns None"""
    from rust_raytracing_amd import scenes
    deep = tied = 0

    def check(objs, cam, o, d, lists, what):
        nonlocal deep, tied
        objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
        for r in range(len(o)):
            alive = np.arange(len(objs))
            for j in range(len(lists[r]) + 1):
                i, dist = oracle.closest_object(oracle.make_scene(objs[alive], cam), o[r], d[r])
                if j == len(lists[r]):
                    assert i == -1, (what, r, j)                             # the list is complete
                    break
                assert i >= 0 and (dist, int(alive[i])) == lists[r][j], (what, r, j, dist, lists[r][j])
                alive = np.delete(alive, i)
            deep += len(lists[r]) >= 3
            tied += sum(1 for a, b in zip(lists[r], lists[r][1:]) if a[0] == b[0])

    for s, c in enumerate(fuzz_cases):
        check(c["objs"], c["cam"], c["o"], c["d"], c["lists"], "fuzzed scene %d" % s)
    both, twin = doubled(np.concatenate([scenes.compact(scenes.random_spheres(60, 1)), scenes.compact(scenes.random_triangles(60, 2))]), 5)
    rng = np.random.default_rng(6)
    oi, di = incoherent_rays(rng, both, 300)
    op, dp = pierce_rays(rng, both, 300)
    g = both["geom"]                                                         # ... and rays through the centres of two objects each
    centres = np.where((both["kind"] == 0)[:, None], g[:, :3], g[:, :9].reshape(-1, 3, 3).mean(axis=1))
    a, b = centres[rng.integers(0, len(both), 600)], centres[rng.integers(0, len(both), 600)]
    line = np.linalg.norm(b - a, axis=1) > 1e-3
    dl = (b - a)[line] / np.linalg.norm(b - a, axis=1)[line, None]
    ol = a[line] - 3.0 * dl
    o, d = np.concatenate([oi, op, ol]), np.concatenate([di, dp, dl])
    lists = oracle_lists(oracle, both, o, d)
    for l in lists:                                                          # twins: equal distances, the lower index first
        for a, b in zip(l[0::2], l[1::2]):
            assert a[0] == b[0] and twin[a[1]] == b[1] and a[1] < b[1], (a, b)
    check(both, DEFAULT_CAM, o, d, lists, "doubled scene")
    print("rays with >= 3 entries: %d, tied pairs: %d" % (deep, tied))
    assert deep >= 500 and tied >= 100


def test_cpp_wrapper_with_the_multi_hit_methods_compiles(tmp_path):
    src = tmp_path / "multi.cpp"
    src.write_text('#include "rtx.hpp"\n'
                   "std::vector<RtxHit> f(const rtx::Scene &s, const std::vector<RtxRay> &r, std::vector<std::uint32_t> &c)\n"
                   "{ std::vector<RtxHit> a = s.multi_hits(r, 4); std::vector<RtxHit> b = s.multi_hits(r, 4, std::vector<double>(r.size(), 1.0), &c);\n"
                   "  a.insert(a.end(), b.begin(), b.end()); return a; }\n"
                   "void g(rtx::Scene::Resident &h, const RtxRay *r, const double *t, RtxHit *o, std::uint32_t *c, RtxStats *st)\n"
                   "{ h.multi_hits(r, t, 10, 4, o); h.multi_hits(r, nullptr, 10, 4, o, c, nullptr, st); h.primary_multi_hits(64, 40, 4, o);\n"
                   "  h.primary_multi_hits(64, 40, 4, o, c, nullptr, st); }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_multi_hits_equal_the_oracle_lists_on_fuzzed_scenes(gpu, fuzz_cases):
    import torch
    full = partial = walked = 0
    for s, c in enumerate(fuzz_cases):
        rays = gpu.make_rays(c["o"], c["d"])
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            scene = hip_scene(gpu, c["objs"], cam=c["cam"], kernel=kernel)
            hnd = scene.upload(0)
            closest = run_closest_records(hnd, rays, torch)
            for k in (1, 3, 8):
                want, want_cnt = c["rec"][:, :k], np.minimum(c["cnt"], k).astype(np.uint32)
                rec, cnt, st = run_multi(hnd, rays, None, k, torch)
                check_records(rec, cnt, want, want_cnt, "scene %d, kernel %d, k %d" % (s, kernel, k))
                assert st.segments == len(rays) and st.trace_launches == 1
                if kernel == gpu.RTX_KERNEL_AUTO and k == 8:
                    walked += st.kernel == gpu.RTX_KERNEL_BVH
                rec_nc, none, _ = run_multi(hnd, rays, None, k, torch, counts=False)        # d_counts = NULL
                assert none is None and rec_nc.tobytes() == rec.tobytes()
                if k == 1:
                    assert rec.tobytes() == closest.tobytes(), "scene %d, kernel %d: k = 1 is not closest_hits' record" % (s, kernel)
                if k == 8 and kernel == gpu.RTX_KERNEL_AUTO:                                 # the convenience form
                    qd, qo, qp, qn, qc = hnd.query_all(c["o"], c["d"], 8)
                    assert same(qd, rec["distance"]) and np.array_equal(qo, rec["object"]) and same(qp, rec["position"])
                    assert same(qn, rec["normal"]) and np.array_equal(qc, cnt)
                if k != 3 and s % 5:                # the host form uploads the scene again: k = 3 everywhere, every k on four scenes
                    continue
                hd, ho, hp, hn, hc = scene.multi_hits(c["o"], c["d"], k)                      # the host form
                host = np.zeros((len(rays), k), dtype=HIT)
                host["distance"], host["object"], host["position"], host["normal"] = hd, ho, hp, hn
                assert host.tobytes() == rec.tobytes() and np.array_equal(hc, cnt), "scene %d, kernel %d, k %d, host form" % (s, kernel, k)
            hnd.close()
        f, p, _ = shares(np.minimum(c["cnt"], 8), 8)
        full += f * len(rays)
        partial += p * len(rays)
    print("rays with a full list of 8: %d, a partial one: %d, scenes walked: %d" % (full, partial, walked))
    assert full >= 40 and partial >= 3000 and walked >= 6                   # (the oracle's own lists: 44 and 3705)


@pytest.mark.gpu
def test_limits_cut_the_list_to_the_prefix_below_them(gpu, oracle, fuzz_cases):
    import torch
    k = 4
    cut = 0
    for s, c in enumerate(fuzz_cases):
        rays = gpu.make_rays(c["o"], c["d"])
        n = len(rays)
        third = np.array([l[2][0] if len(l) >= 3 else (l[0][0] if l else INF) for l in c["lists"]])
        t_max = ladder(third)
        want, want_cnt = expected_records(oracle, c["objs"], c["o"], c["d"], c["lists"], k, t_max)
        cut += int((want_cnt < np.minimum(c["cnt"], k)).sum())
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            hnd = hip_scene(gpu, c["objs"], cam=c["cam"], kernel=kernel).upload(0)
            rec, cnt, _ = run_multi(hnd, rays, t_max, k, torch)
            check_records(rec, cnt, want, want_cnt, "scene %d, kernel %d" % (s, kernel))
            occ, _ = run_any(hnd, rays, t_max, torch)
            assert np.array_equal(cnt > 0, occ.astype(bool)), "scene %d, kernel %d: count > 0 is not any_hits" % (s, kernel)
            free, free_cnt, _ = run_multi(hnd, rays, None, k, torch)
            with np.errstate(invalid="ignore"):
                below = free["distance"] < t_max[:, None]
            assert np.array_equal(below.sum(axis=1), cnt)                          # the prefix of the unlimited list
            for j in range(k):
                assert rec[:, j][below[:, j]].tobytes() == free[:, j][below[:, j]].tobytes()
            for lim in (NAN, 0.0, -1.0):                                           # nothing is tested, nothing is reported
                rec0, cnt0, st0 = run_multi(hnd, rays, np.full(n, lim), k, torch)
                check_records(rec0, cnt0, _nothing(n, k), np.zeros(n, dtype=np.uint32),
                              "scene %d, kernel %d, limit %r" % (s, kernel, lim))
                assert st0.exact_tests == 0 and st0.box_tests == 0 and st0.segments == n
            hnd.close()
    print("rays whose list the limit cut short: %d" % cut)
    assert cut >= 300


def _nothing(n, k):
    rec = np.zeros((n, k), dtype=HIT)
    rec["position"], rec["normal"], rec["distance"], rec["object"] = NAN, NAN, INF, -1
    return rec


def _walk_equals_sweep(gpu, torch, auto, exact, rays, k, t_max=None):
    a, ca, sa = run_multi(auto, rays, t_max, k, torch)
    e, ce, se = run_multi(exact, rays, t_max, k, torch)
    assert sa.kernel == gpu.RTX_KERNEL_BVH and se.kernel == gpu.RTX_KERNEL_EXACT
    if a.tobytes() != e.tobytes():
        bad = np.nonzero((a.view(np.uint8).reshape(len(rays), -1) != e.view(np.uint8).reshape(len(rays), -1)).any(axis=1))[0]
        raise AssertionError("k %d: %d rays differ, first %s: walk %r sweep %r" % (k, len(bad), bad[:5], a[bad[0]], e[bad[0]]))
    assert ca.tobytes() == ce.tobytes()
    assert sa.exact_tests < se.exact_tests
    return a, ca, sa


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "T", "J"])
def test_multi_hit_walk_equals_the_exhaustive_sweep(gpu, name):
    import torch
    from rust_raytracing_amd import scenes
    objs = dense_scene(name)
    half = 1 << 13
    o, d = dense_rays(gpu, objs, half)
    rays = gpu.make_rays(o, d)
    auto = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    box = {}
    for k in (4, 16):
        rec, cnt, st = _walk_equals_sweep(gpu, torch, auto, exact, rays, k)
        box[k] = st.box_tests
        print("%s k %d: exact tests per ray %.2f, box tests per ray %.2f" % (name, k, st.exact_tests / len(rays), st.box_tests / len(rays)))
        d_ = rec["distance"]
        assert (d_[:, :-1] <= d_[:, 1:]).all()                                          # sorted (the nothing records' +inf last)
    _, cnt8, _ = run_multi(auto, rays, None, 8, torch)
    full, partial, empty = shares(cnt8, 8)
    print("%s k 8: full %.3f partial %.3f empty %.3f" % (name, full, partial, empty))
    assert full >= 0.20 and partial >= 0.15 and empty >= 0.02
    _, _, st1 = run_multi(auto, rays, None, 1, torch)
    print("%s box tests: k 1 %d, k 4 %d, k 16 %d" % (name, st1.box_tests, box[4], box[16]))
    assert st1.box_tests < box[16]
    _, _, st_near = run_multi(auto, rays, np.full(len(rays), 1e-3), 4, torch)
    print("%s box tests at k 4: t_max 1e-3 %d, +inf %d" % (name, st_near.box_tests, box[4]))
    assert st_near.box_tests < box[4]
    auto.close()
    exact.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "J"])
def test_multi_hits_after_moving_a_tenth_of_the_spheres(gpu, name):
    import torch
    from rust_raytracing_amd import scenes
    objs = dense_scene(name)
    o, d = dense_rays(gpu, objs, 1 << 13)
    rays = gpu.make_rays(o, d)
    rng = np.random.default_rng(21)
    sph = np.nonzero(objs["kind"] == 0)[0]
    idx = np.sort(rng.choice(sph, len(sph) // 10, replace=False))
    moved = objs.copy()
    moved["geom"][idx, :3] += rng.normal(size=(len(idx), 3)) * 0.3
    hnd = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    before, _, _ = run_multi(hnd, rays, None, 4, torch)
    how = hnd.update_objects(idx, moved[idx])
    fresh = hip_scene(gpu, moved, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, moved, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    rec, cnt, _ = _walk_equals_sweep(gpu, torch, hnd, exact, rays, 4)
    rec_f, cnt_f, _ = run_multi(fresh, rays, None, 4, torch)
    print("%s: update ran as %s; %d of %d lists changed" % (name, how, int((rec["object"] != before["object"]).any(axis=1).sum()), len(rays)))
    assert rec.tobytes() == rec_f.tobytes() and cnt.tobytes() == cnt_f.tobytes()
    assert rec.tobytes() != before.tobytes()
    for h in (hnd, fresh, exact):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "T"])
def test_ties_come_in_index_order(gpu, name):
    import torch
    from rust_raytracing_amd import scenes
    objs, twin = doubled(dense_scene(name), 31)
    o, d = dense_rays(gpu, objs, 1 << 12)
    rays = gpu.make_rays(o, d)
    auto = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    pairs = 0
    for k in (8, 7):
        rec, cnt, _ = _walk_equals_sweep(gpu, torch, auto, exact, rays, k)
        obj, dist = rec["object"], rec["distance"]
        for j in range(0, k - 1, 2):
            have = cnt >= j + 2                                                    # a full pair
            assert (dist[have, j] == dist[have, j + 1]).all() and (obj[have, j] < obj[have, j + 1]).all(), (k, j)
            assert np.array_equal(twin[obj[have, j]], obj[have, j + 1]), (k, j)
            pairs += int(have.sum())
        if k % 2:
            last = cnt == k                                                        # the odd entry: the lower index of its pair
            assert last.sum() > 100 and (obj[last, k - 1] < twin[obj[last, k - 1]]).all()
        assert (cnt[cnt < k] % 2 == 0).all()                                       # a list that ends before k holds whole pairs
    print("%s: %d full pairs" % (name, pairs))
    assert pairs >= 10000
    auto.close()
    exact.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "J"])
def test_entry_j_is_closest_hits_with_the_earlier_winners_hidden(gpu, name):
    import torch
    from rust_raytracing_amd import scenes
    objs = dense_scene(name)
    o, d = dense_rays(gpu, objs, 256, seed=5)
    hnd = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    dist, obj, pos, nrm, cnt = hnd.query_all(o, d, 4)
    pick = np.nonzero(cnt == 4)[0][:8]
    assert len(pick) == 8
    for r in pick:
        for j in range(4):
            if j:
                hnd.hide(obj[r, :j])
            cd, co, cp, cn = hnd.query(o[r:r + 1], d[r:r + 1])
            if j:
                ld, lo, _, _, lc = hnd.query_all(o[r:r + 1], d[r:r + 1], 4)          # hidden objects never appear in a list
                assert not np.isin(lo[0], obj[r, :j]).any() and same(ld[0, :4 - j], dist[r, j:]) and np.array_equal(lo[0, :4 - j], obj[r, j:])
                hnd.show(obj[r, :j])
            assert same(cd[0], dist[r, j]) and co[0] == obj[r, j] and same(cp[0], pos[r, j]) and same(cn[0], nrm[r, j]), (r, j)
    again = hnd.query_all(o, d, 4)
    assert same(again[0], dist) and np.array_equal(again[1], obj)                    # everything is shown again
    hnd.close()


@pytest.mark.gpu
def test_multi_hit_fallbacks_and_api_behaviour(gpu, fuzz_cases):
    import torch
    from rust_raytracing_amd import scenes
    dev = torch.device("cuda", 0)
    # a tiny scratch limit: the walk has no stack columns in memory, the rays whose stack overflows are swept -- the same bytes
    objs = dense_scene("J")
    o, d = dense_rays(gpu, objs, 1 << 12)
    rays = gpu.make_rays(o, d)
    n = len(rays)
    hnd = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    ref, ref_cnt, st = run_multi(hnd, rays, None, 8, torch)
    assert st.kernel == gpu.RTX_KERNEL_BVH and st.segments == n and st.trace_launches == 1 and st.trace_ms > 0.0
    assert st.box_tests > 0 and st.exact_tests > 0 and st.filter_tests > 0
    hnd.set_scratch_limit(1)
    small, small_cnt, _ = run_multi(hnd, rays, None, 8, torch)
    assert small.tobytes() == ref.tobytes() and small_cnt.tobytes() == ref_cnt.tobytes()
    hnd.set_scratch_limit(0)
    # stats == NULL: asynchronous on the caller's stream
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    outs = []
    for s in (s1, s2, s1):
        out, c = torch.full((n * 8 * 64,), 1, dtype=torch.uint8, device=dev), torch.full((n,), 9, dtype=torch.int32, device=dev)
        with torch.cuda.stream(s):
            assert hnd.multi_hits(d_rays.data_ptr(), None, n, 8, out.data_ptr(), c.data_ptr(), stream=s.cuda_stream, want_stats=False) is None
        outs.append((out, c))
    torch.cuda.synchronize(dev)
    for out, c in outs:
        assert out.cpu().numpy().tobytes() == ref.tobytes() and c.cpu().numpy().view(np.uint32).tobytes() == ref_cnt.tobytes()
    # k outside 1 .. RTX_MULTI_HIT_MAX, overlapping arrays: refused on a live handle, which stays good
    out, c = outs[0]
    for k in (0, gpu.abi.RTX_MULTI_HIT_MAX + 1):
        with pytest.raises(gpu.RtxError):
            hnd.multi_hits(d_rays.data_ptr(), None, n, k, out.data_ptr(), c.data_ptr())
        with pytest.raises(gpu.RtxError):
            hnd.primary_multi_hits(8, 8, k, out.data_ptr(), c.data_ptr())
    with pytest.raises(gpu.RtxError):
        hnd.multi_hits(d_rays.data_ptr(), None, n, 8, out.data_ptr(), out.data_ptr() + 64)
    top, top_cnt, _ = run_multi(hnd, rays, None, gpu.abi.RTX_MULTI_HIT_MAX, torch)
    assert top[:, :8].tobytes() == ref.tobytes() and np.array_equal(np.minimum(top_cnt, 8), ref_cnt)
    # n = 1 and n = 65: the bytes the same rays get inside the batch
    for m in (1, 65):
        for first in (0, 3000):
            part, part_cnt, st_m = run_multi(hnd, rays[first:first + m].copy(), None, 8, torch)
            assert part.tobytes() == ref[first:first + m].tobytes() and st_m.segments == m, (m, first)
    hnd.close()
    # a tuning bit of RTX_TUNE_LAB_MASK: refused by the product library
    lab_cfg = gpu.Config(rays_per_pixel=1, tuning=gpu.RTX_TUNE_NO_PACKETS)
    packed = np.ascontiguousarray(objs[:50], dtype=gpu.OBJECT_DTYPE)
    sc = gpu._scene_c(lab_cfg, gpu.Camera(*DEFAULT_CAM), packed)
    host = np.zeros((16, 2), dtype=HIT)
    assert gpu.load_library().rtx_multi_hits(C.byref(sc), rays[:16].ctypes.data, None, 16, 2, host.ctypes.data, None) == gpu.abi.RTX_ERR_UNSUPPORTED
    # the rays no walk takes -- non-unit and NaN directions, far origins: the fuzz set at k = 8, the walk's handle against the sweep's
    swept = 0
    for c in fuzz_cases[:8]:
        fr = gpu.make_rays(c["o"], c["d"])
        a = hip_scene(gpu, c["objs"], cam=c["cam"]).upload(0)
        e = hip_scene(gpu, c["objs"], cam=c["cam"], kernel=gpu.RTX_KERNEL_EXACT).upload(0)
        ra, ca, _ = run_multi(a, fr, None, 8, torch)
        re_, ce, _ = run_multi(e, fr, None, 8, torch)
        assert ra.tobytes() == re_.tobytes() and ca.tobytes() == ce.tobytes()
        unit = np.abs((c["d"] * c["d"]).sum(axis=1) - 1.0) <= 2.0 ** -40
        swept += int(((~unit | (np.abs(c["o"]).max(axis=1) > 1e5)) & (ca > 0)).sum())
        a.close()
        e.close()
    assert swept >= 100
    # an empty scene: the nothing records
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE))
    hnd = empty.upload(0)
    rec, cnt, st = run_multi(hnd, rays[:1000].copy(), None, 3, torch)
    check_records(rec, cnt, _nothing(1000, 3), np.zeros(1000, dtype=np.uint32), "empty scene")
    assert st.segments == 1000
    hnd.close()
    assert (empty.multi_hits(o[:10], d[:10], 2)[4] == 0).all()
    # k larger than the object count: every object a ray meets, then nothing
    few = scenes.compact(scenes.random_spheres(5, 3))
    of, df = pierce_rays(np.random.default_rng(2), few, 2000)
    hnd = hip_scene(gpu, few, rays_per_pixel=1).upload(0)
    d16, o16, _, _, c16 = hnd.query_all(of, df, 16)
    assert c16.max() <= 5 and c16.max() >= 2 and (o16[np.arange(16)[None, :] >= c16[:, None]] == -1).all()
    d1 = hnd.query(of, df)[0]
    assert same(d16[:, 0], d1)
    hnd.close()


@pytest.mark.gpu
def test_primary_multi_hits_are_the_pick_buffers_rays(gpu):
    import torch
    from rust_raytracing_amd import scenes
    objs = dense_scene("J")
    w, h = 64, 40
    dev = torch.device("cuda", 0)

    def run(hnd, k):
        d_hits = torch.full((w * h * k * 64,), 3, dtype=torch.uint8, device=dev)
        d_cnt = torch.full((w * h,), 5, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        st = hnd.primary_multi_hits(w, h, k, d_hits.data_ptr(), d_cnt.data_ptr())
        return d_hits.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint32), st

    auto = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    d_pick = torch.empty(w * h * 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    auto.primary_hits(w, h, d_pick.data_ptr())
    one, cnt1, st = run(auto, 1)
    assert one.tobytes() == d_pick.cpu().numpy().tobytes() and st.segments == w * h and st.kernel == gpu.RTX_KERNEL_BVH
    assert np.array_equal(cnt1, (one.view(HIT)["object"] >= 0).astype(np.uint32)) and 0 < cnt1.sum()
    a4, ca4, _ = run(auto, 4)
    e4, ce4, se = run(exact, 4)
    assert a4.tobytes() == e4.tobytes() and ca4.tobytes() == ce4.tobytes() and se.kernel == gpu.RTX_KERNEL_EXACT
    assert (ca4 == 4).sum() > 100
    dist, obj, pos, nrm, cnt = auto.pick_through(w, h, 4)
    pd, po, pp, pn = auto.pick(w, h)
    assert dist.shape == (h, w, 4) and obj.shape == (h, w, 4) and pos.shape == (h, w, 4, 3) and nrm.shape == (h, w, 4, 3) and cnt.shape == (h, w)
    assert same(dist[:, :, 0], pd) and np.array_equal(obj[:, :, 0], po) and same(pos[:, :, 0], pp) and same(nrm[:, :, 0], pn)
    assert np.array_equal(cnt.reshape(-1), ca4) and dist.tobytes() == a4.view(HIT)["distance"].tobytes()
    assert not np.array_equal(po, po[::-1]) and not np.array_equal(po, po[:, ::-1])      # (an image with an orientation to get wrong)
    auto.close()
    exact.close()
