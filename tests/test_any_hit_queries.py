"""Occlusion (any-hit) ray queries with a per-ray distance limit (rtx_scene_any_hits, rtx_any_hits).

The contract: occluded[i] = 1 iff some object's Object::distance is normal, positive (scene.rs:249's filter) and < t_max[i].  A minimum
is below a bound iff some element is, so this is (rtx_scene_closest_hits' distance < t_max[i]) -- the yardstick of every GPU test
here, itself pinned on the oracle alone by test_any_equals_closest_below_the_limit_on_the_oracle.  Every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from helpers import DEFAULT_CAM, fuzz_rays, fuzz_scene, hip_scene, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
ANY_FNS = ("rtx_scene_any_hits", "rtx_any_hits")
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def ladder(d):
    """the t_max of each ray, by its closest distance d (+inf: a miss), cycled by ray index"""
    d = np.asarray(d, dtype=np.float64)
    i = np.arange(len(d))
    with np.errstate(invalid="ignore", over="ignore"):
        hit = np.stack([np.full(len(d), INF), d, np.nextafter(d, INF), np.nextafter(d, 0.0), d / 2, 2 * d, np.zeros(len(d)),
                        np.full(len(d), -1.0), np.full(len(d), NAN)])
    miss = np.array([INF, 1e30, 1.0, NAN])
    return np.where(np.isfinite(d), hit[i % 9, i], miss[i % 4])


def expect(d, t_max):
    with np.errstate(invalid="ignore"):
        return np.asarray(d) < np.asarray(t_max)                             # (NaN limit: False)


def incoherent_rays(rng, objs, n):                                           # (tests/test_ray_queries.py's recipe)
    g = objs["geom"]
    allp = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3)])
    lo, hi = allp.min(axis=0), allp.max(axis=0)
    o = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d


def aimed_rays(rng, objs, n):
    """the same kind of origin; the direction points at a random sphere centre or triangle centroid"""
    g = objs["geom"]
    allp = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3)])
    lo, hi = allp.min(axis=0), allp.max(axis=0)
    o = lo + (hi - lo) * rng.random((n, 3))
    targets = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3, 3).mean(axis=1)])
    d = targets[rng.integers(0, len(targets), n)] - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d


def run_any(hnd, rays, t_max, torch, **kw):
    """(n bytes, stats) of rtx_scene_any_hits on device buffers; t_max None = a null d_t_max"""
    dev = torch.device("cuda", hnd.device)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_lim = torch.from_numpy(np.ascontiguousarray(t_max, dtype=np.float64)).to(dev) if t_max is not None else None
    d_out = torch.full((len(rays),), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    st = hnd.any_hits(d_rays.data_ptr(), d_lim.data_ptr() if d_lim is not None else None, len(rays), d_out.data_ptr(), **kw)
    return d_out.cpu().numpy(), st


def run_closest(hnd, rays, torch):
    dev = torch.device("cuda", hnd.device)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    st = hnd.closest_hits(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
    return d_hits.cpu().numpy().view(HIT)["distance"].copy(), st


HIT = np.dtype([("position", "<f8", (3,)), ("normal", "<f8", (3,)), ("distance", "<f8"), ("object", "<i8")])


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_abi_and_libraries_carry_the_any_hit_entry_points(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in ANY_FNS:
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
        assert fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        for lab in (False, True):
            assert getattr(rtx.load_library(lab), fn) is not None, (fn, lab)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    names = kernel_instances.kernel_names(rtx.abi.LIB_PATH)
    assert len(names) <= 25, names                                      # the mode lives inside the two existing instances
    assert "query_closest_kernel<false>" in names and "query_closest_kernel<true>" in names, names


def test_sphere_query_kernel_keeps_its_walk_out_of_scratch(rtx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    rows = [r for r in kernel_instances.kernels(rtx.abi.LIB_PATH) if r["name"] == "query_closest_kernel<false>"]
    assert len(rows) == 1, rows
    print("query_closest_kernel<false>:", rows[0])
    assert rows[0]["vgpr_spill"] == 0, rows[0]


def test_host_form_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    bad, ok = rtx.abi.RTX_ERR_INVALID_ARGUMENT, rtx.abi.RTX_OK
    assert lib.rtx_any_hits(None, None, None, 5, None) == bad
    sc = rtx.abi.RtxScene()
    sc.config.rays_per_pixel = 1
    assert lib.rtx_any_hits(C.byref(sc), None, None, 0, None) == ok
    rays = rtx.make_rays(np.zeros((3, 3)), np.ones((3, 3)))
    out = np.zeros(3, dtype=np.uint8)
    assert lib.rtx_any_hits(C.byref(sc), None, None, 3, out.ctypes.data) == bad
    assert lib.rtx_any_hits(C.byref(sc), rays.ctypes.data, None, 3, None) == bad
    assert lib.rtx_scene_any_hits(None, None, None, 1, None, None, None) == bad


def test_any_equals_closest_below_the_limit_on_the_oracle(rtx, oracle):
    """the identity the GPU tests lean on, without the min-fold: any(t normal, positive, < t_max) over a per-object loop of
    Object::distance == (closest_object's distance < t_max), on every rung of the ladder for every ray"""
    L = oracle.lib()
    L.rtxo_object_distance.restype = C.c_int
    L.rtxo_object_distance.argtypes = [C.c_void_p, oracle.Vec3, oracle.Vec3, C.POINTER(C.c_double)]
    rng = np.random.default_rng(4242)
    tiny = np.finfo(np.float64).tiny
    n_hit = 0
    for s in range(40):
        objs, cam = fuzz_scene(rtx, rng)
        o, d = fuzz_rays(rng, objs, 256)
        objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
        sc = oracle.make_scene(objs, cam)
        t = C.c_double()
        for k in range(len(o)):
            po, di = oracle.vec(o[k]), oracle.vec(d[k])
            ts = []
            for j in range(len(objs)):
                if L.rtxo_object_distance(objs.ctypes.data + j * objs.itemsize, po, di, C.byref(t)):
                    ts.append(t.value)
            ts = np.array(ts, dtype=np.float64)
            ts = ts[np.isfinite(ts) & (ts >= tiny)]                            # is_normal && is_sign_positive
            i, dist = oracle.closest_object(sc, o[k], d[k])
            dist = dist if i >= 0 else INF
            n_hit += i >= 0
            if i >= 0:
                rungs = [INF, dist, np.nextafter(dist, INF), np.nextafter(dist, 0.0), dist / 2, 2 * dist, 0.0, -1.0, NAN]
            else:
                rungs = [INF, 1e30, 1.0, NAN]
            for t_max in rungs:
                assert bool((ts < t_max).any()) == bool(dist < t_max), (s, k, t_max, dist)
    assert n_hit > 2000


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_any_hits_equal_closest_hits_and_the_oracle_on_fuzzed_scenes(gpu, oracle):
    import torch
    rng = np.random.default_rng(4242)
    hits = unit_hits = walked = 0
    for s in range(40):
        objs, cam = fuzz_scene(gpu, rng)
        o, d = fuzz_rays(rng, objs, 1024)
        rays = gpu.make_rays(o, d)
        sc = oracle.make_scene(objs, cam)
        oracle_hit = np.array([oracle.closest_object(sc, o[k], d[k])[0] >= 0 for k in range(len(o))])
        auto = hip_scene(gpu, objs, cam=cam).upload(0)
        dist, _ = run_closest(auto, rays, torch)
        t_max = ladder(dist)
        want = expect(dist, t_max)
        assert np.array_equal(np.isfinite(dist), oracle_hit), s
        got = hip_scene(gpu, objs, cam=cam).any_hits(o, d, t_max)             # the host form (device 0)
        assert got.dtype == bool and np.array_equal(got, want), "scene %d, host form" % s
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            hnd = auto if kernel == gpu.RTX_KERNEL_AUTO else hip_scene(gpu, objs, cam=cam, kernel=kernel).upload(0)
            b, st = run_any(hnd, rays, t_max, torch)
            assert np.array_equal(b, want.astype(np.uint8)), "scene %d, kernel %d: %s" % (s, kernel, np.nonzero(b != want)[0][:5])
            assert st.segments == len(rays)
            if kernel == gpu.RTX_KERNEL_AUTO:
                walked += st.kernel == gpu.RTX_KERNEL_BVH
            # the +inf rung: the oracle itself; a null d_t_max is the all-+inf array
            b_inf, _ = run_any(hnd, rays, np.full(len(rays), INF), torch)
            b_null, _ = run_any(hnd, rays, None, torch)
            assert np.array_equal(b_inf, oracle_hit.astype(np.uint8)), "scene %d, kernel %d, +inf" % (s, kernel)
            assert np.array_equal(b_null, b_inf), "scene %d, kernel %d, null limits" % (s, kernel)
            assert np.array_equal(hnd.occluded(o, d, t_max), want) and np.array_equal(hnd.occluded(o, d), oracle_hit)
            hnd.close()
        hits += int(oracle_hit.sum())
        unit_hits += int((oracle_hit & (np.abs((d * d).sum(axis=1) - 1.0) <= 2.0 ** -40)).sum())
    print("hits %d, with unit directions %d, scenes walked %d" % (hits, unit_hits, walked))
    assert hits >= 10000 and unit_hits >= 5000 and walked > 20


def _deep_scene(name):
    from rust_raytracing_amd import scenes
    if name == "S":
        return scenes.random_spheres(2000, 1, box=1.0)
    if name == "T":
        return scenes.random_triangles(20000, 2, box=1.0)
    return np.concatenate([scenes.random_spheres(1000, 4, box=1.0), scenes.random_triangles(10000, 5, box=1.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "T", "J"])
def test_any_hit_walk_equals_the_exhaustive_sweep(gpu, name):
    import torch
    from rust_raytracing_amd import scenes
    objs = _deep_scene(name)
    rng = np.random.default_rng(11)
    half = 1 << 15
    oi, di = incoherent_rays(rng, objs, half)
    oa, da = aimed_rays(rng, objs, half)
    rays = gpu.make_rays(np.concatenate([oi, oa]), np.concatenate([di, da]))
    auto = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    dist, _ = run_closest(auto, rays, torch)
    t_max = ladder(dist)
    want = expect(dist, t_max).astype(np.uint8)
    a, sa = run_any(auto, rays, t_max, torch)
    e, se = run_any(exact, rays, t_max, torch)
    assert sa.kernel == gpu.RTX_KERNEL_BVH and se.kernel == gpu.RTX_KERNEL_EXACT
    assert np.array_equal(a, want), np.nonzero(a != want)[0][:5]
    assert a.tobytes() == e.tobytes()
    print("%s: occluded %d of %d, exact tests AUTO %d EXACT %d" % (name, int(want.sum()), len(want), sa.exact_tests, se.exact_tests))
    assert int(want.sum()) >= 2000 and int((want == 0).sum()) >= 2000
    assert sa.exact_tests * 20 <= se.exact_tests
    # retirement: toward a target, the first certain hit ends the walk the closest-hit query has to finish
    aimed = rays[half:]
    _, sc = run_closest(auto, aimed, torch)
    _, sn = run_any(auto, aimed, np.full(half, INF), torch)
    print("%s: aimed half, box tests any %d closest %d" % (name, sn.box_tests, sc.box_tests))
    assert sn.box_tests < sc.box_tests
    # pruning by the limit: nothing that starts behind it is entered
    _, s_inf = run_any(auto, rays[:half], np.full(half, INF), torch)
    _, s_near = run_any(auto, rays[:half], np.full(half, 1e-3), torch)
    print("%s: incoherent half, box tests t_max 1e-3 %d, +inf %d" % (name, s_near.box_tests, s_inf.box_tests))
    assert s_near.box_tests < s_inf.box_tests
    auto.close()
    exact.close()


@pytest.mark.gpu
def test_any_hits_on_the_render_transcripts(gpu):
    """every segment of the exhaustive kernel's paths -- bounced rays that start on the surface they left included: occluded just
    past its recorded distance, not at it; a segment that ends its path on a miss is not occluded at all"""
    from rust_raytracing_amd import scenes
    cases = [("mixed", scenes.mixed_scene(60, 50, 2, seed=21), 64, 40, DEFAULT_CAM, dict(rays_per_pixel=4, seed=3)),
             ("mesh", scenes.light_every(scenes.compact(scenes.random_triangles(3000, 5)), 3), 48, 32, DEFAULT_CAM, dict(rays_per_pixel=3, seed=8)),
             ("joint", np.concatenate([scenes.light_every(scenes.compact(scenes.random_spheres(400, 4))),
                                       scenes.light_every(scenes.compact(scenes.random_triangles(2000, 6)))]), 48, 32, DEFAULT_CAM,
              dict(rays_per_pixel=3, seed=5)),
             ("axis-aligned mesh", scenes.axis_aligned_mesh(), 64, 36, ((11.0, 0.2, 0.1), (0.3, 1.0, 0.2), 1.4), dict(rays_per_pixel=2, seed=42))]
    self_hits = 0
    for name, objs, w, h, cam, cfg in cases:
        lab = hip_scene(gpu, objs, cam=cam, kernel=gpu.RTX_KERNEL_EXACT, **cfg).upload(0, lab=True)
        steps = []
        for row in range(0, h, 3):
            st, cnt = lab.debug_paths(w, h, row, 12)
            k = np.minimum(cnt, 12)
            mask = np.arange(12)[None, None, :] < k[:, :, None]
            steps.append(st[mask])
        lab.close()
        steps = np.concatenate(steps)
        assert len(steps) > 1000, name
        hit = steps["object"] >= 0
        dist = steps["distance"]
        assert np.isfinite(dist[hit]).all() and hit.sum() > 0 and (~hit).sum() > 0, name
        hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)
        p, d = steps["position"], steps["direction"]
        past = hnd.occluded(p[hit], d[hit], np.nextafter(dist[hit], INF))
        at = hnd.occluded(p[hit], d[hit], dist[hit])
        free = hnd.occluded(p[~hit], d[~hit], INF)
        hnd.close()
        assert past.all(), (name, np.nonzero(~past)[0][:5])
        assert not at.any(), (name, np.nonzero(at)[0][:5])
        assert not free.any(), (name, np.nonzero(free)[0][:5])
        self_hits += int((dist[hit] < 1e-9).sum())
    assert self_hits > 0


@pytest.mark.gpu
def test_any_hit_api_behaviour(gpu):
    import torch
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(300, 300, 1, seed=9)
    rng = np.random.default_rng(3)
    n = 1 << 14
    o, d = incoherent_rays(rng, objs, n)
    rays = gpu.make_rays(o, d)
    hnd = hip_scene(gpu, objs, rays_per_pixel=2).upload(0)
    dist, _ = run_closest(hnd, rays, torch)
    t_max = ladder(dist)
    want = expect(dist, t_max).astype(np.uint8)
    ref, st = run_any(hnd, rays, t_max, torch)
    assert np.array_equal(ref, want) and 0 < want.sum() < n
    assert st.segments == n and st.trace_launches == 1 and st.trace_ms > 0.0 and st.primary_rays == 0
    assert st.kernel == gpu.RTX_KERNEL_BVH and st.box_tests > 0 and st.exact_tests > 0
    # stats == NULL: asynchronous on the caller's stream; a second stream works
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_lim = torch.from_numpy(t_max).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    outs = []
    for s in (s1, s2, s1, s2):
        out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(s):
            assert hnd.any_hits(d_rays.data_ptr(), d_lim.data_ptr(), n, out.data_ptr(), stream=s.cuda_stream, want_stats=False) is None
        outs.append(out)
    torch.cuda.synchronize(dev)
    for out in outs:
        assert out.cpu().numpy().tobytes() == ref.tobytes()
    # any two of the three arrays overlapping: refused
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    for args in ((d_rays.data_ptr(), d_lim.data_ptr(), d_rays.data_ptr() + 48 * (n - 1)),           # output inside the rays
                 (d_rays.data_ptr(), d_lim.data_ptr(), d_lim.data_ptr() + 8 * n - 1),               # output inside the limits
                 (d_rays.data_ptr(), d_rays.data_ptr() + 48, out.data_ptr())):                      # limits inside the rays
        with pytest.raises(gpu.RtxError):
            hnd.any_hits(args[0], args[1], n, args[2])
    assert np.array_equal(run_any(hnd, rays, t_max, torch)[0], ref)                                 # (the handle is still good)
    # a tuning bit of RTX_TUNE_LAB_MASK: refused by the product library
    lab_cfg = gpu.Config(rays_per_pixel=1, tuning=gpu.RTX_TUNE_NO_PACKETS)
    assert gpu.RTX_TUNE_NO_PACKETS & gpu.abi.RTX_TUNE_LAB_MASK
    packed = np.ascontiguousarray(objs, dtype=gpu.OBJECT_DTYPE)
    sc = gpu._scene_c(lab_cfg, gpu.Camera(*DEFAULT_CAM), packed)
    host_out = np.zeros(16, dtype=np.uint8)
    assert gpu.load_library().rtx_any_hits(C.byref(sc), rays[:16].ctypes.data, None, 16, host_out.ctypes.data) == gpu.abi.RTX_ERR_UNSUPPORTED
    c = lab_cfg.to_c()
    assert hnd._lib.rtx_scene_set_config(hnd._h, C.byref(c)) == gpu.abi.RTX_ERR_UNSUPPORTED
    assert np.array_equal(run_any(hnd, rays, t_max, torch)[0], ref)
    # n = 1 and n = 65 (a partial wave, the lane 63 / 64 boundary): the bytes the same rays get inside the batch
    for k in (1, 65):
        for first in (0, 1000):
            b, st_k = run_any(hnd, rays[first:first + k].copy(), t_max[first:first + k].copy(), torch)
            assert np.array_equal(b, ref[first:first + k]) and st_k.segments == k, (k, first)
    # append_objects: a sphere across a free ray's path
    free = int(np.nonzero(~np.isfinite(dist))[0][0])
    one = gpu.make_rays(o[free:free + 1], d[free:free + 1])
    assert run_any(hnd, one, None, torch)[0].tolist() == [0]
    ball = np.zeros(1, dtype=gpu.OBJECT_DTYPE)
    ball[0]["kind"] = 0
    ball[0]["geom"][:4] = (*(o[free] + 5.0 * d[free]), 1.0)
    hnd.append_objects(ball)
    assert run_any(hnd, one, None, torch)[0].tolist() == [1]
    assert run_any(hnd, one, np.array([3.5]), torch)[0].tolist() == [0]              # (the sphere starts at t = 4)
    dist2, _ = run_closest(hnd, rays, torch)
    ref2, _ = run_any(hnd, rays, t_max, torch)
    assert np.array_equal(ref2, expect(dist2, t_max).astype(np.uint8))
    # set_config(kernel=EXACT): the same bytes, reported as EXACT
    hnd.set_config(gpu.Config(rays_per_pixel=2, kernel=gpu.RTX_KERNEL_EXACT))
    b, st = run_any(hnd, rays, t_max, torch)
    assert st.kernel == gpu.RTX_KERNEL_EXACT and st.box_tests == 0 and np.array_equal(b, ref2)
    hnd.close()
    # an empty scene: all zeros, whatever the limit
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE)).upload(0)
    b, st = run_any(empty, rays[:1000].copy(), None, torch)
    assert not b.any() and st.segments == 1000
    assert not empty.occluded(o[:1000], d[:1000], t_max[:1000]).any()
    empty.close()
    assert not gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM),
                                     np.zeros(0, dtype=gpu.OBJECT_DTYPE)).any_hits(o[:100], d[:100]).any()
