"""Batched closest-hit ray queries and the pick buffer (rtx_scene_closest_hits, rtx_scene_primary_hits, rtx_closest_hits).

Every GPU comparison is bit for bit on the raw f64 patterns (NaN matches NaN): a query answers exactly what the reference's
closest_object (scene.rs:243-251) returns, with scene.rs:234's hit point and object.rs:37-39's normal there."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from helpers import DEFAULT_CAM, check_equal, fuzz_rays, fuzz_scene, hip_scene, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
QUERY_FNS = ("rtx_scene_closest_hits", "rtx_scene_primary_hits", "rtx_closest_hits")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def oracle_answers(oracle, objs, sc, origins, dirs):
    """(distance, object, position, normal) of closest_object on the libm oracle + normal_at of the winner"""
    L = oracle.lib()
    L.rtxo_object_normal_at.restype = oracle.Vec3
    L.rtxo_object_normal_at.argtypes = [C.c_void_p, oracle.Vec3]
    objs = np.ascontiguousarray(objs, dtype=oracle.OBJECT_DTYPE)
    n = len(origins)
    dist = np.full(n, np.inf)
    obj = np.full(n, -1, dtype=np.int64)
    pos = np.full((n, 3), np.nan)
    nrm = np.full((n, 3), np.nan)
    for k in range(n):
        i, d = oracle.closest_object(sc, origins[k], dirs[k])
        if i < 0:
            continue
        dist[k], obj[k] = d, i
        p = origins[k] + dirs[k] * d                                       # scene.rs:234 (no fused multiply-add either side)
        pos[k] = p
        nrm[k] = L.rtxo_object_normal_at(objs.ctypes.data + i * objs.itemsize, oracle.vec(p)).tuple()
    return dist, obj, pos, nrm


def incoherent_rays(rng, objs, n):
    g = objs["geom"]
    allp = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3)])
    lo, hi = allp.min(axis=0), allp.max(axis=0)
    o = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d


def run_query(hnd, rays, torch):
    dev = torch.device("cuda", hnd.device)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    st = hnd.closest_hits(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
    return d_hits.cpu().numpy().view(HIT), st


HIT = np.dtype([("position", "<f8", (3,)), ("normal", "<f8", (3,)), ("distance", "<f8"), ("object", "<i8")])


def split(h):
    return h["distance"], h["object"], h["position"], h["normal"]


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_the_query_abi(rtx, tmp_path):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for fn in QUERY_FNS:
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
        assert fn in [s[0] for s in rtx.abi.SYMBOLS], fn
    for st in ("RtxRay", "RtxHit"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{.*?\}\s*%s\s*;" % (st, st), hdr, flags=re.S), st
    src = tmp_path / "q.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtx_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(RtxRay), offsetof(RtxRay, direction), sizeof(RtxHit), offsetof(RtxHit, normal), offsetof(RtxHit, distance),'
                   'offsetof(RtxHit, object));return 0;}\n')
    exe = tmp_path / "q"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    a = rtx.abi
    assert got == [48, 24, 64, 24, 48, 56]
    assert got == [C.sizeof(a.RtxRay), a.RtxRay.direction.offset, C.sizeof(a.RtxHit), a.RtxHit.normal.offset,
                   a.RtxHit.distance.offset, a.RtxHit.object.offset]
    assert a.RAY_DTYPE.itemsize == 48 and a.HIT_DTYPE.itemsize == 64 and a.HIT_DTYPE.fields["object"][1] == 56


def test_product_library_holds_the_query_kernel(rtx):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    names = kernel_instances.kernel_names(rtx.abi.LIB_PATH)
    assert any(n.startswith("query_closest_kernel") for n in names), names
    assert len(names) <= 25, names


def test_host_form_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    assert lib.rtx_closest_hits(None, None, 5, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    sc = rtx.abi.RtxScene()
    sc.config.rays_per_pixel = 1
    assert lib.rtx_closest_hits(C.byref(sc), None, 0, None) == rtx.abi.RTX_OK
    assert lib.rtx_closest_hits(C.byref(sc), None, 3, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert lib.rtx_scene_closest_hits(None, None, 1, None, None, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert lib.rtx_scene_primary_hits(None, 4, 4, None, None, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_queries_equal_the_oracle_on_fuzzed_scenes(gpu, oracle):
    rng = np.random.default_rng(2024)
    kinds, walked = 0, 0
    for s in range(150):
        objs, cam = fuzz_scene(gpu, rng)
        o, d = fuzz_rays(rng, objs, 2048)
        sc = oracle.make_scene(objs, cam)
        want = oracle_answers(oracle, objs, sc, o, d)
        scene = hip_scene(gpu, objs, cam=cam)
        got = scene.closest_hits(o, d)                                  # the host form (device 0)
        check_equal(got, want, "scene %d, host form" % s)
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel).upload(0)
            check_equal(hnd.query(o, d), want, "scene %d, kernel %d" % (s, kernel))
            if kernel == gpu.RTX_KERNEL_AUTO:
                import torch
                _, st = run_query(hnd, gpu.make_rays(o, d), torch)
                walked += st.kernel == gpu.RTX_KERNEL_BVH
            hnd.close()
        kinds += int((want[1] >= 0).sum())
    assert kinds > 50000 and walked > 50


@pytest.mark.gpu
def test_queries_replay_the_render_transcripts(gpu):
    """every segment the exhaustive kernel's paths asked closest_object about -- bounced rays that start on the surface they
    left included -- asked again through the query on a product handle: the same distance and object"""
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
        hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)
        dist, obj, _, _ = hnd.query(steps["position"], steps["direction"])
        hnd.close()
        assert same(dist, steps["distance"]) and np.array_equal(obj, steps["object"]), name
        self_hits += int((steps["distance"] < 1e-9).sum())
        assert len(steps) > 1000, name
    assert self_hits > 0


def _bench_like(name):
    from rust_raytracing_amd import scenes
    if name == "C2":
        return scenes.random_spheres(10000, 1, box=1.0)
    if name == "C3":
        return scenes.random_triangles(100000, 2, box=1.0)
    return np.concatenate([scenes.random_spheres(5000, 4, box=1.0), scenes.random_triangles(50000, 5, box=1.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C2", "C3", "J1"])
def test_tree_walk_equals_the_exhaustive_sweep(gpu, oracle, name):
    import torch
    from rust_raytracing_amd import scenes
    objs = _bench_like(name)
    rng = np.random.default_rng(7)
    o, d = incoherent_rays(rng, objs, 1 << 20)
    rays = gpu.make_rays(o, d)
    auto = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, cam=scenes.CAMERA, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    a, sa = run_query(auto, rays, torch)
    e, se = run_query(exact, rays, torch)
    assert sa.kernel == gpu.RTX_KERNEL_BVH and se.kernel == gpu.RTX_KERNEL_EXACT
    assert sa.exact_tests * 20 < se.exact_tests
    assert a.tobytes() == e.tobytes()
    assert (a["object"] >= 0).sum() > 1000
    sub = rng.choice(len(rays), 2000, replace=False)
    sc = oracle.make_scene(objs, scenes.CAMERA)
    check_equal(split(a[sub]), oracle_answers(oracle, objs, sc, o[sub], d[sub]), name)
    if name == "C3":                                                  # the 1080p view of the scene: the pick buffers agree
        pa = auto.pick(1920, 1080)
        pe = exact.pick(1920, 1080)
        for x, y in zip(pa, pe):
            assert same(x, y)
        assert (pa[1] >= 0).sum() > 10000
    auto.close()
    exact.close()


@pytest.mark.gpu
def test_pick_buffer_equals_the_oracle_and_the_render(gpu, oracle):
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(60, 50, 2, seed=21)
    w, h = 64, 48
    cfg = dict(rays_per_pixel=1, seed=3)
    hnd = hip_scene(gpu, objs, **cfg).upload(0)
    got = hnd.pick(w, h)
    sc = oracle.make_scene(objs, DEFAULT_CAM, **cfg)
    L = oracle.lib()
    p = np.array(DEFAULT_CAM[0], dtype=np.float64)
    vfov = float(h) / float(w) * DEFAULT_CAM[2]                                # scene.rs:145
    o, d = np.zeros((h * w, 3)), np.zeros((h * w, 3))
    for y in range(h):
        for x in range(w):
            rd = np.array(L.rtxo_get_ray_dir(C.byref(sc), float(x) / float(w), float(y) / float(h), vfov).tuple())
            focal = p + rd * 10.0                                              # scene.rs:203, focal_length 10
            o[y * w + x] = p
            d[y * w + x] = L.rtxo_norm(oracle.vec(focal - p)).tuple()          # scene.rs:205-207 without the offsets
    want = oracle_answers(oracle, objs, sc, o, d)
    check_equal(tuple(a.reshape(h * w, *a.shape[2:]) for a in got), want, "pick buffer")
    assert (want[1] >= 0).sum() > 200
    # both offsets 0: the render's primary ray and its hit are step 0 of the transcript
    lab = hip_scene(gpu, objs, kernel=gpu.RTX_KERNEL_EXACT, focal_offset=0.0, non_focal_offset=0.0, **cfg).upload(0, lab=True)
    for y in range(h):
        st, _ = lab.debug_paths(w, h, y, 1)
        s0 = st[:, 0, 0]
        assert same(s0["distance"], got[0][y]) and np.array_equal(s0["object"], got[1][y]), y
        assert same(s0["direction"], d[y * w:(y + 1) * w])
    lab.close()
    # ... and the answer does not depend on the seed or the offsets
    hnd.set_config(gpu.Config(rays_per_pixel=1, seed=99, focal_offset=0.3, non_focal_offset=0.7))
    for x, y in zip(hnd.pick(w, h), got):
        assert same(x, y)
    hnd.close()


@pytest.mark.gpu
def test_pick_buffer_orientation(gpu):
    """scene.rs:145,153-157,213-221 alone, no oracle: +y of camera space is image row y > h/2, +x column x > w/2, the centre pixel
    looks along camera.direction"""
    w, h = 64, 48
    cam = gpu.Camera((1.0, -2.0, 0.5), (0.8, 0.3, -0.1), 1.2)
    a = 0.25

    def one_sphere(cam_dir=None, r=0.4, dist=10.0):
        """a sphere of radius r at distance dist along camera-space cam_dir (None: along camera.direction itself)"""
        o = np.zeros(1, dtype=gpu.OBJECT_DTYPE)
        wd = np.array(list(cam.rotate_to_world_space(cam_dir) if cam_dir is not None else cam.get_direction()))
        o[0]["geom"][:4] = (*(np.array(list(cam.position)) + wd / np.linalg.norm(wd) * dist), r)
        return gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), cam, o).upload(0)

    hnd = one_sphere((0.0, math.sin(a), math.cos(a)))
    obj = hnd.pick(w, h)[1]
    ys, xs = np.nonzero(obj >= 0)
    assert len(ys) > 0 and ys.min() > h // 2
    hnd.close()
    hnd = one_sphere((math.sin(a), 0.0, math.cos(a)))
    obj = hnd.pick(w, h)[1]
    ys, xs = np.nonzero(obj >= 0)
    assert len(xs) > 0 and xs.min() > w // 2
    hnd.close()
    r = 0.5
    hnd = one_sphere(None, r=r)
    dist, obj, _, _ = hnd.pick(w, h)
    assert obj[h // 2, w // 2] == 0
    assert abs(dist[h // 2, w // 2] - (10.0 - r)) <= 1e-12
    hnd.close()


@pytest.mark.gpu
def test_query_api_behaviour(gpu):
    import torch
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(300, 300, 1, seed=9)
    rng = np.random.default_rng(3)
    o, d = incoherent_rays(rng, objs, 1 << 16)
    rays = gpu.make_rays(o, d)
    hnd = hip_scene(gpu, objs, rays_per_pixel=2).upload(0)
    ref, st = run_query(hnd, rays, torch)
    # stats as documented
    assert st.segments == len(rays) and st.trace_launches == 1 and st.trace_ms > 0.0 and st.primary_rays == 0
    assert st.kernel == gpu.RTX_KERNEL_BVH and st.box_tests > 0 and st.exact_tests > 0
    ex = hip_scene(gpu, objs, rays_per_pixel=2, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    e, se = run_query(ex, rays, torch)
    assert se.kernel == gpu.RTX_KERNEL_EXACT and se.exact_tests == len(rays) * len(objs) and se.box_tests == 0
    assert e.tobytes() == ref.tobytes()
    ex.close()
    # stats == NULL: asynchronous on the caller's stream
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    outs = []
    img_ref = torch.empty(32 * 24 * 3, dtype=torch.float64, device=dev)
    hnd.render_rows(32, 24, 0, 1, 24, img_ref.data_ptr())
    img_ref = img_ref.cpu().numpy()
    for k, s in enumerate((s1, s2, s1, s2)):          # one handle, two streams, renders and queries in turn
        hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
        img = torch.empty(32 * 24 * 3, dtype=torch.float64, device=dev)
        with torch.cuda.stream(s):
            hnd.closest_hits(d_rays.data_ptr(), len(rays), hits.data_ptr(), stream=s.cuda_stream, want_stats=False)
            hnd.render_rows(32, 24, 0, 1, 24, img.data_ptr(), stream=s.cuda_stream, want_stats=False)
        outs.append((hits, img))
    torch.cuda.synchronize(dev)
    for hits, img in outs:
        assert hits.cpu().numpy().tobytes() == ref.tobytes()
        assert img.cpu().numpy().tobytes() == img_ref.tobytes()
    hnd.close()
    # an empty scene hits nothing
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE)).upload(0)
    dist, obj, pos, nrm = empty.query(o[:1000], d[:1000])
    assert (obj == -1).all() and np.isinf(dist).all() and np.isnan(pos).all() and np.isnan(nrm).all()
    dist, obj, _, _ = empty.pick(16, 8)
    assert (obj == -1).all() and np.isposinf(dist).all()
    empty.close()
    # a stack limited by the scratch cap: the same bits (the rays whose stack would spill are swept)
    deep = hip_scene(gpu, scenes.random_triangles(20000, 3), rays_per_pixel=1).upload(0)
    o2, d2 = incoherent_rays(rng, scenes.random_triangles(20000, 3), 1 << 14)
    want = deep.query(o2, d2)
    deep.set_scratch_limit(1)
    for x, y in zip(deep.query(o2, d2), want):
        assert same(x, y)
    deep.close()
