"""Path-radiance ray queries (rtx_scene_trace_paths, rtx_trace_paths): render_ray (scene.rs:223-242) for the caller's rays.

The contract: entry i starts a path at its ray (direction as given), resulting_color = 0, light_color = 1; up to max_bounces + 1
times: stop if light_color == zeros, closest_object (None: stop), position += direction * dst, ray_hit; bounce b draws indices
6 + 2b and 7 + 2b of the key rng_key(seed, ids[i]) -- the render's own draws, so render_pixel's ray for (pixel, sample) gives that
sample of the render.  The yardstick of the GPU tests is oracle_render_ray below, a per-ray loop over the oracle's closest_object /
normal_at / random_bounce_dir / RNG, itself pinned on the oracle's transcripts and pixels by the CPU test.  Every comparison is exact."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from helpers import DEFAULT_CAM, bits, fuzz_rays, fuzz_scene, hip_scene, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
RUST_SHIM = os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")
PATH_FNS = ("rtx_scene_trace_paths", "rtx_trace_paths")
INF = np.inf


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


# ------------------------------------------------------------------------------------------------------------ the yardstick
def oracle_render_ray(oracle, sc, pos, direction, pixel, sample):
    """render_ray from (pos, direction) on the oracle's scene sc, with the draws of (pixel, sample) -> (rgb, steps); steps: one
    (position, direction, distance, object) per closest_object call (a miss: inf, -1)"""
    L = oracle.lib()
    L.rtxo_object_normal_at.restype = oracle.Vec3
    L.rtxo_object_normal_at.argtypes = [C.c_void_p, oracle.Vec3]
    objs = sc._keepalive
    key = L.rtxo_rng_key(int(sc.config.seed), int(pixel), int(sample))
    pos = [float(v) for v in pos]
    d = [float(v) for v in direction]
    result, light, steps = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], []
    for b in range(int(sc.config.max_bounces) + 1):                              # scene.rs:227
        if light[0] == 0.0 and light[1] == 0.0 and light[2] == 0.0:             # scene.rs:228
            break
        i, dst = oracle.closest_object(sc, pos, d)                               # scene.rs:232
        steps.append((tuple(pos), tuple(d), dst if i >= 0 else INF, i))
        if i < 0:
            break
        pos = [pos[k] + d[k] * dst for k in range(3)]                            # scene.rs:234
        o = objs[i]
        normal = L.rtxo_object_normal_at(objs.ctypes.data + i * objs.itemsize, oracle.vec(pos))
        u_z, u_theta = L.rtxo_rng_u01(key, 6 + 2 * b), L.rtxo_rng_u01(key, 7 + 2 * b)
        d = list(L.rtxo_random_bounce_dir(oracle.vec(d), normal, float(o["roughness"]), u_z, u_theta).tuple())     # scene.rs:275
        em, base = o["emission_color"], o["base_color"]
        result = [result[k] + light[k] * float(em[k]) for k in range(3)]        # scene.rs:276
        light = [light[k] * float(base[k]) for k in range(3)]                   # scene.rs:277
    return result, steps


def oracle_paths(oracle, sc, o, d, ids=None):
    """(rgb (n, 3), segments (n,)) of oracle_render_ray over a batch; ids None = (i, 0)"""
    rgb = np.zeros((len(o), 3), dtype=np.float64)
    seg = np.zeros(len(o), dtype=np.uint32)
    for k in range(len(o)):
        pix, smp = (k, 0) if ids is None else ids[k]
        rgb[k], steps = oracle_render_ray(oracle, sc, o[k], d[k], pix, smp)
        seg[k] = len(steps)
    return rgb, seg


def fold(samples):
    """iter_ops.rs:4-8 / scene.rs:253-259: the left fold from zeros in sample order, divided by the count; samples [s][...][3]"""
    acc = np.zeros(samples.shape[1:], dtype=np.float64)
    for s in range(samples.shape[0]):
        acc = acc + samples[s]
    return acc / float(samples.shape[0])


def run_paths(hnd, rays, ids, torch, want_segments=True, **kw):
    """(rgb (n, 3), segments (n,) or None, stats) of rtx_scene_trace_paths on device buffers; ids None = a null d_ids"""
    dev = torch.device("cuda", hnd.device)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint64).view(np.int64)).to(dev) if ids is not None else None
    d_rgb = torch.full((max(n, 1) * 3,), float("nan"), dtype=torch.float64, device=dev)
    d_seg = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev) if want_segments else None
    torch.cuda.synchronize(dev)
    st = hnd.trace_paths(d_rays.data_ptr(), d_ids.data_ptr() if d_ids is not None else None, n, d_rgb.data_ptr(),
                         d_seg.data_ptr() if d_seg is not None else None, **kw)
    torch.cuda.synchronize(dev)
    seg = d_seg[:n].cpu().numpy().view(np.uint32) if d_seg is not None else None
    return d_rgb[:3 * n].cpu().numpy().reshape(n, 3), seg, st


def incoherent_rays(rng, objs, n):                                           # (tests/test_any_hit_queries.py's recipe)
    from test_any_hit_queries import incoherent_rays as recipe
    return recipe(rng, objs, n)


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_abi_libraries_and_rust_shim_carry_the_path_entry_points(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    shim = open(RUST_SHIM).read()
    for fn in PATH_FNS:
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
        assert fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        assert re.search(r"\bpub fn %s\s*\(" % fn, shim), fn
        for lab in (False, True):
            assert getattr(rtx.load_library(lab), fn) is not None, (fn, lab)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    rows = kernel_instances.kernels(rtx.abi.LIB_PATH)
    names = sorted(r["name"] for r in rows)
    assert len(names) <= 25, names                                      # the mode lives inside the two existing instances
    assert "query_closest_kernel<false>" in names and "query_closest_kernel<true>" in names, names
    sph = [r for r in rows if r["name"] == "query_closest_kernel<false>"]
    assert len(sph) == 1, sph
    print("query_closest_kernel<false>:", sph[0])
    assert sph[0]["vgpr_spill"] == 0 and sph[0]["vgpr"] <= 128, sph[0]     # (4 workgroups of 256 per CU: 128 VGPRs)


def test_host_form_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    bad, ok = rtx.abi.RTX_ERR_INVALID_ARGUMENT, rtx.abi.RTX_OK
    assert lib.rtx_trace_paths(None, None, None, 5, None, None) == bad
    sc = rtx.abi.RtxScene()
    sc.config.rays_per_pixel = 1
    assert lib.rtx_trace_paths(C.byref(sc), None, None, 0, None, None) == ok
    rays = rtx.make_rays(np.zeros((3, 3)), np.ones((3, 3)))
    rgb = np.zeros(9, dtype=np.float64)
    assert lib.rtx_trace_paths(C.byref(sc), None, None, 3, rgb.ctypes.data, None) == bad
    assert lib.rtx_trace_paths(C.byref(sc), rays.ctypes.data, None, 3, None, None) == bad
    for n in ((1 << 32) - 1, 1 << 32, 1 << 40):
        assert lib.rtx_trace_paths(C.byref(sc), rays.ctypes.data, None, n, rgb.ctypes.data, None) == bad, n
    assert lib.rtx_scene_trace_paths(None, None, None, 1, None, None, None, None) == bad


def test_the_yardstick_reproduces_the_oracles_transcripts_and_pixels(rtx, oracle):
    """oracle_render_ray, started from segment 0 of each of rtxo_trace_row's transcripts with the ids (pixel, sample), walks the
    same steps, makes the same number of closest_object calls and -- folded over the samples in order -- gives rtxo_render's pixel.
    (Computed when this test was written: 896 paths, 75 with light, 100 of more than two segments.)"""
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(60, 50, 2, seed=21)
    w, h, spp = 32, 20, 4
    sc = oracle.make_scene(objs, DEFAULT_CAM, rays_per_pixel=spp, seed=3)
    img = oracle.render(sc, w, h)
    paths = lit = long_ = 0
    for row in range(0, h, 3):
        steps, counts = oracle.trace_row(sc, w, h, row, 12)
        rgb = np.zeros((spp, w, 3), dtype=np.float64)
        for x in range(w):
            for s in range(spp):
                first = steps[x, s, 0]
                rgb[s, x], mine = oracle_render_ray(oracle, sc, first["position"], first["direction"], row * w + x, s)
                assert len(mine) == counts[x, s], (row, x, s)
                for k, (p, d, dst, obj) in enumerate(mine):
                    t = steps[x, s, k]
                    assert same(p, t["position"]) and same(d, t["direction"]) and same(dst, t["distance"]) and obj == t["object"], (row, x, s, k)
                paths += 1
                lit += bool(rgb[s, x].any())
                long_ += len(mine) > 2
        assert same(fold(rgb), img[row]), row
    print("paths %d, with light %d, of more than two segments %d" % (paths, lit, long_))
    assert paths == 896 and lit >= 50 and long_ >= 50


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_paths_equal_the_yardstick_on_fuzzed_scenes(gpu, oracle):
    import torch
    rng = np.random.default_rng(4242)
    import time
    lit = long_ = hit = walked = 0
    longest = 0
    t_oracle = 0.0
    for s in range(40):
        objs, cam = fuzz_scene(gpu, rng)
        o, d = fuzz_rays(rng, objs, 1024)
        rays = gpu.make_rays(o, d)
        sc = oracle.make_scene(objs, cam)
        t0 = time.perf_counter()
        with oracle.device_sincos():
            want_rgb, want_seg = oracle_paths(oracle, sc, o, d)
        t_oracle += time.perf_counter() - t0
        hnd = hip_scene(gpu, objs, cam=cam).upload(0)
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            if kernel == gpu.RTX_KERNEL_EXACT:
                hnd.set_config(gpu.Config(kernel=kernel))
            rgb, seg, st = run_paths(hnd, rays, None, torch)
            bad = np.nonzero((bits(rgb) != bits(want_rgb)).any(axis=1))[0]
            assert same(rgb, want_rgb), "scene %d, kernel %d: rays %s" % (s, kernel, bad[:5])
            assert np.array_equal(seg, want_seg), "scene %d, kernel %d: %s" % (s, kernel, np.nonzero(seg != want_seg)[0][:5])
            assert st.segments == int(want_seg.sum()) and st.primary_rays == len(rays)
            if kernel == gpu.RTX_KERNEL_AUTO:
                walked += st.kernel == gpu.RTX_KERNEL_BVH
                assert same(hnd.radiance(o, d), want_rgb), "scene %d, radiance()" % s
            else:
                assert st.kernel == gpu.RTX_KERNEL_EXACT and st.box_tests == 0
        hnd.close()
        h_rgb, h_seg = hip_scene(gpu, objs, cam=cam).trace_paths(o, d)           # the host form (device 0)
        assert same(h_rgb, want_rgb) and np.array_equal(h_seg, want_seg), "scene %d, host form" % s
        lit += int(want_rgb.any(axis=1).sum())
        long_ += int((want_seg > 2).sum())
        hit += int((want_seg > 1).sum())
        longest = max(longest, int(want_seg.max()))
    print("non-zero radiance %d, more than two segments %d, more than one %d, longest %d, scenes walked %d; the yardstick took %.1f s"
          % (lit, long_, hit, longest, walked, t_oracle))
    assert lit >= 4000 and long_ >= 3000 and longest == 11 and walked > 20


RENDER_CASES = ("mixed", "mesh", "joint", "axis-aligned mesh")


def _render_case(name):
    """the cases of test_any_hits_on_the_render_transcripts: (objects, width, height, camera, config)"""
    from rust_raytracing_amd import scenes
    if name == "mixed":
        return scenes.mixed_scene(60, 50, 2, seed=21), 64, 40, DEFAULT_CAM, dict(rays_per_pixel=4, seed=3)
    if name == "mesh":
        return scenes.light_every(scenes.compact(scenes.random_triangles(3000, 5)), 3), 48, 32, DEFAULT_CAM, dict(rays_per_pixel=3, seed=8)
    if name == "joint":
        return (np.concatenate([scenes.light_every(scenes.compact(scenes.random_spheres(400, 4))),
                                scenes.light_every(scenes.compact(scenes.random_triangles(2000, 6)))]), 48, 32, DEFAULT_CAM,
                dict(rays_per_pixel=3, seed=5))
    return scenes.axis_aligned_mesh(), 64, 36, ((11.0, 0.2, 0.1), (0.3, 1.0, 0.2), 1.4), dict(rays_per_pixel=2, seed=42)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RENDER_CASES)
def test_the_renders_own_rays_give_the_renders_samples(gpu, name):
    """no oracle: the first ray of every path of the exhaustive render kernel's transcripts, with ids (pixel, sample), gives the
    transcript's segment count, the colour a plain replay of the transcript over the materials gives, and -- folded over the samples
    in order -- the row of Scene.render"""
    import torch
    objs, w, h, cam, cfg = _render_case(name)
    spp = cfg["rays_per_pixel"]
    lab = hip_scene(gpu, objs, cam=cam, kernel=gpu.RTX_KERNEL_EXACT, **cfg).upload(0, lab=True)
    rows = list(range(0, h, 3))
    first, counts, replay = [], [], []
    em, base = objs["emission_color"], objs["base_color"]
    for row in rows:
        st, cnt = lab.debug_paths(w, h, row, 12)
        assert cnt.max() <= 11
        first.append(st[:, :, 0])
        counts.append(cnt)
        col = np.zeros((w, spp, 3), dtype=np.float64)
        for x in range(w):
            for s in range(spp):
                result, light = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
                for k in range(int(cnt[x, s])):
                    obj = int(st[x, s, k]["object"])
                    if obj < 0:
                        break
                    result = [result[c] + light[c] * float(em[obj][c]) for c in range(3)]
                    light = [light[c] * float(base[obj][c]) for c in range(3)]
                col[x, s] = result
        replay.append(col)
    lab.close()
    first, counts, replay = np.stack(first), np.stack(counts), np.stack(replay)          # [row][x][s]
    pix = (np.array(rows)[:, None, None] * w + np.arange(w)[None, :, None]) * np.ones((1, 1, spp), dtype=np.int64)
    smp = np.broadcast_to(np.arange(spp)[None, None, :], pix.shape)
    ids = np.stack([pix.ravel(), smp.ravel()], axis=1).astype(np.uint64)
    rays = gpu.make_rays(first["position"].reshape(-1, 3), first["direction"].reshape(-1, 3))
    hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)
    rgb, seg, st = run_paths(hnd, rays, ids, torch)
    hnd.close()
    assert np.array_equal(seg, counts.ravel()), (name, np.nonzero(seg != counts.ravel())[0][:5])
    assert st.segments == int(counts.sum())
    assert same(rgb, replay.reshape(-1, 3)), name
    assert rgb.any() and (seg > 2).any(), name
    img = hip_scene(gpu, objs, cam=cam, **cfg).render(w, h)
    folded = fold(np.moveaxis(rgb.reshape(len(rows), w, spp, 3), 2, 0))                 # [s][row][x][3] -> [row][x][3]
    assert same(folded, img[rows]), name


def _deep_scene(name):
    from rust_raytracing_amd import scenes
    if name == "S":
        objs = scenes.random_spheres(2000, 1)
    elif name == "T":
        objs = scenes.random_triangles(20000, 2)
    else:
        objs = np.concatenate([scenes.random_spheres(1000, 4), scenes.random_triangles(10000, 5)])
    return scenes.light_every(scenes.compact(objs), 4)


def _deep_rays(gpu, hnd, objs):
    """2^14 incoherent rays, then the 128 x 128 zero-offset primary rays (directions from pick()'s hit points; a miss has none: NaN)"""
    n = 1 << 14
    o, d = incoherent_rays(np.random.default_rng(11), objs, n)
    _, _, pos, _ = hnd.pick(128, 128)
    cam = np.array(DEFAULT_CAM[0])
    pd = pos.reshape(-1, 3) - cam
    with np.errstate(invalid="ignore"):
        pd = pd / np.linalg.norm(pd, axis=1)[:, None]
    return np.concatenate([o, np.broadcast_to(cam, pd.shape)]), np.concatenate([d, pd]), n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S", "T", "J"])
def test_path_walk_equals_the_exhaustive_sweep_on_deep_trees(gpu, name):
    import torch
    objs = _deep_scene(name)
    auto = hip_scene(gpu, objs, rays_per_pixel=1).upload(0)
    exact = hip_scene(gpu, objs, rays_per_pixel=1, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    o, d, n = _deep_rays(gpu, auto, objs)
    rays = gpu.make_rays(o, d)
    a_rgb, a_seg, sa = run_paths(auto, rays, None, torch)
    e_rgb, e_seg, se = run_paths(exact, rays, None, torch)
    auto.close()
    exact.close()
    assert sa.kernel == gpu.RTX_KERNEL_BVH and se.kernel == gpu.RTX_KERNEL_EXACT
    assert a_rgb.tobytes() == e_rgb.tobytes() and a_seg.tobytes() == e_seg.tobytes()
    assert sa.segments == se.segments == int(a_seg.sum())
    lit, long_ = int(a_rgb[:n].any(axis=1).sum()), int((a_seg[:n] > 2).sum())
    print("%s: incoherent half: non-zero radiance %d, more than two segments %d of %d; segments %d; exact tests AUTO %d EXACT %d"
          % (name, lit, long_, n, sa.segments, sa.exact_tests, se.exact_tests))
    assert sa.exact_tests * 20 <= se.exact_tests
    assert lit >= n // 4 and long_ >= n // 4


@pytest.mark.gpu
def test_a_path_does_not_depend_on_its_place_in_the_batch(gpu):
    """the refill: lanes take new rays whenever their path ends, so which wave and lane a path runs on depends on its neighbours --
    its answer must not"""
    import torch
    objs = _deep_scene("J")
    hnd = hip_scene(gpu, objs, rays_per_pixel=1).upload(0)
    o, d, _ = _deep_rays(gpu, hnd, objs)
    rays = gpu.make_rays(o, d)
    n = len(rays)
    ids = np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.uint64)
    rgb, seg, _ = run_paths(hnd, rays, ids, torch)
    assert rgb.any() and (seg > 2).sum() > n // 8
    # d_ids == NULL is (i, 0)
    r0, s0, _ = run_paths(hnd, rays, None, torch)
    assert r0.tobytes() == rgb.tobytes() and s0.tobytes() == seg.tobytes()
    # a permutation of the entries with their ids permutes the answers and nothing else
    perm = np.random.default_rng(5).permutation(n)
    rp, sp, _ = run_paths(hnd, rays[perm].copy(), ids[perm].copy(), torch)
    assert rp.tobytes() == rgb[perm].tobytes() and sp.tobytes() == seg[perm].tobytes()
    # n = 1, n = 65 (the lane 63 / 64 boundary) and a slice, with their original ids: the bytes they got inside the batch
    for first, k in ((0, 1), (1000, 1), (0, 65), (4321, 65), (7000, 1000)):
        rk, sk, st = run_paths(hnd, rays[first:first + k].copy(), ids[first:first + k].copy(), torch)
        assert rk.tobytes() == rgb[first:first + k].tobytes() and sk.tobytes() == seg[first:first + k].tobytes(), (first, k)
        assert st.segments == int(seg[first:first + k].sum()) and st.primary_rays == k
    # without the segment counts: the same colours
    rn, sn, _ = run_paths(hnd, rays, ids, torch, want_segments=False)
    assert sn is None and rn.tobytes() == rgb.tobytes()
    hnd.close()


@pytest.mark.gpu
def test_one_segment_paths_are_the_emission_of_the_closest_hit(gpu):
    import torch
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(300, 300, 1, seed=9)
    n = 1 << 14
    o, d = incoherent_rays(np.random.default_rng(3), objs, n)
    rays = gpu.make_rays(o, d)
    hnd = hip_scene(gpu, objs, rays_per_pixel=1, max_bounces=0).upload(0)
    _, obj, _, _ = hnd.query(o, d)
    want = np.where((obj >= 0)[:, None], objs["emission_color"][np.maximum(obj, 0)], 0.0)
    rgb, seg, st = run_paths(hnd, rays, None, torch)
    assert same(rgb, want) and (seg == 1).all() and st.segments == n
    assert 0 < (obj >= 0).sum() < n and want.any()
    # max_bounces = 10: a path that hit a non-light goes on; one that hit a light or nothing is what it was
    hnd.set_config(gpu.Config(rays_per_pixel=1, max_bounces=10))
    rgb10, seg10, _ = run_paths(hnd, rays, None, torch)
    hnd.close()
    ends = (obj < 0) | ~objs["base_color"][np.maximum(obj, 0)].any(axis=1)
    assert same(rgb10[ends], want[ends]) and (seg10[ends] == 1).all()
    assert (seg10[~ends] >= 2).all() and (~ends).sum() > 1000
    changed = ~np.all(rgb10 == want, axis=1)
    assert changed[~ends].sum() > 100 and not changed[ends].any()


@pytest.mark.gpu
def test_path_api_behaviour(gpu):
    import torch
    from rust_raytracing_amd import scenes
    objs = scenes.mixed_scene(300, 300, 1, seed=9)
    n = 1 << 14
    o, d = incoherent_rays(np.random.default_rng(3), objs, n)
    rays = gpu.make_rays(o, d)
    hnd = hip_scene(gpu, objs, rays_per_pixel=2).upload(0)
    ref, ref_seg, st = run_paths(hnd, rays, None, torch)
    assert ref.any() and not np.isnan(ref).any()
    assert st.primary_rays == n and st.segments == int(ref_seg.sum()) and st.trace_launches == 1 and st.trace_ms > 0.0
    assert st.kernel == gpu.RTX_KERNEL_BVH and st.box_tests > 0 and st.exact_tests > 0 and st.filter_tests > 0
    # stats == NULL: asynchronous on the caller's stream; a second stream works
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
    d_ids = torch.from_numpy(np.stack([np.arange(n), np.zeros(n)], axis=1).astype(np.int64)).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    outs = []
    for s in (s1, s2, s1, s2):
        out = torch.full((3 * n,), float("nan"), dtype=torch.float64, device=dev)
        cnt = torch.full((n,), 77, dtype=torch.int32, device=dev)
        with torch.cuda.stream(s):
            assert hnd.trace_paths(d_rays.data_ptr(), d_ids.data_ptr(), n, out.data_ptr(), cnt.data_ptr(), stream=s.cuda_stream,
                                   want_stats=False) is None
        outs.append((out, cnt))
    torch.cuda.synchronize(dev)
    for out, cnt in outs:
        assert out.cpu().numpy().tobytes() == ref.tobytes() and cnt.cpu().numpy().tobytes() == ref_seg.tobytes()
    # any two of the four arrays overlapping: refused
    out = torch.empty(3 * n, dtype=torch.float64, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    R, I, O, S = d_rays.data_ptr(), d_ids.data_ptr(), out.data_ptr(), cnt.data_ptr()
    for args in ((R, I, R + 48 * (n - 1), S),          # rgb inside the rays
                 (R, R + 48, O, S),                    # ids inside the rays
                 (R, I, O, R + 4),                     # segments inside the rays
                 (R, I, I + 16 * n - 8, S),            # rgb inside the ids
                 (R, I, O, I + 16 * n - 4),            # segments inside the ids
                 (R, I, O, O + 24 * n - 4),            # segments inside the rgb
                 (R, None, O, O),                      # the same, without ids
                 (R, None, R, None)):                  # rgb on the rays, nothing optional
        with pytest.raises(gpu.RtxError):
            hnd.trace_paths(args[0], args[1], n, args[2], args[3])
    assert run_paths(hnd, rays, None, torch)[0].tobytes() == ref.tobytes()                          # (the handle is still good)
    # a tuning bit of RTX_TUNE_LAB_MASK: refused by the product library
    lab_cfg = gpu.Config(rays_per_pixel=1, tuning=gpu.RTX_TUNE_NO_PACKETS)
    assert gpu.RTX_TUNE_NO_PACKETS & gpu.abi.RTX_TUNE_LAB_MASK
    packed = np.ascontiguousarray(objs, dtype=gpu.OBJECT_DTYPE)
    sc = gpu._scene_c(lab_cfg, gpu.Camera(*DEFAULT_CAM), packed)
    host_out = np.zeros(48, dtype=np.float64)
    assert gpu.load_library().rtx_trace_paths(C.byref(sc), rays[:16].ctypes.data, None, 16, host_out.ctypes.data, None) == gpu.abi.RTX_ERR_UNSUPPORTED
    c = lab_cfg.to_c()
    assert hnd._lib.rtx_scene_set_config(hnd._h, C.byref(c)) == gpu.abi.RTX_ERR_UNSUPPORTED
    assert run_paths(hnd, rays, None, torch)[0].tobytes() == ref.tobytes()
    # the seed keys the bounces: another seed, other colours on paths that bounce; the same seed again, the same bytes
    hnd.set_config(gpu.Config(rays_per_pixel=2, seed=7))
    other = run_paths(hnd, rays, None, torch)[0]
    assert other.tobytes() != ref.tobytes() and same(other[ref_seg == 1], ref[ref_seg == 1])
    hnd.set_config(gpu.Config(rays_per_pixel=2))
    assert run_paths(hnd, rays, None, torch)[0].tobytes() == ref.tobytes()
    # radiance(samples=S): ids (i, s), folded in order
    few = slice(0, 512)
    per = np.stack([run_paths(hnd, rays[few].copy(), np.stack([np.arange(512), np.full(512, s)], axis=1), torch)[0] for s in range(3)])
    assert same(hnd.radiance(o[few], d[few], samples=3), fold(per)) and same(per[0], ref[few])
    # append_objects: a light across a free ray's path makes its radiance that light's emission
    free = int(np.nonzero(ref_seg == 1)[0][np.nonzero(~ref[ref_seg == 1].any(axis=1))[0][0]])
    _, obj, _, _ = hnd.query(o[free:free + 1], d[free:free + 1])
    assert obj[0] == -1
    one = gpu.make_rays(o[free:free + 1], d[free:free + 1])
    lamp = np.zeros(1, dtype=gpu.OBJECT_DTYPE)
    lamp[0]["kind"] = 0
    lamp[0]["geom"][:4] = (*(o[free] + 5.0 * d[free]), 1.0)
    lamp[0]["emission_color"] = (1.5, 0.25, 3.0)
    lamp[0]["roughness"] = 1.0
    hnd.append_objects(lamp)
    r1, s1_, _ = run_paths(hnd, one, None, torch)
    assert same(r1[0], [1.5, 0.25, 3.0]) and s1_.tolist() == [1]
    ref2, seg2, _ = run_paths(hnd, rays, None, torch)
    # set_config(kernel=EXACT): the same bytes, reported as EXACT
    hnd.set_config(gpu.Config(rays_per_pixel=2, kernel=gpu.RTX_KERNEL_EXACT))
    b, bs, st = run_paths(hnd, rays, None, torch)
    assert st.kernel == gpu.RTX_KERNEL_EXACT and st.box_tests == 0 and b.tobytes() == ref2.tobytes() and bs.tobytes() == seg2.tobytes()
    hnd.close()
    # an empty scene: zeros, no closest_object call, no launch
    nothing = np.zeros(0, dtype=gpu.OBJECT_DTYPE)
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), nothing).upload(0)
    b, bs, st = run_paths(empty, rays[:1000].copy(), None, torch)
    assert not b.any() and not np.isnan(b).any() and not bs.any()
    assert st.segments == 0 and st.trace_launches == 0 and st.primary_rays == 1000
    assert not empty.radiance(o[:100], d[:100]).any()
    empty.close()
    h_rgb, h_seg = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), nothing).trace_paths(o[:100], d[:100])
    assert not h_rgb.any() and not h_seg.any()


@pytest.mark.gpu
def test_the_panorama_example_is_radiance_over_its_own_rays(gpu, tmp_path):
    """examples/panorama.cpp (Resident::trace_paths of rtx.hpp): its equirectangular frame equals SceneHandle.radiance over the same
    rays, ids (pixel, sample), folded over the samples"""
    import math
    import subprocess
    exe = os.path.join(ROOT, "examples", "panorama")
    assert os.path.exists(exe), "examples/panorama is built by __graft_entry__.build()"
    w, h, spp = 48, 24, 3
    out = tmp_path / "pano.f64"
    done = subprocess.run([exe, str(w), str(h), str(spp), str(out)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    frame = np.fromfile(out, dtype=np.float64).reshape(h, w, 3)
    objs = np.zeros(6, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene
    for k, (kind, geom, base, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (-5, 1.2, 0, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (0, -7, -1, 2), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-3, 4, -2, 3, 4, -2, 0, 4, 3), (0.2, 0.6, 0.9), (0, 0, 0), 1.0),
            (2, (-8, -8, -3, 8, -8, -3, 0, 8, -3), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base, em, rough
    d = np.zeros((h, w, 3))
    pi = math.acos(-1.0)
    for y in range(h):
        for x in range(w):
            lon, lat = 2.0 * pi * (x + 0.5) / w - pi, pi / 2 - pi * (y + 0.5) / h
            v = (math.cos(lat) * math.cos(lon), math.cos(lat) * math.sin(lon), math.sin(lat))
            ln = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            d[y, x] = (v[0] / ln, v[1] / ln, v[2] / ln)
    hnd = hip_scene(gpu, objs, rays_per_pixel=spp).upload(0)
    want = hnd.radiance(np.zeros((w * h, 3)), d.reshape(-1, 3), samples=spp).reshape(h, w, 3)
    hnd.close()
    assert same(frame, want) and frame.any()
    assert "segments" in done.stdout
