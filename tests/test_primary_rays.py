"""The primary rays of the device path -- the pixel -> angle map, vertical_fov, get_ray_dir, the camera's un-normalised basis, the
[y][x] layout, render_to_image's flip and the lens (scene.rs:144-222, camera.rs:42-49) -- against frames the reference's TEXT
determines (tests/closed_form.py): no oracle in the loop.  Every comparison is bit for bit; the statistical lens cases are 5 sigma of
a known Bernoulli plus an analytic systematic term.  The per-tile candidate lists of the primary rays (both built by
build_mesh_tile_lists_kernel) assume exactly this map and the [0, offset) lens box: the 1024 x 1024 frames check them against the
text, and test_tile_list_bound_on_a_stack_of_nearly_coplanar_triangles aims at the list builder's sorting bound."""
import math

import numpy as np
import pytest

import closed_form as cf
from helpers import hip_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _kernels(rtx):
    """every kernel id through the product library, and RTX_KERNEL_BVH and RTX_KERNEL_WAVEFRONT through the lab library (as
    test_gpu_parity._kernels: the lab library's RTX_KERNEL_BVH_REGROUP is its RTX_KERNEL_BVH on every tree)"""
    L = rtx.LabKernel
    return [rtx.RTX_KERNEL_EXACT, rtx.RTX_KERNEL_MIXED, rtx.RTX_KERNEL_BVH, rtx.RTX_KERNEL_BVH_REGROUP, rtx.RTX_KERNEL_WAVEFRONT,
            L(rtx.RTX_KERNEL_BVH), L(rtx.RTX_KERNEL_WAVEFRONT)]


def _rows(hnd, w, h, row_begin=0, n_rows=None):
    """rows row_begin .. row_begin + n_rows of the w x h frame -> (numpy [n_rows][w][3], stats)"""
    import torch
    n_rows = h if n_rows is None else n_rows
    buf = torch.zeros((n_rows, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, row_begin, 1, n_rows, buf.data_ptr())
    return buf.cpu().numpy(), st


def _blocks(gpu, hnd, w, h, block, part, n_parts):
    """the band of blocks of part `part` -> (numpy [n][w][3], the frame rows it holds)"""
    import torch
    n = int(gpu.abi.load_library(hnd.lab).rtx_blocks_row_count(h, block, part, n_parts))
    rows = [r for r0 in range(part * block, h, n_parts * block) for r in range(r0, min(r0 + block, h))]
    assert len(rows) == n
    buf = torch.zeros((max(n, 1), w, 3), dtype=torch.float64, device="cuda:0")
    if n:
        hnd.render_blocks(w, h, block, part, n_parts, buf.data_ptr())
    return buf.cpu().numpy()[:n], rows


def test_pixel_map_and_orientation_are_pinned_without_the_oracle(gpu):
    """closed_form.pixel_map_case -- one small light per marked pixel (the corners, the centre, both sides of 8 x 8 tile borders) where
    the text puts that pixel's ray; three cameras (two with an un-normalised right / up, one off the origin) x 24x10, 17x16, 9x20 x
    sphere and triangle marks -- for every kernel id and AUTO:
      * the frame equals the closed form bit for bit (the marks' emissions at img[y][x], 0 elsewhere), one segment per ray;
      * rtx_render_to_image lights exactly the rows h - 1 - y (scene.rs:176);
      * the same frame as two row bands (render_rows with a row offset) and as blocks dealt to two parts (render_blocks, blocks of 8
        and of 3 rows): the marks land in the right rows of each band -- v = y / h uses the FRAME's h, not the band's;
      * the pick buffer names mark k on mark k's pixel and nothing elsewhere; a sphere mark's distance is 50 - r within 1e-12 * 50
        (test_pick_buffer_orientation's bound, scaled by the distance)."""
    n_cases = 0
    for name, objs, cam, cfg, w, h, expected, info, shape in cf.pixel_map_cases(gpu.OBJECT_DTYPE):
        n_cases += 1
        want_u8 = cf.quantized(expected)
        want_obj = np.full((h, w), -1, dtype=np.int64)
        for k, (x, y) in enumerate(info["marks"]):
            want_obj[y, x] = k
        assert sorted(set(np.nonzero(want_u8.any(axis=2))[0].tolist())) == sorted({h - 1 - y for _, y in info["marks"]})
        for kern in _kernels(gpu) + [gpu.RTX_KERNEL_AUTO]:
            tag = (name, kern)
            scene = hip_scene(gpu, objs, cam=cam, kernel=kern, **cfg)
            hnd = scene.upload(0)
            img, st = _rows(hnd, w, h)
            assert np.array_equal(img, expected), tag
            assert st.segments == w * h * cfg["rays_per_pixel"], tag
            cut = h // 2 + 1                                             # (never a multiple of 8 here: the second band starts inside a tile row)
            for r0, n in ((0, cut), (cut, h - cut)):
                band, _ = _rows(hnd, w, h, r0, n)
                assert np.array_equal(band, expected[r0:r0 + n]), tag + (r0,)
            for block in (8, 3):
                for part in (0, 1):
                    band, rows = _blocks(gpu, hnd, w, h, block, part, 2)
                    assert np.array_equal(band, expected[rows]), tag + (block, part)
            dist, obj, _, _ = hnd.pick(w, h)
            assert np.array_equal(obj, want_obj), tag
            assert np.all(np.isinf(dist[want_obj < 0])), tag
            if shape == "sphere":
                for k, (x, y) in enumerate(info["marks"]):
                    assert abs(dist[y, x] - (cf.MARK_DISTANCE - info["radius"][k])) <= 1e-12 * cf.MARK_DISTANCE, tag + (k,)
            hnd.close()
            assert np.array_equal(scene.render_to_image(w, h), want_u8), tag
    assert n_cases == 18


def test_pixel_map_at_two_stage_size_through_the_tile_lists(gpu):
    """The same closed form at 1024 x 1024 x 1 (2^20 primary rays), through the paths that build per-tile candidate lists for the
    primary rays and assume this pixel map: sphere marks through AUTO (= the sphere kernel in two stages, stage 1 as packets over
    their tiles' lists), also without lists (RTX_TUNE_NO_TILE_LISTS), per lane (RTX_TUNE_NO_PACKETS) and in one stage
    (RTX_TUNE_ONE_STAGE); triangle marks (1209 triangles) through RTX_KERNEL_WAVEFRONT and through AUTO, which must resolve to it,
    with and without lists.  Every run equals the closed form bit for bit, and the lists were USED: fewer box tests than the
    packets' own walks."""
    n_cases = 0
    for name, objs, cam, cfg, w, h, expected, info, shape in cf.pixel_map_cases(gpu.OBJECT_DTYPE, big=True):
        n_cases += 1
        assert w * h * cfg["rays_per_pixel"] == 1 << 20
        if shape == "sphere":
            runs = [("lists", gpu.RTX_KERNEL_AUTO, 0), ("walks", gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_NO_TILE_LISTS),
                    ("lanes", gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_NO_PACKETS), ("one stage", gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_ONE_STAGE)]
        else:
            runs = [("lists", gpu.RTX_KERNEL_WAVEFRONT, 0), ("walks", gpu.RTX_KERNEL_WAVEFRONT, gpu.RTX_TUNE_NO_TILE_LISTS),
                    ("auto lists", gpu.RTX_KERNEL_AUTO, 0), ("auto walks", gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_NO_TILE_LISTS)]
        stats = {}
        for tag, kern, tune in runs:
            hnd = hip_scene(gpu, objs, cam=cam, kernel=kern, tuning=tune, **cfg).upload(0)
            img, st = _rows(hnd, w, h)
            hnd.close()
            stats[tag] = st
            print("%s / %s: kernel %d, stage1_ms %.3f, box_tests %d, stage1_box_tests %d, lit pixels %d"
                  % (name, tag, st.kernel, st.stage1_ms, st.box_tests, st.stage1_box_tests, int(img.any(axis=2).sum())))
            assert np.array_equal(img, expected), (name, tag)
            assert st.segments == w * h, (name, tag)
            if shape == "sphere":
                assert st.kernel == gpu.RTX_KERNEL_BVH, (name, tag)
                assert st.stage1_ms > 0 or tag == "one stage", (name, tag)
            else:
                assert st.kernel == gpu.RTX_KERNEL_WAVEFRONT, (name, tag)
        if shape == "sphere":
            assert stats["lists"].stage1_box_tests < stats["walks"].stage1_box_tests, name
        else:
            assert stats["lists"].box_tests < stats["walks"].box_tests, name
            assert stats["auto lists"].box_tests < stats["auto walks"].box_tests, name
    assert n_cases == 4


def test_lens_is_pinned_without_the_oracle(gpu):
    """closed_form.lens_cases on the device, for every kernel id (the sphere kernel also in its two-stage form): the jitters' support
    is [0, offset) -- occluders just outside it are never hit: a 24 x 16 x 5 frame is the light's emission bit for bit, for two
    seeds --, they are uniform on it (1/2 and 1/4 lit) and the origin's and the target's draws are independent (1/8 lit where one
    draw serving both gives 1/4): 4 seeds x 64 x 64 x 256 samples, 5 sigma of the Bernoulli plus the case's systematic term."""
    import torch
    E = np.array(cf.LENS_EMIT)
    n_exact = n_stat = 0
    for name, objs, cam, cfg, p, exact, systematic in cf.lens_cases(gpu.OBJECT_DTYPE):
        for kern in _kernels(gpu):
            for tune in ((0, gpu.RTX_TUNE_TWO_STAGE) if int(kern) == gpu.RTX_KERNEL_BVH else (0,)):
                if exact:
                    for seed in (1, 99):
                        hnd = hip_scene(gpu, objs, cam=cam, kernel=kern, tuning=tune, rays_per_pixel=cf.LENS_SPP, seed=seed, **cfg).upload(0)
                        img, st = _rows(hnd, cf.LENS_W, cf.LENS_H)
                        hnd.close()
                        assert np.all(img == E), (name, kern, tune, seed)
                        assert st.segments == cf.LENS_W * cf.LENS_H * cf.LENS_SPP, (name, kern, tune, seed)
                    continue
                total = 0.0
                for seed in (41, 42, 43, 44):
                    hnd = hip_scene(gpu, objs, cam=cam, kernel=kern, tuning=tune, rays_per_pixel=256, seed=seed, **cfg).upload(0)
                    buf = torch.zeros((64, 64, 3), dtype=torch.float64, device="cuda:0")
                    hnd.render_rows(64, 64, 0, 1, 64, buf.data_ptr())
                    hnd.close()
                    total += float((buf.cpu().numpy() / E).mean())
                err, bound = cf.lens_check(total / 4, 4 * 64 * 64 * 256, p, systematic)
                print("%s / %r / %d: lit share %.6f, |error| %.3g, bound %.3g" % (name, kern, tune, total / 4, err, bound))
                assert err <= bound, (name, kern, tune, err, bound)
        n_exact += exact
        n_stat += not exact
    assert n_exact == 9 and n_stat == 6


# ---- the list builder's sorting bound ------------------------------------------------------------------------------------------------
STACK_FRAMES = [(1, 1), (2, 1), (3, 1), (5, 1), (8, 1), (64, 64)]
STACK_FOVS = [1e-6, 1e-5, 1e-4, 1e-3, 0.02]


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


def stack_scene(dtype, rng):
    """16 large, nearly coplanar triangles one unit in front of the camera, facing it: plane k lies 1 + s_k along the view direction
    with relative gaps s_{k+1} - s_k = 10^-7 .. 10^-5, its normal tilted by ~1e-6 rad, every triangle wide enough (circumradius 3 .. 5
    about the view axis) to fill any of the views used; distinct emissions, base colour 0: a pixel is the emission of the NEAREST
    plane, and a record skipped by a bound that overshoots shows as another colour.  300 small triangles spread over a cube of side
    1000 make the mesh's extent S ~ 1000, so S / |n . (v0 - p)| ~ 1000: the f32 record's rounding (~ ulp_f32 * S) is ~ 10^-4 of the
    distance, a hundred to a thousand times the gaps.  Scene order is shuffled (the nearest is not the first)."""
    pos = np.array([3.0, -2.0, 40.0])
    view = _unit((0.25, 0.15, -1.0) + rng.normal(size=3) * 0.02)
    e1 = _unit(np.cross(view, (0.0, 0.0, 1.0)))
    e2 = np.cross(view, e1)
    o = np.zeros(16 + 300, dtype=dtype)
    o["kind"] = 2
    o["roughness"] = 1.0
    s = np.cumsum(10.0 ** rng.uniform(-7.0, -5.0, 16))
    for k in range(16):
        n = _unit(view + (e1 * rng.normal() + e2 * rng.normal()) * 1e-6)
        a1 = _unit(np.cross(n, e2))
        a2 = np.cross(n, a1)
        c = pos + view * (1.0 + s[k])
        phi, R = rng.uniform(0.0, 2.0 * math.pi), rng.uniform(3.0, 5.0)
        v = [c + R * (math.cos(phi + j * 2.0 * math.pi / 3.0) * a1 + math.sin(phi + j * 2.0 * math.pi / 3.0) * a2) for j in range(3)]
        if float(_unit(np.cross(v[1] - v[0], v[2] - v[0])) @ v[0]) < 0.0:
            v[1], v[2] = v[2], v[1]
        assert float(_unit(np.cross(v[1] - v[0], v[2] - v[0])) @ v[0]) > 1.0          # triangle.rs:115 never culls it
        o[k]["geom"] = np.concatenate(v)
        o[k]["emission_color"] = ((k + 1) / 32.0, ((5 * k) % 16 + 1) / 16.0, ((3 * k) % 16 + 1) / 16.0)
    for k in range(16, 316):
        c = rng.uniform(-500.0, 500.0, 3)
        o[k]["geom"] = np.concatenate([c, c + rng.normal(size=3) * 2.0, c + rng.normal(size=3) * 2.0])
        o[k]["emission_color"] = (1.0 / 64.0, (k % 7 + 1) / 8.0, 1.0)          # (no plane of the stack has this red)
    rng.shuffle(o)
    return o, (tuple(pos), tuple(view))


def test_tile_list_bound_on_a_stack_of_nearly_coplanar_triangles(gpu):
    """build_mesh_tile_lists_kernel sorts a tile's records by t_lb, a lower bound of the distance evaluated in f64 from the f32 filter
    record with no allowance for the record's own rounding, and the packets stop sweeping the list at the first t_lb above their
    best upper bound.  Reading the code, t_lb is only ever compared with an upper bound that tri_bounds padded by 16 ulp_f32 * S,
    taken from a record of the same precision, so an overshoot of ~1 ulp_f32 * S cannot skip the nearest record.  This is the test
    of that reading: stack_scene's planes lie closer together than the record's rounding, under degenerate beams (a pinhole lens,
    frames from 1 x 1 to 8 x 1 and 64 x 64, fields of view from 1e-6 to 0.02 rad, looking down the stack's normal), 6 frames x 5 fields
    of view x seeded variations.  RTX_KERNEL_WAVEFRONT over its tiles' lists against the exhaustive f64 kernel and against the packets' own walks
    (RTX_TUNE_NO_TILE_LISTS): image and segment count bit for bit.  The lists must have been built and used on most frames: fewer
    box tests than the walks."""
    rng = np.random.default_rng(20261016)
    used = n_cases = 0
    for it in range(60):
        w, h = STACK_FRAMES[it % len(STACK_FRAMES)]
        fov = STACK_FOVS[(it // len(STACK_FRAMES)) % len(STACK_FOVS)]
        objs, (pos, view) = stack_scene(gpu.OBJECT_DTYPE, rng)
        cam = (pos, view, fov)
        cfg = dict(rays_per_pixel=2, seed=it, focal_offset=0.0, non_focal_offset=0.0)
        out = {}
        for tag, kern, tune in (("lists", gpu.RTX_KERNEL_WAVEFRONT, 0), ("walks", gpu.RTX_KERNEL_WAVEFRONT, gpu.RTX_TUNE_NO_TILE_LISTS),
                                ("exact", gpu.RTX_KERNEL_EXACT, 0)):
            hnd = hip_scene(gpu, objs, cam=cam, kernel=kern, tuning=tune, **cfg).upload(0)
            out[tag] = _rows(hnd, w, h)
            hnd.close()
        a, sa = out["lists"]
        assert sa.kernel == gpu.RTX_KERNEL_WAVEFRONT, it
        lit = a.reshape(-1, 3)
        assert np.all(lit[:, 0] * 32.0 == np.round(lit[:, 0] * 32.0)) and np.all(lit[:, 0] > 0), it        # every pixel shows a plane of the stack
        for other in ("walks", "exact"):
            b, sb = out[other]
            assert np.array_equal(a, b) and sa.segments == sb.segments, (it, w, h, fov, other)
        print("stack %d: %dx%d fov %g: box tests %d (lists) %d (walks)" % (it, w, h, fov, sa.box_tests, out["walks"][1].box_tests))
        assert sa.box_tests <= out["walks"][1].box_tests, it
        used += sa.box_tests < out["walks"][1].box_tests
        n_cases += 1
    assert used > n_cases // 2, (used, n_cases)
