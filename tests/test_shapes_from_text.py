"""The device's intersection arithmetic, closest_object, shading and averaging against the reference's TEXT, no oracle in the loop.

The closest-hit query answers (distance, object, hit point, normal) for any ray, directions used as given; tests/text_shapes.py
restates Sphere / Plane / Triangle::distance, normal_at and closest_object from the text in scalar f64.  Every comparison here is ==
on the raw bit patterns (NaN matches NaN) of those four, for tests/shape_families.py's crafted families -- both sides of every
threshold of the text --, the cross-kind ties and the fuzz, each three ways: the resident query on AUTO (which must walk a tree), on
RTX_KERNEL_EXACT, and the host form.  The shading and averaging tests render tests/closed_form.py's non-dyadic scenes and compare
with plain Python floats, bit for bit, for every kernel id and AUTO.

Not pinned here: the order of avg's fold among UNEQUAL non-zero samples -- that needs the RNG stream and stays with the oracle."""
import numpy as np
import pytest

import closed_form as cf
import shape_families as sf
import text_shapes as ts
from helpers import check_equal, hip_scene, same

pytestmark = pytest.mark.gpu
CAM = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1.0)


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


def three_ways(gpu, objs, o, d, want, what, cam=CAM):
    """the resident query on AUTO (a tree walk) and on the exhaustive kernel, and the host form: each equals `want` bit for bit"""
    import torch
    for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
        hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel, rays_per_pixel=1).upload(0)
        check_equal(hnd.query(o, d), want, "%s, kernel %d" % (what, kernel))
        dev = torch.device("cuda", 0)
        rays = gpu.make_rays(o, d)
        d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
        d_hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        st = hnd.closest_hits(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
        hnd.close()
        assert st.kernel == (gpu.RTX_KERNEL_BVH if kernel == gpu.RTX_KERNEL_AUTO else gpu.RTX_KERNEL_EXACT), (what, kernel, st.kernel)
    check_equal(hip_scene(gpu, objs, cam=cam, rays_per_pixel=1).closest_hits(o, d), want, what + ", host form")


def test_crafted_families_equal_the_text(gpu):
    """tests/shape_families.py: spheres (origin outside / inside / on the surface, grazing rays on both sides of 1e-100 and of 0,
    negative and zero radius, direction lengths 1e-160 ... 1e160), planes (normal lengths, origin on the plane, direction parallel,
    behind, -0.0), triangles (the cull by direction across its threshold, phantom hits, non-unit directions, every row-swap branch of
    contains, edges and vertices, dir . n == 0, a subnormal distance)."""
    n = 0
    for name, objs, o, d in sf.families(gpu.OBJECT_DTYPE):
        three_ways(gpu, objs, o, d, ts.answers(objs, o, d), name)
        n += 1
    assert n == 9


def test_ties_across_kinds_go_to_the_first_in_scene_order(gpu):
    """scene.rs:250 across the device's three shape arrays: a plane, a sphere and a triangle all at exactly 4.0, in all six orders and
    as ordered pairs -- the first in scene order wins --, and with one of the three one place nearer -- that one wins."""
    n = 0
    for name, objs, o, d, first in sf.tie_scenes(gpu.OBJECT_DTYPE):
        want = ts.answers(objs, o, d)
        assert want[1][0] == first
        three_ways(gpu, objs, o, d, want, name)
        n += 1
    assert n == 6 + 6 + 18


def test_fuzz_equals_the_text(gpu):
    """the scenes and rays of test_queries_equal_the_oracle_on_fuzzed_scenes, compared with the f64 reading of the text instead of the
    oracle: 24 000 of its rays plus 48 000 aimed at the shapes (shape_families.fuzz_cases); more than half hit something"""
    import torch
    n_rays = n_hit = walked = 0
    for s, objs, cam, o, d in sf.fuzz_cases(gpu.OBJECT_DTYPE):
        want = ts.answers(objs, o, d)
        check_equal(hip_scene(gpu, objs, cam=cam).closest_hits(o, d), want, "scene %d, host form" % s)
        for kernel in (gpu.RTX_KERNEL_AUTO, gpu.RTX_KERNEL_EXACT):
            hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel).upload(0)
            check_equal(hnd.query(o, d), want, "scene %d, kernel %d" % (s, kernel))
            if kernel == gpu.RTX_KERNEL_AUTO:
                dev = torch.device("cuda", 0)
                rays = gpu.make_rays(o, d)
                d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
                d_hits = torch.empty(len(rays) * 64, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                walked += hnd.closest_hits(d_rays.data_ptr(), len(rays), d_hits.data_ptr()).kernel == gpu.RTX_KERNEL_BVH
            hnd.close()
        n_rays += len(o)
        n_hit += int((want[1] >= 0).sum())
    assert n_rays >= 20000 + 150 * sf.AIMED_RAYS and 2 * n_hit > n_rays, (n_rays, n_hit)
    assert walked > 50


def _frame(hnd, w, h):
    import torch
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    return buf.cpu().numpy(), st


def test_shading_and_averaging_of_equal_samples_from_the_text(gpu):
    """closed_form.closed_box_coloured: emission (0.13, 0.6, 1/7) and base colour (0.9, 0.3, 0.77) on every object of the closed box.
    Every sample is the value of `res += light * e; light *= b` run max_bounces + 1 times (scene.rs:276-277), every pixel that value
    added n times from zero and divided by n (scene.rs:253-259) -- computed with plain Python floats, compared bit for bit, for
    max_bounces 0, 3, 10 x 1, 3, 7, 10, 64 samples x 0 and 40 spheres, every kernel id and AUTO; and with a scratch limit that
    forces several sample batches."""
    w, h = 24, 16
    cam = ((0.3, -0.2, 0.1), (1.0, 0.1, -0.05), 1.5)
    for n_sph in (0, 40):
        box = cf.closed_box_coloured(gpu.OBJECT_DTYPE, n_sph)
        for kern in _kernels(gpu) + [gpu.RTX_KERNEL_AUTO]:
            hnd = hip_scene(gpu, box, cam=cam, kernel=kern, rays_per_pixel=1, seed=3).upload(0)
            for mb in cf.COLOUR_BOUNCES:
                for spp in cf.COLOUR_SPP:
                    hnd.set_config(gpu.Config(rays_per_pixel=spp, max_bounces=mb, seed=17 + spp + mb, kernel=kern))
                    img, _ = _frame(hnd, w, h)
                    want = np.broadcast_to(np.array(cf.coloured_pixel(mb, spp)), img.shape)
                    assert same(img, want), (n_sph, kern, mb, spp, img[0, 0], want[0, 0])
            hnd.close()
        for kern in (gpu.RTX_KERNEL_EXACT, gpu.RTX_KERNEL_AUTO):
            hnd = hip_scene(gpu, box, cam=cam, kernel=kern, rays_per_pixel=64, seed=5).upload(0)
            hnd.set_scratch_limit(1 << 20)                      # 300 * 200 * 32 B = 1.92 MB per sample: one sample per launch
            img, st = _frame(hnd, 300, 200)
            hnd.close()
            assert st.trace_launches > 1, (kern, st.trace_launches)
            assert same(img, np.broadcast_to(np.array(cf.coloured_pixel(10, 64)), img.shape)), (n_sph, kern)


def test_averaging_of_lit_and_unlit_samples_from_the_text(gpu):
    """closed_form.lens_coloured_cases: a sample is E = (0.13, 0.6, 1/7) or 0, so every pixel equals fold(E, k) / n in all three
    channels for one k -- set membership with a common k, bit for bit, for 7, 10, 64 and 257 samples on a 64 x 64 frame, every
    kernel id and AUTO; at least half of the possible k occur."""
    size = cf.LENS_COLOUR_FRAME
    for kern in _kernels(gpu) + [gpu.RTX_KERNEL_AUTO]:
        seen = {n: set() for n in cf.LENS_COLOUR_SPP}
        for name, objs, cam, cfg in cf.lens_coloured_cases(gpu.OBJECT_DTYPE):
            hnd = hip_scene(gpu, objs, cam=cam, kernel=kern, rays_per_pixel=1, **cfg).upload(0)
            for n in cf.LENS_COLOUR_SPP:
                hnd.set_config(gpu.Config(rays_per_pixel=n, seed=100 + n, kernel=kern, **cfg))
                img, _ = _frame(hnd, size, size)
                k = cf.lens_lit_counts(img, n)
                assert (k >= 0).all(), (name, kern, n, img[k < 0][:3])
                seen[n] |= set(k.ravel().tolist())
            hnd.close()
        for n in cf.LENS_COLOUR_SPP:
            assert 2 * len(seen[n]) >= n + 1, (kern, n, len(seen[n]))
