"""Zero samples are neither written nor read (store_sample, rtx_device.h; resolve_kernel, rtx_kernels.hip).

A sample whose three components compare equal to zero leaves no record and a clear bit in the launch's non-zero mask; resolve_kernel
reads a record only where the bit is set.  What can go wrong: a mask that is not cleared between launches (of two frames, or of two
sample batches of one frame), so that a record an earlier launch left is added again; a bit or a record at the wrong slot (partial
tiles, a band, the second of several batches); and a value that is not zero taken for one (-0.0 is zero, NaN and the infinities are
not).  Every frame here is compared bit for bit -- with a fresh handle's, or with the oracle on the device's sin / cos.
"""
import numpy as np
import pytest

from helpers import hip_scene, oracle_render, same

pytestmark = pytest.mark.gpu
SIZES = ((64, 36), (61, 35))                  # whole 8x8 tiles; partial tiles on both edges
SPP = 3
BAND = (1, 3)                                 # row_begin, row_stride of the band through render_rows
SEED = 42
AWAY = ((0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), 1.5707963267948966)      # the scenes lie at x > 0: nothing is hit, every sample is zero


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _families(rtx):
    """(name, kernel id, tuning): every kernel id through the product library, the three tree ids through the lab library (the same
    dispatch from the -DRTX_LAB build: on these sphere scenes all three run the sphere kernels there), and the sphere kernel's two stages"""
    L = rtx.LabKernel
    out = [("exact", rtx.RTX_KERNEL_EXACT, 0), ("mixed", rtx.RTX_KERNEL_MIXED, 0), ("bvh", rtx.RTX_KERNEL_BVH, 0),
           ("regroup", rtx.RTX_KERNEL_BVH_REGROUP, 0), ("wavefront", rtx.RTX_KERNEL_WAVEFRONT, 0), ("lab-bvh", L(rtx.RTX_KERNEL_BVH), 0),
           ("lab-regroup", L(rtx.RTX_KERNEL_BVH_REGROUP), 0), ("lab-wavefront", L(rtx.RTX_KERNEL_WAVEFRONT), 0),
           ("two-stage", rtx.RTX_KERNEL_BVH, rtx.RTX_TUNE_TWO_STAGE)]
    return out


FAMILIES = ("exact", "mixed", "bvh", "regroup", "wavefront", "lab-bvh", "lab-regroup", "lab-wavefront", "two-stage")


def _family(rtx, name):
    return {f[0]: f[1:] for f in _families(rtx)}[name]


def _all_lights():
    from rust_raytracing_amd import scenes
    return scenes.light_every(scenes.compact(scenes.random_spheres(300, 5)), n=1)


def _mesh_of_lights():
    from rust_raytracing_amd import scenes
    return scenes.light_every(scenes.compact(scenes.random_triangles(2000, 6), k=0.05, x0=5.0), n=1)


def _odd_emissions():
    """Spheres that bounce on (their base colour stays) and emit, in turn: nothing, -0.0, a negative colour, a colour with one NaN, one
    with +inf, one with -inf, an ordinary one, +0.0 / -0.0 mixed, and one of subnormals and the smallest normal (not zero: stored)."""
    from rust_raytracing_amd import scenes
    o = scenes.compact(scenes.random_spheres(300, 5)).copy()
    inf, nan = float("inf"), float("nan")
    kinds = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-1.5, -0.25, -3.0), (0.5, nan, 0.0), (inf, 0.0, 1.0), (0.0, -inf, 0.0), (2.0, 1.0, 0.5),
             (0.0, -0.0, 0.0), (5e-324, 1e-310, 2.2250738585072014e-308)]
    for k, e in enumerate(kinds):
        o["emission_color"][k::len(kinds)] = e
    o["base_color"] = np.maximum(o["base_color"], 0.3)
    return o


def _subnormal(a):
    return (a != 0.0) & (np.abs(a) < 2.2250738585072014e-308)


def _rows(h, band):
    if band is None:
        return 0, 1, h
    rb, rs = band
    return rb, rs, len(range(rb, h, rs))


def _render(hnd, w, h, band=None):
    import torch
    rb, rs, n = _rows(h, band)
    buf = torch.zeros((n, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, rb, rs, n, buf.data_ptr())
    return buf.cpu().numpy(), st


def _handle(gpu, objs, cam, kernel, tuning, scratch=0, spp=SPP):
    hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel, tuning=tuning, rays_per_pixel=spp, seed=SEED).upload(0)
    if scratch:
        hnd.set_scratch_limit(scratch)
    return hnd


_ORACLE = {}


def _oracle_frame(oracle, key, objs, w, h, spp=SPP):
    """the oracle's frame on the device's sin / cos, computed once per (scene, size, samples per pixel)"""
    from rust_raytracing_amd import scenes
    if (key, w, h, spp) not in _ORACLE:
        with oracle.device_sincos():
            _ORACLE[(key, w, h, spp)] = oracle_render(oracle, objs, w, h, cam=scenes.CAMERA, rays_per_pixel=spp, seed=SEED)
    return _ORACLE[(key, w, h, spp)]


def _shapes():
    """(w, h, band): both sizes as whole frames, and the partial-tile size as a band with a row stride"""
    return [(w, h, None) for w, h in SIZES] + [(SIZES[1][0], SIZES[1][1], BAND)]


def _lit_then_dark(gpu, objs, kernel, tuning, scratch, want_launches):
    from rust_raytracing_amd import scenes
    for w, h, band in _shapes():
        hnd = _handle(gpu, objs, scenes.CAMERA, kernel, tuning, scratch)
        lit, st = _render(hnd, w, h, band)
        assert (st.trace_launches > 1) == want_launches, (w, h, band, st.trace_launches)
        frac = float(np.mean(np.any(lit != 0.0, axis=2)))
        assert frac > 0.3, (w, h, band, frac)                               # nearly every slot of the scratch now holds a record
        fresh_hnd = _handle(gpu, objs, scenes.CAMERA, kernel, tuning, 0)    # (one launch, whatever the first handle's limit)
        fresh_lit, _ = _render(fresh_hnd, w, h, band)
        fresh_hnd.close()
        assert same(lit, fresh_lit), (w, h, band)
        hnd.set_camera(gpu.Camera(*AWAY))
        dark, st2 = _render(hnd, w, h, band)
        hnd.close()
        fresh_hnd = _handle(gpu, objs, AWAY, kernel, tuning, 0)
        fresh, _ = _render(fresh_hnd, w, h, band)
        fresh_hnd.close()
        assert st2.segments == st2.primary_rays                             # every ray left the scene at once
        assert same(dark, fresh), (w, h, band, float(np.abs(dark).max()))
        assert not dark.view(np.uint64).any(), (w, h, band)                 # +0.0 / 3 in every component


@pytest.mark.parametrize("name", FAMILIES)
def test_a_dark_frame_after_a_lit_one_reads_no_stale_record(gpu, name):
    """One handle, two renders: a scene of lights seen (nearly every sample a record), then the camera turned away (no record at all).
    The second frame is a fresh handle's, bit for bit."""
    kernel, tuning = _family(gpu, name)
    _lit_then_dark(gpu, _all_lights(), kernel, tuning, 0, False)


@pytest.mark.parametrize("name", FAMILIES)
def test_the_same_over_several_sample_batches(gpu, name):
    """A scratch limit below one sample's floor: one sample per launch, three launches per frame, the mask cleared before each."""
    kernel, tuning = _family(gpu, name)
    _lit_then_dark(gpu, _all_lights(), kernel, tuning, 1 << 12, True)


def test_a_mesh_through_auto(gpu):
    _lit_then_dark(gpu, _mesh_of_lights(), gpu.RTX_KERNEL_AUTO, 0, 0, False)
    _lit_then_dark(gpu, _mesh_of_lights(), gpu.RTX_KERNEL_AUTO, 0, 1 << 12, True)


@pytest.mark.parametrize("name", FAMILIES)
def test_only_zero_counts_as_zero(gpu, oracle, name):
    """Emission -0.0, negative, NaN and infinite: each frame equals the oracle's (device sin / cos) bit for bit, NaN by position, in
    one launch and one sample per launch."""
    from rust_raytracing_amd import scenes
    kernel, tuning = _family(gpu, name)
    objs = _odd_emissions()
    for w, h, band in _shapes():
        ref = _oracle_frame(oracle, "odd", objs, w, h)
        rb, rs, n = _rows(h, band)
        ref = ref[rb::rs][:n]
        assert np.isnan(ref).any() and np.isinf(ref).any() and (ref < 0).any() and (ref == 0).all(axis=2).any()
        assert _subnormal(ref).any(), (w, h, band)       # a pixel all of whose samples saw the subnormal emitter or nothing
        for scratch in (0, 1 << 12):
            hnd = _handle(gpu, objs, scenes.CAMERA, kernel, tuning, scratch)
            img, st = _render(hnd, w, h, band)
            hnd.close()
            assert (st.trace_launches > 1) == bool(scratch)
            assert same(img, ref), (name, w, h, band, scratch, int((img.view(np.uint64) != ref.view(np.uint64)).sum()))


@pytest.mark.parametrize("spp", (9, 17))
@pytest.mark.parametrize("name", FAMILIES)
def test_only_zero_counts_as_zero_beyond_one_group_of_samples(gpu, oracle, name, spp):
    """resolve_kernel folds eight samples at a time: the same comparison at 9 (a second group of one) and 17 samples per pixel (a third,
    ragged one) on the frame with partial tiles, in one launch and one sample per launch."""
    from rust_raytracing_amd import scenes
    kernel, tuning = _family(gpu, name)
    objs = _odd_emissions()
    w, h = SIZES[1]
    ref = _oracle_frame(oracle, "odd", objs, w, h, spp)
    assert np.isnan(ref).any() and np.isinf(ref).any() and (ref < 0).any() and (ref == 0).all(axis=2).any() and _subnormal(ref).any()
    for scratch in (0, 1 << 12):
        hnd = _handle(gpu, objs, scenes.CAMERA, kernel, tuning, scratch, spp)
        img, st = _render(hnd, w, h)
        hnd.close()
        assert st.trace_launches == (spp if scratch else 1), (name, spp, scratch, st.trace_launches)
        assert same(img, ref), (name, spp, scratch, int((img.view(np.uint64) != ref.view(np.uint64)).sum()))


def test_the_mask_counts_against_the_scratch_limit(gpu):
    """The exhaustive kernel at 300 x 200 x 7 (tests/test_gpu_parity.py::test_sample_batching_keeps_the_left_fold): a batch of two samples
    holds 2 * 60000 records of 32 bytes and nonzero_mask_bytes(120000) = 15000 bytes of mask.  A limit of exactly that takes two samples
    per launch -- 4 launches -- and one byte less takes one -- 7.  (render_band's `fixed` part is zero for this kernel: no tile lists, no
    survivors' queue, no wavefront or sweep state; the limit is far below 3/4 of the device's free memory.)"""
    import torch
    from rust_raytracing_amd import scenes
    objs = scenes.three_spheres()
    need = 2 * 60000 * 32 + (120000 + 31) // 32 * 4
    assert need == 3855000
    frames = []
    for limit, launches in ((need, 4), (need - 1, 7)):
        hnd = hip_scene(gpu, objs, kernel=gpu.RTX_KERNEL_EXACT, rays_per_pixel=7, seed=5).upload(0)
        hnd.set_scratch_limit(limit)
        buf = torch.zeros((200, 300, 3), dtype=torch.float64, device="cuda:0")
        st = hnd.render_rows(300, 200, 0, 1, 200, buf.data_ptr())
        hnd.close()
        assert st.trace_launches == launches, (limit, st.trace_launches)
        frames.append(buf.cpu().numpy())
    assert same(frames[0], frames[1])
