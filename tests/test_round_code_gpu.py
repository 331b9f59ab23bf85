"""The round code around the walk of the sphere kernels (rtx_bvh_spheres.hip: the refill from the survivors' queue, whose record now
carries the path's RNG key, the RNG cursor made from the bounce count, the scene's records read as global memory) on the GPU:
RTX_KERNEL_AUTO in one stage, in two stages and in two stages walked per lane against the exhaustive f64 kernel bit for bit, where a
rewrite of the refill, of the queue cursors and of the counters can break --

    frames of 1, 63, 64, 65 and 4097 rays      a wave's share that ends inside the wave, on its last lane, one ray behind it
                                               (4097 = 241 x 17: fewer rays than 96 x 54 x 2, the largest frame here)
    95 x 53 x 2 = 10070 rays                   no multiple of 64, so of no grab size
    rows 1, 4, 7 ... of a 96 x 54 frame        a band with a row stride: the RNG key is the pixel's index in the full image
    5 rays per pixel, three launches           a scratch limit under which two samples fit and three do not: sample_begin 0, 2, 4
    max_bounces 0 and 10                       every survivor of stage 1 refills once / the paths of the benchmark

-- and every count the launch reports (segments, exact tests, filter tests, box tests, the three stage-1 counts, primary rays) against
what the parent commit's library counted for the same launch (COUNTS, recorded on an MI355X through RTX_HIP_LIB in the visit that then
ran this file on the new library).
"""
import numpy as np
import pytest

from helpers import hip_scene
from test_stage2_visit import _cameras, _scenes

FIELDS = ("segments", "exact_tests", "filter_tests", "box_tests", "stage1_exact_tests", "stage1_filter_tests", "stage1_box_tests", "primary_rays")

# name: (scene, width, height, rays per pixel, (first row, row stride) or None, launches asked for or 0, Config fields; "camera": one of
# tests/test_stage2_visit.py _cameras by name, else the benchmark's)
CASES = {
    "1 ray": ("random200", 1, 1, 1, None, 0, dict(camera="inside")),
    "63 rays": ("random200", 9, 7, 1, None, 0, {}),
    "64 rays": ("few3", 8, 8, 1, None, 0, dict(camera="along+y")),
    "65 rays": ("random200", 13, 5, 1, None, 0, {}),
    "4097 rays": ("deep", 241, 17, 1, None, 0, {}),
    "10070 rays": ("deep", 95, 53, 2, None, 0, {}),
    "band": ("random200", 96, 54, 2, (1, 3), 0, {}),
    "three batches": ("random200", 48, 27, 5, None, 3, {}),
    "no bounce": ("deep", 96, 54, 2, None, 0, dict(max_bounces=0)),
    "ten bounces": ("deep", 96, 54, 2, None, 0, dict(max_bounces=10)),
}
TUNINGS = ("one stage", "two stages", "two stages per lane")

# FIELDS of RTX_KERNEL_AUTO per case and tuning, seed 42, counted by the parent commit's library
COUNTS = {
    "1 ray": {"one stage": (1, 0, 20, 20, 0, 0, 0, 1),
        "two stages": (1, 0, 0, 0, 0, 0, 0, 1),
        "two stages per lane": (1, 0, 20, 20, 0, 20, 20, 1)},
    "63 rays": {"one stage": (70, 7, 1259, 1240, 0, 0, 0, 63),
        "two stages": (70, 7, 8690, 8664, 7, 8530, 8512, 63),
        "two stages per lane": (70, 7, 1255, 1236, 7, 1095, 1084, 63)},
    "64 rays": {"one stage": (64, 0, 1536, 0, 0, 0, 0, 64),
        "two stages": (64, 0, 1536, 0, 0, 0, 0, 64),
        "two stages per lane": (64, 0, 1536, 0, 0, 0, 0, 64)},
    "65 rays": {"one stage": (74, 10, 1739, 1712, 0, 0, 0, 65),
        "two stages": (74, 10, 6872, 6428, 9, 6673, 6240, 65),
        "two stages per lane": (74, 10, 1726, 1700, 9, 1527, 1512, 65)},
    "4097 rays": {"one stage": (4257, 215, 664059, 663576, 0, 0, 0, 4097),
        "two stages": (4257, 215, 32285, 13904, 185, 18213, 0, 4097),
        "two stages per lane": (4257, 215, 650584, 650140, 185, 636512, 636236, 4097)},
    "10070 rays": {"one stage": (10562, 608, 1792822, 1791240, 0, 0, 0, 10070),
        "two stages": (10562, 608, 263995, 42912, 532, 220571, 0, 10070),
        "two stages per lane": (10562, 608, 1753149, 1751700, 532, 1709725, 1708788, 10070)},
    "band": {"one stage": (3788, 364, 75972, 75008, 0, 0, 0, 3456),
        "two stages": (3788, 364, 32206, 6860, 334, 24967, 0, 3456),
        "two stages per lane": (3788, 364, 74697, 73752, 334, 67458, 66892, 3456)},
    "three batches": {"one stage": (7117, 688, 142080, 140260, 0, 0, 0, 6480),
        "two stages": (7117, 688, 117665, 78680, 633, 104049, 65792, 6480),
        "two stages per lane": (7117, 688, 139681, 137904, 633, 126065, 125016, 6480)},
    "no bounce": {"one stage": (10368, 545, 1803300, 1802204, 0, 0, 0, 10368),
        "two stages": (10368, 545, 1803300, 1802204, 0, 0, 0, 10368),
        "two stages per lane": (10368, 545, 1803300, 1802204, 0, 0, 0, 10368)},
    "ten bounces": {"one stage": (10869, 638, 1848196, 1846568, 0, 0, 0, 10368),
        "two stages": (10869, 638, 272393, 44364, 545, 227497, 0, 10368),
        "two stages per lane": (10869, 638, 1805568, 1804080, 545, 1760672, 1759716, 10368)},
}


def _objects(name):
    from rust_raytracing_amd import scenes
    return scenes.random_spheres(200, 11, box=0.2) if name == "random200" else _scenes()[name]


def _tuning(gpu, name):
    return {"one stage": 0, "two stages": gpu.RTX_TUNE_TWO_STAGE, "two stages per lane": gpu.RTX_TUNE_TWO_STAGE | gpu.RTX_TUNE_NO_PACKETS}[name]


def _render(gpu, case, kernel, tuning):
    """(the band's pixels, RtxStats) of one case; with `launches` asked for, under the largest scratch limit that still takes that many"""
    import torch
    from rust_raytracing_amd import scenes
    scene, w, h, spp, band, launches, cfg = CASES[case]
    rb, rs = band if band else (0, 1)
    n = len(range(rb, h, rs))
    objs, cfg, cam = _objects(scene), dict(cfg), scenes.CAMERA
    if "camera" in cfg:
        _, cam, more = {c[0]: c for c in _cameras(objs)}[cfg.pop("camera")]
        cfg.update(more)
    hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel, rays_per_pixel=spp, seed=42, tuning=tuning, **cfg).upload(0)
    buf = torch.zeros((n, w, 3), dtype=torch.float64, device="cuda:0")

    def once(limit):
        if limit:
            hnd.set_scratch_limit(limit)
        buf.zero_()
        return hnd.render_rows(w, h, rb, rs, n, buf.data_ptr())

    if launches:
        lo, hi = 1 << 12, 1 << 30                     # launches(lo) = spp (one sample each), launches(hi) = 1; fewer with more room
        assert once(lo).trace_launches >= launches >= once(hi).trace_launches
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if once(mid).trace_launches >= launches:
                lo = mid
            else:
                hi = mid
        st = once(lo)
        assert st.trace_launches == launches, (case, lo, st.trace_launches)
    else:
        st = once(0)
    img = buf.cpu().numpy()
    hnd.close()
    return img, st


def counts_of(st):
    return tuple(int(getattr(st, f)) for f in FIELDS)


def measure(gpu):
    """{case: {tuning: FIELDS}} of the library that is loaded: what COUNTS holds"""
    return {case: {t: counts_of(_render(gpu, case, gpu.RTX_KERNEL_AUTO, _tuning(gpu, t))[1]) for t in TUNINGS} for case in CASES}


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_auto_equals_the_exhaustive_kernel_and_counts_what_the_parent_counted(gpu, case):
    ref, st_ref = _render(gpu, case, gpu.RTX_KERNEL_EXACT, 0)
    scene, w, h, spp, band, launches, cfg = CASES[case]
    assert int(st_ref.primary_rays) == ref.shape[0] * w * spp, (case, st_ref.primary_rays)
    for t in TUNINGS:
        img, st = _render(gpu, case, gpu.RTX_KERNEL_AUTO, _tuning(gpu, t))
        got = counts_of(st)
        print(case, "|", t, "|", dict(zip(FIELDS, got)))
        assert np.array_equal(img.view(np.int64), ref.view(np.int64)), (case, t, float(np.nanmax(np.abs(img - ref))))
        assert st.segments == st_ref.segments, (case, t, st.segments, st_ref.segments)
        assert got == tuple(COUNTS[case][t]), (case, t, dict(zip(FIELDS, got)), COUNTS[case][t])
