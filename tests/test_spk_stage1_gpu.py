"""Stage 1 of the sphere path (trace_sph_packet_kernel, rtx_bvh_spheres.hip) on the GPU, where its work units (a run of samples of one
tile) and the box-walk ray made inside the walking branch can go wrong: frames of RTX_KERNEL_AUTO | RTX_TUNE_TWO_STAGE against
RTX_KERNEL_EXACT bit for bit, and the eight counts of RtxStats (tests/test_round_code_gpu.py FIELDS) against what the library of the
parent commit 68cefc0 counted for the same launches on an MI355X (COUNTS).

A work unit is a run of G samples of one tile; G = 2 x the launch's grab / 64: 2 for the small launches here, 16 from 2^25 rays on.
The sample counts of the 20 x 12 frames end a tile's runs on a full one and on a single sample, with partial tiles on both edges;
"runs of 16" is the one launch big enough for the benchmark's G (640 x 360 x 147 samples in halves of 74 and 73: four full runs and
one of 10 or 9), over six spheres so that the exhaustive kernel stays quick.

TILES: the tiles of each case with an empty list / a list / no list (they walk), from the parent's lab library (rtx_debug_tile_lists).
    (0, 0, 0)    the packet kernel never ran.  few3 (three spheres get no tree) and mixed (its 40 triangles go into the tree, which
                 is then no sphere tree) render in one stage: they hold RTX_TUNE_TWO_STAGE to that fallback.  With
                 RTX_TUNE_NO_TILE_LISTS there are no lists and every tile walks.
    empty        a tile whose every ray misses the tree: few6, "over the limit", and "mixed, loose triangles", where a plane and three
                 triangles outside the tree lie behind the empty lists.  "beyond the range" and "NaN camera": no ray may walk, every
                 ray is swept, whatever the tile's list says.
    walking      "centre" (every tile, mixed octants on the centre row and column), "over the limit" (the slack of a far origin is
                 not 0), "NaN camera".  "clustered, inside" was meant to overflow its lists and does not: all 40 tiles have one.
"""
import numpy as np
import pytest

from helpers import hip_scene, same
from test_round_code_gpu import FIELDS, counts_of
from test_stage2_visit import _cameras, _origin_limit, _scenes

# name: (scene, width, height, rays per pixel, how, Config fields; "camera": see _camera).  how: None one render call; ("band", first row,
# row stride); ("launches", n) under the largest scratch limit that still takes n launches; ("accumulate", (first, n), ...) sample ranges
# of rtx_render_blocks_accumulate; ("no lists",) RTX_TUNE_NO_TILE_LISTS
CASES = {
    "1 spp": ("random200", 20, 12, 1, None, {}),
    "15 spp": ("random200", 20, 12, 15, None, {}),
    "16 spp": ("random200", 20, 12, 16, None, {}),
    "17 spp": ("random200", 20, 12, 17, None, {}),
    "33 spp": ("random200", 20, 12, 33, None, {}),
    "17 spp, three launches": ("random200", 20, 12, 17, ("launches", 3), {}),
    "17 spp from sample 5": ("random200", 20, 12, 17, ("accumulate", (0, 5), (5, 12)), {}),
    "17 spp, band": ("random200", 20, 12, 17, ("band", 1, 3), {}),
    "few3": ("few3", 64, 36, 3, None, {}),
    "few3, one bounce": ("few3", 64, 36, 3, None, dict(max_bounces=1)),
    "mixed": ("mixed", 64, 36, 3, None, {}),
    "mixed, loose triangles": ("mixed3", 64, 36, 3, None, {}),
    "few3, beyond the range": ("few3", 64, 36, 3, None, dict(camera="beyond")),
    "few3, NaN camera": ("few3", 64, 36, 3, None, dict(camera="nan")),
    "runs of 16": ("few6", 640, 360, 147, None, {}),
    # (three spheres get no tree, so the four few3 cases never reach the packet kernel: the same with six)
    "few6":("few6", 64, 36, 3, None, {}),
    "few6, one bounce": ("few6", 64, 36, 3, None, dict(max_bounces=1)),
    "few6, beyond the range": ("few6", 64, 36, 3, None, dict(camera="beyond")),
    "few6, NaN camera": ("few6", 64, 36, 3, None, dict(camera="nan")),
    "clustered, inside": ("clustered", 64, 36, 3, None, dict(camera="inside")),
    "clustered, centre": ("clustered", 64, 36, 3, None, dict(camera="centre")),
    "clustered, over the limit": ("clustered", 64, 36, 3, None, dict(camera="over the limit")),
    "clustered, over the limit, no lists": ("clustered", 64, 36, 3, ("no lists",), dict(camera="over the limit")),
}

# (tiles with an empty list, with a list, that walk) per case: the parent's lab library, the last launch of the case
TILES = {
    "1 spp": (1, 4, 1),
    "15 spp": (1, 4, 1),
    "16 spp": (1, 4, 1),
    "17 spp": (1, 4, 1),
    "33 spp": (1, 4, 1),
    "17 spp, three launches": (1, 4, 1),
    "17 spp from sample 5": (1, 4, 1),
    "17 spp, band": (0, 2, 1),
    "few3": (0, 0, 0),
    "few3, one bounce": (0, 0, 0),
    "mixed": (0, 0, 0),
    "mixed, loose triangles": (9, 31, 0),
    "few3, beyond the range": (0, 0, 0),
    "few3, NaN camera": (0, 0, 0),
    "runs of 16": (3109, 491, 0),
    "few6": (26, 14, 0),
    "few6, one bounce": (26, 14, 0),
    "few6, beyond the range": (0, 40, 0),
    "few6, NaN camera": (0, 0, 40),
    "clustered, inside": (0, 40, 0),
    "clustered, centre": (0, 0, 40),
    "clustered, over the limit": (20, 6, 14),
    "clustered, over the limit, no lists": (0, 0, 0),
}

# FIELDS of RTX_KERNEL_AUTO | RTX_TUNE_TWO_STAGE per case, seed 42, counted by the parent commit's library
COUNTS = {
    "1 spp": (262, 24, 15839, 14544, 23, 15352, 14080, 240),
    "15 spp": (3945, 387, 234661, 215212, 364, 227195, 208128, 3600),
    "16 spp": (4206, 411, 249909, 229168, 388, 242034, 221696, 3840),
    "17 spp": (4469, 437, 265759, 243732, 413, 257377, 235776, 4080),
    "33 spp": (8682, 855, 519781, 477028, 796, 503223, 461312, 7920),
    "17 spp, three launches": (4469, 437, 265759, 243732, 413, 257377, 235776, 4080),
    "17 spp from sample 5": (4469, 437, 265759, 243732, 413, 257377, 235776, 4080),
    "17 spp, band": (1495, 157, 108570, 101412, 145, 105572, 98560, 1360),
    "few3": (6916, 160, 26112, 0, 0, 0, 0, 6912),
    "few3, one bounce": (6916, 160, 26112, 0, 0, 0, 0, 6912),
    "mixed": (12575, 16171, 252217, 225088, 0, 0, 0, 6912),
    "mixed, loose triangles": (11899, 49030, 58607, 41956, 28816, 14926, 0, 6912),
    "few3, beyond the range": (6912, 609, 21504, 0, 0, 0, 0, 6912),
    "few3, NaN camera": (6912, 27648, 21504, 0, 0, 0, 0, 6912),
    "runs of 16": (34383947, 1401303, 9293933, 4134876, 1387061, 4619328, 0, 33868800),
    "few6": (7018, 293, 3933, 848, 289, 2976, 0, 6912),
    "few6, one bounce": (7018, 293, 3933, 848, 289, 2976, 0, 6912),
    "few6, beyond the range": (6912, 41472, 0, 0, 41472, 0, 0, 6912),
    "few6, NaN camera": (6912, 0, 27648, 27648, 0, 27648, 27648, 6912),
    "clustered, inside": (23621, 23758, 2671151, 2468420, 6932, 53737, 0, 6912),
    "clustered, centre": (15453, 11920, 1521505, 1459256, 6916, 946505, 919296, 6912),
    "clustered, over the limit": (8751, 2661, 789746, 760628, 1835, 687008, 664320, 6912),
    "clustered, over the limit, no lists": (8751, 2661, 819508, 807348, 1835, 716770, 711040, 6912),
}


def _objects(name):
    from rust_raytracing_amd import scenes
    if name == "random200":
        return scenes.random_spheres(200, 11, box=0.2)            # tests/golden/spheres200_48x27's scene
    if name == "mixed":
        return scenes.mixed_scene()                               # its 40 triangles go into the tree: no sphere kernel
    if name == "mixed3":
        return scenes.mixed_scene(40, 3, 1)                       # a plane and three triangles outside a sphere tree
    return _scenes()[name]


def _camera(name, objs):
    """(camera, Config fields) by name: tests/test_stage2_visit.py's, or
    centre    the benchmark's view turned to the middle of the spheres: the image's centre row and column hold rays of mixed octants
    beyond    an origin past 2^27 x the tree's origin limit: no ray walks, every ray is swept
    nan       a NaN coordinate in the camera's position: the same"""
    from rust_raytracing_amd import scenes
    g = objs["geom"]
    mid = g[:, :3].mean(axis=0)
    if name == "centre":
        return ((0.0, float(mid[1]), float(mid[2])), (1.0, 0.0, 0.0), 1.2), {}
    if name == "beyond":
        o = (-_origin_limit(objs) * 2.0 ** 27 * 1.5, float(mid[1]), float(mid[2]))
        return (o, tuple(float(x) for x in (mid - np.array(o))), 1e-9), {}
    if name == "nan":
        return ((float("nan"), 0.0, 0.0), (1.0, 0.0, 0.0), scenes.CAMERA[2]), {}
    _, cam, more = {c[0]: c for c in _cameras(objs)}[name]
    return cam, more


def _render(gpu, case, kernel, tuning, lab=None):
    """(the pixels -- of an accumulate case: the sums --, FIELDS summed over the case's calls, the tile lists' counts or None)"""
    import torch
    from rust_raytracing_amd import scenes
    scene, w, h, spp, how, cfg = CASES[case]
    objs, cfg, cam = _objects(scene), dict(cfg), scenes.CAMERA
    if "camera" in cfg:
        cam, more = _camera(cfg.pop("camera"), objs)
        cfg.update(more)
    kind = how[0] if how else None
    if kind == "no lists":
        tuning |= gpu.RTX_TUNE_NO_TILE_LISTS
    rb, rs = (how[1], how[2]) if kind == "band" else (0, 1)
    n = len(range(rb, h, rs))
    hnd = hip_scene(gpu, objs, cam=cam, kernel=kernel, rays_per_pixel=spp, seed=42, tuning=tuning, **cfg).upload(0, lab=lab)
    buf = torch.zeros((n, w, 3), dtype=torch.float64, device="cuda:0")

    def once(limit):
        if limit:
            hnd.set_scratch_limit(limit)
        buf.zero_()
        return hnd.render_rows(w, h, rb, rs, n, buf.data_ptr())

    if kind == "launches":
        launches = how[1]
        lo, hi = 1 << 12, 1 << 30
        assert once(lo).trace_launches >= launches >= once(hi).trace_launches
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if once(mid).trace_launches >= launches:
                lo = mid
            else:
                hi = mid
        st = once(lo)
        assert st.trace_launches == launches, (case, lo, st.trace_launches)
        got = counts_of(st)
    elif kind == "accumulate":
        got = (0,) * len(FIELDS)
        for first, count in how[1:]:
            st = hnd.render_accumulate(w, h, first, count, buf.data_ptr())
            got = tuple(a + b for a, b in zip(got, counts_of(st)))
    else:
        got = counts_of(once(0))
    lists = hnd.debug_tile_lists() if lab else None
    img = buf.cpu().numpy()
    hnd.close()
    return img, got, lists


def measure(gpu):
    """{case: FIELDS} of the library that is loaded: what COUNTS holds"""
    return {case: _render(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE)[1] for case in CASES}


def tile_classes(gpu):
    """{case: (empty, listed, walking)} of the lab library that is loaded: what TILES holds"""
    out = {}
    for case in CASES:
        tl = _render(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE, lab=True)[2]
        c = tl["count"] if tl["form"] == 1 else np.zeros(0, dtype=np.uint32)
        out[case] = (int((c == 0).sum()), int(((c != 0) & (c != gpu.TILE_LIST_WALK)).sum()), int((c == gpu.TILE_LIST_WALK).sum()))
    return out


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_stages_equal_the_exhaustive_kernel_and_count_what_the_parent_counted(gpu, case):
    ref, got_ref, _ = _render(gpu, case, gpu.RTX_KERNEL_EXACT, 0)
    img, got, _ = _render(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE)
    print(case, "|", dict(zip(FIELDS, got)), "| tiles (empty, listed, walking)", TILES[case])
    assert same(img, ref), (case, float(np.nanmax(np.abs(img - ref))))
    assert got[0] == got_ref[0], (case, "segments", got[0], got_ref[0])
    assert got == tuple(COUNTS[case]), (case, dict(zip(FIELDS, got)), COUNTS[case])
