"""The packet kernel's pool of primary hits (rtx_spk_pool.h, trace_sph_packet_kernel) on the GPU: frames of RTX_KERNEL_AUTO |
RTX_TUNE_TWO_STAGE against RTX_KERNEL_EXACT bit for bit, and the eight counts of RtxStats (tests/test_round_code_gpu.py FIELDS)
against constants.  The pool changes WHEN a primary hit is shaded -- with 63 others, or in the flush of the leaving wave -- and never
whether, so every pixel and every count is what it was.

The shapes are the smallest at which the pool can go wrong (a wave here meets a handful of packets, so most hits leave in a flush;
the 17 spp frames and the 64 x 36 ones carry the pool across samples, units and tiles and shade full passes too):
    one packet              8 x 8, 1 spp: one wave, one packet, the flush alone (few6: the packet holds no hit and the pool stays
                            empty; random200 and clustered: a few hits, which all leave in the flush)
    few6                    26 of 40 tiles are empty: the pool fills over many packets and ends partly filled
    17 spp                  20 x 12: the pool carried across samples and units, partial tiles whose padding lanes pull
    17 spp, band            rows 1, 4, 7, ...
    17 spp, three launches  the pool emptied at every launch's end
    mixed, loose triangles  a plane and three loose triangles behind the lists: kinds 1 and 2 through the pool
    few6, one bounce        every pooled hit is done after its shading: a store, no survivor
    clustered, centre       walking tiles feed the pool too
    few6, NaN camera        swept rays
All but the one-packet cases are cases of tests/test_spk_stage1_gpu.py, rendered by its _render and held to its COUNTS.  NEW_COUNTS: counted by
the library of the parent commit 8b5de0d (no pool) on an MI355X, loaded through RTX_HIP_LIB in the GPU visit that then ran this file.
"""
import numpy as np
import pytest

import test_spk_stage1_gpu as stage1
from helpers import hip_scene, same
from test_round_code_gpu import FIELDS, counts_of

SHARED = ("few6", "17 spp", "17 spp, band", "17 spp, three launches", "mixed, loose triangles", "few6, one bounce", "clustered, centre",
          "few6, NaN camera")

# name: (scene of test_spk_stage1_gpu._objects, width, height, rays per pixel).  The one packet of few6 holds no hit at all (its one
# exact test misses): the wave leaves with an empty pool; random200's and clustered's hold hits, all of which leave in the flush
NEW_CASES = {"one packet": ("few6", 8, 8, 1), "one packet, random200": ("random200", 8, 8, 1), "one packet, clustered": ("clustered", 8, 8, 1)}
NEW_COUNTS = {
    "one packet": (64, 1, 384, 0, 1, 384, 0, 64),
    "one packet, random200": (70, 6, 9128, 9104, 4, 8973, 8960, 64),
    "one packet, clustered": (116, 78, 65081, 64724, 54, 62150, 61952, 64),
}


def _render_new(gpu, case, kernel, tuning):
    import torch
    from rust_raytracing_amd import scenes
    scene, w, h, spp = NEW_CASES[case]
    hnd = hip_scene(gpu, stage1._objects(scene), cam=scenes.CAMERA, kernel=kernel, rays_per_pixel=spp, seed=42, tuning=tuning).upload(0)
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    img = buf.cpu().numpy()
    hnd.close()
    return img, counts_of(st)


def measure(gpu):
    """{case: FIELDS} of the library that is loaded: what NEW_COUNTS holds"""
    return {case: _render_new(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE)[1] for case in NEW_CASES}


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHARED)
def test_pooled_hits_give_the_exhaustive_kernels_bits_and_the_parents_counts(gpu, case):
    ref, got_ref, _ = stage1._render(gpu, case, gpu.RTX_KERNEL_EXACT, 0)
    img, got, _ = stage1._render(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE)
    print(case, "|", dict(zip(FIELDS, got)))
    assert same(img, ref), (case, float(np.nanmax(np.abs(img - ref))))
    assert got[0] == got_ref[0], (case, "segments", got[0], got_ref[0])
    assert got == tuple(stage1.COUNTS[case]), (case, dict(zip(FIELDS, got)), stage1.COUNTS[case])


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(NEW_CASES))
def test_one_packet_leaves_in_the_flush_alone(gpu, case):
    ref, got_ref = _render_new(gpu, case, gpu.RTX_KERNEL_EXACT, 0)
    img, got = _render_new(gpu, case, gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE)
    print(case, "|", dict(zip(FIELDS, got)))
    assert got[5] > 0, "the packet kernel ran"
    assert same(img, ref), (case, float(np.nanmax(np.abs(img - ref))))
    assert got[0] == got_ref[0], (case, "segments", got[0], got_ref[0])
    assert got == tuple(NEW_COUNTS[case]), (case, dict(zip(FIELDS, got)), NEW_COUNTS[case])


# ---- the tile lists across render calls: a call that renders the frame of the call before it builds no lists, and
# whatever changes the tree, the shapes, the camera, the frame or the buffer makes the next call build them again.  The count of the
# launches asked to build lists is rtx_debug_tile_lists' info[5] (the lab library: same files, same dispatch); every frame is held to
# RTX_KERNEL_EXACT on a fresh handle of the product library in the same state.
W, H, SPP = 64, 36, 3
FULL, BAND = (0, 1), (1, 3)                                          # (first row, row stride)
LIST_SCENES = ("random200", "clustered", "mesh")
CAM2 = ((0.3, -0.2, 0.1), (1.0, 0.08, -0.05), 1.1)


def _list_scene(gpu, name):
    """(objects, kernel, tuning) of a scene whose primary rays run over tile lists"""
    if name == "mesh":
        import tile_list_cases as tlc
        return np.array(tlc.scene("bench", "mesh", "whole")[0]), gpu.RTX_KERNEL_WAVEFRONT, 0
    return np.array(stage1._objects(name)), gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE


def _rows(h, rows):
    return len(range(rows[0], h, rows[1]))


def _frame(hnd, w=W, h=H, rows=FULL):
    import torch
    n = _rows(h, rows)
    buf = torch.zeros((n, w, 3), dtype=torch.float64, device="cuda:0")
    hnd.render_rows(w, h, rows[0], rows[1], n, buf.data_ptr())
    return buf.cpu().numpy()


def _exact(gpu, objs, cam, w=W, h=H, rows=FULL):
    hnd = hip_scene(gpu, objs, cam=cam, kernel=gpu.RTX_KERNEL_EXACT, rays_per_pixel=SPP, seed=42).upload(0)
    img = _frame(hnd, w, h, rows)
    hnd.close()
    return img


def _resident(gpu, name):
    from rust_raytracing_amd import scenes
    objs, kernel, tuning = _list_scene(gpu, name)
    hnd = hip_scene(gpu, objs, cam=scenes.CAMERA, kernel=kernel, rays_per_pixel=SPP, seed=42, tuning=tuning).upload(0, lab=True)
    return objs, hnd


@pytest.mark.gpu
@pytest.mark.parametrize("scene", LIST_SCENES)
def test_the_second_render_of_a_frame_builds_no_lists_and_gives_the_same_bits(gpu, scene):
    from rust_raytracing_amd import scenes
    objs, hnd = _resident(gpu, scene)
    first = _frame(hnd)
    lists = hnd.debug_tile_lists()
    assert lists["form"] == (2 if scene == "mesh" else 1) and lists["builds"] == 1, (lists["form"], lists["builds"])
    second = _frame(hnd)
    again = hnd.debug_tile_lists()
    assert again["builds"] == 1, "the second call of the frame launched the builder again"
    assert again["form"] == lists["form"] and np.array_equal(again["count"], lists["count"]) and np.array_equal(again["raw"], lists["raw"])
    band = _frame(hnd, rows=BAND)                                       # another band: built; the same band again: not
    assert hnd.debug_tile_lists()["builds"] == 2
    band2 = _frame(hnd, rows=BAND)
    assert hnd.debug_tile_lists()["builds"] == 2
    hnd.close()
    ref = _exact(gpu, objs, scenes.CAMERA)
    assert same(first, ref) and same(second, ref), (scene, float(np.nanmax(np.abs(second - ref))))
    ref_band = _exact(gpu, objs, scenes.CAMERA, rows=BAND)
    assert same(band, ref_band) and same(band2, ref_band), scene


def _moved(objs, idx, delta):
    o = np.array(objs[idx])
    kind = np.asarray(o["kind"]).astype(int)
    g = o["geom"]
    for k in range(len(o)):
        cols = range(3) if kind[k] == 0 else range(9)
        for c in cols:
            g[k, c] += delta[c % 3]
    return o


# name -> what changes between two renders of one handle.  Each returns (objects of the new state, camera, width, rows)
def _change(gpu, name, hnd, objs, cam):
    from rust_raytracing_amd import scenes
    w, rows = W, FULL
    if name == "set_camera":
        cam = CAM2
        hnd.set_camera(gpu.Camera(*cam))
    elif name == "another width":
        w = 60                                                          # (the same 8 tiles per row)
    elif name == "another band":
        rows = BAND
    elif name in ("sphere refit", "rebuild"):
        idx = np.arange(0, len(objs), max(1, len(objs) // 12))[:12]
        new = _moved(objs, idx, (0.03, -0.02, 0.025))
        how = hnd.update_objects(idx, new, mode="rebuild" if name == "rebuild" else "auto")
        assert how == ("rebuilt" if name == "rebuild" else "refit"), how
        objs = np.array(objs)
        objs[idx] = new
    elif name == "set_visible":
        idx = np.arange(0, len(objs), 3)
        hnd.set_visible(idx, False)
        objs = np.delete(objs, idx)                                     # (frames equal the list with the hidden objects deleted)
    elif name == "append_objects":
        extra = _moved(objs, np.arange(3), (0.0, 0.15, -0.1))
        hnd.append_objects(extra)
        objs = np.concatenate([objs, extra])
    else:
        raise KeyError(name)
    return objs, cam, w, rows


CHANGES = ("set_camera", "another width", "another band", "sphere refit", "rebuild", "set_visible", "append_objects")
CHANGE_CASES = [(s, c) for s in LIST_SCENES for c in CHANGES if not (s == "mesh" and c == "sphere refit")]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,change", CHANGE_CASES, ids=["%s-%s" % sc for sc in CHANGE_CASES])
def test_a_change_between_two_renders_gives_the_bits_of_a_fresh_handle(gpu, scene, change):
    from rust_raytracing_amd import scenes
    objs, hnd = _resident(gpu, scene)
    before = _frame(hnd)
    assert hnd.debug_tile_lists()["builds"] == 1
    objs2, cam2, w, rows = _change(gpu, change, hnd, objs, scenes.CAMERA)
    after = _frame(hnd, w=w, rows=rows)
    lists = hnd.debug_tile_lists()
    if lists["form"] != 0:                                              # (a mesh with an appended sphere may leave the list path)
        assert lists["builds"] == 2, "the lists of the frame before the change were reused"
    after2 = _frame(hnd, w=w, rows=rows)
    assert hnd.debug_tile_lists()["builds"] == lists["builds"]
    hnd.close()
    assert same(before, _exact(gpu, objs, scenes.CAMERA)), (scene, change, "before")
    ref = _exact(gpu, objs2, cam2, w=w, rows=rows)
    assert same(after, ref), (scene, change, float(np.nanmax(np.abs(after - ref))))
    assert same(after2, ref), (scene, change, "the frame after the change, again")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", LIST_SCENES)
def test_a_smaller_scratch_limit_then_the_default(gpu, scene):
    """under a limit of which the lists would take more than a quarter the packets walk (no lists); back at the default they are built"""
    from rust_raytracing_amd import scenes
    objs, hnd = _resident(gpu, scene)
    ref = _exact(gpu, objs, scenes.CAMERA)
    assert same(_frame(hnd), ref)
    assert hnd.debug_tile_lists()["builds"] == 1
    hnd.set_scratch_limit(1 << 16)
    small = _frame(hnd)
    lists = hnd.debug_tile_lists()
    assert lists["form"] == 0 and lists["builds"] == 1, (lists["form"], lists["builds"])
    hnd.set_scratch_limit(0)
    back = _frame(hnd)
    lists = hnd.debug_tile_lists()
    assert lists["form"] != 0 and lists["builds"] == 2, (lists["form"], lists["builds"])
    assert same(_frame(hnd), ref) and hnd.debug_tile_lists()["builds"] == 2
    hnd.close()
    assert same(small, ref) and same(back, ref), scene
