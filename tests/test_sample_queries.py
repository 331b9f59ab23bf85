"""Sparse samples of the render (rtx_scene_trace_samples, rtx_trace_samples) and the Python Progressive helper on top of them.

Entry i names (pixel, sample); the kernel builds render_pixel's own ray for it and runs render_ray, so the entry is that sample of the
render bit for bit, wherever it stands in the batch.  The yardsticks: progressive_cases.replay (the exhaustive render kernel's path
transcripts replayed over the materials), the render itself, and rtx_scene_trace_paths fed the transcripts' first rays.  Every
comparison is exact (helpers.same / bytes)."""
import ctypes as C

import numpy as np
import pytest

from helpers import DEFAULT_CAM, hip_scene, same
from progressive_cases import CASES, case, left_fold, replay


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_host_form_and_null_handle_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    bad, ok = rtx.abi.RTX_ERR_INVALID_ARGUMENT, rtx.abi.RTX_OK
    assert lib.rtx_trace_samples(None, 8, 8, None, 5, None, None) == bad
    sc = rtx.abi.RtxScene()
    sc.config.rays_per_pixel = 1
    assert lib.rtx_trace_samples(C.byref(sc), 8, 8, None, 0, None, None) == ok
    ids = np.zeros((3, 2), dtype=np.uint64)
    rgb = np.zeros(9, dtype=np.float64)
    assert lib.rtx_trace_samples(C.byref(sc), 8, 8, None, 3, rgb.ctypes.data, None) == bad                  # null ids
    assert lib.rtx_trace_samples(C.byref(sc), 8, 8, ids.ctypes.data, 3, None, None) == bad                  # null rgb
    for n in ((1 << 32) - 1, 1 << 32, 1 << 40):
        assert lib.rtx_trace_samples(C.byref(sc), 8, 8, ids.ctypes.data, n, rgb.ctypes.data, None) == bad, n
    assert lib.rtx_trace_samples(C.byref(sc), 0, 8, ids.ctypes.data, 3, rgb.ctypes.data, None) == bad        # no pixel to name
    assert lib.rtx_trace_samples(C.byref(sc), 65536, 65536, ids.ctypes.data, 3, rgb.ctypes.data, None) == bad
    assert lib.rtx_scene_trace_samples(None, 8, 8, None, 1, None, None, None, None) == bad


# ----------------------------------------------------------------------------------------------------------------- GPU
def run_samples(hnd, w, h, ids, want_segments=True, **kw):
    """(rgb (n, 3), segments (n,) or None, stats) of rtx_scene_trace_samples on device buffers pre-filled with 7.5 / 77"""
    import torch
    dev = torch.device("cuda", hnd.device)
    ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1, 2)
    n = len(ids)
    d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
    d_rgb = torch.full((max(n, 1) * 3,), 7.5, dtype=torch.float64, device=dev)
    d_seg = torch.full((max(n, 1),), 77, dtype=torch.int32, device=dev) if want_segments else None
    torch.cuda.synchronize(dev)
    st = hnd.trace_samples(w, h, d_ids.data_ptr(), n, d_rgb.data_ptr(), d_seg.data_ptr() if d_seg is not None else None, **kw)
    torch.cuda.synchronize(dev)
    seg = d_seg[:n].cpu().numpy().view(np.uint32) if d_seg is not None else None
    return d_rgb[:3 * n].cpu().numpy().reshape(n, 3), seg, st


def frame_ids(w, h, spp):
    """(pixel, sample) of every sample of a frame, [h][w][S] order -> (h * w * S, 2) uint64"""
    pix = np.repeat(np.arange(w * h, dtype=np.uint64), spp)
    return np.stack([pix, np.tile(np.arange(spp, dtype=np.uint64), w * h)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_every_sample_of_the_frame_in_a_shuffled_order(gpu, name):
    import torch
    from test_path_queries import run_paths
    objs, w, h, cam, cfg = case(name)
    S = cfg["rays_per_pixel"]
    ref = replay(gpu, name)
    ids = frame_ids(w, h, S)
    perm = np.random.default_rng(31).permutation(len(ids))
    hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)
    rgb, seg, st = run_samples(hnd, w, h, ids[perm])
    back = np.argsort(perm)
    rgb, seg = rgb[back], seg[back]                                               # frame order again
    assert same(rgb, ref["colour"].reshape(-1, 3)), (name, np.nonzero((rgb != ref["colour"].reshape(-1, 3)).any(axis=1))[0][:5])
    assert np.array_equal(seg, ref["segments"].ravel()), name
    assert st.primary_rays == len(ids) and st.segments == int(ref["segments"].sum()) and st.trace_launches == 1
    assert rgb.any() and (seg > 2).any()
    # the in-order sum / S is the render
    img = np.zeros((h, w, 3), dtype=np.float64)
    d_img = torch.from_numpy(img).to("cuda:0")
    hnd.render_rows(w, h, 0, 1, h, d_img.data_ptr())
    assert same(left_fold(rgb.reshape(h, w, S, 3)) / float(S), d_img.cpu().numpy()), name
    # the path mode fed the transcripts' first rays and the same ids: the same bytes
    first = ref["first"].reshape(-1)[perm]
    p_rgb, p_seg, _ = run_paths(hnd, gpu.make_rays(first["position"], first["direction"]), ids[perm], torch)
    assert p_rgb[back].tobytes() == rgb.tobytes() and p_seg[back].tobytes() == seg.tobytes(), name
    # RTX_KERNEL_EXACT: every segment swept, the same bytes
    hnd.set_config(gpu.Config(kernel=gpu.RTX_KERNEL_EXACT, **cfg))
    e_rgb, e_seg, st = run_samples(hnd, w, h, ids[perm])
    hnd.close()
    assert st.kernel == gpu.RTX_KERNEL_EXACT and st.box_tests == 0
    assert e_rgb[back].tobytes() == rgb.tobytes() and e_seg[back].tobytes() == seg.tobytes(), name


@pytest.mark.gpu
def test_an_entry_does_not_depend_on_its_batch(gpu):
    objs, w, h, cam, cfg = case("joint")
    S = cfg["rays_per_pixel"]
    hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)
    ids = frame_ids(w, h, S)
    n = len(ids)
    rgb, seg, _ = run_samples(hnd, w, h, ids)
    assert rgb.any() and (seg > 2).sum() > n // 16
    perm = np.random.default_rng(5).permutation(n)
    rp, sp, _ = run_samples(hnd, w, h, ids[perm])
    assert rp.tobytes() == rgb[perm].tobytes() and sp.tobytes() == seg[perm].tobytes()
    for first, k in ((0, 1), (1000, 1), (0, 65), (4321, 65), (2000, 1000)):              # n = 1, the lane 63 / 64 boundary, a slice
        rk, sk, st = run_samples(hnd, w, h, ids[first:first + k])
        assert rk.tobytes() == rgb[first:first + k].tobytes() and sk.tobytes() == seg[first:first + k].tobytes(), (first, k)
        assert st.primary_rays == k and st.segments == int(seg[first:first + k].sum())
    # repeated ids: every copy gets the entry's bytes
    pick = np.random.default_rng(6).integers(0, n, 3000)
    rr, sr, _ = run_samples(hnd, w, h, ids[pick])
    assert len(np.unique(pick)) < len(pick) and rr.tobytes() == rgb[pick].tobytes() and sr.tobytes() == seg[pick].tobytes()
    same_one, _, _ = run_samples(hnd, w, h, np.repeat(ids[777:778], 200, axis=0))
    assert same_one.tobytes() == np.repeat(rgb[777:778], 200, axis=0).tobytes()
    # d_segments == NULL: the same colours
    rn, sn, _ = run_samples(hnd, w, h, ids, want_segments=False)
    assert sn is None and rn.tobytes() == rgb.tobytes()
    # out-of-range entries between valid ones: NaN and 0 segments, nothing traced for them, the valid ones unchanged
    mixed = ids[:4000].copy()
    bad = np.arange(0, 4000, 7)
    mixed[bad[0::3], 0] = w * h                                                           # the first pixel past the frame
    mixed[bad[1::3], 0] = 1 << 40
    mixed[bad[2::3], 1] = 1 << 32                                                         # the first sample index past 2^32 - 1
    mixed[bad[3], 0] = (1 << 64) - 1
    rm, sm, st = run_samples(hnd, w, h, mixed)
    good = np.ones(4000, dtype=bool)
    good[bad] = False
    assert np.isnan(rm[bad]).all() and not sm[bad].any()
    assert rm[good].tobytes() == rgb[:4000][good].tobytes() and sm[good].tobytes() == seg[:4000][good].tobytes()
    assert st.segments == int(seg[:4000][good].sum()) and st.primary_rays == 4000
    # the last pixel and a sample index of 2^32 - 1 are in range
    edge = np.array([[w * h - 1, (1 << 32) - 1], [w * h - 1, S - 1]], dtype=np.uint64)
    re_, se, _ = run_samples(hnd, w, h, edge)
    assert not np.isnan(re_).any() and (se >= 1).all() and re_[1].tobytes() == rgb[-1].tobytes()
    # overlapping arrays are refused; the handle stays good
    import torch
    d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    with pytest.raises(gpu.RtxError):
        hnd.trace_samples(w, h, d_ids.data_ptr(), 100, d_ids.data_ptr() + 8)
    assert run_samples(hnd, w, h, ids[:100])[0].tobytes() == rgb[:100].tobytes()
    # the host form
    h_rgb = np.zeros((500, 3), dtype=np.float64)
    h_seg = np.zeros(500, dtype=np.uint32)
    sc_obj = np.ascontiguousarray(objs, dtype=gpu.OBJECT_DTYPE)
    sc = gpu._scene_c(gpu.Config(**cfg), gpu.Camera(*cam), sc_obj)
    some = np.ascontiguousarray(ids[3000:3500])
    gpu.abi.check(gpu.load_library().rtx_trace_samples(C.byref(sc), w, h, some.ctypes.data, 500, h_rgb.ctypes.data, h_seg.ctypes.data))
    assert h_rgb.tobytes() == rgb[3000:3500].tobytes() and h_seg.tobytes() == seg[3000:3500].tobytes()
    hnd.close()
    # a scene without objects: zeros, no launch, the ids are not read
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=1), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE)).upload(0)
    b, bs, st = run_samples(empty, w, h, mixed)
    assert not b.any() and not np.isnan(b).any() and not bs.any()
    assert st.segments == 0 and st.trace_launches == 0 and st.primary_rays == 4000
    empty.close()


@pytest.mark.gpu
def test_progressive_add_and_refine(gpu):
    """add(2); add(3) is the 5-spp render; refining a random tenth of the pixels by 3 makes those the 8-spp render's and leaves the rest"""
    import torch
    objs, w, h, cam, cfg = case("spheres")
    hnd = hip_scene(gpu, objs, cam=cam, **cfg).upload(0)

    def render(spp):
        hnd.set_config(gpu.Config(**dict(cfg, rays_per_pixel=spp)))
        buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
        return buf.cpu().numpy()

    img5, img8 = render(5), render(8)
    assert img5.any() and img5.tobytes() != img8.tobytes()
    p = hnd.progressive(w, h, moments=True)
    assert isinstance(p, gpu.Progressive) and np.isnan(p.mean()).all()
    p.add(2)
    p.add(3)
    assert int(p.count.min()) == int(p.count.max()) == 5 and p.traced == 5 * w * h
    assert same(p.mean(), img5)
    chosen = np.sort(np.random.default_rng(12).permutation(w * h)[:w * h // 10])
    st = p.refine(chosen, 3)
    assert st.primary_rays == 3 * len(chosen) and p.traced == 5 * w * h + 3 * len(chosen)
    mean = p.mean().reshape(-1, 3)
    rest = np.ones(w * h, dtype=bool)
    rest[chosen] = False
    assert same(mean[chosen], img8.reshape(-1, 3)[chosen]) and same(mean[rest], img5.reshape(-1, 3)[rest])
    assert (img8.reshape(-1, 3)[chosen] != img5.reshape(-1, 3)[chosen]).any()
    count = p.count.cpu().numpy().ravel()
    assert (count[chosen] == 8).all() and (count[rest] == 5).all()
    # both moments of the refined pixels are what eight samples everywhere leave there
    q = hnd.progressive(w, h)
    q.add(8)
    for mine, full in ((p.sum, q.sum), (p.sum_sq, q.sum_sq)):
        assert mine.cpu().numpy().reshape(-1, 3)[chosen].tobytes() == full.cpu().numpy().reshape(-1, 3)[chosen].tobytes()
    var = p.variance()
    assert var.shape == (h, w, 3) and np.isfinite(var).all() and var.any()                 # (an estimate: no bits are pinned)
    with pytest.raises(ValueError):
        p.add(1)                                                                       # the counts differ now
    with pytest.raises(ValueError):
        p.refine([3, 3], 1)
    plain = hnd.progressive(w, h, moments=False)
    plain.add(5)
    assert plain.sum_sq is None and same(plain.mean(), img5)
    hnd.close()


@pytest.mark.gpu
def test_the_adaptive_example_keeps_the_renders_pixels(gpu, tmp_path):
    """examples/adaptive.cpp (Resident::render_blocks_accumulate and trace_samples of rtx.hpp): 4 samples everywhere, 9 on a tenth of the pixels --
    every pixel of its frame is the 4-spp render's or the 9-spp render's, and as many samples were traced as it says"""
    import os
    import re
    import subprocess
    import torch
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "adaptive")
    assert os.path.exists(exe), "examples/adaptive is built by __graft_entry__.build()"
    w, h, base, top = 40, 24, 4, 9
    out = tmp_path / "adaptive.f64"
    done = subprocess.run([exe, str(w), str(h), str(out), str(base), str(top)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    frame = np.fromfile(out, dtype=np.float64).reshape(h * w, 3)
    objs = np.zeros(5, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene
    for k, (kind, geom, base_c, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (7, 1.6, 0.3, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (5, -3, 2, 0.6), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-8, -8, -1.5, 30, -8, -1.5, 8, 20, -1.5), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base_c, em, rough
    hnd = hip_scene(gpu, objs).upload(0)
    imgs = {}
    for spp in (base, top):
        hnd.set_config(gpu.Config(rays_per_pixel=spp))
        buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
        hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
        imgs[spp] = buf.cpu().numpy().reshape(h * w, 3)
    hnd.close()
    coarse = (frame.view(np.uint64) == imgs[base].view(np.uint64)).all(axis=1)
    fine = (frame.view(np.uint64) == imgs[top].view(np.uint64)).all(axis=1)
    assert (coarse | fine).all() and frame.any()
    differ = (imgs[base] != imgs[top]).any(axis=1)
    assert (fine & differ).sum() >= 10 and (fine & differ).sum() <= w * h // 10 and (coarse & differ).sum() >= 10
    traced = w * h * base + (w * h // 10) * (top - base)
    m = re.search(r"(\d+) samples traced, (\d+) for a uniform", done.stdout)
    assert m and int(m.group(1)) == traced and int(m.group(2)) == w * h * top, done.stdout
