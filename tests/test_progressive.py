"""Progressive sampling (rtx_render_blocks_accumulate): a range of every pixel's samples added to the caller's running sums of the
samples and of their squares, so that ranges which tile [0, S) in order leave sum / S == the render at rays_per_pixel = S, bit for bit.

The yardsticks: the render itself (rtx_render_rows) for the sums, and for both moments the per-sample colours of
progressive_cases.replay -- the exhaustive kernel's path transcripts replayed over the materials -- folded with plain numpy adds; the
lab hook rtx_debug_resolve_moments is held to Python float loops.  Every comparison is exact (helpers.same / bytes)."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import DEFAULT_CAM, hip_scene, same
from progressive_cases import CAMERA_B, CASES, band_rows, case, check_census, left_fold, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtx_hip.h")
RUST_SHIM = os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")
NEW_FNS = ("rtx_render_blocks_accumulate", "rtx_scene_trace_samples", "rtx_trace_samples", "rtx_debug_resolve_moments")
GUARD = 96                                           # doubles of NaN behind each buffer: must come back untouched
NAN = float("nan")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_header_abi_libraries_and_rust_shim_carry_the_new_entry_points(rtx):
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    shim = open(RUST_SHIM).read()
    for fn in NEW_FNS:
        assert re.search(r"\b%s\s*\(" % fn, hdr), fn
        assert fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        assert re.search(r"\bpub fn %s\s*\(" % fn, shim), fn
        for lab in (False, True):
            assert getattr(rtx.load_library(lab), fn) is not None, (fn, lab)
    # the lab hook is the lab library's: the product refuses it before it looks at an argument
    assert rtx.load_library().rtx_debug_resolve_moments(None, None, 13, 11, 0, 0, None, 0, None, 0) == rtx.abi.RTX_ERR_UNSUPPORTED


def test_the_product_library_gained_no_kernel_and_the_sphere_query_kernel_no_spill(rtx):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    rows = kernel_instances.kernels(rtx.abi.LIB_PATH)
    names = sorted(r["name"] for r in rows)
    assert len(names) <= 25, names
    assert names.count("resolve_kernel") == 1, names                    # the squares' accumulator is an argument, not an instance
    sph = [r for r in rows if r["name"] == "query_closest_kernel<false>"]
    assert len(sph) == 1, sph
    print("query_closest_kernel<false>:", sph[0])
    print("resolve_kernel:", [r for r in rows if r["name"] == "resolve_kernel"][0])
    assert sph[0]["vgpr_spill"] == 0 and sph[0]["vgpr"] <= 128, sph[0]


def test_accumulate_argument_checks_touch_no_device(rtx):
    lib = rtx.load_library()
    bad = rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert lib.rtx_render_blocks_accumulate(None, 8, 8, 8, 0, 1, 0, 1, None, None, None, None) == bad
    assert b"null scene" in lib.rtx_last_error()


# ----------------------------------------------------------------------------------------------------------------- GPU
def _handle(gpu, name, kernel=None, tuning=0, cam=None):
    objs, w, h, c, cfg = case(name)
    return hip_scene(gpu, objs, cam=cam or c, kernel=kernel, tuning=tuning, **cfg).upload(0)


def _buffers(torch, n_rows, w, fill, moments=True):
    """(sum, sum_sq or None): n_rows * w * 3 doubles of `fill` each, GUARD doubles of NaN behind them"""
    def one():
        t = torch.full((n_rows * w * 3 + GUARD,), NAN, dtype=torch.float64, device="cuda:0")
        t[:n_rows * w * 3] = fill
        return t
    return one(), (one() if moments else None)


def _host(t, n_rows, w):
    """a buffer's pixels [n_rows][w][3]; its guard must still be NaN"""
    a = t.cpu().numpy()
    assert np.isnan(a[n_rows * w * 3:]).all(), "the guard behind the buffer was written"
    return a[:n_rows * w * 3].reshape(n_rows, w, 3).copy()


def accumulate(gpu, hnd, w, h, ranges, moments=True, part=(8, 0, 1), fill=0.0, want_stats=True):
    """the calls `ranges` = [(sample_begin, n_samples), ...] into fresh buffers -> (sum, sum_sq or None [rows][w][3], the calls' stats)"""
    import torch
    n_rows = len(band_rows(h, *part))
    total, sq = _buffers(torch, n_rows, w, fill, moments)
    torch.cuda.synchronize()
    stats = [hnd.render_accumulate(w, h, a, n, total.data_ptr(), sq.data_ptr() if sq is not None else None, *part, want_stats=want_stats)
             for a, n in ranges]
    torch.cuda.synchronize()
    return _host(total, n_rows, w), (_host(sq, n_rows, w) if sq is not None else None), stats


def _render_rows(hnd, w, h):
    import torch
    buf = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    return buf.cpu().numpy(), st


def _variants(gpu):
    return [("mixed", None, 0), ("mesh", None, 0), ("joint", None, 0), ("axis-aligned mesh", None, 0), ("spheres", None, 0),
            ("spheres", None, gpu.RTX_TUNE_TWO_STAGE), ("mixed", gpu.RTX_KERNEL_EXACT, 0), ("mixed", gpu.RTX_KERNEL_MIXED, 0),
            ("mesh", gpu.RTX_KERNEL_WAVEFRONT, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("v", range(9))
def test_any_split_of_the_range_gives_the_render(gpu, v):
    """one call [0, S), S calls of one sample and (1, S - 1): identical sums, sum / S == rtx_render_rows of the same config; the parts
    (8, 1, 3) and (1, 1, 2) equal the matching rows of the full-frame result byte for byte"""
    name, kernel, tuning = _variants(gpu)[v]
    objs, w, h, cam, cfg = case(name)
    S = cfg["rays_per_pixel"]
    hnd = _handle(gpu, name, kernel, tuning)
    img, st_img = _render_rows(hnd, w, h)
    assert img.any()
    one, one_sq, st = accumulate(gpu, hnd, w, h, [(0, S)])
    assert st[0].primary_rays == w * h * S and st[0].kernel == st_img.kernel and st[0].segments == st_img.segments
    assert st[0].trace_launches == st_img.trace_launches
    assert same(one / float(S), img), (name, kernel, tuning)
    for ranges in ([(s, 1) for s in range(S)], [(0, 1), (1, S - 1)]):
        total, sq, _ = accumulate(gpu, hnd, w, h, ranges)
        assert total.tobytes() == one.tobytes() and sq.tobytes() == one_sq.tobytes(), (name, kernel, tuning, ranges)
    for part in ((8, 1, 3), (1, 1, 2)):
        rows = band_rows(h, *part)
        assert len(rows) == gpu.load_library().rtx_blocks_row_count(h, *part)
        total, sq, _ = accumulate(gpu, hnd, w, h, [(0, 2), (2, S - 2)] if S > 2 else [(0, S)], part=part)
        assert total.tobytes() == one[rows].tobytes() and sq.tobytes() == one_sq[rows].tobytes(), (name, kernel, tuning, part)
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_both_moments_equal_plain_folds_of_the_replayed_samples(gpu, name):
    """a reference that never runs the new code: the transcripts' per-sample colours c, folded in sample order with numpy adds -- sum of
    c and sum of c * c (numpy multiplies and adds separately: no fused operation) -- equal d_sum and d_sum_sq; without d_sum_sq the same
    d_sum; the NaN guards behind both buffers stay NaN (accumulate checks them)"""
    objs, w, h, cam, cfg = case(name)
    S = cfg["rays_per_pixel"]
    colour = replay(gpu, name)["colour"]
    check_census(name, colour)
    hnd = _handle(gpu, name)
    total, sq, _ = accumulate(gpu, hnd, w, h, [(0, S)])
    assert same(total, left_fold(colour)), name
    assert same(sq, left_fold(colour * colour)), name
    alone, none, _ = accumulate(gpu, hnd, w, h, [(0, 1), (1, S - 1)], moments=False)
    assert none is None and alone.tobytes() == total.tobytes()
    # a later range on its own is the fold of those samples from zero
    part, part_sq, _ = accumulate(gpu, hnd, w, h, [(1, S - 1)])
    assert same(part, left_fold(colour[:, :, 1:])) and same(part_sq, left_fold((colour * colour)[:, :, 1:])), name
    hnd.close()


@pytest.mark.gpu
def test_sample_batches_inside_a_call_keep_the_bits(gpu):
    """a scratch limit below one sample's floor: one sample per launch, five launches for five samples, the fold continued in the
    caller's buffers from batch to batch"""
    objs, w, h, cam, cfg = case("spheres")
    hnd = _handle(gpu, "spheres")
    one, one_sq, st = accumulate(gpu, hnd, w, h, [(0, 5)])
    assert st[0].trace_launches == 1
    hnd.set_scratch_limit(1 << 12)
    cut, cut_sq, st = accumulate(gpu, hnd, w, h, [(0, 5)])
    assert st[0].trace_launches >= 2, st[0].trace_launches
    assert cut.tobytes() == one.tobytes() and cut_sq.tobytes() == one_sq.tobytes()
    two, two_sq, st = accumulate(gpu, hnd, w, h, [(0, 2), (2, 3)])
    assert [s.trace_launches for s in st] == [2, 3]
    assert two.tobytes() == one.tobytes() and two_sq.tobytes() == one_sq.tobytes()
    hnd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spheres", "mesh"])
def test_every_call_rebuilds_the_tile_lists(gpu, name):
    """[0, 2) under camera A, set_camera(B), [2, 5) into fresh zero buffers: the range as a fresh handle uploaded with camera B gives it
    (the primary rays' tile lists are per camera: a call that reused the previous call's would walk the wrong candidates)"""
    kernel, tuning = (None, gpu.RTX_TUNE_TWO_STAGE) if name == "spheres" else (gpu.RTX_KERNEL_WAVEFRONT, 0)
    objs, w, h, cam, cfg = case(name)
    hnd = _handle(gpu, name, kernel, tuning)
    first, _, st = accumulate(gpu, hnd, w, h, [(0, 2)])
    assert first.any() and st[0].kernel == (gpu.RTX_KERNEL_BVH if name == "spheres" else gpu.RTX_KERNEL_WAVEFRONT)
    hnd.set_camera(gpu.Camera(*CAMERA_B))
    moved, moved_sq, _ = accumulate(gpu, hnd, w, h, [(2, 3)])
    hnd.close()
    fresh = _handle(gpu, name, kernel, tuning, cam=CAMERA_B)
    want, want_sq, _ = accumulate(gpu, fresh, w, h, [(2, 3)])
    fresh.close()
    exact = _handle(gpu, name, gpu.RTX_KERNEL_EXACT, 0, cam=CAMERA_B)                  # (and the exhaustive kernel, which has no lists)
    swept, swept_sq, _ = accumulate(gpu, exact, w, h, [(2, 3)])
    exact.close()
    assert want.any() and want.tobytes() != first.tobytes()
    assert moved.tobytes() == want.tobytes() and moved_sq.tobytes() == want_sq.tobytes(), name
    assert swept.tobytes() == want.tobytes() and swept_sq.tobytes() == want_sq.tobytes(), name


@pytest.mark.gpu
def test_no_ops_refusals_and_the_asynchronous_call(gpu):
    import torch
    objs, w, h, cam, cfg = case("mixed")
    hnd = _handle(gpu, "mixed")
    # n_samples == 0: NaN-filled buffers stay NaN-filled
    total, sq, st = accumulate(gpu, hnd, w, h, [(0, 0), (7, 0)], fill=NAN)
    assert np.isnan(total).all() and np.isnan(sq).all() and st[0].primary_rays == 0 and st[0].trace_launches == 0
    # a scene without objects: every sample is zero, nothing is touched
    empty = gpu.Scene.from_packed(gpu.Config(rays_per_pixel=4), gpu.Camera(*DEFAULT_CAM), np.zeros(0, dtype=gpu.OBJECT_DTYPE)).upload(0)
    total, sq, st = accumulate(gpu, empty, w, h, [(0, 3)], fill=NAN)
    assert np.isnan(total).all() and np.isnan(sq).all() and st[0].primary_rays == w * h * 3 and st[0].trace_launches == 0
    empty.close()
    # refusals: a range past 2^32 - 1, a null d_sum, a bad partition; the buffers stay as they were
    buf, _ = _buffers(torch, h, w, NAN, moments=False)
    for begin, n in (((1 << 32) - 3, 3), (1 << 32, 1), (0, 1 << 32), ((1 << 64) - 1, 2)):
        with pytest.raises(gpu.RtxError) as e:
            hnd.render_accumulate(w, h, begin, n, buf.data_ptr())
        assert e.value.status == gpu.abi.RTX_ERR_INVALID_ARGUMENT, (begin, n)
    for args, kw in (((w, h, 0, 1, None), {}), ((w, h, 0, 1, buf.data_ptr()), dict(block_rows=0)),
                     ((w, h, 0, 1, buf.data_ptr()), dict(part=2, n_parts=2)), ((w, h, 0, 1, buf.data_ptr(), buf.data_ptr() + 8), {})):
        with pytest.raises(gpu.RtxError) as e:
            hnd.render_accumulate(*args, **kw)
        assert e.value.status == gpu.abi.RTX_ERR_INVALID_ARGUMENT, (args, kw)
    torch.cuda.synchronize()
    assert np.isnan(buf.cpu().numpy()).all()
    # the last samples a range may name: [2^32 - 3, 2^32 - 1) is accepted and equals trace_samples' of the same ids, folded
    edge, _, _ = accumulate(gpu, hnd, w, h, [((1 << 32) - 3, 2)], moments=False)
    pix = np.arange(w * h, dtype=np.uint64)
    ids = np.stack([np.tile(pix, 2), np.repeat(np.array([(1 << 32) - 3, (1 << 32) - 2], dtype=np.uint64), w * h)], axis=1)
    d_ids = torch.from_numpy(ids.view(np.int64)).to("cuda:0")
    d_rgb = torch.empty(len(ids) * 3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    hnd.trace_samples(w, h, d_ids.data_ptr(), len(ids), d_rgb.data_ptr())
    rgb = d_rgb.cpu().numpy().reshape(2, h, w, 3)
    assert edge.any() and same(edge, (np.zeros((h, w, 3)) + rgb[0]) + rgb[1])
    # stats == NULL: asynchronous on the caller's stream; after a sync the same bits
    ref, ref_sq, _ = accumulate(gpu, hnd, w, h, [(0, 2), (2, 2)])
    stream = torch.cuda.Stream("cuda:0")
    total, sq = _buffers(torch, h, w, 0.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for a, n in ((0, 2), (2, 2)):
            assert hnd.render_accumulate(w, h, a, n, total.data_ptr(), sq.data_ptr(), stream=stream.cuda_stream, want_stats=False) is None
    torch.cuda.synchronize()
    assert _host(total, h, w).tobytes() == ref.tobytes() and _host(sq, h, w).tobytes() == ref_sq.tobytes()
    hnd.close()


# ---- the lab hook: launch_resolve with first = last = 0 and a squares buffer, against Python float loops
HW, HH, HS = 13, 11, 3                               # 143 pixels: 2 x 2 tiles of 8 x 8, partial on both edges; 3 samples
SPECIALS = [(0.0, -0.0, 5.0), (-0.0, 1.5, 0.0), (NAN, 1.0, -2.0), (float("inf"), -1.0, 0.25), (-float("inf"), float("inf"), 3.0),
            (1e200, -1e200, 1e-200), (1e-200, 1e-160, -1e-200), (1e200, 2.0, 1e200), (0.1, 0.2, 0.3), (-0.7, 1e16, 1.0)]


def _hook_inputs(tiled):
    """records [3 * per_sample][4], which of them are set [3 * per_sample], the local pixel of every slot of a sample (-1: padding)"""
    rng = np.random.default_rng(77 + int(tiled))
    if tiled:
        tiles_x, tiles_y = (HW + 7) // 8, (HH + 7) // 8
        t = np.arange(tiles_x * tiles_y * 64)
        tile, j = t // 64, t % 64
        x, k = (tile % tiles_x) * 8 + j % 8, (tile // tiles_x) * 8 + j // 8
        pix = np.where((x < HW) & (k < HH), k * HW + x, -1)
    else:
        pix = np.arange(HW * HH)
    per = len(pix)
    rec = np.full((HS * per, 4), NAN)                                            # NaN garbage under every clear bit and in the fourth double
    bits = (rng.random(HS * per) < 0.6) & np.tile(pix >= 0, HS)
    vals = 10.0 ** rng.uniform(-8, 8, (HS * per, 3)) * rng.choice([-1.0, 1.0], (HS * per, 3))
    special = rng.integers(0, 3 * len(SPECIALS), HS * per)
    for k, sp in enumerate(SPECIALS):
        vals[special == k] = sp
    rec[bits, :3] = vals[bits]
    for k in range(len(SPECIALS)):
        assert (bits & (special == k)).any(), k
    return rec, bits, pix


def _python_moments(rec, bits, pix, start, start_sq):
    total, sq = [float(v) for v in start], [float(v) for v in start_sq]
    per = len(pix)
    for s in range(HS):
        for slot in range(per):
            if bits[s * per + slot]:
                p = int(pix[slot])
                for c in range(3):
                    v = float(rec[s * per + slot, c])
                    total[3 * p + c] = total[3 * p + c] + v
                    sq[3 * p + c] = sq[3 * p + c] + v * v
    return np.array(total), np.array(sq)


@pytest.mark.gpu
@pytest.mark.parametrize("tiled", (False, True))
def test_the_moments_hook_equals_python_float_loops(gpu, tiled):
    from test_support_kernels import pack_mask
    rec, bits, pix = _hook_inputs(tiled)
    rng = np.random.default_rng(5)
    n = 3 * HW * HH
    start = np.concatenate([rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n), np.full(GUARD, NAN)])
    start_sq = np.concatenate([rng.random(n) * 10.0 ** rng.uniform(-3, 3, n), np.full(GUARD, NAN)])
    start[:6], start_sq[:6] = 0.0, 0.0
    want, want_sq = _python_moments(rec, bits, pix, start[:n], start_sq[:n])
    assert np.isinf(want_sq).any() and np.isnan(want).any() and (want_sq[~np.isnan(want_sq)] >= 0).all()
    got, got_sq = gpu.debug_resolve_moments(rec, pack_mask(bits), HW, HH, tiled, HS, start, start_sq)
    assert np.isnan(got[n:]).all() and np.isnan(got_sq[n:]).all()
    assert same(got[:n], want) and same(got_sq[:n], want_sq), tiled
    alone, none = gpu.debug_resolve_moments(rec, pack_mask(bits), HW, HH, tiled, HS, start, None)
    assert none is None and same(alone[:n], want)
    # the hook with no squares buffer is rtx_debug_resolve with first = last = 0
    _, acc = gpu.debug_resolve(rec, pack_mask(bits), HW, HH, tiled, HS, HS, first=False, last=False, acc=start)
    assert same(acc, alone)
