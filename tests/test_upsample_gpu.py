"""rtx_upsample_device / rtx_upsample on the GPU against tests/upsample_model.py: out and var_out must equal the model's array reading as
uint64 patterns (one pattern for every NaN: the device's default NaN is +NaN, x86's is -NaN, and the header promises values) -- on
fuzzed hostile frames at low sizes and factors that put output pixels off every workgroup multiple, through a handle on rendered frames
of the golden scenes (Progressive and Temporal), and through the example.  Then the one quality condition with the device's own
lens-jittered features: the guided frame is nearer the same handle's 256-spp frame than the bilinear one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_model as dm
import upsample_model as um
from helpers import hip_scene
from upsample_cases import GUIDES, QUALITY, bilinear_params, bits_equal, fuzz_case, model_params, option_sets, params_record, rmse, to_records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOW_SIZES = [(1, 1), (3, 2), (9, 7), (33, 17), (23, 11)]                  # (wl, hl)
FACTORS = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _golden(gpu, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    objs = np.frombuffer(z["objects"].tobytes(), dtype=gpu.OBJECT_DTYPE)
    return objs, int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def run_device(gpu, lo, hi, p, stream=None, want_var_out=True):
    """rtx_upsample_device on device copies of a case; d_out and d_var_out hold NaN bytes beforehand -> (out, var_out)"""
    import torch
    dev = torch.device("cuda", 0)
    lib = gpu.load_library()
    h, w = hi["depth"].shape
    rec = params_record(gpu.UPSAMPLE_PARAMS_DTYPE, p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    with_var = lo.get("var") is not None
    d_lo, d_lo_feat, d_feat = up(np.asarray(lo["rgb"], dtype=np.float64)), up(to_records(gpu.FEATURE_DTYPE, lo)), up(to_records(gpu.FEATURE_DTYPE, hi))
    d_var = up(np.asarray(lo["var"], dtype=np.float64)) if with_var else None
    nan_bytes = lambda n: torch.full((max(int(n), 16),), 255, dtype=torch.uint8, device=dev)
    d_out = nan_bytes(24 * w * h)
    d_vout = nan_bytes(24 * w * h) if (with_var and want_var_out) else None
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    gpu.abi.check(lib.rtx_upsample_device(ptr(d_lo), ptr(d_var), ptr(d_lo_feat), ptr(d_feat), w, h, rec.ctypes.data, ptr(d_out), ptr(d_vout), 0,
                                          stream.cuda_stream if stream is not None else None), lib)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    out = d_out[:24 * w * h].cpu().numpy().view(np.float64).reshape(h, w, 3)
    vout = d_vout[:24 * w * h].cpu().numpy().view(np.float64).reshape(h, w, 3) if d_vout is not None else None
    return out, vout


def check(gpu, lo, hi, p, what):
    out, vout = run_device(gpu, lo, hi, p)
    want, vwant = um.upsample(lo, hi, p)
    bad = int((~np.isclose(out, want, rtol=0, atol=0, equal_nan=True)).sum())
    assert bits_equal(out, want), "%s: out differs from the model on %d values" % (what, bad)
    assert (vout is None) == (vwant is None)
    if vout is not None:
        assert bits_equal(vout, vwant), "%s: var_out differs from the model" % (what,)
    return out, vout


_FUZZ = {}


def fuzz(wl, hl, s):
    if (wl, hl, s) not in _FUZZ:
        _FUZZ[(wl, hl, s)] = fuzz_case(np.random.default_rng(10000 * wl + 10 * hl + s), hl, wl, s)
    return _FUZZ[(wl, hl, s)]


FULL = dict(option_sets()[0][1])


@pytest.mark.parametrize("wl,hl", LOW_SIZES, ids=["%dx%d" % s for s in LOW_SIZES])
def test_fuzzed_frames_equal_the_model(gpu, wl, hl):
    """every factor, with and without the variance, demodulated and not: outputs from 1 x 1 to 264 x 136 (141 workgroups; rows of 23,
    33, 46, 66, 69, 99 ... pixels put a workgroup's 256 pixels on several rows and a wave across a row's end)"""
    for s in FACTORS:
        lo, hi = fuzz(wl, hl, s)
        assert wl * hl < 50 or (not np.isfinite(lo["rgb"]).all() and np.isinf(hi["depth"]).any())
        for flags in (um.DEMODULATE, 0):
            p = um.Params(factor=s, **dict(FULL, flags=flags))
            out, _ = check(gpu, lo, hi, p, "%dx%d x%d flags %d" % (wl, hl, s, flags))
            check(gpu, dict(lo, var=None), hi, p, "%dx%d x%d flags %d, no variance" % (wl, hl, s, flags))
    assert wl * hl < 50 or np.isfinite(out).any()


@pytest.mark.parametrize("name,fields,with_var", option_sets(), ids=[o[0] for o in option_sets()])
def test_every_term_and_flag_equals_the_model(gpu, name, fields, with_var):
    for (wl, hl), s in (((9, 7), 3), ((33, 17), 2), ((3, 2), 8), ((23, 11), 4)):
        lo, hi = fuzz(wl, hl, s)
        check(gpu, lo if with_var else dict(lo, var=None), hi, um.Params(factor=s, **fields), "%s, %dx%d x%d" % (name, wl, hl, s))


def test_factor_one_without_demodulation_copies_the_finite_bytes(gpu):
    lo, hi = fuzz(23, 11, 1)
    out, vout = run_device(gpu, lo, hi, um.Params(factor=1, **dict(FULL, flags=0)))
    fin = np.isfinite(lo["rgb"])
    assert np.array_equal(out.view(np.uint64)[fin], np.ascontiguousarray(lo["rgb"]).view(np.uint64)[fin]) and (out.view(np.uint64)[~fin] == 0).all()
    assert bits_equal(vout[fin], lo["var"][fin])


def test_a_variance_output_is_optional(gpu):
    lo, hi = fuzz(33, 17, 2)
    p = um.Params(factor=2, **FULL)
    out, vout = run_device(gpu, lo, hi, p, want_var_out=False)
    assert vout is None and bits_equal(out, um.upsample(lo, hi, p)[0])


def test_side_stream_repeatability_and_the_host_form(gpu):
    import torch
    (lo, hi), p = fuzz(33, 17, 3), um.Params(factor=3, **FULL)
    first = run_device(gpu, lo, hi, p)
    again = run_device(gpu, lo, hi, p)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()          # the same bytes, NaNs included
    side = run_device(gpu, lo, hi, p, stream=torch.cuda.Stream(device=0))                                # read only after its sync
    assert side[0].tobytes() == first[0].tobytes() and side[1].tobytes() == first[1].tobytes()
    # the host form, through the Python wrapper and the tuple features() returns
    tup = lambda g: tuple(g[k] for k in GUIDES) + (np.ones(g["depth"].shape), np.zeros(g["depth"].shape, dtype=np.int64))
    kw = dict(flags=p.flags, normal_power_log2=p.normal_power_log2, sigma_depth=p.sigma_depth, sigma_albedo=p.sigma_albedo,
              albedo_min=p.albedo_min, min_weight=p.min_weight)
    host, host_v = gpu.upsample(lo["rgb"], tup(lo), tup(hi), 3, variance=lo["var"], **kw)
    assert host.tobytes() == first[0].tobytes() and host_v.tobytes() == first[1].tobytes()
    only = gpu.upsample(lo["rgb"], to_records(gpu.FEATURE_DTYPE, lo), to_records(gpu.FEATURE_DTYPE, hi), 3, **kw)
    assert bits_equal(only, um.upsample(dict(lo, var=None), hi, p)[0])
    with pytest.raises(gpu.RtxError):
        gpu.upsample(lo["rgb"], tup(lo), tup(hi), 3, sigma_depth=-1.0)
    with pytest.raises(TypeError):
        gpu.upsample(lo["rgb"], tup(lo), tup(hi), 3, sigma_color=1.0)


# ---- rendered frames --------------------------------------------------------------------------------------------------------------
def _guides(gpu, t, h, w):
    """the guides of a device feature buffer (a torch uint8 tensor) as the model's dict"""
    f = t.cpu().numpy().view(gpu.FEATURE_DTYPE).reshape(h, w)
    return {k: np.ascontiguousarray(f[k]) for k in GUIDES}


@pytest.mark.parametrize("name", ["mixed_40x24", "c1_three_spheres_32x32"])
def test_progressive_and_temporal_upsample_equal_the_model_on_the_devices_own_buffers(gpu, name):
    """through a handle at s = 2: the Progressive 4-spp low mean and variance and the device's features of both sizes go to upsample();
    the result equals the model fed with the device's own buffers.  The same through Temporal after three frames -- its accumulated
    mean and variance, and its denoised frame."""
    objs, w, h, cfg = _golden(gpu, name)
    s, wl, hl = 2, w // 2, h // 2
    hnd = hip_scene(gpu, objs, **dict(cfg, rays_per_pixel=4)).upload(0)
    p = model_params(gpu, s)
    prog = hnd.progressive(wl, hl)
    prog.add(4)
    out, f_lo, f_hi = prog.upsample(s, return_features=True)
    assert tuple(out.shape) == (h, w, 3) and out.is_cuda
    lo = dict(_guides(gpu, f_lo, hl, wl), rgb=prog.mean(), var=prog.variance())
    hi = _guides(gpu, f_hi, h, w)
    assert bits_equal(out.cpu().numpy(), um.upsample(lo, hi, p)[0]), "Progressive.upsample, %s" % name
    assert np.isfinite(out.cpu().numpy()).all() and float(out.abs().max()) > 0
    one = hnd.progressive(wl, hl)
    one.add(1)                                                            # one sample: no variance goes along
    assert bits_equal(one.upsample(s, min_weight=0.0).cpu().numpy(),
                      um.upsample(dict(lo, rgb=one.mean(), var=None), hi, p.replace(min_weight=0.0))[0])
    temp = hnd.temporal(wl, hl)
    for _ in range(3):
        temp.frame(4)
    out = temp.upsample(s).cpu().numpy()
    lo_t = dict(lo, rgb=temp.mean(), var=temp.variance())
    assert lo_t["var"] is not None and bits_equal(out, um.upsample(lo_t, hi, p)[0]), "Temporal.upsample, %s" % name
    den = temp.denoise(on_device=True)                                    # the denoised frame stays on the device ...
    assert den.is_cuda and bits_equal(den.cpu().numpy(), temp.denoise())
    out = temp.upsample(s, frame=den).cpu().numpy()
    den = den.cpu().numpy()
    assert bits_equal(out, um.upsample(dict(lo, rgb=den, var=None), hi, p)[0]), "Temporal.upsample of the denoised frame, %s" % name
    assert bits_equal(out, temp.upsample(s, frame=den).cpu().numpy())     # ... and a host array gives the same
    assert bits_equal(prog.upsample(s, frame=prog.denoise(on_device=True)).cpu().numpy(),
                      um.upsample(dict(lo, rgb=prog.denoise(), var=None), hi, p)[0]), "Progressive.upsample of the denoised frame, %s" % name
    assert not bits_equal(out, um.upsample(lo_t, hi, p)[0])
    hnd.close()


@pytest.mark.parametrize("name,s", QUALITY)
def test_the_guided_frame_is_nearer_the_converged_one_than_the_bilinear_one(gpu, name, s):
    """the quality condition with the device's lens-jittered features and the library's defaults: the low frame at 4 s^2 spp with its
    variance, the features of both sizes from the same handle (at 4 s^2 rays per pixel), RMSE(guided, 256 spp) < RMSE(bilinear, 256
    spp), the 256-spp frame being the same handle's at the full size.  A condition, not a tuned number."""
    objs, w, h, cfg = _golden(gpu, name)
    wl, hl, spp = w // s, h // s, 4 * s * s
    hnd = hip_scene(gpu, objs, **dict(cfg, rays_per_pixel=spp)).upload(0)
    prog = hnd.progressive(wl, hl)
    prog.add(spp)
    lo = dict(rgb=prog.mean(), var=prog.variance())
    lo["albedo"], lo["emission"], lo["normal"], lo["depth"], _, _ = hnd.features(wl, hl)
    hi = dict(zip(GUIDES, hnd.features(w, h)[:4]))
    full = hnd.progressive(w, h, moments=False)
    full.add(256)
    ref = full.mean()
    hnd.close()
    guided, _ = run_device(gpu, lo, hi, model_params(gpu, s))
    bilinear, _ = run_device(gpu, dict(lo, var=None), hi, bilinear_params(s))
    nearest = np.repeat(np.repeat(lo["rgb"], s, axis=0), s, axis=1)
    g, b, n = rmse(guided, ref), rmse(bilinear, ref), rmse(nearest, ref)
    print("%s, s = %d, device features: RMSE against 256 spp: nearest %.4f, bilinear %.4f, guided %.4f (ratio %.3f)" % (name, s, n, b, g, g / b))
    assert np.isfinite(guided).all()
    assert g < b


def test_the_upsample_example(gpu, tmp_path):
    """examples/upsample.cpp (Resident::upsample of rtx.hpp): 8 spp at half size, features at both sizes, denoise, upsample x2, quantize
    -- its frame is the two models chained on the same sums, its PPM the oracle's quantisation of that"""
    exe = os.path.join(ROOT, "examples", "upsample")
    assert os.path.exists(exe), "examples/upsample is built by __graft_entry__.build()"
    w, h, spp = 40, 24, 8
    wl, hl = w // 2, h // 2
    ppm, raw = tmp_path / "out.ppm", tmp_path / "out.f64"
    done = subprocess.run([exe, str(w), str(h), str(ppm), str(spp), str(raw)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert subprocess.run([exe, "41", "24", str(ppm)], capture_output=True, timeout=120).returncode == 2     # an odd width: no lattice
    objs = np.zeros(5, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene (examples/denoise.cpp's)
    for k, (kind, geom, base_c, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (7, 1.6, 0.3, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (5, -3, 2, 0.6), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-8, -8, -1.5, 30, -8, -1.5, 8, 20, -1.5), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base_c, em, rough
    hnd = hip_scene(gpu, objs, rays_per_pixel=spp).upload(0)
    prog = hnd.progressive(wl, hl)
    prog.add(spp)
    sm, q, n = prog.sum.cpu().numpy(), prog.sum_sq.cpu().numpy(), float(spp)
    lo = dict(rgb=sm / n, var=(q - sm * sm / n) / (n - 1.0) / n)
    lo["albedo"], lo["emission"], lo["normal"], lo["depth"], _, _ = hnd.features(wl, hl)
    hi = dict(zip(GUIDES, hnd.features(w, h)[:4]))
    hnd.close()
    d = gpu.denoise_params()
    dp = dm.Params(**{k: d[k].item() for k in ("passes", "flags", "normal_power_log2", "sigma_color", "sigma_depth", "sigma_albedo", "epsilon",
                                               "albedo_min")})
    den, _ = dm.denoise(lo["rgb"], lo["var"], lo["albedo"], lo["emission"], lo["normal"], lo["depth"], dp)
    want, _ = um.upsample(dict(lo, rgb=den, var=None), hi, model_params(gpu, 2))
    got = np.fromfile(raw, dtype=np.float64).reshape(h, w, 3)
    assert bits_equal(got, want)
    from oracle import rtx_oracle
    rtx_oracle.build()
    head = b"P6\n%d %d\n255\n" % (w, h)
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and data[len(head):] == rtx_oracle.quantize_image(want).tobytes()


def test_the_product_library_keeps_its_instance_count_and_the_epilogue_its_limits(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    rows = kernel_instances.kernels(gpu.abi.LIB_PATH)
    names = sorted(r["name"] for r in rows)
    assert len(names) <= 25 and "epilogue_kernel" in names, names          # the upsampling is a form of epilogue_kernel, not a new kernel
    ep = [r for r in rows if r["name"] == "epilogue_kernel"][0]
    assert ep["vgpr"] <= 128 and ep["vgpr_spill"] == 0 and ep["scratch"] == 0 and ep["lds"] == 0, ep
