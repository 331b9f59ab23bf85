"""rtx_denoise_device / rtx_denoise on the GPU against tests/denoise_model.py: out and var_out must equal the model's array reading as
uint64 patterns (one pattern for every NaN: the device's default NaN is +NaN, x86's is -NaN, and the header promises values) -- on fuzzed
frames with every hostile value, on 4-spp frames of the golden scenes with their own variance and guides, for every term and flag, at
sizes below a tile, off the tile grid and of several workgroups, with steps larger than the frame.  Then the one quality condition:
with the default parameters the denoised 4-spp frame is nearer the 256-spp frame than the 4-spp frame itself."""
import json
import os

import numpy as np
import pytest

import denoise_model as dm
from denoise_cases import bits_equal, fuzz_frame, option_sets, params_of, params_record, to_records
from helpers import hip_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = [(1, 1), (3, 2), (17, 13), (67, 35), (300, 200)]                   # (width, height)
SCENES = ("c1_three_spheres_32x32", "spheres200_48x27", "mixed_40x24", "tris300_32x18")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _golden(gpu, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    objs = np.frombuffer(z["objects"].tobytes(), dtype=gpu.OBJECT_DTYPE)
    return objs, int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def run_device(gpu, fr, p, with_var=True, stream=None, want_var_out=True):
    """rtx_denoise_device on device copies of a frame; d_out, d_var_out and d_work hold NaN bytes beforehand -> (out, var_out)"""
    import torch
    dev = torch.device("cuda", 0)
    lib = gpu.load_library()
    h, w = fr["depth"].shape
    rec = params_record(gpu.DENOISE_PARAMS_DTYPE, p)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_rgb, d_feat = up(np.asarray(fr["rgb"], dtype=np.float64)), up(to_records(gpu.FEATURE_DTYPE, fr))
    d_var = up(np.asarray(fr["var"], dtype=np.float64)) if with_var else None
    nan_bytes = lambda n: torch.full((max(int(n), 16),), 255, dtype=torch.uint8, device=dev)
    d_out = nan_bytes(24 * w * h)
    d_vout = nan_bytes(24 * w * h) if (with_var and want_var_out) else None
    d_work = nan_bytes(gpu.denoise_work_bytes(w, h, rec))
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    gpu.abi.check(lib.rtx_denoise_device(ptr(d_rgb), ptr(d_var), ptr(d_feat), w, h, rec.ctypes.data, ptr(d_out), ptr(d_vout), ptr(d_work), 0,
                                         stream.cuda_stream if stream is not None else None), lib)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    out = d_out[:24 * w * h].cpu().numpy().view(np.float64).reshape(h, w, 3)
    vout = d_vout[:24 * w * h].cpu().numpy().view(np.float64).reshape(h, w, 3) if d_vout is not None else None
    return out, vout


def run_model(fr, p, with_var=True):
    return dm.denoise(fr["rgb"], fr["var"] if with_var else None, fr["albedo"], fr["emission"], fr["normal"], fr["depth"], p)


def check(gpu, fr, p, with_var, what):
    out, vout = run_device(gpu, fr, p, with_var)
    want, vwant = run_model(fr, p, with_var)
    bad = int((~np.isclose(out, want, rtol=0, atol=0, equal_nan=True)).sum())
    assert bits_equal(out, want), "%s: out differs from the model on %d values" % (what, bad)
    if with_var:
        assert bits_equal(vout, vwant), "%s: var_out differs from the model" % (what,)
    return out, vout


_FUZZ = {}


def fuzz(w, h):
    if (w, h) not in _FUZZ:
        _FUZZ[(w, h)] = fuzz_frame(np.random.default_rng(1000 * w + h), h, w)
    return _FUZZ[(w, h)]


FULL = dict(option_sets()[0][1])


@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_fuzzed_frames_equal_the_model_for_every_pass_count(gpu, w, h):
    """passes 1..6: steps 1..32, beyond the frame at the small sizes; 300 x 200 is 13 x 19 tiles of the step-1 pass and one tile per
    sub-lattice from step 16 on"""
    fr = fuzz(w, h)
    assert w * h < 100 or (np.isnan(fr["rgb"]).any() and np.isinf(fr["depth"]).any())
    for passes, want, vwant in dm.denoise_each(fr["rgb"], fr["var"], fr["albedo"], fr["emission"], fr["normal"], fr["depth"], params_of(FULL, 6)):
        out, vout = run_device(gpu, fr, params_of(FULL, passes))
        assert bits_equal(out, want) and bits_equal(vout, vwant), "%dx%d, %d passes" % (w, h, passes)
    assert w * h < 100 or (np.isfinite(out).any() and not bits_equal(out, fr["rgb"]))
    if w * h < 10000:
        check(gpu, fr, params_of(FULL, 8), False, "%dx%d, 8 passes, no variance" % (w, h))


@pytest.mark.parametrize("name,fields,with_var", option_sets(), ids=[o[0] for o in option_sets()])
def test_every_term_and_flag_equals_the_model(gpu, name, fields, with_var):
    for (w, h), passes in (((17, 13), 3), ((67, 35), 2), ((3, 2), 2)):
        check(gpu, fuzz(w, h), params_of(fields, passes), with_var, "%s, %dx%d" % (name, w, h))


def test_zero_passes_copy_the_bytes(gpu):
    fr = fuzz(17, 13)
    out, vout = run_device(gpu, fr, params_of(FULL, 0), True)
    assert out.tobytes() == np.ascontiguousarray(fr["rgb"]).tobytes() and vout.tobytes() == np.ascontiguousarray(fr["var"]).tobytes()


def test_a_variance_output_is_optional(gpu):
    fr = fuzz(67, 35)
    out, vout = run_device(gpu, fr, params_of(FULL, 3), True, want_var_out=False)
    assert vout is None and bits_equal(out, run_model(fr, params_of(FULL, 3))[0])


def test_side_stream_repeatability_and_the_host_form(gpu):
    import torch
    fr, p = fuzz(67, 35), params_of(FULL, 4)
    first = run_device(gpu, fr, p)
    again = run_device(gpu, fr, p)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()          # the same bytes, NaNs included
    side = run_device(gpu, fr, p, stream=torch.cuda.Stream(device=0))                                    # read only after its sync
    assert side[0].tobytes() == first[0].tobytes() and side[1].tobytes() == first[1].tobytes()
    # the host form, through the Python wrapper and the tuple features() returns
    feats = (fr["albedo"], fr["emission"], fr["normal"], fr["depth"], np.ones(fr["depth"].shape), np.zeros(fr["depth"].shape, dtype=np.int64))
    kw = dict(passes=4, flags=p.flags, normal_power_log2=p.normal_power_log2, sigma_color=p.sigma_color, sigma_depth=p.sigma_depth,
              sigma_albedo=p.sigma_albedo, epsilon=p.epsilon, albedo_min=p.albedo_min)
    host, host_v = gpu.denoise(fr["rgb"], feats, variance=fr["var"], **kw)
    assert host.tobytes() == first[0].tobytes() and host_v.tobytes() == first[1].tobytes()
    only = gpu.denoise(fr["rgb"], to_records(gpu.FEATURE_DTYPE, fr), **kw)
    assert bits_equal(only, run_model(fr, p, with_var=False)[0])


# ---- rendered frames --------------------------------------------------------------------------------------------------------------
_RENDERED = {}


def rendered(gpu, name, w=None, h=None, spp=4, reference=0):
    """dict(rgb, var, albedo, emission, normal, depth[, ref]) of a golden scene: the Progressive spp-sample mean, its variance, the
    handle's features at spp rays per pixel and, when asked, the same handle's `reference`-spp mean.  Computed once per key."""
    objs, gw, gh, cfg = _golden(gpu, name)
    w, h = w or gw, h or gh
    key = (name, w, h, spp, reference)
    if key not in _RENDERED:
        cfg = dict(cfg, rays_per_pixel=spp)
        hnd = hip_scene(gpu, objs, **cfg).upload(0)
        prog = hnd.progressive(w, h)
        prog.add(spp)
        fr = dict(rgb=prog.mean(), var=prog.variance())
        fr["albedo"], fr["emission"], fr["normal"], fr["depth"], _, _ = hnd.features(w, h)
        fr["wrapped"] = prog.denoise()                                    # Progressive.denoise with the defaults, for the test below
        if reference:
            prog.add(reference - spp)
            fr["ref"] = prog.mean()
        hnd.close()
        _RENDERED[key] = fr
    return _RENDERED[key]


def default_params(gpu, **kw):
    d = gpu.denoise_params(**kw)
    return dm.Params(**{k: d[k].item() for k in ("passes", "flags", "normal_power_log2", "sigma_color", "sigma_depth", "sigma_albedo", "epsilon",
                                                  "albedo_min")})


@pytest.mark.parametrize("name", ["mixed_40x24", "spheres200_48x27"])
def test_rendered_frames_equal_the_model(gpu, name):
    """a Progressive 4-spp mean, its variance and the handle's features, at every size, for 1..6 passes at the two middle sizes and the
    default parameters everywhere; with and without the variance, with and without demodulation"""
    for w, h in SIZES:
        fr = rendered(gpu, name, w, h)
        p = default_params(gpu)
        check(gpu, fr, p, True, "%s %dx%d, defaults" % (name, w, h))
        assert bits_equal(fr["wrapped"], run_model(fr, p)[0]), "Progressive.denoise, %s %dx%d" % (name, w, h)
        check(gpu, fr, p.replace(flags=0), False, "%s %dx%d, no demodulation, no variance" % (name, w, h))
        if (w, h) in ((17, 13), (67, 35)):
            for passes in range(1, 7):
                check(gpu, fr, p.replace(passes=passes), True, "%s %dx%d, %d passes" % (name, w, h, passes))
                check(gpu, fr, p.replace(passes=passes, flags=0), True, "%s %dx%d, %d passes, no demodulation" % (name, w, h, passes))


def _rmse(a, b):
    d = (a - b)[np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)]
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("name", SCENES)
def test_the_denoised_frame_is_nearer_the_converged_one(gpu, name):
    """the one quality claim: the golden scenes at their golden sizes and seeds, the default parameters -- RMSE(denoised 4 spp, 256 spp)
    < RMSE(4 spp, 256 spp), the 256-spp frame being the same handle's.  A condition, not a threshold.  (All four golden scenes.)"""
    fr = rendered(gpu, name, spp=4, reference=256)
    out, _ = run_device(gpu, fr, default_params(gpu))
    noisy, den = _rmse(fr["rgb"], fr["ref"]), _rmse(out, fr["ref"])
    print("%s: RMSE against 256 spp: 4 spp %.6f, denoised %.6f (ratio %.3f)" % (name, noisy, den, den / noisy if noisy else float("nan")))
    assert np.isfinite(out).all()
    assert den < noisy


def test_the_denoise_example(gpu, tmp_path):
    """examples/denoise.cpp (Resident::denoise of rtx.hpp): 8 spp, features, denoise, quantize -- its frame is the model's on the same sums"""
    import subprocess
    exe = os.path.join(ROOT, "examples", "denoise")
    assert os.path.exists(exe), "examples/denoise is built by __graft_entry__.build()"
    w, h, spp = 40, 24, 8
    ppm, raw = tmp_path / "out.ppm", tmp_path / "out.f64"
    done = subprocess.run([exe, str(w), str(h), str(ppm), str(spp), str(raw)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    objs = np.zeros(5, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene (examples/adaptive.cpp's)
    for k, (kind, geom, base_c, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (7, 1.6, 0.3, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (5, -3, 2, 0.6), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-8, -8, -1.5, 30, -8, -1.5, 8, 20, -1.5), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base_c, em, rough
    hnd = hip_scene(gpu, objs, rays_per_pixel=spp).upload(0)
    prog = hnd.progressive(w, h)
    prog.add(spp)
    s, q, n = prog.sum.cpu().numpy(), prog.sum_sq.cpu().numpy(), float(spp)
    fr = dict(rgb=s / n, var=(q - s * s / n) / (n - 1.0) / n)
    fr["albedo"], fr["emission"], fr["normal"], fr["depth"], _, _ = hnd.features(w, h)
    hnd.close()
    want, _ = run_model(fr, default_params(gpu))
    got = np.fromfile(raw, dtype=np.float64).reshape(h, w, 3)
    assert bits_equal(got, want)
    from oracle import rtx_oracle
    rtx_oracle.build()
    head = b"P6\n%d %d\n255\n" % (w, h)
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and data[len(head):] == rtx_oracle.quantize_image(want).tobytes()
