"""Inputs of tests/test_denoise.py and tests/test_denoise_gpu.py: fuzzed frames with the values the header's rules name, the option
sets every test walks, and the conversion between guide arrays and RtxPixelFeatures records."""
import numpy as np

from denoise_model import DEMODULATE, NO_NORMAL, Params

INF = float("inf")


def fuzz_frame(rng, height, width, hostile=True):
    """dict(rgb, var, albedo, emission, normal [h][w][3], depth [h][w]): smooth patches with noise on top; with hostile=True also
    +inf depths, zero normals, zero and tiny albedo, zero variance, -0.0, and NaN and inf pixels"""
    shape = (height, width)
    patch = rng.integers(0, 3, shape)                                     # three "surfaces"
    base = np.array([[0.8, 0.3, 0.2], [0.2, 0.7, 0.9], [0.5, 0.5, 0.5]])
    albedo = base[patch] * rng.uniform(0.9, 1.0, shape + (1,))
    emission = np.where(rng.random(shape + (1,)) < 0.2, rng.uniform(0.0, 2.0, shape + (3,)), 0.0)
    nrm = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])[patch] + rng.normal(0, 0.05, shape + (3,))
    depth = np.array([2.0, 5.0, 9.0])[patch] * rng.uniform(0.95, 1.05, shape)
    var = rng.uniform(0.0, 0.05, shape + (3,))
    rgb = albedo * rng.uniform(0.2, 1.5, shape + (1,)) + emission + rng.normal(0, 0.1, shape + (3,))
    if hostile:
        n = height * width
        def some(frac):
            return rng.random(shape) < max(frac, 1.5 / n)
        depth[some(0.1)] = INF
        nrm[some(0.08)] = 0.0
        albedo[some(0.08)] = 0.0
        albedo[some(0.05), 1] = 5e-4                                      # below the default albedo_min on one channel
        var[some(0.1)] = 0.0
        rgb[some(0.05), 0] = -0.0
        emission[some(0.05)] = -0.0
        rgb[some(0.04), 2] = np.nan
        rgb[some(0.04), 1] = INF
        rgb[some(0.02)] = -INF
        var[some(0.03), 0] = np.nan
        var[some(0.03), 1] = INF
        nrm[some(0.02), 0] = np.nan
        depth[some(0.02)] = np.nan
        depth[some(0.02)] = 0.0
    return dict(rgb=rgb, var=var, albedo=albedo, emission=emission, normal=nrm, depth=depth)


def option_sets():
    """(name, Params fields, with variance?): every flag and term on and off, NO_NORMAL and the ends of the power's range"""
    full = dict(sigma_color=2.0, sigma_depth=0.3, sigma_albedo=0.5, epsilon=1e-6, albedo_min=1e-3, normal_power_log2=2, flags=DEMODULATE)
    out = [("all terms", dict(full), True),
           ("no variance", dict(full), False),
           ("no demodulation", dict(full, flags=0), True),
           ("no demodulation, no variance", dict(full, flags=0), False),
           ("no normal term", dict(full, normal_power_log2=NO_NORMAL), True),
           ("normal power 2^0", dict(full, normal_power_log2=0), True),
           ("normal power 2^8", dict(full, normal_power_log2=8), True),
           ("no depth term", dict(full, sigma_depth=INF), True),
           ("no albedo term", dict(full, sigma_albedo=INF), True),
           ("no colour term", dict(full, sigma_color=INF), True),
           ("no term at all", dict(full, sigma_color=INF, sigma_depth=INF, sigma_albedo=INF, normal_power_log2=NO_NORMAL), True),
           ("zero epsilon, zero albedo_min", dict(full, epsilon=0.0, albedo_min=0.0), True)]
    return out


def params_of(fields, passes):
    return Params(passes=passes, **fields)


def to_records(dtype, frame):
    """RtxPixelFeatures records [h][w] of a frame's guides (coverage 1, object 0: the filter reads neither)"""
    h, w = frame["depth"].shape
    f = np.zeros((h, w), dtype=dtype)
    f["albedo"], f["emission"], f["normal"], f["depth"] = frame["albedo"], frame["emission"], frame["normal"], frame["depth"]
    f["coverage"] = 1.0
    return f


def params_record(dtype, p):
    """the RtxDenoiseParams record of a model Params"""
    r = np.zeros((), dtype=dtype)
    for k in ("passes", "flags", "normal_power_log2", "sigma_color", "sigma_depth", "sigma_albedo", "epsilon", "albedo_min"):
        r[k] = getattr(p, k)
    return r


def bits_equal(a, b):
    """the same f64 patterns, every NaN counted as one pattern (the device and numpy may differ in a NaN's payload and sign)"""
    a, b = np.array(a, dtype=np.float64, copy=True), np.array(b, dtype=np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
