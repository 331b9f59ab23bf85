"""The guided upsampler's specification (include/rtx_hip.h, "Guided upsampling") without a GPU: the two numpy readings of
tests/upsample_model.py held to each other bit for bit on hostile cases that reach every branch of the text, properties that follow from
the text, the lattice identity the construction rests on, the struct layout, every argument the entry points refuse before they look for
a device, and the one quality condition on oracle frames."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import upsample_model as um
from upsample_cases import (BRANCHES, QUALITY, bilinear_params, bits_equal, branches_reached, cases, fuzz_case, option_sets, model_params,
                            params_record, quality_inputs, rmse, to_records)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
LOW_SIZES = [(1, 1), (2, 3), (4, 5), (7, 9)]                             # (hl, wl): 1 x 1, 3 x 2, 5 x 4 and 9 x 7
FACTORS = (1, 2, 3, 4, 8)


@pytest.mark.parametrize("name,fields,with_var", option_sets(), ids=[o[0] for o in option_sets()])
def test_the_two_readings_agree_bit_for_bit(name, fields, with_var):
    seen_nan = 0
    for lo, hi, p in cases(LOW_SIZES, FACTORS, name, fields, with_var):   # (cases() asserts that every branch is reached)
        a, av = um.upsample(lo, hi, p)
        b, bv = um.upsample_scalar(lo, hi, p)
        assert a.shape == hi["albedo"].shape and bits_equal(a, b), (name, lo["depth"].shape, p.factor)
        assert (av is None) == (bv is None) == (not with_var)
        if with_var:
            assert bits_equal(av, bv), (name, lo["depth"].shape, p.factor)
        seen_nan += int(np.isnan(av).sum()) if with_var else int(np.isinf(a).sum())
    # the hostile values were there: a NaN variance goes through; a colour that is not finite is never usable, so without D the frame
    # is finite whatever the low frame holds, and with D only an output pixel's own emission can make it infinite
    assert seen_nan > 0 or (not with_var and fields["flags"] == 0)
    assert with_var or fields["flags"] or seen_nan == 0


def test_every_branch_has_a_name_and_a_case_that_lacks_it_is_caught():
    """the branch check of upsample_cases.cases() can fail: a 1 x 1 low frame has no second tap, a clean case no tent fallback"""
    rng = np.random.default_rng(1)
    lo, hi = fuzz_case(rng, 1, 1, 1)
    assert branches_reached(lo, hi, um.Params(factor=1)) <= {"lattice"}
    lo, hi = fuzz_case(rng, 4, 5, 2, hostile=False)
    got = branches_reached(lo, hi, um.Params(factor=2))
    assert {"lattice", "last column", "last row", "h == 0", "guided"} <= got and not got & {"no usable tap", "dark at both"}
    with pytest.raises(AssertionError):
        cases([(1, 1)], (2,), "all terms", option_sets()[0][1], True)     # one low pixel: never two taps, never every branch
    assert len(set(BRANCHES)) == len(BRANCHES) == 12


def test_factor_one_without_demodulation_is_a_byte_copy():
    """every pixel is a lattice pixel: finite values (-0.0 among them) are moved, not computed"""
    rng = np.random.default_rng(3)
    lo, hi = fuzz_case(rng, 6, 5, 1, hostile=False)
    lo["rgb"][rng.random((6, 5)) < 0.2, 0] = -0.0
    p = um.Params(factor=1, flags=0)
    for fn in (um.upsample, um.upsample_scalar):
        out, vout = fn(lo, hi, p)
        assert out.tobytes() == lo["rgb"].tobytes() and vout.tobytes() == lo["var"].tobytes()
        out, vout = fn(dict(lo, var=None), hi, p)
        assert out.tobytes() == lo["rgb"].tobytes() and vout is None
    lo["rgb"][2, 3, 1] = np.nan                                           # ... and a value that is not finite is not usable: +0.0
    out, _ = um.upsample(lo, hi, p)
    assert out[2, 3, 1] == 0.0 and not np.signbit(out[2, 3, 1]) and out[2, 3, 0] == lo["rgb"][2, 3, 0]


def test_lattice_pixels_are_the_low_frame():
    rng = np.random.default_rng(4)
    for s in (2, 3, 8):
        lo, hi = fuzz_case(rng, 4, 5, s, hostile=False)
        out, vout = um.upsample(lo, hi, um.Params(factor=s, flags=0))
        assert out[::s, ::s].tobytes() == lo["rgb"].tobytes() and vout[::s, ::s].tobytes() == lo["var"].tobytes()


def test_an_infinite_sigma_deletes_its_term():
    """each term deleted another way than through its sigma: a guide that is one constant on both sizes gives the depth, the albedo and
    the normal weight exactly 1 (r = 0, da = 0, t = 1)"""
    rng = np.random.default_rng(5)
    base = dict(sigma_depth=0.3, sigma_albedo=0.5, normal_power_log2=2, flags=0, min_weight=1e-2)
    for (hl, wl), s in itertools.product([(4, 5), (7, 9)], (2, 3)):
        lo, hi = fuzz_case(rng, hl, wl, s, hostile=False)

        def const(key, value):
            fill = lambda g: dict(g, **{key: np.broadcast_to(np.asarray(value, dtype=np.float64), g[key].shape).copy()})
            return fill(lo), fill(hi)
        for off, (key, value) in ((dict(base, sigma_depth=INF), ("depth", 3.0)), (dict(base, sigma_albedo=INF), ("albedo", [0.5, 0.25, 0.75])),
                                  (dict(base, normal_power_log2=um.NO_NORMAL), ("normal", [1.0, 0.0, 0.0]))):
            a, av = um.upsample(lo, hi, um.Params(factor=s, **off))
            b, bv = um.upsample(*const(key, value), um.Params(factor=s, **base))
            assert bits_equal(a, b) and bits_equal(av, bv), (key, hl, wl, s)
            c, _ = um.upsample(lo, hi, um.Params(factor=s, **base))
            assert not bits_equal(a, c)                                   # ... and the term does something when it is there


def test_a_constant_low_frame_stays_constant():
    """Not D, every u_Q = U (per channel), clean guides (every weight well above the denormals, so no product underflows).  A lattice
    pixel moves U.  Any other pixel is fl(sc / sw) with sc the left fold of n <= 4 terms fl(w_i U) and sw the fold of the same w_i, all
    w_i > 0: each product carries a factor (1 + d), |d| <= eps = 2^-53; the first add (to +0.0) is exact and each of the up to 3 others
    adds a factor (1 + d), so sc = U sum w_i (1 + t_i) with |t_i| <= (1 + eps)^4 - 1 and sw = sum w_i (1 + f_i), |f_i| <= (1 + eps)^3 -
    1.  The w_i being positive, sc / sw lies within U (1 + eps)^4 / (1 - eps)^3 of U, and the division rounds once more: |u - U| <=
    ((1 + eps)^5 / (1 - eps)^3 - 1) |U| < 9 eps |U|.  The tent sum is the same expression in h."""
    eps = 2.0 ** -53
    rng = np.random.default_rng(6)
    U = np.array([0.7, 3.25e5, -1.3e-3])
    worst = 0.0
    for (hl, wl), s in itertools.product([(1, 1), (4, 5), (7, 9)], (2, 3, 8)):
        lo, hi = fuzz_case(rng, hl, wl, s, hostile=False)
        lo["rgb"] = np.broadcast_to(U, lo["rgb"].shape).copy()
        for fields in (dict(), dict(min_weight=0.5), dict(sigma_depth=INF, sigma_albedo=INF, normal_power_log2=um.NO_NORMAL)):
            out, _ = um.upsample(lo, hi, um.Params(factor=s, flags=0, **fields))
            rel = np.abs(out - U) / np.abs(U)
            worst = max(worst, float(rel.max()))
            assert (rel <= 9 * eps).all() and (out[::s, ::s] == U).all()
    print("a constant frame comes back within %.3g eps" % (worst / eps))


def test_missed_pixels_and_black_channels_come_out_as_the_render_gives_them():
    """under D: a channel with a_k <= albedo_min at p is exactly e_k (its bits, -0.0 included), its variance +0.0; a missed pixel (a = e
    = 0) is exactly +0.0 -- whatever the neighbours hold"""
    n_dark = n_miss = 0
    for name, fields, with_var in option_sets():
        if not fields["flags"] & um.DEMODULATE:
            continue
        for lo, hi, p in cases(LOW_SIZES[1:], (1, 2, 4), name, fields, with_var):
            out, vout = um.upsample(lo, hi, p)
            dark = hi["albedo"] <= p.albedo_min
            assert np.array_equal(out.view(np.uint64)[dark], hi["emission"].view(np.uint64)[dark])
            miss = np.isinf(hi["depth"]) & (hi["albedo"] == 0.0).all(axis=2) & (hi["emission"] == 0.0).all(axis=2) & ~np.signbit(hi["emission"]).any(axis=2)
            assert (out.view(np.uint64)[miss] == 0).all()
            if with_var:
                assert (vout.view(np.uint64)[dark] == 0).all()
            n_dark, n_miss = n_dark + int(dark.sum()), n_miss + int(miss.sum())
    assert n_dark > 100 and n_miss > 30


# ---- the lattice identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov", [math.pi / 2, math.pi, 0.05])
def test_a_low_pixel_has_the_ray_of_its_lattice_pixel(oracle, fov):
    """what the construction rests on (and why width % s != 0 is refused): the oracle's rtxo_get_ray_dir of pixel (X, Y) of the wl x hl
    frame equals that of pixel (s X, s Y) of the s wl x s hl frame as bits -- X / wl and s X / (s wl) are correctly rounded quotients of
    the same rational, and so are hl / wl and (s hl) / (s wl)"""
    L = oracle.lib()
    cam = ((0.1, -0.2, 0.3), (1.0, 0.25, -0.125), fov)
    sc = oracle.make_scene(np.zeros(0, dtype=oracle.OBJECT_DTYPE), cam)
    n = 0
    for (wl, hl), s in itertools.product([(5, 3), (12, 7), (33, 20), (100, 37)], (2, 3, 5, 7, 8)):
        w, h = wl * s, hl * s
        assert w & (w - 1) and wl & (wl - 1)                              # no power of two among the widths
        assert (hl / wl * fov).hex() == (h / w * fov).hex()
        for X, Y in itertools.product(sorted({0, 1, wl // 2, wl - 2, wl - 1}), sorted({0, 1, hl // 2, hl - 1})):
            a = L.rtxo_get_ray_dir(C.byref(sc), X / wl, Y / hl, hl / wl * fov).tuple()
            b = L.rtxo_get_ray_dir(C.byref(sc), (s * X) / w, (s * Y) / h, h / w * fov).tuple()
            assert [v.hex() for v in a] == [v.hex() for v in b], (wl, hl, s, X, Y)
            n += 1
    assert n > 300


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_struct_layout_matches_the_dtype(rtx, tmp_path):
    names = rtx.UPSAMPLE_PARAMS_DTYPE.names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rtx_hip.h"\nint main(void){ printf("%zu", sizeof(RtxUpsampleParams));\n' +
                   "".join('printf(" %%zu", offsetof(RtxUpsampleParams, %s));\n' % n for n in names) +
                   'printf(" %d %u", RTX_UPSAMPLE_MAX_FACTOR, RTX_UPSAMPLE_DEMODULATE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    dt = rtx.UPSAMPLE_PARAMS_DTYPE
    assert got[0] == dt.itemsize == C.sizeof(rtx.abi.RtxUpsampleParams) == 48
    assert got[1:1 + len(names)] == [dt.fields[n][1] for n in names] == [getattr(rtx.abi.RtxUpsampleParams, n).offset for n in names]
    assert got[-2:] == [rtx.RTX_UPSAMPLE_MAX_FACTOR, rtx.RTX_UPSAMPLE_DEMODULATE] == [8, 1]
    hdr = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"RTX_STATIC_ASSERT\(sizeof\(RtxUpsampleParams\) == 48", hdr)
    d = rtx.upsample_params()
    assert 1 <= int(d["factor"]) <= 8 and int(d["flags"]) == rtx.RTX_UPSAMPLE_DEMODULATE and int(d["normal_power_log2"]) <= 8 and int(d["reserved"]) == 0
    assert all(float(d[k]) > 0 and np.isfinite(float(d[k])) for k in ("sigma_depth", "sigma_albedo"))
    assert float(d["albedo_min"]) >= 0 and float(d["min_weight"]) >= 0
    with pytest.raises(TypeError):
        rtx.upsample_params(sigma=1.0)
    assert np.isinf(float(rtx.upsample_params(sigma_depth=None)["sigma_depth"]))
    assert int(rtx.upsample_params(normal_power_log2=None, demodulate=False)["flags"]) == 0
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")).read()
    assert re.search(r"pub struct RtxUpsampleParams", rs)
    for fn in ("rtx_upsample_default_params", "rtx_upsample_device", "rtx_upsample"):     # header, Python and Rust: the same argument count
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % fn, plain)
        assert m and fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        n_args = m.group(1).count(",") + 1
        assert len([s for s in rtx.abi.SYMBOLS if s[0] == fn][0][2]) == n_args, fn
        r = re.search(r"pub fn %s\s*\(([^;]*)\)" % fn, rs)
        assert r and r.group(1).count(":") == n_args, fn


KEYS = ("lo_rgb", "lo_var", "lo_feat", "feat", "out", "var_out")


def _call_device(lib, bufs, w, h, p, skip=(), **swap):
    """rtx_upsample_device on HOST arrays: only for calls the argument check refuses (it runs before any device is looked for)"""
    a = {k: bufs[k].ctypes.data for k in KEYS}
    for k in skip:
        a[k] = None
    a.update(swap)
    return lib.rtx_upsample_device(a["lo_rgb"], a["lo_var"], a["lo_feat"], a["feat"], w, h, p.ctypes.data if p is not None else None,
                                   a["out"], a["var_out"], 0, None)


def test_invalid_arguments_are_refused_without_a_device(rtx):
    lib = rtx.load_library()
    INVALID = rtx.abi.RTX_ERR_INVALID_ARGUMENT
    s, wl, hl = 2, 3, 4
    w, h = wl * s, hl * s
    good = rtx.upsample_params(factor=s)
    bufs = dict(lo_rgb=np.zeros((hl, wl, 3)), lo_var=np.zeros((hl, wl, 3)), lo_feat=np.zeros((hl, wl), dtype=rtx.FEATURE_DTYPE),
                feat=np.zeros((h, w), dtype=rtx.FEATURE_DTYPE), out=np.zeros((h, w, 3)), var_out=np.zeros((h, w, 3)))

    def host(p, **swap):
        a = dict({k: bufs[k].ctypes.data for k in KEYS}, **swap)
        return lib.rtx_upsample(a["lo_rgb"], a["lo_var"], a["lo_feat"], a["feat"], w, h, p.ctypes.data, a["out"], a["var_out"])
    # the baseline is acceptable: the host form takes the same arguments past the check (and then finds a device, or reports none)
    assert host(good) == (rtx.abi.RTX_OK if rtx.device_count() > 0 else rtx.abi.RTX_ERR_NO_DEVICE)
    for k in ("lo_rgb", "lo_feat", "feat", "out"):                        # null pointers
        assert _call_device(lib, bufs, w, h, good, skip=(k,)) == INVALID, k
        assert host(good, **{k: None}) == INVALID, k
    assert _call_device(lib, bufs, w, h, None) == INVALID
    assert _call_device(lib, bufs, w, h, good, skip=("lo_var",)) == INVALID                    # a variance output without an input
    assert host(good, lo_var=None) == INVALID
    for a, b in itertools.combinations(KEYS, 2):                          # overlaps: every pair among the inputs and the outputs
        assert _call_device(lib, bufs, w, h, good, **{a: bufs[b].ctypes.data}) == INVALID, (a, b)
        assert b"overlap" in lib.rtx_last_error(), (a, b)
    assert _call_device(lib, bufs, w, h, good, out=bufs["feat"].ctypes.data + 96 * (w * h - 1)) == INVALID         # by one record
    assert _call_device(lib, bufs, w, h, good, out=bufs["lo_rgb"].ctypes.data + 24 * (wl * hl - 1)) == INVALID     # by one low pixel
    for ww, hh in ((0, 8), (6, 0), (0, 0), (65536, 65536), (0xFFFFFFF0, 2), (2, 0xFFFFFFF0), (0xFFFE, 0x10002)):   # sizes
        assert _call_device(lib, bufs, ww, hh, good) == INVALID, (ww, hh)
    for ww, hh in ((7, 8), (6, 9), (5, 7)):                               # not multiples of the factor
        assert _call_device(lib, bufs, ww, hh, good) == INVALID, (ww, hh)
        assert b"multiple" in lib.rtx_last_error()
    bad = [dict(factor=0), dict(factor=9), dict(factor=0xFFFFFFFF), dict(flags=2), dict(flags=3), dict(normal_power_log2=9),
           dict(normal_power_log2=0xFFFFFFFE), dict(reserved=1)]
    for k in ("sigma_depth", "sigma_albedo"):
        bad += [{k: 0.0}, {k: -1.0}, {k: np.nan}, {k: -INF}]
    for k in ("albedo_min", "min_weight"):
        bad += [{k: -1e-300}, {k: np.nan}, {k: INF}]
    for fields in bad:
        p = rtx.upsample_params(**dict(dict(factor=s), **fields))
        assert _call_device(lib, bufs, w, h, p) == INVALID, fields
        assert host(p) == INVALID, fields
    # ... and what is allowed gets past the check: it finds a device, or reports that there is none
    past = (rtx.abi.RTX_OK, rtx.abi.RTX_ERR_NO_DEVICE)
    for fields in (dict(sigma_depth=INF, sigma_albedo=INF), dict(normal_power_log2=0), dict(normal_power_log2=8), dict(normal_power_log2=None),
                   dict(albedo_min=0.0, min_weight=0.0), dict(min_weight=2.0), dict(demodulate=False), dict(factor=1)):
        p = rtx.upsample_params(**dict(dict(factor=s), **fields))
        ww, hh = (wl, hl) if fields.get("factor") == 1 else (w, h)
        assert lib.rtx_upsample(bufs["lo_rgb"].ctypes.data, None, bufs["lo_feat"].ctypes.data, bufs["feat"].ctypes.data, ww, hh, p.ctypes.data,
                                bufs["out"].ctypes.data, None) in past, fields


def test_records_carry_the_guides(rtx):
    """to_records / params_record, which the GPU tests feed the library with, say what the model reads"""
    lo, hi = fuzz_case(np.random.default_rng(1), 3, 4, 2)
    f = to_records(rtx.FEATURE_DTYPE, hi)
    assert f.shape == (6, 8) and bits_equal(f["albedo"], hi["albedo"]) and bits_equal(f["depth"], hi["depth"])
    r = params_record(rtx.UPSAMPLE_PARAMS_DTYPE, um.Params(factor=4, flags=0, normal_power_log2=um.NO_NORMAL, sigma_depth=INF, min_weight=0.25))
    assert int(r["factor"]) == 4 and int(r["normal_power_log2"]) == rtx.RTX_DENOISE_NO_NORMAL and np.isinf(float(r["sigma_depth"]))
    assert float(r["min_weight"]) == 0.25 and int(r["flags"]) == 0


# ---- quality ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,s", QUALITY)
def test_the_guided_frame_is_nearer_the_converged_one_than_the_bilinear_one(oracle, rtx, name, s):
    """the one quality condition, with the model on oracle frames and the library's default parameters: RMSE(guided, 256 spp) <
    RMSE(bilinear, 256 spp), bilinear being the same model with both sigmas +inf, no normal term and no demodulation.  A condition, not
    a tuned number.  Also here: the low guides are the output guides on the lattice, bit for bit (the lattice identity on whole picks)."""
    lo, hi, ref = quality_inputs(oracle, rtx, name, s)
    for k in ("albedo", "emission", "normal", "depth"):
        assert bits_equal(lo[k], hi[k][::s, ::s]), k
    guided, _ = um.upsample(lo, hi, model_params(rtx, s))
    bilinear, _ = um.upsample(lo, hi, bilinear_params(s))
    nearest = np.repeat(np.repeat(lo["rgb"], s, axis=0), s, axis=1)
    g, b, n = rmse(guided, ref), rmse(bilinear, ref), rmse(nearest, ref)
    print("%s, s = %d: RMSE against 256 spp: nearest %.4f, bilinear %.4f, guided %.4f (ratio %.3f)" % (name, s, n, b, g, g / b))
    assert g < b
