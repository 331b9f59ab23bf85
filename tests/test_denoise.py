"""The denoiser's specification (include/rtx_hip.h, "Denoising") without a GPU: the two numpy readings of tests/denoise_model.py held to
each other bit for bit and to properties that follow from the header's text, the struct layout, and every argument the entry points
refuse before they look for a device."""
import ctypes as C
import itertools
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import denoise_model as dm
from denoise_cases import bits_equal, fuzz_frame, option_sets, params_of, params_record, to_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SIZES = [(1, 1), (2, 3), (5, 4), (7, 9)]                                 # (height, width), up to 9 x 7


def _run(fn, fr, p, with_var=True):
    return fn(fr["rgb"], fr["var"] if with_var else None, fr["albedo"], fr["emission"], fr["normal"], fr["depth"], p)


@pytest.mark.parametrize("name,fields,with_var", option_sets(), ids=[o[0] for o in option_sets()])
def test_the_two_readings_agree_bit_for_bit(name, fields, with_var):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    seen_nan = 0
    for (h, w), passes in itertools.product(SIZES, (1, 2, 4)):
        fr = fuzz_frame(rng, h, w)
        p = params_of(fields, passes)
        a, av = _run(dm.denoise, fr, p, with_var)
        b, bv = _run(dm.denoise_scalar, fr, p, with_var)
        assert bits_equal(a, b), (name, h, w, passes)
        assert (av is None) == (bv is None) == (not with_var)
        if with_var:
            assert bits_equal(av, bv), (name, h, w, passes)
        seen_nan += int(np.isnan(a).sum())
    assert seen_nan > 0                                                   # the hostile values were there


def _b3_blur(img):
    """an independent B3 blur with border renormalisation: explicit per-pixel loops, weights and values summed tap by tap"""
    h, w, _ = img.shape
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    out = np.zeros_like(img)
    for y in range(h):
        for x in range(w):
            acc, tot = np.zeros(3), 0.0
            for j in range(5):
                for i in range(5):
                    yy, xx = y + j - 2, x + i - 2
                    if 0 <= yy < h and 0 <= xx < w:
                        acc = acc + (k[i] * k[j]) * img[yy, xx]
                        tot = tot + k[i] * k[j]
            out[y, x] = acc / tot
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (3, 2), (7, 9)])
def test_without_terms_one_pass_is_a_b3_blur_with_border_renormalisation(h, w):
    fr = fuzz_frame(np.random.default_rng(h * 31 + w), h, w, hostile=False)
    p = dm.Params(passes=1, flags=0, normal_power_log2=dm.NO_NORMAL, sigma_color=INF, sigma_depth=INF, sigma_albedo=INF)
    out, vout = _run(dm.denoise, fr, p, with_var=False)
    assert vout is None and bits_equal(out, _b3_blur(fr["rgb"]))
    assert not np.array_equal(out, fr["rgb"]) or (h, w) == (1, 1)


def test_zero_passes_is_a_byte_copy():
    fr = fuzz_frame(np.random.default_rng(3), 6, 5)
    for fn in (dm.denoise, dm.denoise_scalar):
        out, vout = _run(fn, fr, dm.Params(passes=0))
        assert out.tobytes() == fr["rgb"].tobytes() and vout.tobytes() == fr["var"].tobytes()
        out, vout = _run(fn, fr, dm.Params(passes=0), with_var=False)
        assert out.tobytes() == fr["rgb"].tobytes() and vout is None


def test_an_infinite_sigma_deletes_its_term():
    """each term deleted another way than through its sigma: a constant guide gives the depth, albedo and normal weights exactly 1; an
    epsilon so large that d2 / (...) vanishes against 1 gives the colour weight exactly 1"""
    rng = np.random.default_rng(5)
    base = dict(sigma_color=2.0, sigma_depth=0.3, sigma_albedo=0.5, epsilon=1e-6, normal_power_log2=2, flags=0)
    for (h, w), passes in itertools.product([(4, 5), (7, 9)], (1, 3)):
        fr = fuzz_frame(rng, h, w, hostile=False)
        const = lambda key, value: dict(fr, **{key: np.broadcast_to(np.asarray(value, dtype=np.float64), fr[key].shape).copy()})
        cases = [(dict(base, sigma_depth=INF), fr, dict(base), const("depth", 3.0)),
                 (dict(base, sigma_albedo=INF), fr, dict(base), const("albedo", [0.5, 0.25, 0.75])),
                 (dict(base, normal_power_log2=dm.NO_NORMAL), fr, dict(base), const("normal", [1.0, 0.0, 0.0])),
                 (dict(base, sigma_color=INF), fr, dict(base, epsilon=1e300), fr)]
        for off_fields, off_frame, on_fields, on_frame in cases:
            a, av = _run(dm.denoise, off_frame, params_of(off_fields, passes))
            b, bv = _run(dm.denoise, on_frame, params_of(on_fields, passes))
            assert bits_equal(a, b) and bits_equal(av, bv), (off_fields, h, w, passes)
            c, _ = _run(dm.denoise, fr, params_of(base, passes))
            assert not bits_equal(a, c)                                   # ... and the term does something when it is there


def test_taps_of_zero_weight_leave_the_frame_unchanged():
    """normals that are all zero make every neighbour's weight zero: u' = (h u) / h with h = 9/64 -- the frame itself, bit for bit, on
    values whose product with 9 is exact; (h u) / h on any value"""
    rng = np.random.default_rng(9)
    for h, w in [(1, 1), (5, 4), (7, 9)]:
        fr = fuzz_frame(rng, h, w, hostile=False)
        fr["normal"] = np.zeros_like(fr["normal"])
        fr["rgb"] = rng.integers(-4096, 4096, (h, w, 3)) / 64.0
        fr["var"] = rng.integers(0, 4096, (h, w, 3)) / 1024.0
        p = dm.Params(passes=3, flags=0, normal_power_log2=1, sigma_color=2.0, sigma_depth=0.3, sigma_albedo=0.5)
        out, vout = _run(dm.denoise, fr, p)
        assert bits_equal(out, fr["rgb"]) and bits_equal(vout, fr["var"])
        fr["rgb"] = rng.normal(0, 1, (h, w, 3))
        out, _ = _run(dm.denoise, fr, p.replace(passes=1))
        assert bits_equal(out, (0.140625 * fr["rgb"]) / 0.140625)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_header_struct_layout_matches_the_dtype(rtx, tmp_path):
    names = rtx.DENOISE_PARAMS_DTYPE.names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rtx_hip.h"\nint main(void){ printf("%zu", sizeof(RtxDenoiseParams));\n' +
                   "".join('printf(" %%zu", offsetof(RtxDenoiseParams, %s));\n' % n for n in names) +
                   'printf(" %d %u %u", RTX_DENOISE_MAX_PASSES, RTX_DENOISE_DEMODULATE, RTX_DENOISE_NO_NORMAL); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    dt = rtx.DENOISE_PARAMS_DTYPE
    assert got[0] == dt.itemsize == C.sizeof(rtx.abi.RtxDenoiseParams) == 56
    assert got[1:1 + len(names)] == [dt.fields[n][1] for n in names] == [getattr(rtx.abi.RtxDenoiseParams, n).offset for n in names]
    assert got[-3:] == [rtx.RTX_DENOISE_MAX_PASSES, rtx.RTX_DENOISE_DEMODULATE, rtx.RTX_DENOISE_NO_NORMAL]
    hdr = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"RTX_STATIC_ASSERT\(sizeof\(RtxDenoiseParams\) == 56", hdr)
    d = rtx.denoise_params()
    assert int(d["passes"]) == 5 and int(d["flags"]) == rtx.RTX_DENOISE_DEMODULATE and int(d["normal_power_log2"]) <= 8 and int(d["reserved"]) == 0
    assert all(float(d[k]) > 0 and np.isfinite(float(d[k])) for k in ("sigma_color", "sigma_depth", "sigma_albedo"))
    with pytest.raises(TypeError):
        rtx.denoise_params(sigma=1.0)


def _call_device(lib, bufs, w, h, p, skip=(), **swap):
    """rtx_denoise_device on HOST arrays: only for calls the argument check refuses (it runs before any device is looked for)"""
    a = dict(rgb=bufs["rgb"].ctypes.data, var=bufs["var"].ctypes.data, feat=bufs["feat"].ctypes.data, out=bufs["out"].ctypes.data,
             var_out=bufs["var_out"].ctypes.data, work=bufs["work"].ctypes.data)
    for k in skip:
        a[k] = None
    a.update(swap)
    return lib.rtx_denoise_device(a["rgb"], a["var"], a["feat"], w, h, p.ctypes.data if p is not None else None, a["out"], a["var_out"],
                                  a["work"], 0, None)


def test_invalid_arguments_are_refused_without_a_device(rtx):
    lib = rtx.load_library()
    INVALID = rtx.abi.RTX_ERR_INVALID_ARGUMENT
    w, h = 6, 5
    good = rtx.denoise_params(passes=3)
    wb = rtx.denoise_work_bytes(w, h, good)
    assert wb == 2 * 128 * w * h
    bufs = dict(rgb=np.zeros((h, w, 3)), var=np.zeros((h, w, 3)), feat=np.zeros((h, w), dtype=rtx.FEATURE_DTYPE), out=np.zeros((h, w, 3)),
                var_out=np.zeros((h, w, 3)), work=np.zeros(wb // 8 + 2))
    assert bufs["work"].ctypes.data % 16 == 0
    # the baseline is acceptable: the host form takes the same arguments past the check (and then finds a device, or reports none)
    st = lib.rtx_denoise(bufs["rgb"].ctypes.data, bufs["var"].ctypes.data, bufs["feat"].ctypes.data, w, h, good.ctypes.data,
                         bufs["out"].ctypes.data, bufs["var_out"].ctypes.data)
    assert st == (rtx.abi.RTX_OK if rtx.device_count() > 0 else rtx.abi.RTX_ERR_NO_DEVICE)
    # null pointers
    for k in ("rgb", "feat", "out", "work"):
        assert _call_device(lib, bufs, w, h, good, skip=(k,)) == INVALID, k
    assert _call_device(lib, bufs, w, h, None) == INVALID
    assert _call_device(lib, bufs, w, h, good, skip=("var",)) == INVALID                       # a variance output without an input
    assert _call_device(lib, bufs, w, h, good, work=bufs["work"].ctypes.data + 8) == INVALID   # misaligned
    assert b"aligned" in lib.rtx_last_error()
    # overlaps: every pair among the inputs, the outputs and the work buffer
    keys = ("rgb", "var", "feat", "out", "var_out", "work")
    for a, b in itertools.combinations(keys, 2):
        assert _call_device(lib, bufs, w, h, good, **{a: bufs[b].ctypes.data}) == INVALID, (a, b)
        assert b"overlap" in lib.rtx_last_error(), (a, b)
    assert _call_device(lib, bufs, w, h, good, out=bufs["rgb"].ctypes.data + 24 * (w * h - 1)) == INVALID       # by one pixel
    # sizes
    for ww, hh in ((0, 5), (6, 0), (0, 0), (65536, 65536), (0xFFFFFFF0, 1), (1, 0xFFFFFFF0), (0xFFFF, 0x10001)):
        assert _call_device(lib, bufs, ww, hh, good) == INVALID, (ww, hh)
        assert rtx.denoise_work_bytes(ww, hh, good) == 0
    # parameters
    bad = [dict(passes=9), dict(flags=2), dict(flags=3), dict(normal_power_log2=9), dict(normal_power_log2=0xFFFFFFFE), dict(reserved=1)]
    for k in ("sigma_color", "sigma_depth", "sigma_albedo"):
        bad += [{k: 0.0}, {k: -1.0}, {k: np.nan}, {k: -INF}]
    for k in ("epsilon", "albedo_min"):
        bad += [{k: -1e-300}, {k: np.nan}, {k: INF}]
    for fields in bad:
        p = rtx.denoise_params(**dict(dict(passes=3), **fields))
        assert _call_device(lib, bufs, w, h, p) == INVALID, fields
        assert rtx.denoise_work_bytes(w, h, p) == 0, fields
        assert lib.rtx_denoise(bufs["rgb"].ctypes.data, None, bufs["feat"].ctypes.data, w, h, p.ctypes.data, bufs["out"].ctypes.data, None) == INVALID
    # ... and what is allowed: infinite sigmas, the ends of the ranges
    for fields in (dict(sigma_color=INF, sigma_depth=INF, sigma_albedo=INF), dict(normal_power_log2=0), dict(normal_power_log2=8),
                   dict(normal_power_log2=None), dict(epsilon=0.0, albedo_min=0.0), dict(passes=8), dict(demodulate=False)):
        assert rtx.denoise_work_bytes(w, h, rtx.denoise_params(**fields)) > 0, fields
    # the host form's own pointer checks
    assert lib.rtx_denoise(None, None, bufs["feat"].ctypes.data, w, h, good.ctypes.data, bufs["out"].ctypes.data, None) == INVALID
    assert lib.rtx_denoise(bufs["rgb"].ctypes.data, None, bufs["feat"].ctypes.data, w, h, good.ctypes.data, bufs["out"].ctypes.data,
                           bufs["var_out"].ctypes.data) == INVALID
    assert lib.rtx_denoise(bufs["rgb"].ctypes.data, None, bufs["feat"].ctypes.data, w, h, good.ctypes.data, bufs["rgb"].ctypes.data, None) == INVALID


def test_work_bytes_are_monotone_in_the_passes(rtx):
    for w, h in ((1, 1), (17, 13), (1920, 1080)):
        sizes = [rtx.denoise_work_bytes(w, h, rtx.denoise_params(passes=k)) for k in range(rtx.RTX_DENOISE_MAX_PASSES + 1)]
        assert sizes[0] == 0 and sizes[1] == 128 * w * h and sizes[2] == 256 * w * h
        assert all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert all(s % 128 == 0 for s in sizes)


def test_records_carry_the_guides(rtx):
    """to_records / params_record, which the GPU tests feed the library with, say what the model reads"""
    fr = fuzz_frame(np.random.default_rng(1), 3, 4)
    f = to_records(rtx.FEATURE_DTYPE, fr)
    assert f.shape == (3, 4) and bits_equal(f["albedo"], fr["albedo"]) and bits_equal(f["depth"], fr["depth"])
    r = params_record(rtx.DENOISE_PARAMS_DTYPE, dm.Params(passes=4, flags=0, normal_power_log2=dm.NO_NORMAL, sigma_depth=INF))
    assert int(r["passes"]) == 4 and int(r["normal_power_log2"]) == rtx.RTX_DENOISE_NO_NORMAL and np.isinf(float(r["sigma_depth"]))
