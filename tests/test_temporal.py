"""Temporal accumulation without a GPU: the model's two readings (tests/temporal_model.py) against each other on every fuzzed case, the
tables, the C ABI's refusals and layout, the reprojection's accuracy on the pixels' own rays, the running mean it becomes with
alpha_min = 0, and the one quality condition on oracle frames."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import temporal_model as tm
from helpers import DEFAULT_CAM
from temporal_cases import PARAMS, bits_equal, fuzz_case, table_edge_case, tiny_fov_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PAIRS = [(math.pi / 2, 1920, 1080), (math.pi / 2, 8, 8), (math.pi, 8, 8), (math.pi, 1920, 1080), (1.0, 40, 24)]     # (fov, width, height)
CASES = [(17, 13, math.pi / 2, True), (67, 35, math.pi / 2, True), (67, 35, math.pi / 2, False), (40, 24, math.pi, True),
         (17, 13, 0.05, False), (3, 2, math.pi / 2, True), (1, 1, math.pi / 2, True), (300, 1, 1.0, True)]


def _both(case, first=False):
    hist = None if first else case["hist"]
    a = tm.accumulate(case["cur"], hist, case["params"])
    b = tm.accumulate_scalar(case["cur"], hist, case["params"])
    for name, x, y in zip(("rgb", "var", "len", "motion"), a, b):
        assert (x is None) == (y is None), name
        if x is not None:
            assert bits_equal(x, y), name
    return a


@pytest.mark.parametrize("w,h,fov,with_var", CASES)
def test_the_two_readings_agree_bit_for_bit(w, h, fov, with_var):
    case = fuzz_case(w * 31 + h, w, h, fov, with_var, planted=(w >= 12 and h >= 10))      # (checked when made: temporal_cases.check_case)
    out = _both(case)
    assert (out[1] is None) == (not with_var)
    first = _both(case, first=True)
    assert first[0].tobytes() == case["cur"]["rgb"].tobytes() and (first[2] == 1).all() and np.isnan(first[3]).all()


def test_the_two_readings_agree_on_table_edges_and_equal_entries():
    case, n = table_edge_case()
    assert n >= 40
    _both(case)
    _both(tiny_fov_case())


# ---- the tables -------------------------------------------------------------------------------------------------------------------
def test_tables_are_math_sin_of_the_written_expression(rtx):
    for fov, w, h in PAIRS + [(1e-3, 33, 7), (2e-323, 16, 8), (3.0, 5, 9)]:
        got = rtx.temporal_tables(fov, w, h)
        assert got.shape == (w + h + 2,)
        assert np.array_equal(got.view(np.uint64), tm.tables(fov, w, h).view(np.uint64)), (fov, w, h)
    t = rtx.temporal_tables(math.pi, 64, 64)
    assert (np.diff(t[:65]) >= 0).all() and t[0] == -1.0 and t[64] == 1.0                      # monotone up to pi
    lib = rtx.load_library()
    buf = np.zeros(32)
    for fov in (0.0, -1.0, math.nextafter(math.pi, 4.0), 4.0, float("nan"), float("inf")):
        assert lib.rtx_temporal_tables(fov, 4, 4, buf.ctypes.data) == rtx.abi.RTX_ERR_INVALID_ARGUMENT, fov
        with pytest.raises(rtx.RtxError):
            rtx.temporal_tables(fov, 4, 4)
    assert lib.rtx_temporal_tables(1.0, 4, 4, None) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert lib.rtx_temporal_tables(1.0, 0, 4, buf.ctypes.data) == rtx.abi.RTX_ERR_INVALID_ARGUMENT
    assert lib.rtx_temporal_tables(1.0, 65536, 65536, buf.ctypes.data) == rtx.abi.RTX_ERR_INVALID_ARGUMENT


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_struct_layout_matches_the_dtype(rtx, tmp_path):
    names = rtx.TEMPORAL_PARAMS_DTYPE.names
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rtx_hip.h"\nint main(void){ printf("%zu", sizeof(RtxTemporalParams));\n' +
                   "".join('printf(" %%zu", offsetof(RtxTemporalParams, %s));\n' % n for n in names) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    dt = rtx.TEMPORAL_PARAMS_DTYPE
    assert got[0] == dt.itemsize == C.sizeof(rtx.abi.RtxTemporalParams) == 48
    assert got[1:] == [dt.fields[n][1] for n in names] == [getattr(rtx.abi.RtxTemporalParams, n).offset for n in names]
    hdr = open(os.path.join(ROOT, "include", "rtx_hip.h")).read()
    assert re.search(r"RTX_STATIC_ASSERT\(sizeof\(RtxTemporalParams\) == 48", hdr)
    d = rtx.temporal_params()
    assert 0 <= float(d["alpha_min"]) <= 1 and float(d["max_history"]) >= 1 and int(d["flags"]) == 0 and int(d["reserved"]) == 0
    with pytest.raises(TypeError):
        rtx.temporal_params(alpha=1.0)
    fns = ("rtx_temporal_default_params", "rtx_temporal_tables", "rtx_temporal_accumulate_device", "rtx_temporal_accumulate")
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rs = open(os.path.join(ROOT, "rust", "src", "raytracing", "hip.rs")).read()
    for fn in fns:                                           # declared in the header, bound in Python and in Rust with the same argument count
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % fn, plain)
        assert m and fn in [s[0] for s in rtx.abi.SYMBOLS], fn
        n_args = m.group(1).count(",") + 1
        assert len([s for s in rtx.abi.SYMBOLS if s[0] == fn][0][2]) == n_args, fn
        r = re.search(r"pub fn %s\s*\(([^;]*)\)" % fn, rs)
        assert r and r.group(1).count(":") == n_args, fn


KEYS = ("rgb", "var", "hits", "hist_rgb", "hist_var", "hist_len", "hist_hits", "tables", "out_rgb", "out_var", "out_len", "motion")


def _call_device(rtx, bufs, w, h, p, cam, skip=(), **swap):
    """rtx_temporal_accumulate_device on HOST arrays: only for calls the argument check refuses (it runs before any device is looked for)"""
    a = {k: bufs[k].ctypes.data for k in KEYS}
    a["cam"] = C.addressof(cam) if cam is not None else None
    for k in skip:
        a[k] = None
    a.update(swap)
    return rtx.load_library().rtx_temporal_accumulate_device(
        a["rgb"], a["var"], a["hits"], a["hist_rgb"], a["hist_var"], a["hist_len"], a["hist_hits"], a["cam"], a["tables"], w, h,
        p.ctypes.data if p is not None else None, a["out_rgb"], a["out_var"], a["out_len"], a["motion"], 0, None)


def test_invalid_arguments_are_refused_without_a_device(rtx):
    lib = rtx.load_library()
    INVALID = rtx.abi.RTX_ERR_INVALID_ARGUMENT
    w, h = 6, 5
    good = rtx.temporal_params()
    cam = rtx.Camera(*DEFAULT_CAM).to_c()
    f3 = lambda: np.zeros((h, w, 3))
    hits = lambda: np.zeros((h, w), dtype=rtx.HIT_DTYPE)
    bufs = dict(rgb=f3(), var=f3(), hits=hits(), hist_rgb=f3(), hist_var=f3(), hist_len=np.ones((h, w)), hist_hits=hits(),
                tables=rtx.temporal_tables(cam.fov, w, h), out_rgb=f3(), out_var=f3(), out_len=np.zeros((h, w)), motion=np.zeros((h, w, 2)))
    host = lambda p, c=cam: lib.rtx_temporal_accumulate(
        bufs["rgb"].ctypes.data, bufs["var"].ctypes.data, bufs["hits"].ctypes.data, bufs["hist_rgb"].ctypes.data, bufs["hist_var"].ctypes.data,
        bufs["hist_len"].ctypes.data, bufs["hist_hits"].ctypes.data, C.addressof(c), w, h, p.ctypes.data, bufs["out_rgb"].ctypes.data,
        bufs["out_var"].ctypes.data, bufs["out_len"].ctypes.data, bufs["motion"].ctypes.data)
    # the baseline is acceptable: the host form takes the same arguments past the check (and then finds a device, or reports none)
    assert host(good) == (rtx.abi.RTX_OK if rtx.device_count() > 0 else rtx.abi.RTX_ERR_NO_DEVICE)
    # null pointers where something is required; a history that is only partly given; variances that do not go together
    for k in ("rgb", "hits", "out_rgb", "out_len"):
        assert _call_device(rtx, bufs, w, h, good, cam, skip=(k,)) == INVALID, k
    assert _call_device(rtx, bufs, w, h, None, cam) == INVALID
    for k in ("hist_rgb", "hist_len", "hist_hits", "tables"):
        assert _call_device(rtx, bufs, w, h, good, cam, skip=(k,)) == INVALID, k
    assert _call_device(rtx, bufs, w, h, good, None) == INVALID
    assert _call_device(rtx, bufs, w, h, good, cam, skip=("hist_rgb", "hist_len", "hist_hits")) == INVALID         # hist_var alone
    assert _call_device(rtx, bufs, w, h, good, cam, skip=("hist_var",)) == INVALID                                # d_var without d_hist_var
    assert _call_device(rtx, bufs, w, h, good, cam, skip=("var", "out_var")) == INVALID                           # ... and the reverse
    assert _call_device(rtx, bufs, w, h, good, cam, skip=("var", "hist_var")) == INVALID                          # d_out_var without d_var
    assert _call_device(rtx, bufs, w, h, good, None, skip=("var", "hist_rgb", "hist_var", "hist_len", "hist_hits", "tables")) == INVALID
    # overlaps: every pair among the inputs and the outputs
    for a, b in itertools.combinations(KEYS, 2):
        assert _call_device(rtx, bufs, w, h, good, cam, **{a: bufs[b].ctypes.data}) == INVALID, (a, b)
        assert b"overlap" in lib.rtx_last_error(), (a, b)
    assert _call_device(rtx, bufs, w, h, good, cam, out_rgb=bufs["rgb"].ctypes.data + 24 * (w * h - 1)) == INVALID      # by one pixel
    # sizes
    for ww, hh in ((0, 5), (6, 0), (0, 0), (65536, 65536), (0xFFFFFFF0, 1), (1, 0xFFFFFFF0), (0xFFFF, 0x10001)):
        assert _call_device(rtx, bufs, ww, hh, good, cam) == INVALID, (ww, hh)
    # parameters
    nan, inf = float("nan"), float("inf")
    bad = [dict(flags=1), dict(reserved=1), dict(alpha_min=-1e-300), dict(alpha_min=1.0000001), dict(alpha_min=nan), dict(max_history=0.5),
           dict(max_history=inf), dict(max_history=nan), dict(plane_tolerance=-1e-9), dict(plane_tolerance=inf), dict(plane_tolerance=nan),
           dict(normal_min=-0.1), dict(normal_min=1.1), dict(normal_min=nan), dict(min_weight=-0.1), dict(min_weight=1.0), dict(min_weight=nan)]
    for fields in bad:
        p = rtx.temporal_params(**fields)
        assert _call_device(rtx, bufs, w, h, p, cam) == INVALID, fields
        assert host(p) == INVALID, fields
    for fields in (dict(alpha_min=0.0), dict(alpha_min=1.0), dict(max_history=1.0), dict(plane_tolerance=0.0), dict(normal_min=0.0),
                   dict(normal_min=1.0), dict(min_weight=0.0)):
        assert host(rtx.temporal_params(**fields)) != INVALID, fields
    # the previous camera's fov
    for fov in (0.0, -1.0, math.nextafter(math.pi, 4.0), nan, inf):
        c2 = rtx.Camera(*DEFAULT_CAM).to_c()
        c2.fov = fov
        assert _call_device(rtx, bufs, w, h, good, c2) == INVALID, fov
        assert host(good, c2) == INVALID, fov


# ---- the reprojection ---------------------------------------------------------------------------------------------------------------
def _own_ray_frame(fov, w, h, dist=3.7):
    """every pixel's own ray through the identity camera at the origin: the frame, and the history of the same frame"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    ax, ay = fov * (xs / w - 0.5), (h / w * fov) * (ys / h - 0.5)
    d = np.stack([np.sin(ax), np.sin(ay), np.cos(ax) * np.cos(ay)], axis=-1)
    pos = dist * d
    nrm = -d
    cur = dict(rgb=np.ones((h, w, 3)), var=None, position=pos, normal=nrm, object=np.zeros((h, w), dtype=np.int64))
    hist = dict(rgb=np.ones((h, w, 3)), var=None, len=np.ones((h, w)), position=pos, normal=nrm, object=cur["object"], cam_pos=np.zeros(3),
                to_cam=np.eye(3).reshape(9), tables=tm.tables(fov, w, h))
    return cur, hist, xs, ys


@pytest.mark.parametrize("fov,w,h", PAIRS)
def test_the_pixels_own_rays_come_back_to_their_own_coordinates(fov, w, h):
    cur, hist, xs, ys = _own_ray_frame(fov, w, h)
    *_, motion = tm.accumulate(cur, hist, PARAMS)
    front = cur["position"][..., 2] > 0                      # (at fov = pi column 0 looks along the image plane: cos(-pi/2) is 6e-17, in front)
    assert front.all()
    err = np.maximum(np.abs(motion[..., 0] - xs), np.abs(motion[..., 1] - ys))
    print("fov %.4f %dx%d: own rays come back to %.3g px" % (fov, w, h, np.nanmax(err)))
    assert not np.isnan(motion).any() and err.max() < 1e-9


def test_the_interpolation_error_between_the_pixels_own_rays():
    """what the header documents: linear interpolation in sine space against the exact angle map, half way between the pixels' rays"""
    for fov, w, bound in ((math.pi / 2, 1920, 2e-4), (math.pi / 2, 8, 0.03), (math.pi, 8, 0.3)):
        T = tm.tables(fov, w, 1)[:w + 1]
        f = np.arange(w) + 0.5
        got = tm._unmap(T, w, np.sin(fov * (f / w - 0.5)))
        worst = np.abs(got - f).max()
        print("fov %.4f, %d wide: half-way points are off by up to %.3g px" % (fov, w, worst))
        assert worst < bound


def _golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    import json
    return z["objects"], int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def _oracle_pick(oracle, rtx, objs_raw, cam, w, h, **cfg):
    """the pick buffer from the oracle's closest_object on every pixel's zero-offset ray (rtxo_get_ray_dir)"""
    objs = np.frombuffer(objs_raw.tobytes(), dtype=rtx.OBJECT_DTYPE)
    sc = oracle.make_scene(np.frombuffer(objs_raw.tobytes(), dtype=oracle.OBJECT_DTYPE), cam, **cfg)
    L = oracle.lib()
    vfov = h / w * cam[2]
    pos, nrm, obj = np.full((h, w, 3), np.nan), np.full((h, w, 3), np.nan), np.full((h, w), -1, dtype=np.int64)
    o = np.array(cam[0], dtype=np.float64)
    for y in range(h):
        for x in range(w):
            rd = np.array(L.rtxo_get_ray_dir(C.byref(sc), x / w, y / h, vfov).tuple())
            i, dist = oracle.closest_object(sc, cam[0], tuple(rd))
            if i < 0:
                continue
            P = o + rd * dist
            g = objs[i]["geom"]
            if objs[i]["kind"] == rtx.RTX_SPHERE:
                n = (P - g[:3]) / np.linalg.norm(P - g[:3])
            elif objs[i]["kind"] == rtx.RTX_PLANE:
                n = g[3:6] / np.linalg.norm(g[3:6])
            else:
                n = np.array(oracle.triangle_normal(g[0:3], g[3:6], g[6:9]))
            pos[y, x], nrm[y, x], obj[y, x] = P, n, i
    return dict(position=pos, normal=nrm, object=obj)


def _cam_hist(rtx, cam, w, h):
    c = rtx.Camera(*cam).to_c()
    return dict(cam_pos=np.array(c.position[:]), to_cam=np.array(c.to_cam_space[:]), tables=rtx.temporal_tables(c.fov, w, h))


def test_the_same_camera_maps_a_golden_pick_onto_itself(oracle, rtx):
    objs, w, h, cfg = _golden("mixed_40x24")
    pick = _oracle_pick(oracle, rtx, objs, DEFAULT_CAM, w, h, **cfg)
    assert (pick["object"] >= 0).sum() > w * h // 4
    cur = dict(pick, rgb=np.ones((h, w, 3)), var=None)
    hist = dict(pick, rgb=np.ones((h, w, 3)), var=None, len=np.ones((h, w)), **_cam_hist(rtx, DEFAULT_CAM, w, h))
    *_, ln, motion = tm.accumulate(cur, hist, PARAMS)
    ys, xs = np.mgrid[0:h, 0:w]
    hit = pick["object"] >= 0
    err = np.maximum(np.abs(motion[..., 0] - xs), np.abs(motion[..., 1] - ys))[hit]
    print("the same camera: |motion - (x, y)| up to %.3g px" % err.max())
    assert err.max() < 1e-9 and np.isnan(motion[~hit]).all() and (ln[hit] == 2).all()


def _frames(oracle, objs_raw, cams, w, h, spp, cfg, seed0):
    objs = np.frombuffer(objs_raw.tobytes(), dtype=oracle.OBJECT_DTYPE)
    out = []
    for k, cam in enumerate(cams):
        sc = oracle.make_scene(objs, cam, **dict(cfg, rays_per_pixel=spp, seed=seed0 + k))
        out.append(oracle.render(sc, w, h))
    return out


def test_with_alpha_min_zero_a_static_sequence_is_the_plain_mean(oracle, rtx):
    """K = 4 oracle frames of one camera with distinct seeds through the model with alpha_min = 0: the result is the plain mean of the
    four frames up to rounding (another fold, and neighbour taps of weight ~1e-13).  Measured here: at most 5.55e-17 on a frame whose
    largest value is 1.0; asserted: ten times that, which is below 1e-9 x the frame's largest value (the project's libm-sized figure)."""
    objs, w, h, cfg = _golden("c1_three_spheres_32x32")
    frames = _frames(oracle, objs, [DEFAULT_CAM] * 4, w, h, 4, cfg, 100)
    pick = _oracle_pick(oracle, rtx, objs, DEFAULT_CAM, w, h, **cfg)
    p = PARAMS.replace(alpha_min=0.0, max_history=1e6, min_weight=0.01)
    cam = _cam_hist(rtx, DEFAULT_CAM, w, h)
    hist = None
    for f in frames:
        out, _, ln, _ = tm.accumulate(dict(pick, rgb=f, var=None), hist, p)
        hist = dict(pick, rgb=out, var=None, len=ln, **cam)
    hit = pick["object"] >= 0
    assert (ln[hit] == 4).all() and (ln[~hit] == 1).all()
    mean = (((frames[0] + frames[1]) + frames[2]) + frames[3]) / 4.0
    worst, top = float(np.abs(out - mean)[hit].max()), float(np.abs(mean).max())
    print("static sequence against the plain mean: %.3g (largest value %.3g)" % (worst, top))
    assert worst <= 10 * 5.55e-17 and 10 * 5.55e-17 <= 1e-9 * top
    assert out[~hit].tobytes() == frames[3][~hit].tobytes()


def _rmse(a, b):
    d = a - b
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("name", ["c1_three_spheres_32x32", "mixed_40x24"])
def test_the_accumulated_frame_is_nearer_the_converged_one(oracle, rtx, name):
    """the one quality condition, with the model on oracle frames and the library's default parameters: 6 frames at 4 spp, the camera
    turned a third of a degree per frame, distinct seeds -- RMSE(accumulated last frame, 256 spp of the last camera) < RMSE(the last
    4-spp frame, the same).  A condition, not a tuned number."""
    objs, w, h, cfg = _golden(name)
    cams = [((0.0, 0.0, 0.0), (math.cos(0.006 * k), math.sin(0.006 * k), 0.0), DEFAULT_CAM[2]) for k in range(6)]
    frames = _frames(oracle, objs, cams, w, h, 4, cfg, 7)
    ref = _frames(oracle, objs, cams[-1:], w, h, 256, cfg, 999)[0]
    d = rtx.temporal_params()
    p = tm.Params(**{k: d[k].item() for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")})
    hist = None
    for cam, f in zip(cams, frames):
        pick = _oracle_pick(oracle, rtx, objs, cam, w, h, **cfg)
        out, _, ln, _ = tm.accumulate(dict(pick, rgb=f, var=None), hist, p)
        hist = dict(pick, rgb=out, var=None, len=ln, **_cam_hist(rtx, cam, w, h))
    noisy, acc = _rmse(frames[-1], ref), _rmse(out, ref)
    print("%s: RMSE against 256 spp: last 4-spp frame %.6f, accumulated %.6f (ratio %.3f); mean history length %.2f" %
          (name, noisy, acc, acc / noisy, ln.mean()))
    assert acc < noisy
