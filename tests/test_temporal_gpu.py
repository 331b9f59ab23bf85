"""rtx_temporal_accumulate_device / rtx_temporal_accumulate on the GPU against tests/temporal_model.py: out_rgb, out_var, out_len and
motion must equal the model's array reading as uint64 patterns (one pattern for every NaN) -- on the fuzzed cases with every way of
losing history and every hostile value, at sizes of one pixel, below a workgroup, of several workgroups with a ragged last one, and on
one thin frame wide enough for the tables to be searched in global memory; with and without a variance and d_motion, and as a first
frame.  Then end to end through SceneHandle.temporal on golden scenes: every frame equals the model fed with the device's own frames,
picks and tables, and pixels uncovered by a moved or hidden object start again."""
import json
import math
import os
import sys

import numpy as np
import pytest

import denoise_model as dm
import temporal_model as tm
from helpers import DEFAULT_CAM, hip_scene
from temporal_cases import bits_equal, fuzz_case, hit_records, params_record, table_edge_case, tiny_fov_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
THIN = 4095                                                   # (4095 + 1) + (1 + 1) doubles > 32768 B of LDS: the global-memory tables
SIZES = [(1, 1), (3, 2), (17, 13), (67, 35), (THIN, 1)]       # (width, height)
NAMES = ("rgb", "var", "len", "motion")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


_CASES = {}


def case_of(w, h, fov=math.pi / 2):
    key = (w, h, fov)
    if key not in _CASES:
        _CASES[key] = fuzz_case(1000 + w, w, h, fov, with_var=True, planted=(w >= 12 and h >= 10))
    return _CASES[key]


def camera_of(gpu, hist):
    cam = gpu.abi.RtxCamera()
    cam.fov = float(hist["fov"])
    cam.position[:] = [float(x) for x in hist["cam_pos"]]
    cam.to_cam_space[:] = [float(x) for x in hist["to_cam"]]
    return cam


def run_device(gpu, case, with_var=True, with_motion=True, first=False, stream=None):
    """rtx_temporal_accumulate_device on device copies of a case; every output holds NaN bytes beforehand -> (rgb, var, len, motion)"""
    import torch
    dev = torch.device("cuda", 0)
    lib = gpu.load_library()
    cur, hist, w, h = case["cur"], case["hist"], case["w"], case["h"]
    rec = params_record(gpu.TEMPORAL_PARAMS_DTYPE, case["params"])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    f64 = lambda a: up(np.asarray(a, dtype=np.float64))
    nan_bytes = lambda n: torch.full((int(n),), 255, dtype=torch.uint8, device=dev)
    d_rgb, d_hits = f64(cur["rgb"]), up(hit_records(gpu.HIT_DTYPE, cur))
    d_var = f64(cur["var"]) if with_var else None
    d_h = [None] * 5
    cam = None
    if not first:
        d_h = [f64(hist["rgb"]), f64(hist["var"]) if with_var else None, f64(hist["len"]), up(hit_records(gpu.HIT_DTYPE, hist)), f64(hist["tables"])]
        cam = camera_of(gpu, hist)
    d_out, d_len = nan_bytes(24 * w * h), nan_bytes(8 * w * h)
    d_vout = nan_bytes(24 * w * h) if with_var else None
    d_mot = nan_bytes(16 * w * h) if with_motion else None
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    gpu.abi.check(lib.rtx_temporal_accumulate_device(
        ptr(d_rgb), ptr(d_var), ptr(d_hits), ptr(d_h[0]), ptr(d_h[1]), ptr(d_h[2]), ptr(d_h[3]),
        gpu.abi.C.addressof(cam) if cam is not None else None, ptr(d_h[4]), w, h, rec.ctypes.data, ptr(d_out), ptr(d_vout), ptr(d_len), ptr(d_mot),
        0, stream.cuda_stream if stream is not None else None), lib)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    back = lambda t, shape: t.cpu().numpy().view(np.float64).reshape(shape) if t is not None else None
    return back(d_out, (h, w, 3)), back(d_vout, (h, w, 3)), back(d_len, (h, w)), back(d_mot, (h, w, 2))


def run_model(case, with_var=True, first=False):
    cur = dict(case["cur"], var=case["cur"]["var"] if with_var else None)
    hist = None if first else dict(case["hist"], var=case["hist"]["var"] if with_var else None)
    return tm.accumulate(cur, hist, case["params"])


def check(gpu, case, what, with_var=True, with_motion=True, first=False):
    got = run_device(gpu, case, with_var, with_motion, first)
    want = run_model(case, with_var, first)
    for name, g, m in zip(NAMES, got, want):
        if (name == "var" and not with_var) or (name == "motion" and not with_motion):
            assert g is None
            continue
        bad = int((~np.isclose(g, m, rtol=0, atol=0, equal_nan=True)).sum())
        assert bits_equal(g, m), "%s: %s differs from the model on %d values" % (what, name, bad)
    return got


@pytest.mark.parametrize("w,h", SIZES)
def test_fuzzed_cases_equal_the_model(gpu, w, h):
    case = case_of(w, h)
    what = "%dx%d" % (w, h)
    got = check(gpu, case, what)
    if case["planted"]:
        assert (got[2] > 1).sum() * 4 >= w * h                # (history was taken: the case is not vacuous on the device either)
    check(gpu, case, what + ", no variance, no motion", with_var=False, with_motion=False)
    check(gpu, case, what + ", variance, no motion", with_motion=False)
    first = check(gpu, case, what + ", first frame", first=True)
    assert first[0].tobytes() == np.ascontiguousarray(case["cur"]["rgb"]).tobytes()            # byte copies: payloads and signs kept
    assert first[1].tobytes() == np.ascontiguousarray(case["cur"]["var"]).tobytes()
    assert (first[2] == 1).all() and np.isnan(first[3]).all()
    check(gpu, case, what + ", first frame, no variance", with_var=False, first=True)


def test_the_table_paths_agree(gpu):
    """the widest single row whose tables are staged in LDS, and the first that searches them in global memory: each equals the model"""
    for w in (THIN - 2, THIN):
        case = case_of(w, 1)
        got = check(gpu, case, "%dx1" % w)
        assert np.isfinite(got[3]).all(axis=-1).sum() * 2 >= w


@pytest.mark.parametrize("fov", [math.pi, 0.05])
def test_other_fields_of_view(gpu, fov):
    check(gpu, case_of(67, 35, fov), "67x35 at fov %g" % fov)
    check(gpu, case_of(17, 13, fov), "17x13 at fov %g" % fov, with_var=False)


def test_table_edges_and_equal_entries(gpu):
    """sx exactly on a table entry and one ulp to either side; a fov so small that neighbouring entries are equal (den == 0)"""
    case, n = table_edge_case()
    check(gpu, case, "table edges (%d aims)" % n)
    check(gpu, tiny_fov_case(), "equal table entries")


def test_side_stream_repeatability_and_the_host_form(gpu):
    import torch
    case = case_of(67, 35)
    first = run_device(gpu, case)
    again = run_device(gpu, case)
    side = run_device(gpu, case, stream=torch.cuda.Stream(device=0))                          # read only after its sync
    for a, b, c in zip(first, again, side):
        assert a.tobytes() == b.tobytes() == c.tobytes()                                      # the same bytes, NaNs included
    cur, hist, p = case["cur"], case["hist"], case["params"]
    kw = {k: getattr(p, k) for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")}
    history = dict(rgb=hist["rgb"], var=hist["var"], len=hist["len"], hits=hit_records(gpu.HIT_DTYPE, hist))
    host = gpu.temporal_accumulate(cur["rgb"], hit_records(gpu.HIT_DTYPE, cur), history=history, prev_camera=camera_of(gpu, hist),
                                   variance=cur["var"], want_motion=True, **kw)
    for name, a in zip(NAMES, first):
        assert host[name].tobytes() == a.tobytes(), name
    start = gpu.temporal_accumulate(cur["rgb"], hit_records(gpu.HIT_DTYPE, cur), **kw)
    assert start["var"] is None and start["motion"] is None and (start["len"] == 1).all()
    assert start["rgb"].tobytes() == np.ascontiguousarray(cur["rgb"]).tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _golden(gpu, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    objs = np.frombuffer(z["objects"].tobytes(), dtype=gpu.OBJECT_DTYPE).copy()
    return objs, int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def _state(gpu, T, w, h):
    """what the last frame left: the next frame's history, as the model reads it"""
    hits = T.frame_hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(h, w)
    cam = T._hist[4]
    return dict(rgb=T.mean(), var=T.variance(), len=T.length(), position=hits["position"].copy(), normal=hits["normal"].copy(),
                object=hits["object"].copy(), cam_pos=np.array(cam.position[:]), to_cam=np.array(cam.to_cam_space[:]),
                tables=gpu.temporal_tables(cam.fov, w, h), frame_rgb=T.frame_mean.cpu().numpy(),
                frame_var=T.frame_variance.cpu().numpy() if T.frame_variance is not None else None)


def _model_params(gpu):
    d = gpu.temporal_params()
    return tm.Params(**{k: d[k].item() for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")})


def _nudged(gpu, k):
    a = 0.004 * k                                            # a quarter of a degree per frame, and a small step sideways
    return gpu.Camera((0.0, 0.02 * k, 0.0), (math.cos(a), math.sin(a), 0.0), DEFAULT_CAM[2])


@pytest.mark.parametrize("name", ["mixed_40x24", "c1_three_spheres_32x32"])
def test_a_sequence_on_a_golden_scene_equals_the_model(gpu, name):
    objs, w, h, cfg = _golden(gpu, name)
    hnd = hip_scene(gpu, objs, **cfg).upload(0)
    T = hnd.temporal(w, h)
    p = _model_params(gpu)
    prev = None
    seq = [_nudged(gpu, 0), _nudged(gpu, 1), _nudged(gpu, 2), None, None]          # then two frames with the camera held
    for k, cam in enumerate(seq):
        if k == 3:                                           # move the sphere most pixels see, by its own size
            seen = np.bincount(prev["object"][prev["object"] >= 0].ravel(), minlength=len(objs))
            spheres = [int(i) for i in np.argsort(-seen) if objs[i]["kind"] == gpu.RTX_SPHERE and seen[i] > 0]
            assert len(spheres) >= 2, "the scene shows fewer than two spheres"
            moved = objs[spheres[0]:spheres[0] + 1].copy()
            moved["geom"][0, 1] += 0.8 * moved["geom"][0, 3]
            hnd.update_objects([spheres[0]], moved)
        if k == 4:
            hnd.hide([spheres[1]])
        out = T.frame(4, cam)
        now = _state(gpu, T, w, h)
        cur = dict(rgb=now["frame_rgb"], var=now["frame_var"], position=now["position"], normal=now["normal"], object=now["object"])
        want = tm.accumulate(cur, prev, p)
        got = (out, now["var"], now["len"], T.motion())
        for nm, g, m in zip(NAMES, got, want):
            assert bits_equal(g, m), "%s frame %d: %s differs from the model" % (name, k, nm)
        if k in (1, 2):
            assert (now["len"] > 1).sum() * 2 >= (now["object"] >= 0).sum(), "a nudged camera lost most of the history"
        if k >= 3:                                           # the camera is held: a pixel that shows another object starts again
            changed = now["object"] != prev["object"]
            assert changed.sum() >= 4, "the update changed nothing on screen"
            assert (now["len"][changed] == 1).all()
            assert now["rgb"][changed].tobytes() == now["frame_rgb"][changed].tobytes()
            assert now["var"][changed].tobytes() == now["frame_var"][changed].tobytes()
            still = ~changed & (now["object"] >= 0) & ((now["object"] != spheres[0]) | (k == 4))    # (the moved sphere's own pixels
            assert (now["len"][still] > 1).mean() > 0.9                                              # fail the plane test once)
        prev = now
    # Temporal.denoise: the accumulated mean and variance with the handle's features through the denoiser
    d = gpu.denoise_params()
    dp = dm.Params(**{k: d[k].item() for k in ("passes", "flags", "normal_power_log2", "sigma_color", "sigma_depth", "sigma_albedo", "epsilon",
                                               "albedo_min")})
    albedo, emission, normal, depth, _, _ = hnd.features(w, h)
    want, _ = dm.denoise(prev["rgb"], prev["var"], albedo, emission, normal, depth, dp)
    assert bits_equal(T.denoise(), want)
    T.reset()
    assert T.frame_index == 0 and (T.frame(1) is not None) and T.variance() is None and (T.length() == 1).all()
    hnd.close()


def test_the_temporal_orbit_example(gpu, tmp_path):
    """examples/temporal_orbit.cpp (Resident::temporal_accumulate of rtx.hpp): 4 frames at 4 spp on an orbit, accumulated, denoised,
    quantised -- its accumulated frame and history length are the temporal model's chained over the same frames and picks, its
    denoised frame the denoise model's on that, its PPM the quantisation of that"""
    import subprocess
    exe = os.path.join(ROOT, "examples", "temporal_orbit")
    assert os.path.exists(exe), "examples/temporal_orbit is built by __graft_entry__.build()"
    w, h, frames, spp = 40, 24, 4, 4
    ppm, raw = tmp_path / "out.ppm", tmp_path / "out.f64"
    done = subprocess.run([exe, str(w), str(h), str(ppm), str(frames), str(spp), str(raw)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    objs = np.zeros(5, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene (examples/denoise.cpp's)
    for k, (kind, geom, base_c, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (7, 1.6, 0.3, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (5, -3, 2, 0.6), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-8, -8, -1.5, 30, -8, -1.5, 8, 20, -1.5), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base_c, em, rough
    hnd = hip_scene(gpu, objs, rays_per_pixel=spp).upload(0)
    T = hnd.temporal(w, h)
    p = _model_params(gpu)
    prev = None
    for k in range(frames):
        a = 0.006 * k
        pos = (6.0 - 6.0 * math.cos(a), -6.0 * math.sin(a), 0.0)
        T.frame(spp, gpu.Camera(pos, (6.0 - pos[0], 0.0 - pos[1], 0.0 - pos[2]), DEFAULT_CAM[2]))
        now = _state(gpu, T, w, h)
        cur = dict(rgb=now["frame_rgb"], var=now["frame_var"], position=now["position"], normal=now["normal"], object=now["object"])
        out, var, ln, _ = tm.accumulate(cur, prev, p)
        prev = dict(now, rgb=out, var=var, len=ln)          # the model's own chain
    albedo, emission, normal, depth, _, _ = hnd.features(w, h)
    hnd.close()
    d = gpu.denoise_params()
    dp = dm.Params(**{k: d[k].item() for k in ("passes", "flags", "normal_power_log2", "sigma_color", "sigma_depth", "sigma_albedo", "epsilon",
                                               "albedo_min")})
    want, _ = dm.denoise(prev["rgb"], prev["var"], albedo, emission, normal, depth, dp)
    got = np.fromfile(raw, dtype=np.float64)
    n = w * h
    assert got.size == 7 * n
    assert bits_equal(got[:3 * n].reshape(h, w, 3), prev["rgb"]) and bits_equal(got[3 * n:4 * n].reshape(h, w), prev["len"])
    assert (prev["len"] > 1).sum() * 2 >= (prev["object"] >= 0).sum()
    assert bits_equal(got[4 * n:].reshape(h, w, 3), want)
    from oracle import rtx_oracle
    rtx_oracle.build()
    head = b"P6\n%d %d\n255\n" % (w, h)
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and data[len(head):] == rtx_oracle.quantize_image(want).tobytes()


def test_the_product_library_keeps_its_instance_count(gpu):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    names = kernel_instances.kernel_names(gpu.abi.LIB_PATH)
    assert len(names) <= 25 and "epilogue_kernel" in names, names      # the accumulation is a form of epilogue_kernel, not a new kernel
