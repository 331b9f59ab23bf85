"""rtx_rewind_hits_device / rtx_rewind_hits on the GPU against tests/rewind_model.py: the output records must equal the model's array
reading as uint64 patterns (one pattern for every NaN) -- on the fuzzed cases with every way of being unmoved and of being lost and
every hostile value, at 1, 6, 221 and 2345 hits (below a workgroup, several workgroups with a ragged last one), with lists of 0, 1, 2
and 37 moved objects and one list on each side of the LDS budget.  Then end to end through SceneHandle.temporal(w, h, objects=...) on
golden scenes: every frame equals the temporal model fed with the rewind model's output on the device's own pick, and a moved
sphere's pixels keep the history that the same sequence without rewinding loses."""
import json
import math
import os
import sys

import numpy as np
import pytest

import denoise_model as dm
import rewind_model as rm
import temporal_model as tm
from helpers import DEFAULT_CAM, hip_scene
from rewind_cases import (PLANT_M, PLANT_N, bits_equal, four_tap_pixels, fuzz_case, hit_records, hits_of, motion_records, motions_of,
                          same_hits)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LDS_ENTRIES = 4096                                            # 32768 B of LDS / 8 B: the longest list that is staged
SIZES = [1, 6, 221, 2345]
LISTS = [0, 1, 2, 37]
NAMES = ("rgb", "var", "len", "motion")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


_CASES = {}


def case_of(n, m):
    if (n, m) not in _CASES:
        _CASES[(n, m)] = fuzz_case(5000 + 7 * n + m, n, m)
    return _CASES[(n, m)]


def run_device(gpu, case, stream=None):
    """rtx_rewind_hits_device on device copies of a case; the output holds NaN bytes beforehand -> a hits dict"""
    import torch
    dev = torch.device("cuda", 0)
    lib = gpu.load_library()
    n, m = case["n"], case["m"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_hits = up(hit_records(gpu.HIT_DTYPE, case["hits"]))
    d_obj = up(case["objects"]) if m else None
    d_mot = up(motion_records(gpu.OBJECT_MOTION_DTYPE, case["motions"])) if m else None
    d_out = torch.full((64 * n,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None
    gpu.abi.check(lib.rtx_rewind_hits_device(ptr(d_hits), n, ptr(d_obj), ptr(d_mot), m, 0, ptr(d_out), 0,
                                             stream.cuda_stream if stream is not None else None), lib)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    return d_out.cpu().numpy().view(gpu.HIT_DTYPE)


def check(gpu, case, what):
    got = run_device(gpu, case)
    want = rm.rewind(case["hits"], case["objects"], case["motions"])
    g = hits_of(got)
    for k in ("object", "distance", "position", "normal"):
        ok = np.array_equal(g[k], want[k]) if k == "object" else bits_equal(g[k], want[k])
        if not ok:                                           # say where: the hits, and the planted ones among them by name
            same = (g[k] == want[k]) | ((g[k] != g[k]) & (want[k] != want[k]))
            bad = np.flatnonzero(~same.reshape(len(same), -1).all(axis=-1))
            names = [nm for nm, p in case["plants"].items() if p in set(bad.tolist())]
            p = int(bad[0]) if len(bad) else -1
            detail = "" if p < 0 else "; hit %d: device %r, model %r, input object %d position %r" % (
                p, g[k][p].tolist(), want[k][p].tolist(), int(case["hits"]["object"][p]), case["hits"]["position"][p].tolist())
            assert ok, "%s: %s differs from the model on hits %s (planted: %s)%s" % (what, k, bad[:12].tolist(), names, detail)
    return got


@pytest.mark.parametrize("m", LISTS)
@pytest.mark.parametrize("n", SIZES)
def test_fuzzed_cases_equal_the_model(gpu, n, m):
    case = case_of(n, m)
    got = check(gpu, case, "%d hits, %d moved" % (n, m))
    if m == 0:                                               # a copy: payloads and signs kept
        assert got.tobytes() == hit_records(gpu.HIT_DTYPE, case["hits"]).tobytes()
    if n >= PLANT_N and m >= PLANT_M:
        assert case["planted"]
        moved = (got["object"] >= 0) & (got["position"] != case["hits"]["position"]).any(axis=-1)
        assert moved.sum() * 4 >= n                          # (hits were rewound: the case is not vacuous on the device either)


@pytest.mark.parametrize("m", [LDS_ENTRIES - 1, LDS_ENTRIES, LDS_ENTRIES + 1])
def test_the_list_on_both_sides_of_the_lds_budget(gpu, m):
    """the longest lists that are staged in LDS and the first that is searched in global memory (most entries match no hit): each equals
    the model, planted branches included"""
    case = case_of(2345, m)
    assert case["planted"]
    check(gpu, case, "2345 hits, %d moved" % m)


def test_side_stream_repeatability_and_the_host_form(gpu):
    import torch
    case = case_of(2345, 37)
    first = run_device(gpu, case)
    again = run_device(gpu, case)
    side = run_device(gpu, case, stream=torch.cuda.Stream(device=0))                          # read only after its sync
    assert first.tobytes() == again.tobytes() == side.tobytes()                               # the same bytes, NaNs included
    motions = motion_records(gpu.OBJECT_MOTION_DTYPE, case["motions"])
    legal = np.isin(motions["kind"], (0, 1, 2, gpu.RTX_MOTION_LOST))
    assert not legal.all()
    with pytest.raises(gpu.RtxError):                        # the planted unknown kind: the host form refuses what the device form loses
        gpu.rewind_hits(hit_records(gpu.HIT_DTYPE, case["hits"]), case["objects"], motions)
    motions["kind"][~legal] = gpu.RTX_MOTION_LOST             # (LOST in the model and on the device alike)
    host = gpu.rewind_hits(hit_records(gpu.HIT_DTYPE, case["hits"]), case["objects"], motions)
    assert host.tobytes() == first.tobytes()
    small = case_of(6, 2)
    unaligned = np.zeros(64 * 6 + 8, dtype=np.uint8)[8:].view(gpu.HIT_DTYPE)
    unaligned[:] = hit_records(gpu.HIT_DTYPE, small["hits"])
    host = gpu.rewind_hits(unaligned, small["objects"], motion_records(gpu.OBJECT_MOTION_DTYPE, small["motions"]))
    assert same_hits(hits_of(host), rm.rewind(small["hits"], small["objects"], small["motions"]))
    none = gpu.rewind_hits(hit_records(gpu.HIT_DTYPE, small["hits"]), [], np.zeros(0, dtype=gpu.OBJECT_MOTION_DTYPE))
    assert none.tobytes() == hit_records(gpu.HIT_DTYPE, small["hits"]).tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _golden(gpu, name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    objs = np.frombuffer(z["objects"].tobytes(), dtype=gpu.OBJECT_DTYPE).copy()
    return objs, int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def _state(gpu, T, w, h):
    """what the last frame left: the next frame's history, as the model reads it (the UNREWOUND pick), and the rewound pick"""
    hits = T.frame_hits.cpu().numpy().view(gpu.HIT_DTYPE).reshape(h, w)
    cam = T._hist[4]
    back = None if T.frame_rewound is None else T.frame_rewound.cpu().numpy().view(gpu.HIT_DTYPE).reshape(h, w)
    return dict(rgb=T.mean(), var=T.variance(), len=T.length(), position=hits["position"].copy(), normal=hits["normal"].copy(),
                object=hits["object"].copy(), cam_pos=np.array(cam.position[:]), to_cam=np.array(cam.to_cam_space[:]),
                tables=gpu.temporal_tables(cam.fov, w, h), frame_rgb=T.frame_mean.cpu().numpy(),
                frame_var=T.frame_variance.cpu().numpy() if T.frame_variance is not None else None, hits=hits, rewound=back, motion=T.motion())


def _model_params(gpu):
    d = gpu.temporal_params()
    return tm.Params(**{k: d[k].item() for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight")})


def _nudged(gpu, k):
    a = 0.004 * k                                            # tests/test_temporal_gpu.py's cameras
    return gpu.Camera((0.0, 0.02 * k, 0.0), (math.cos(a), math.sin(a), 0.0), DEFAULT_CAM[2])


def _model_frame(gpu, now, prev, p, objects=None, motions=None):
    """the models chained on the device's own pick and frame: -> (the four outputs, the rewound pick or None)"""
    cur = dict(rgb=now["frame_rgb"], var=now["frame_var"], position=now["position"], normal=now["normal"], object=now["object"])
    back = None
    if objects is not None and len(objects):
        h, w = now["object"].shape
        back = rm.rewind(hits_of(now["hits"]), objects, motions_of(motions))
        cur.update(position=back["position"].reshape(h, w, 3), normal=back["normal"].reshape(h, w, 3), object=back["object"].reshape(h, w))
    return tm.accumulate(cur, prev, p), back


def _frames_equal(name, k, now, want):
    got = (now["rgb"], now["var"], now["len"], now["motion"])
    for nm, g, m in zip(NAMES, got, want):
        assert bits_equal(g, m), "%s frame %d: %s differs from the model" % (name, k, nm)


_RUNS = {}


def sequence(gpu, name, own=False):
    """The sequence of a scene, run once: three frames at 4 spp with the nudged cameras, the camera then held; the sphere most pixels
    see moved by 0.8 of its radius through Temporal.update_objects (rewound) and, on a second handle, through the handle's plain
    update (not rewound); one more frame of each.  Every frame of both is held to the chained models here."""
    if not own and name in _RUNS:                            # own=True: a run of the caller's, with an open handle it closes itself
        return _RUNS[name]
    objs, w, h, cfg = _golden(gpu, name)
    p = _model_params(gpu)
    hnd, plain_hnd = hip_scene(gpu, objs, **cfg).upload(0), hip_scene(gpu, objs, **cfg).upload(0)
    T, plain = hnd.temporal(w, h, objects=objs), plain_hnd.temporal(w, h)
    prev = plain_prev = None
    for k in range(3):
        for which in (0, 1):
            t = (T, plain)[which]
            t.frame(4, _nudged(gpu, k))
            now = _state(gpu, t, w, h)
            assert now["rewound"] is None
            want, _ = _model_frame(gpu, now, (prev, plain_prev)[which], p)
            _frames_equal(name, k, now, want)
            if which == 0:
                prev = now
            else:
                plain_prev = now
    assert all(bits_equal(prev[k], plain_prev[k]) for k in ("rgb", "var", "len"))        # two handles, one sequence so far
    seen = np.bincount(prev["object"][prev["object"] >= 0].ravel(), minlength=len(objs))
    s = [int(i) for i in np.argsort(-seen) if objs[i]["kind"] == gpu.RTX_SPHERE and seen[i] > 0][0]
    moved = objs[s:s + 1].copy()
    moved["geom"][0, 1] += 0.8 * moved["geom"][0, 3]
    objects, motions = gpu.object_motions([s], objs[s:s + 1], moved)
    assert objects.tolist() == [s]
    T.update_objects([s], moved)
    plain_hnd.update_objects([s], moved)
    T.frame(4)
    plain.frame(4)
    now, plain_now = _state(gpu, T, w, h), _state(gpu, plain, w, h)
    assert now["rewound"] is not None and plain_now["rewound"] is None
    assert now["hits"].tobytes() == plain_now["hits"].tobytes()                          # the pick itself is the unrewound one
    want, back = _model_frame(gpu, now, prev, p, objects, motions)
    assert same_hits(hits_of(now["rewound"]), back), "%s: the rewound pick differs from the model" % name
    _frames_equal(name, 3, now, want)
    plain_want, _ = _model_frame(gpu, plain_now, plain_prev, p)
    _frames_equal(name + " (not rewound)", 3, plain_now, plain_want)
    on = now["object"] == s
    four = four_tap_pixels(want[3], prev["object"], now["object"], s)                    # the model's motion, the previous pick
    objs2 = objs.copy()
    objs2[s] = moved[0]
    plain_hnd.close()
    run = dict(objs=objs2, w=w, h=h, p=p, now=now, plain_now=plain_now, on=on, four=four, sphere=s, cfg=cfg)
    if own:
        return dict(run, hnd=hnd, T=T)
    hnd.close()                                              # the shared run keeps arrays only: no test can change it for another
    _RUNS[name] = run
    return run


@pytest.mark.parametrize("name", ["mixed_40x24", "c1_three_spheres_32x32"])
def test_a_sequence_with_a_moved_sphere_equals_the_chained_models(gpu, name):
    """every output buffer of every frame -- the rewound pick included -- equals the temporal model fed with the rewind model's output
    on the device's own pick, tables and frames; without rewinding strictly fewer of the sphere's pixels take history"""
    run = sequence(gpu, name)
    on = run["on"]
    kept, plain_kept = int((run["now"]["len"][on] > 1).sum()), int((run["plain_now"]["len"][on] > 1).sum())
    print("%s: sphere %d on %d pixels; len > 1 on %d rewound, %d not rewound; %d four-tap pixels" %
          (name, run["sphere"], on.sum(), kept, plain_kept, run["four"].sum()))
    assert plain_kept < kept
    assert run["four"].sum() >= 4
    # every pixel of another object is as it would be without the rewind
    other = ~on & (run["now"]["object"] == run["plain_now"]["object"])
    for k in ("rgb", "var", "len"):
        assert bits_equal(run["now"][k][other], run["plain_now"][k][other]), k


@pytest.mark.parametrize("name", ["mixed_40x24", "c1_three_spheres_32x32"])
def test_every_four_tap_pixel_of_the_moved_sphere_keeps_its_history(gpu, name):
    """The pixels of the moved sphere whose four reprojection taps (the model's motion on the rewound pick) all lie on that sphere in
    the previous pick must have len > 1 in the rewound sequence; there are at least four of them (on an MI355X: 14 on mixed_40x24, 66 on
    c1_three_spheres_32x32, none of them left at len == 1)."""
    run = sequence(gpu, name)
    four, ln = run["four"], run["now"]["len"]
    print("%s: %d four-tap pixels, %d of them at len == 1" % (name, four.sum(), (ln[four] == 1).sum()))
    assert four.sum() >= 4
    assert (ln[four] > 1).all()


def test_a_deformed_triangle_is_rewound(gpu):
    """after the sphere: a triangle of the mixed scene gets new vertices through mode="deform"; the next frame's buffers equal the
    chained models, and its pixels take history"""
    run = sequence(gpu, "mixed_40x24", own=True)
    T, objs, w, h, p = run["T"], run["objs"], run["w"], run["h"], run["p"]
    prev = run["now"]
    seen = np.bincount(prev["object"][prev["object"] >= 0].ravel(), minlength=len(objs))
    tris = [int(i) for i in np.argsort(-seen) if objs[i]["kind"] == gpu.RTX_TRIANGLE and seen[i] > 0]
    assert tris, "the scene shows no triangle"
    t = tris[0]
    moved = objs[t:t + 1].copy()
    g = moved["geom"][0]
    centre = (g[0:3] + g[3:6] + g[6:9]) / 3.0
    for a in (0, 3, 6):                                      # shrunk towards its centre by a tenth, and shifted a little
        g[a:a + 3] = centre + 0.9 * (g[a:a + 3] - centre) + np.array([0.0, 0.03, 0.02])
    objects, motions = gpu.object_motions([t], objs[t:t + 1], moved)
    assert objects.tolist() == [t] and int(motions[0]["kind"]) == gpu.RTX_TRIANGLE
    how = T.update_objects([t], moved, mode="deform")
    assert how in ("refit", "rebuilt", "records")
    T.frame(4)
    now = _state(gpu, T, w, h)
    assert now["rewound"] is not None
    want, back = _model_frame(gpu, now, prev, p, objects, motions)
    assert same_hits(hits_of(now["rewound"]), back)
    _frames_equal("mixed_40x24, deformed triangle", 4, now, want)
    on = now["object"] == t
    print("triangle %d on %d pixels, len > 1 on %d" % (t, on.sum(), (now["len"][on] > 1).sum()))
    assert on.sum() >= 1 and (now["len"][on] > 1).any()
    # moved=... given to frame() does the same as update_objects() remembered: the (objects, motions) pair, nothing moved
    T.frame(4, moved=(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=gpu.OBJECT_MOTION_DTYPE)))
    assert T.frame_rewound is None
    T.reset()
    assert T.frame_index == 0 and T._moved == {}
    run["hnd"].close()


def test_the_temporal_moving_example(gpu, tmp_path):
    """examples/temporal_moving.cpp (rtx::object_motions, Resident::rewind_hits of rtx.hpp): 4 frames at 4 spp while three spheres
    orbit -- its accumulated frame and history length are both models chained over the same frames and picks, its denoised frame the
    denoise model's on that, its PPM the oracle's quantisation of that"""
    import subprocess
    exe = os.path.join(ROOT, "examples", "temporal_moving")
    assert os.path.exists(exe), "examples/temporal_moving is built by __graft_entry__.build()"
    w, h, frames, spp = 40, 24, 4, 4
    ppm, raw = tmp_path / "out.ppm", tmp_path / "out.f64"
    done = subprocess.run([exe, str(w), str(h), str(ppm), str(frames), str(spp), str(raw)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    objs = np.zeros(5, dtype=gpu.OBJECT_DTYPE)                                    # the example's scene (examples/temporal_orbit.cpp's)
    for k, (kind, geom, base_c, em, rough) in enumerate([
            (0, (6, 0, 8, 5), (0, 0, 0), (1, 1, 1), 1.0), (0, (6, -1.2, 0, 1), (0.8, 0.2, 0.2), (0, 0, 0), 1.0),
            (0, (7, 1.6, 0.3, 1.5), (0.9, 0.9, 0.9), (0, 0, 0), 0.1), (0, (5, -3, 2, 0.6), (0, 0, 0), (0.9, 0.6, 0.2), 1.0),
            (2, (-8, -8, -1.5, 30, -8, -1.5, 8, 20, -1.5), (0.6, 0.6, 0.6), (0, 0, 0), 1.0)]):
        objs[k]["kind"] = kind
        objs[k]["geom"][:len(geom)] = geom
        objs[k]["base_color"], objs[k]["emission_color"], objs[k]["roughness"] = base_c, em, rough
    balls = [(1, 0.8, 0.3), (2, 0.5, 2.0), (3, 0.6, 4.0)]                         # (index, orbit, phase)

    def at(k):
        out = objs[[b[0] for b in balls]].copy()
        t = 0.05 * float(k)
        for r, (i, orbit, phase) in zip(out, balls):
            r["geom"][1] = objs[i]["geom"][1] + orbit * (math.cos(t + phase) - math.cos(phase))
            r["geom"][2] = objs[i]["geom"][2] + orbit * (math.sin(t + phase) - math.sin(phase))
        return out

    idx = [b[0] for b in balls]
    hnd = hip_scene(gpu, objs, rays_per_pixel=spp).upload(0)
    T = hnd.temporal(w, h, objects=objs)
    p = _model_params(gpu)
    prev = None
    for k in range(frames):
        objects = motions = None
        if k > 0:
            objects, motions = gpu.object_motions(idx, at(k - 1), at(k))
            assert objects.tolist() == idx
            T.update_objects(idx, at(k))
        T.frame(spp, gpu.Camera(*DEFAULT_CAM) if k == 0 else None)
        now = _state(gpu, T, w, h)
        (out, var, ln, _), _ = _model_frame(gpu, now, prev, p, objects, motions)
        prev = dict(now, rgb=out, var=var, len=ln)          # the models' own chain
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
    moving = np.isin(prev["object"], idx)
    assert moving.sum() >= 8 and (prev["len"][moving] > 1).sum() * 2 >= moving.sum()      # the moving spheres keep their history
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
    assert len(names) <= 25 and "epilogue_kernel" in names, names      # the rewind is a form of epilogue_kernel, not a new kernel
