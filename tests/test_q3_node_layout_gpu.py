"""The interleaved 64-byte sphere node (rtx_bvh.h BvhQ3Node) as the kernels read it: frames (render_rows) and batched queries
(closest_hits) of RTX_KERNEL_AUTO against the exhaustive f64 kernel, bit for bit.

The smallest shapes at which a misplaced word shows: scenes of 3, 5 and 6 spheres (3: under the tree threshold, the list is swept; 5 and
6: one node with empty slots, the smallest trees there are), the 200-sphere golden scene
(full nodes, several levels), a camera inside the cloud and one far beyond the tree's origin limit (the slack path of Ray32S), a
one-stage launch and the two-stage form.
"""
import json
import os

import numpy as np
import pytest

from helpers import check_equal, hip_scene
from test_stage2_visit import _cameras, _render, _scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAMERAS = ("inside", "far over it")


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _case(gpu, name):
    """(objects, width, height, rays per pixel)"""
    if name == "golden200":
        z = np.load(os.path.join(GOLDEN, "spheres200_48x27.npz"))
        assert json.loads(str(z["config"]))["rays_per_pixel"] == 2
        return np.frombuffer(z["objects"].tobytes(), dtype=gpu.OBJECT_DTYPE), int(z["width"]), int(z["height"]), 2
    return _scenes()[name], 64, 36, 3


NAMES = ["few3", "few5", "few6", "golden200"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_frames_equal_the_exhaustive_kernel(gpu, name):
    objs, w, h, spp = _case(gpu, name)
    cams = {c[0]: c for c in _cameras(objs)}
    for cname in CAMERAS:
        _, cam, cfg = cams[cname]
        ref, st_ref = _render(gpu, objs, cam, gpu.RTX_KERNEL_EXACT, 0, w, h, spp, **cfg)
        for tune in (0, gpu.RTX_TUNE_TWO_STAGE):
            img, st = _render(gpu, objs, cam, gpu.RTX_KERNEL_AUTO, tune, w, h, spp, **cfg)
            assert np.array_equal(img.view(np.int64), ref.view(np.int64)), (name, cname, tune)
            assert st.segments == st_ref.segments, (name, cname, tune)


def _rays(objs, cam, n, rng):
    """n rays from the camera's position (inside the cloud, or beyond the origin limit) at points spread over the cloud's box and a
    little around it"""
    g = objs["geom"]
    lo = (g[:, :3] - np.abs(g[:, 3:4])).min(axis=0)
    hi = (g[:, :3] + np.abs(g[:, 3:4])).max(axis=0)
    o = np.tile(np.asarray(cam[0], dtype=np.float64), (n, 1))
    d = lo + (hi - lo) * rng.uniform(-0.1, 1.1, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_queries_equal_the_exhaustive_kernel(gpu, name):
    objs, _, _, _ = _case(gpu, name)
    cams = {c[0]: c for c in _cameras(objs)}
    rng = np.random.default_rng(29)
    auto = hip_scene(gpu, objs, kernel=gpu.RTX_KERNEL_AUTO).upload(0)
    exact = hip_scene(gpu, objs, kernel=gpu.RTX_KERNEL_EXACT).upload(0)
    hit = 0
    for cname in CAMERAS:
        o, d = _rays(objs, cams[cname][1], 4096, rng)
        want = exact.query(o, d)
        check_equal(auto.query(o, d), want, "%s, %s" % (name, cname))
        hit += int((want[1] >= 0).sum())
    auto.close()
    exact.close()
    assert hit > 100, (name, hit)                                              # the rays do reach the spheres
