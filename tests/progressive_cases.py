"""The scenes of tests/test_progressive.py and tests/test_sample_queries.py and their yardstick: the per-sample colours of a frame, taken
from the exhaustive render kernel's path transcripts (rtx_debug_paths, lab library) replayed over the materials in plain Python -- code
that runs neither the fold of rtx_render_blocks_accumulate nor the ray generation of rtx_scene_trace_samples.  Computed once per case."""
import itertools

import numpy as np

from helpers import DEFAULT_CAM, hip_scene

RENDER_CASES = ("mixed", "mesh", "joint", "axis-aligned mesh")           # tests/test_path_queries.py's
CASES = RENDER_CASES + ("spheres",)
CAMERA_B = ((0.6, -0.4, 0.3), (0.9, 0.35, -0.2), DEFAULT_CAM[2])          # another view with the same fov: the trig tables stay, the tile lists must not


def case(name):
    """(objects, width, height, camera, config)"""
    if name == "spheres":
        from rust_raytracing_amd import scenes
        return scenes.light_every(scenes.compact(scenes.random_spheres(400, 4))), 52, 27, DEFAULT_CAM, dict(rays_per_pixel=5, seed=11)
    from test_path_queries import _render_case
    return _render_case(name)


def band_rows(height, block_rows, part, n_parts):
    """image rows of part `part` of `n_parts` (blocks of block_rows rows dealt out round-robin), in increasing order"""
    return [y for y in range(height) if (y // block_rows) % n_parts == part]


_REPLAY = {}


def replay(gpu, name):
    """dict(colour [h][w][S][3], segments [h][w][S], first [h][w][S] PATH_STEP records): every sample of the case's frame, from the lab
    handle's transcripts of every row replayed over the materials (scene.rs:276-277), as
    test_the_renders_own_rays_give_the_renders_samples does for every third row"""
    if name in _REPLAY:
        return _REPLAY[name]
    objs, w, h, cam, cfg = case(name)
    spp = cfg["rays_per_pixel"]
    lab = hip_scene(gpu, objs, cam=cam, kernel=gpu.RTX_KERNEL_EXACT, **cfg).upload(0, lab=True)
    em, base = objs["emission_color"].tolist(), objs["base_color"].tolist()
    colour = np.zeros((h, w, spp, 3), dtype=np.float64)
    segments = np.zeros((h, w, spp), dtype=np.uint32)
    first = []
    for row in range(h):
        st, cnt = lab.debug_paths(w, h, row, 12)
        assert cnt.max() <= 11
        segments[row] = cnt
        first.append(st[:, :, 0].copy())
        winners = st["object"]
        for x in range(w):
            for s in range(spp):
                result, light = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
                for k in range(int(cnt[x, s])):
                    obj = int(winners[x, s, k])
                    if obj < 0:
                        break
                    result = [result[c] + light[c] * em[obj][c] for c in range(3)]
                    light = [light[c] * base[obj][c] for c in range(3)]
                colour[row, x, s] = result
    lab.close()
    _REPLAY[name] = dict(colour=colour, segments=segments, first=np.stack(first))
    return _REPLAY[name]


def left_fold(values):
    """((0 + v0) + v1) + ... along axis 2 of values [h][w][S][3]: plain numpy adds in sample order, every sample included"""
    total = np.zeros(values.shape[:2] + (3,), dtype=np.float64)
    for s in range(values.shape[2]):
        total = total + values[:, :, s]
    return total


def fold_census(colour):
    """what makes a wrong fold visible in a case: (lit samples, samples, pixels with >= 2 lit samples, pixels with a zero sample between
    two lit ones, pixels whose sum of squares differs for some other order of the samples)"""
    h, w, spp, _ = colour.shape
    lit = colour.any(axis=3)                                                    # [h][w][S]
    two = lit.sum(axis=2) >= 2
    between = np.zeros((h, w), dtype=bool)
    for a in range(spp):
        for b in range(a + 2, spp):
            between |= lit[:, :, a] & lit[:, :, b] & ~lit[:, :, a + 1:b].all(axis=2)
    sq = colour * colour
    in_order = left_fold(sq)
    depends = np.zeros((h, w), dtype=bool)
    for perm in itertools.permutations(range(spp)):
        depends |= (left_fold(sq[:, :, list(perm)]).view(np.uint64) != in_order.view(np.uint64)).any(axis=2)
    return int(lit.sum()), int(lit.size), int(two.sum()), int(between.sum()), int(depends.sum())


FLOORS = {"mixed": (100, 5, 0), "mesh": (100, 5, 5), "joint": (100, 5, 5), "axis-aligned mesh": (100, 0, 0), "spheres": (100, 5, 5)}


def check_census(name, colour):
    """prints the census and holds it to the floors: a fold in the wrong order, or a mask skip that drops or double-counts, cannot pass"""
    lit, total, two, between, depends = fold_census(colour)
    print("%s: lit samples %d / %d, pixels with >= 2 lit samples %d, with a zero sample between two lit ones %d, whose squares' sum "
          "depends on the fold order %d" % (name, lit, total, two, between, depends))
    f_two, f_between, f_depends = FLOORS[name]
    assert two >= f_two and between >= f_between and depends >= f_depends, (name, two, between, depends)
