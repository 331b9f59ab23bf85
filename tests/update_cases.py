"""The scenes and the updates of tests/test_scene_update.py (host, no GPU) and tests/test_scene_update_gpu.py: one builder, so the
device is held to the host reference on exactly the inputs the host reference was checked on.

An update is (indices, objects, how): `objects[i]` replaces Scene.objects[indices[i]], `how` is the path include/rtx_hip.h
("Which path runs") prescribes for it.  Moves are drawn inside the bounding box of the sphere centres, shrunk by the largest
radius: no new box can then pass the range the resident tree was built for, so AUTO must refit and never rebuild."""
import numpy as np

from rust_raytracing_amd import scenes
from rust_raytracing_amd.abi import OBJECT_DTYPE, RTX_PLANE, RTX_SPHERE, RTX_TRIANGLE

MOVE_CASES = ("one", "third", "all", "repeat", "radius", "inbox")         # REFIT on every scene with a sphere tree
RECORD_CASES = ("material", "plane")                                       # RECORDS
FALLBACK_CASES = ("far", "nan_radius", "kind", "tri_vertex", "rebuild")    # REBUILT
HOST_SPHERE_COUNTS = (5, 6, 9, 17, 65, 300)
GPU_SPHERE_COUNTS = (5, 9, 65, 300, 3000)


def sphere_scene(n, seed=3):
    return scenes.light_every(scenes.compact(scenes.random_spheres(n, seed)), 3)


def scene(name):
    """'s<N>': N compacted spheres; 'c2': random_spheres(10000) as the benchmark places them; 'mixed': mixed_scene(40, 40, 1)."""
    if name == "mixed":
        return scenes.mixed_scene(40, 40, 1)
    if name == "c2":
        return scenes.random_spheres(10000)
    return sphere_scene(int(name[1:]))


def has(objs, kind):
    return bool(np.any(objs["kind"] == kind))


def cases_for(objs):
    """the update cases that exist on this scene (a plane update needs a plane, a vertex change a triangle)"""
    out = list(MOVE_CASES) + ["material"]
    if has(objs, RTX_PLANE):
        out.append("plane")
    return out


def fallbacks_for(objs):
    return [c for c in FALLBACK_CASES if c != "tri_vertex" or has(objs, RTX_TRIANGLE)]


def _move_box(objs):
    g = objs["geom"][objs["kind"] == RTX_SPHERE]
    rmax = float(np.abs(g[:, 3]).max())
    lo, hi = g[:, :3].min(axis=0) + rmax, g[:, :3].max(axis=0) - rmax
    mid = 0.5 * (lo + hi)
    return np.where(lo <= hi, lo, mid), np.where(lo <= hi, hi, mid)


def update(objs, case, seed=0):
    """-> (indices uint64, objects OBJECT_DTYPE, how)"""
    rng = np.random.default_rng(1000 + seed)
    sph = np.nonzero(objs["kind"] == RTX_SPHERE)[0]
    lo, hi = _move_box(objs)

    def jitter(idx):
        new = objs[idx].copy()
        c = new["geom"][:, :3] + rng.normal(size=(len(idx), 3)) * 0.05 * (hi - lo + 1.0)
        new["geom"][:, :3] = np.clip(c, lo, hi)
        return new

    if case == "one":
        idx = sph[[int(rng.integers(0, len(sph)))]]
        return idx.astype(np.uint64), jitter(idx), "refit"
    if case == "third":
        idx = rng.permutation(sph)[:max(1, len(sph) // 3)]
        return idx.astype(np.uint64), jitter(idx), "refit"
    if case == "all":
        return sph.astype(np.uint64), jitter(sph), "refit"
    if case == "repeat":                            # every index twice or three times: the LAST entry is the one that counts
        idx = rng.permutation(sph)[:max(2, len(sph) // 4)]
        idx = np.concatenate([idx, idx[::-1], idx[:2]])
        return idx.astype(np.uint64), jitter(idx), "refit"
    if case == "radius":
        idx = rng.permutation(sph)[:max(1, len(sph) // 3)]
        new = objs[idx].copy()
        new["geom"][:, 3] *= rng.uniform(0.3, 0.95, len(idx))
        return idx.astype(np.uint64), new, "refit"
    if case == "inbox":
        new = objs[sph].copy()
        new["geom"][:, :3] = lo + (hi - lo) * rng.random((len(sph), 3))
        return sph.astype(np.uint64), new, "refit"
    if case == "material":                          # of every kind the scene has; the geometry stays
        idx = rng.permutation(len(objs))[:max(3, len(objs) // 5)]
        new = objs[idx].copy()
        new["base_color"] = rng.uniform(0.1, 0.9, (len(idx), 3))
        new["roughness"] = rng.uniform(0.0, 1.0, len(idx))
        new["emission_color"][::2] = rng.uniform(0.5, 3.0, (len(new["emission_color"][::2]), 3))
        return idx.astype(np.uint64), new, "records"
    if case == "plane":
        idx = np.nonzero(objs["kind"] == RTX_PLANE)[0][:1]
        new = objs[idx].copy()
        new["geom"][0, :6] = (0.5, -0.25, -3.5, 0.1, -0.05, 1.0)
        return idx.astype(np.uint64), new, "records"
    # ---- what must fall back to a rebuild
    if case == "far":                               # 1e6 times the scene's extent
        idx = sph[[0]]
        new = objs[idx].copy()
        ext = float(np.abs(objs["geom"][sph, :3]).max())
        new["geom"][0, :3] = (1.0e6 * ext, 0.0, 0.0)
        return idx.astype(np.uint64), new, "rebuilt"
    if case == "nan_radius":
        idx = sph[[len(sph) // 2]]
        new = objs[idx].copy()
        new["geom"][0, 3] = np.nan
        return idx.astype(np.uint64), new, "rebuilt"
    if case == "kind":                              # a sphere becomes a plane
        idx = sph[[1]]
        new = np.zeros(1, dtype=OBJECT_DTYPE)
        new["kind"] = RTX_PLANE
        new["geom"][0, :6] = (0, 0, -4.0, 0, 0, 1)
        new["base_color"] = (0.5, 0.6, 0.7)
        new["roughness"] = 0.5
        return idx.astype(np.uint64), new, "rebuilt"
    if case == "tri_vertex":
        idx = np.nonzero(objs["kind"] == RTX_TRIANGLE)[0][[3]]
        new = objs[idx].copy()
        new["geom"][0, 3:6] += (0.05, -0.02, 0.03)
        return idx.astype(np.uint64), new, "rebuilt"
    if case == "rebuild":                           # an ordinary move under RTX_UPDATE_REBUILD
        idx, new, _ = update(objs, "third", seed)
        return idx, new, "rebuilt"
    raise KeyError(case)


def apply(objs, indices, new):
    """the updated object list: entries in order, so the last entry of a repeated index wins"""
    out = objs.copy()
    for i, o in zip(indices, new):
        out[int(i)] = o
    return out
