"""The scenes and the updates of tests/test_scene_update.py (host, no GPU) and tests/test_scene_update_gpu.py: one builder, so the
device is held to the host reference on exactly the inputs the host reference was checked on.

An update is (indices, objects, how): `objects[i]` replaces Scene.objects[indices[i]], `how` is the path include/rtx_hip.h
("Which path runs") prescribes for it.  Moves are drawn inside the bounding box of the sphere centres, shrunk by the largest
radius: no new box can then pass the range the resident tree was built for, so AUTO must refit and never rebuild."""
import numpy as np

from rust_raytracing_amd import scenes
from rust_raytracing_amd.abi import OBJECT_DTYPE, RTX_PLANE, RTX_SPHERE, RTX_TRIANGLE

MOVE_CASES = ("one", "third", "all", "repeat", "radius", "inbox")         # REFIT on every scene with a sphere tree
EDGE_CASES = ("grow", "zero_radius", "neg_radius", "neg_zero", "scale_in")  # REFIT: the edges of the geometry and of the path decision
RECORD_CASES = ("material", "plane")                                       # RECORDS
FALLBACK_CASES = ("far", "nan_radius", "kind", "tri_vertex", "rebuild", "scale_out")    # REBUILT, decided by plan_update
# REBUILT although plan_update alone would refit: the device (mode B) finds a 64-byte node without an encoding -- co-located spheres of
# radius 1e-9 make a node of extent 4 abs_pad, so small for its distance from the origin that |o / s| + 256 < 2^24 fails -- sets
# kUpdateStatusNoQ3, and the host rebuilds over the half-written arrays.  Only on pure sphere scenes (a joint tree has no 64-byte form
# to lose).
DEVICE_FALLBACK_CASES = ("collapse8", "onepoint_tiny")
ONEPOINT_SCENES = ("s9", "s65", "s300", "s3000")                           # where collapse8 / onepoint / onepoint_tiny are stated
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
    out = list(MOVE_CASES) + list(EDGE_CASES) + ["material"]
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


def scene_box(objs):
    """the box of the spheres' own (unpadded) boxes: what the tree was built for"""
    g = objs["geom"][objs["kind"] == RTX_SPHERE]
    r = np.abs(g[:, 3:4])
    return (g[:, :3] - r).min(axis=0), (g[:, :3] + r).max(axis=0)


def inside_build_range(objs, new):
    """no sphere of `new` has a box c +- |r| outside scene_box(objs): such an update cannot pass the build's `scale`"""
    lo, hi = scene_box(objs)
    g = new["geom"][new["kind"] == RTX_SPHERE]
    r = np.abs(g[:, 3:4])
    return bool(((g[:, :3] - r) >= lo).all() and ((g[:, :3] + r) <= hi).all())


def build_scale(objs):
    """the `scale` the resident tree was built for, (origin_limit - 1) / 4, from the restated builder's f32 origin_limit"""
    import bounds_model as bm
    return (float(bm.pack(objs)["limit32"]) - 1.0) / 4.0


def collapse(objs, idx, radius):
    """the spheres `idx` at the `hi` corner of the move box with one radius"""
    _, hi = _move_box(objs)
    new = objs[idx].copy()
    new["geom"][:, :3] = hi
    new["geom"][:, 3] = radius
    return new


def nearest8(objs):
    """the 8 spheres nearest to the first sphere (itself included)"""
    sph = np.nonzero(objs["kind"] == RTX_SPHERE)[0]
    c = objs["geom"][sph, :3]
    return sph[np.argsort(np.linalg.norm(c - c[0], axis=1), kind="stable")[:8]]


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
    # ---- edges of the geometry and of the path decision
    if case == "grow":                              # radii x U(1.05, 1.6), clipped so that no box leaves the box the tree was built for
        blo, bhi = scene_box(objs)
        new = objs[sph].copy()
        c, r = new["geom"][:, :3], np.abs(new["geom"][:, 3])
        room = 0.99 * np.minimum(c - blo, bhi - c).min(axis=1)
        new["geom"][:, 3] = np.maximum(r, np.minimum(r * rng.uniform(1.05, 1.6, len(sph)), room))
        return sph.astype(np.uint64), new, "refit"
    if case in ("zero_radius", "neg_radius"):
        idx = rng.permutation(sph)[:max(1, len(sph) // 3)]
        new = objs[idx].copy()
        new["geom"][:, 3] = 0.0 if case == "zero_radius" else -0.9 * np.abs(new["geom"][:, 3])
        return idx.astype(np.uint64), new, "refit"
    if case == "neg_zero":                          # one sphere per axis gets a coordinate of -0.0, where the move box reaches 0
        axes = [a for a in range(3) if lo[a] <= 0.0 <= hi[a]]
        assert axes, "neg_zero: the move box excludes 0 on every axis of this scene"
        idx = rng.permutation(sph)[:len(axes)]
        new = objs[idx].copy()
        for k, a in enumerate(axes):
            new["geom"][k, a] = -0.0
        return idx.astype(np.uint64), new, "refit"
    if case in ("scale_in", "scale_out"):           # one sphere along +x: its padded hi.x at 0.999 / 1.001 of the build's scale
        idx = sph[[0]]
        new = objs[idx].copy()
        r = abs(float(new["geom"][0, 3]))
        want = (0.999 if case == "scale_in" else 1.001) * build_scale(objs)
        k = 1.0 / 1048576.0
        new["geom"][0, 0] = (want - r * (1.0 + k)) / (1.0 + k)           # x + r + (|x| + r) 2^-20 = want, x > 0
        return idx.astype(np.uint64), new, "refit" if case == "scale_in" else "rebuilt"
    # ---- co-located spheres: every box of their sub-tree (onepoint: of the tree) coincides
    if case == "collapse8":
        idx = nearest8(objs)
        return idx.astype(np.uint64), collapse(objs, idx, 1.0e-9), "rebuilt"
    if case == "onepoint":
        return sph.astype(np.uint64), collapse(objs, sph, 1.0e-4), "refit"
    if case == "onepoint_tiny":
        return sph.astype(np.uint64), collapse(objs, sph, 1.0e-9), "rebuilt"
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
