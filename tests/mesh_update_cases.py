"""The scenes and the updates of tests/test_mesh_update.py (host, no GPU) and tests/test_mesh_update_gpu.py: one builder, as
tests/update_cases.py is for the spheres.

Under RTX_UPDATE_DEFORM a triangle with new vertices is written in place when it keeps its CLASS (include/rtx_hip.h, "Triangles").
The class rule is restated here in Python (tri_class: the zero-pivot swaps of Triangle::contains, n.v0, the det condition), so every
case states on its own which path the library must take: the host suite requires plan_update's `how` to agree with this second
reading on every case.  REFIT / RECORDS cases update only triangles the restatement says keep their class; the `flip` fallback
updates the ones it says change it."""
import math

import numpy as np

import update_cases as uc
from rust_raytracing_amd import scenes
from rust_raytracing_amd.abi import OBJECT_DTYPE, RTX_SPHERE, RTX_TRIANGLE

SCENES = ("t6", "t40", "t300", "t1100", "cubes25", "mixed")
RANDOM_SCENES = ("t6", "t40", "t300", "t1100")
DEFORM_CASES = ("shrink", "slide", "jitter", "one", "third", "repeat", "grow", "material_only")      # REFIT (RECORDS on t6, and material_only)
FALLBACK_CASES = ("flip", "degenerate", "nan_vertex", "far", "free_axis", "kind", "auto_tri_vertex")


def scene(name):
    if name == "mixed":
        return scenes.mixed_scene(40, 40, 1)
    if name == "cubes25":
        return scenes.axis_aligned_mesh(25)
    return scenes.light_every(scenes.compact(scenes.random_triangles(int(name[1:]), 4)), 3)


_cache = {}


def cached_scene(name):
    if name not in _cache:
        _cache[name] = scene(name)
    return _cache[name].copy()


def tri_indices(objs):
    return np.nonzero(objs["kind"] == RTX_TRIANGLE)[0]


# ---- the class rule, restated ------------------------------------------------------------------------------------------------------
def centre_of(objs):
    """pack_scene's centre: the middle of the box of the sphere centres and the triangle vertices (finite coordinates)"""
    pts = [objs["geom"][objs["kind"] == RTX_SPHERE][:, :3], objs["geom"][objs["kind"] == RTX_TRIANGLE].reshape(-1, 3)]
    p = np.concatenate(pts)
    c = np.zeros(3)
    for a in range(3):
        x = p[np.isfinite(p[:, a]), a]
        if len(x):
            c[a] = 0.5 * (x.min() + x.max())
    return c


def tri_class(geom, centre):
    """("none",) / ("always",) / ("qualified", free_axis) of one triangle (9 doubles), as the upload decides it"""
    g = [float(x) for x in geom]
    v0, v1, v2 = g[0:3], g[3:6], g[6:9]
    r = [v1[c] - v0[c] for c in range(3)]
    s = [v2[c] - v0[c] for c in range(3)]
    n = [r[1] * s[2] - r[2] * s[1], r[2] * s[0] - r[0] * s[2], r[0] * s[1] - r[1] * s[0]]
    ln = math.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    n = [x / ln if ln != 0.0 else math.nan for x in n]
    # Triangle::contains' elimination on the (r, s) columns: which rows feed it after the zero-pivot swaps
    ax, ay, idx = list(r), list(s), [0, 1, 2]
    if ax[0] == 0.0:
        k = 1 if ax[1] != 0.0 else 2
        if ax[k] == 0.0:
            return ("none",)
        ax[0], ax[k], ay[0], ay[k], idx[0], idx[k] = ax[k], ax[0], ay[k], ay[0], idx[k], idx[0]
    l1y = ay[0] / ax[0]
    l2y, l3y, j = ay[1] - l1y * ax[1], ay[2] - l1y * ax[2], 1
    if l2y == 0.0:
        if l3y == 0.0:
            return ("none",)
        j = 2
    i, j = idx[0], idx[j]
    kabs = n[0] * v0[0] + n[1] * v0[1] + n[2] * v0[2]
    if not all(math.isfinite(x) for x in n + [kabs]) or kabs < -(1.0 + 1e-9):
        return ("none",)
    f = 3 - i - j
    a0, a1 = (1 if f == 0 else 0), (1 if f == 2 else 2)
    w = [[g[3 * k + c] - centre[c] for c in range(3)] for k in range(3)]
    r0, r1, s0, s1 = w[1][a0] - w[0][a0], w[1][a1] - w[0][a1], w[2][a0] - w[0][a0], w[2][a1] - w[0][a1]
    det = r0 * s1 - r1 * s0
    if all(math.isfinite(x) for x in g) and abs(det) > 1e-6 * math.hypot(r0, r1) * math.hypot(s0, s1):
        return ("qualified", f)
    return ("always",)


def classes(objs, centre=None):
    """{object index: class} of every triangle of the scene"""
    c = centre_of(objs) if centre is None else centre
    return {int(k): tri_class(objs["geom"][k], c) for k in tri_indices(objs)}


def in_tree(objs):
    """the triangles whose record is a tree record: qualified, and more than 4 share their footprint plane"""
    cls = classes(objs)
    per_axis = {f: sum(1 for c in cls.values() if c == ("qualified", f)) for f in range(3)}
    return {k for k, c in cls.items() if c[0] == "qualified" and per_axis[c[1]] > 4}


def build_scale(objs):
    """the largest finite |coordinate| of the boxes the tree was built over (spheres: more than 4 of them), or -1 without a tree"""
    scale, k = -1.0, 1.0 / 1048576.0
    cls, tree = classes(objs), in_tree(objs)
    for i in tree:
        v = objs["geom"][i].reshape(3, 3)
        for a in range(3):
            if a == cls[i][1]:
                continue
            lo, hi = v[:, a].min(), v[:, a].max()
            pad = max(abs(lo), abs(hi)) * k + 1e-300
            scale = max(scale, abs(lo - pad), abs(hi + pad))
    g = objs["geom"][objs["kind"] == RTX_SPHERE]
    if len(g) > 4:
        r = np.abs(g[:, 3:4])
        pad = (np.abs(g[:, :3]) + r) * k + 1e-300
        scale = max(scale, float(np.abs(g[:, :3] - r - pad).max()), float(np.abs(g[:, :3] + r + pad).max()))
    return scale


def reach(geom, centre):
    return float(np.abs(np.asarray(geom, dtype=np.float64).reshape(3, 3) - centre).max())


def tri_extent(objs, centre):
    """the largest |v - centre| coordinate over the qualified triangles: exact f64 operations, so the library's value bit for bit"""
    return max([reach(objs["geom"][k], centre) for k, c in classes(objs, centre).items() if c[0] == "qualified"], default=0.0)


def kept(objs, idx, new, centre=None):
    """mask over the entries: the new geometry has the class (and free axis) of the resident triangle and lies inside the build's range"""
    c = centre_of(objs) if centre is None else centre
    scale = build_scale(objs)
    out = np.zeros(len(idx), dtype=bool)
    for k, (i, o) in enumerate(zip(idx, new)):
        was, now = tri_class(objs["geom"][int(i)], c), tri_class(o["geom"], c)
        ok = was == now and bool(np.isfinite(o["geom"]).all())
        if ok and now[0] == "qualified" and scale >= 0.0:
            v = o["geom"].reshape(3, 3)
            for a in range(3):
                if a != now[1]:
                    m = max(abs(v[:, a].min()), abs(v[:, a].max()))
                    ok = ok and m * (1.0 + 1.0 / 1048576.0) + 1e-300 <= scale
        out[k] = ok
    return out


# ---- the deformations ----------------------------------------------------------------------------------------------------------------
def _vertex_box(objs):
    v = objs["geom"][objs["kind"] == RTX_TRIANGLE].reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


def _deformed(objs, idx, what, rng):
    new = objs[idx].copy()
    v = new["geom"].reshape(len(idx), 3, 3)
    lo, hi = _vertex_box(objs)
    if what == "shrink":
        c = v.mean(axis=1, keepdims=True)
        v = c + 0.8 * (v - c)
    elif what == "slide":
        v = np.clip(v + np.array([0.0, 0.02, 0.1]), lo, hi)
    elif what == "jitter":
        v = np.clip(v + rng.normal(size=v.shape) * 0.03, lo, hi)
    else:
        raise KeyError(what)
    new["geom"] = v.reshape(len(idx), 9)
    return new


def _how(objs, idx):
    tree = in_tree(objs)
    return "refit" if any(int(i) in tree for i in idx) else "records"


def update(objs, case, seed=0, name=None):
    """-> (indices uint64, objects OBJECT_DTYPE, how, mode)"""
    rng = np.random.default_rng(2000 + seed)
    tri = tri_indices(objs)

    def keep(idx, new):
        m = kept(objs, idx, new)
        return idx[m].astype(np.uint64), new[m], m

    if case in ("shrink", "slide", "jitter"):
        idx, new, m = keep(tri, _deformed(objs, tri, case, rng))
        if case == "shrink":
            assert m.all(), "shrink changes the class of %d triangles" % int((~m).sum())
        if case == "jitter" and name in RANDOM_SCENES:         # (six triangles: one of them is 17 %, so there "all but one")
            assert m.mean() >= 0.9 or (~m).sum() <= 1, "jitter keeps only %.0f %% of the classes" % (100 * m.mean())
        assert len(idx)
        return idx, new, _how(objs, idx), "deform"
    if case in ("one", "third", "repeat"):
        allidx, allnew, _ = keep(tri, _deformed(objs, tri, "jitter", rng))
        order = rng.permutation(len(allidx))
        if case == "one":
            pick = order[:1]
        elif case == "third":
            pick = order[:max(1, len(order) // 3)]
        else:                                           # every index twice or three times: the LAST entry is the one that counts
            pick = order[:max(2, len(order) // 4)]
            first = _deformed(objs, allidx[pick].astype(np.int64), "shrink", rng)
            idx = np.concatenate([allidx[pick], allidx[pick][::-1], allidx[pick][:2]])
            new = np.concatenate([first, allnew[pick][::-1], allnew[pick][:2]])
            return idx.astype(np.uint64), new, _how(objs, idx), "deform"
        return allidx[pick], allnew[pick], _how(objs, allidx[pick]), "deform"
    if case == "grow":
        # The extreme vertex of the qualified triangles goes further out, to 1.25 tri_extent -- along the axis its triangle's footprint
        # is unbounded on, so no box can leave the build's range.  The triangle is the one with the largest reach that keeps its class
        # under such a move: the first on the random scenes; an axis-aligned face solved in (x, z) or (y, z) leaves its plane, so on
        # the cubes it is the furthest (x, y) face.
        c = centre_of(objs)
        cls = classes(objs)
        ext = tri_extent(objs, c)
        q = sorted((k for k in tri if cls[int(k)][0] == "qualified"), key=lambda i: -reach(objs["geom"][i], c))
        for k in q:
            f = cls[int(k)][1]
            d = np.abs(objs["geom"][k].reshape(3, 3) - c)
            vtx = int(np.unravel_index(np.argmax(d), d.shape)[0])
            for sign in (1.0, -1.0):
                new = objs[[k]].copy()
                new["geom"][0, 3 * vtx + f] = c[f] + sign * 1.25 * ext
                idx = np.array([k], dtype=np.uint64)
                if kept(objs, idx, new).all():
                    assert tri_extent(uc.apply(objs, idx, new), c) > ext
                    return idx, new, _how(objs, idx), "deform"
        raise AssertionError("grow: no move keeps a class")
    if case == "with_spheres":                          # moved spheres and deformed triangles in one call
        i1, n1, _ = uc.update(objs, "third", seed)
        i2, n2, _, _ = update(objs, "shrink", seed)
        return np.concatenate([i1, i2]), np.concatenate([n1, n2]), "refit", "deform"
    if case == "material_only":
        idx, new, _ = _material(objs, rng)
        return idx, new, "records", "deform"
    # ---- what must fall back to a rebuild (all under DEFORM, but the last)
    if case == "flip":                                  # the triangles whose class the jitter changes
        new = _deformed(objs, tri, "jitter", rng)
        m = kept(objs, tri, new)
        assert (~m).any()
        return tri[~m].astype(np.uint64), new[~m], "rebuilt", "deform"
    if case in ("degenerate", "nan_vertex", "far", "auto_tri_vertex"):
        cls = classes(objs)                             # a qualified triangle: one with a footprint to lose
        idx = np.array([[k for k in tri if cls[int(k)][0] == "qualified"][1]])
        new = objs[idx].copy()
        if case == "degenerate":
            new["geom"][0, 3:6] = new["geom"][0, 0:3]
        elif case == "nan_vertex":
            new["geom"][0, 7] = np.nan
        elif case == "far":
            new["geom"][0, 0:3] = 1.0e6 * float(np.abs(objs["geom"][tri]).max())
        else:
            new["geom"][0, 3:6] += (0.05, -0.02, 0.03)
        assert case == "auto_tri_vertex" or not kept(objs, idx, new).any()
        return idx.astype(np.uint64), new, "rebuilt", "auto" if case == "auto_tri_vertex" else "deform"
    if case == "free_axis":                             # a face solved in (x, z) or (y, z) is rotated out of its plane: now (x, y)
        c = centre_of(objs)
        cls = classes(objs)
        for k in tri:
            if cls[int(k)][0] != "qualified" or cls[int(k)][1] == 2:
                continue
            new = objs[[k]].copy()
            new["geom"][0, 3:6] += (0.11, 0.07, 0.05)
            now = tri_class(new["geom"][0], c)
            if now[0] == "qualified" and now[1] != cls[int(k)][1]:
                return np.array([k], dtype=np.uint64), new, "rebuilt", "deform"
        raise AssertionError("free_axis: no face leaves its plane")
    if case == "kind":                                  # a sphere becomes a triangle
        idx = np.nonzero(objs["kind"] == RTX_SPHERE)[0][[1]]
        new = np.zeros(1, dtype=OBJECT_DTYPE)
        new["kind"] = RTX_TRIANGLE
        new["geom"][0] = objs["geom"][tri[0]] + 0.01
        new["base_color"] = (0.5, 0.6, 0.7)
        new["roughness"] = 0.5
        return idx.astype(np.uint64), new, "rebuilt", "deform"
    raise KeyError(case)


def _material(objs, rng):
    idx = rng.permutation(len(objs))[:max(3, len(objs) // 5)]
    new = objs[idx].copy()
    new["base_color"] = rng.uniform(0.1, 0.9, (len(idx), 3))
    new["roughness"] = rng.uniform(0.0, 1.0, len(idx))
    new["emission_color"][::2] = rng.uniform(0.5, 3.0, (len(new["emission_color"][::2]), 3))
    return idx.astype(np.uint64), new, "records"


def cases_for(name):
    return list(DEFORM_CASES) + (["with_spheres"] if name == "mixed" else [])


def fallbacks_for(name):
    out = ["degenerate", "nan_vertex", "auto_tri_vertex"]
    if name != "t6":                                    # (no tree, so no range a footprint could leave: there `far` is a RECORDS update)
        out.append("far")
    if name != "mixed":                                 # (the jitter keeps every class of the joint scene's 40 triangles)
        out.append("flip")
    if name == "cubes25":
        out.append("free_axis")
    if name == "mixed":
        out.append("kind")
    return out


apply = uc.apply

_cases = {}


def case_of(name, case, seed=0):
    """update(cached_scene(name), case, seed), built once per process: -> (objs, indices, objects, how, mode)"""
    key = (name, case, seed)
    if key not in _cases:
        objs = cached_scene(name)
        _cases[key] = (objs,) + update(objs, case, seed, name=name)
    objs, idx, new, how, mode = _cases[key]
    return objs.copy(), idx.copy(), new.copy(), how, mode


def pairs():
    return [(s, c) for s in SCENES for c in cases_for(s)]
