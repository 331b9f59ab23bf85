"""Scenes and rays aimed at the LDS sweep's two f32 filters (trace_mixed_kernel: filter_from_ray / filter_disc2 over sphere_f32,
tri_filter_from_ray / tri_filter_sign over tri_f32), for tests/test_sweep_filters.py.  Everything is seeded and regenerated on every
run; nothing is stored.

Reused (case()): tests/bounds_cases.py's aimed families on its own scenes -- tangents at 0, +-1, 4, 64 ulps of f32 and of f64,
secants, head-on rays, triangle edges and vertices, the cull threshold, the surface regime.  The sweep has no "no walk" form: the far26
and nowalk regimes count here like every other.  bounds_cases aims at the objects of the TREE; on the scenes below, which have none
(or keep shapes outside it), the same generator aims at every sphere and triangle.

Scenes the tree tests cannot have (scenes()):
  s4t4      four spheres and four (x, y)-solved triangles: no class has more than four shapes, so there is no tree and AUTO sweeps
  s1030     1030 spheres: the sweep's 1024-record LDS chunk and a ragged tail of 6 records + 2 pads
  nan200    golden spheres200 plus one sphere with a NaN radius: no sphere tree, cmax NaN, every record -1e30, every ray pass-all
  mixed3    s6's spheres (a tree) and three qualified (x, y) triangles, which stay outside it: the filter is their only f32 stage
(s5 -- an odd sphere count: the last pair holds a sphere and a sentinel -- and s6_big / s6_tiny with the medge regime, both sides of
filter_from_ray's two range gates, are bounds_cases' own.)

Tangents from the centre (centre_tangents()): origins within 1e-3 ... 1e-1 of the scene's scale of the centre the records are relative
to (cmax, that is), where M = cmax + |p| and with it E are as small as a ray can make them -- the rays that see a cmax left too small.

Limb cameras (limb_cameras(), limb_objects()): for about twenty targets per scene and the inside, edge, outside and far10 distances a
camera whose 32 x 32 frame has the target's silhouette across it, neighbouring pixel rays one f32 ulp of the scene's scale apart at
the tangent point, no lens jitter, every object its own dyadic emission and base colour 0.  A view is kept when the text says that no
other shape stands in it and that its own limb runs through the frame (far away the text's f64 roundings move the limb by more than
the frame is wide).

Adversarial families (adversarial_spheres(), adversarial_triangles()): a seeded random search IN THE MODEL for the rays that make the
filters' own roundings large, N_SEARCH candidates per scene, the worst KEEP kept.
  spheres -- the target is drawn half from the eight spheres with the largest |c - centre| (|c - centre| ~ cmax) and half from all;
      the direction has three components of similar size, or one dominant component (the others 1e-3 ... 1e-1), or is generic; the
      ray is a tangent passing the centre at r + delta, delta from bounds_cases.DELTAS and its secants; the origin lies on the FAR
      side of the scene's centre (the sphere is met after the centre is passed) with |p| of 1, 3, 10 and 1000 cmax.  Radii from cmax
      down to 1e-6 cmax come with the scenes (s6 ... cloud and dust).
      objective: |D (f64 on the f64 inputs) - D_f32 computed with E = 0| / (u M^2), and, among the rays whose f64 D is >= 0, the
      share of E the f32 value needs.
  triangles -- the target is drawn half from the eight records that reach tri_extent; the ray goes through a point delta outside /
      inside an edge or vertex, |n . d| near 1 (within 1e-3 ... 1e-7) or near 4 e_dn = 32u, from |p| of 1, 3, 10 and 1000 tri_extent.
      objective: the share of A the candidate test needs.
"""
import functools

import numpy as np

import bounds_cases as bc
import bounds_model as bm

N_SEARCH = 100000
KEEP = 300
U = 2.0 ** -24
NEW_SCENES = ("s4t4", "s1030", "nan200", "mixed3")
SPHERE_SCENES = ("s5", "s6", "spheres200", "cloud", "dust", "mixed", "s4t4", "mixed3")
TRI_SCENES = ("tris300", "planes_mesh", "mixed", "s4t4", "mixed3")


def _xy_triangles(rng, n, span):
    """n generic triangles, solved in (x, y), facing the origin's side (n . v0 >= 0: a front-facing ray passes the cull)"""
    out = []
    while len(out) < n:
        v = rng.uniform(-span, span, 3) + rng.uniform(-1.0, 1.0, (3, 3))
        if np.dot(np.cross(v[1] - v[0], v[2] - v[0]), v[0]) < 0.0:
            v = v[[0, 2, 1]]
        out.append(v)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _scenes(dtype_key):
    import rust_raytracing_amd as rtx
    dtype = rtx.OBJECT_DTYPE
    base = dict(bc.scenes(dtype))
    rng = np.random.default_rng(20250611)
    out = dict(base)
    s6 = base["s6"]
    out["s4t4"] = np.concatenate([s6[:4], bc._tri_objs(dtype, _xy_triangles(rng, 4, 3.0))])
    out["s1030"] = bc._sphere_objs(dtype, rng.uniform(-20.0, 20.0, (1030, 3)), rng.uniform(0.2, 0.6, 1030))
    nan = bc._sphere_objs(dtype, np.array([[1.0, 2.0, 3.0]]), np.array([np.nan]))
    out["nan200"] = np.concatenate([base["spheres200"], nan])
    out["mixed3"] = np.concatenate([s6, bc._tri_objs(dtype, _xy_triangles(rng, 3, 3.0))])
    return out


def scenes(dtype=None):
    """{name: objects}: bounds_cases' scenes and the four of the module docstring"""
    return _scenes("objects")


def regimes_of(name):
    return bc.regimes_of(name)


@functools.lru_cache(maxsize=None)
def _case(name, regime):
    if name not in NEW_SCENES:
        return bc.case(name, regime)
    objs = scenes()[name]
    rays = bc.aimed(name, objs, regime, None)               # (no pack: every sphere and triangle is a target)
    o, d, target, sign, what, extra = rays["o"], rays["d"], rays["target"], rays["sign"], rays["what"], rays["extra"]
    has = extra >= 0
    o = np.concatenate([o, o[has]]); d = np.concatenate([d, d[has]])
    target = np.concatenate([target, extra[has]])
    aimed_mask = np.concatenate([np.ones(len(sign), dtype=bool), np.zeros(int(has.sum()), dtype=bool)])
    sign = np.concatenate([sign, np.zeros(int(has.sum()))]); what = np.concatenate([what, np.full(int(has.sum()), 4)])
    t, rep, some = bc.text_distances(objs, o, d, target)
    return {"name": name, "regime": regime, "objs": objs, "o": o, "d": d, "target": target, "sign": sign, "what": what,
            "aimed": aimed_mask, "t": t, "reported": rep, "some": some}


@functools.lru_cache(maxsize=None)
def case(name, regime, stride=1):
    """one scene x origin regime as bounds_cases.case() gives it: o, d, target, sign, what, aimed, t, reported"""
    cs = _case(name, regime)
    if stride <= 1:
        return cs
    n = len(cs["t"])
    sel = np.sort(np.random.default_rng(5).choice(n, max(1, n // int(stride)), replace=False))
    return {k: (v[sel] if isinstance(v, np.ndarray) and k != "objs" and len(v) == n else v) for k, v in cs.items()}


def centre_tangents(label, objs, centre, cap=3000):
    """Tangents FROM the centre the records are relative to (|p| of 1e-3 ... 1e-1 of cmax, so M = cmax + |p| is as small
    as a ray can make it and E = 64uM^2 with it): the place where a cmax that is too small shows first.  Every sphere, the deltas and
    secants of bounds_cases, a seeded side of the sphere.  -> a case (o, d, target, t, reported)"""
    rng = np.random.default_rng(sum(map(ord, label)) * 6151)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    sph = np.nonzero(np.asarray(objs["kind"]) == 0)[0]
    scale = bc._scale_of(objs)
    reach = float(np.max(np.linalg.norm(geom[sph, :3] - np.asarray(centre), axis=1) + np.abs(geom[sph, 3])))      # (cmax, of finite spheres)
    O, D, T = [], [], []
    for j in np.tile(sph, max(1, min(8, cap // (len(sph) * bc.NPER)))):
        c, r = geom[j, :3], abs(geom[j, 3])
        dv, _ = bc._delta_values(scale, r)
        for dl in dv:
            o = np.asarray(centre) + bc._unit(rng.normal(size=3)) * reach * 10.0 ** rng.uniform(-3.0, -1.0)
            v = c - o
            dist = np.linalg.norm(v)
            if not dist > r + dl > 0.0:
                continue
            vh = v / dist
            ph = rng.normal(size=3); ph = bc._unit(ph - np.dot(ph, vh) * vh)
            sa = (r + dl) / dist
            O.append(o); D.append(np.sqrt(1.0 - sa * sa) * vh + sa * ph); T.append(j)
    O, D, T = np.array(O).reshape(-1, 3), np.array(D).reshape(-1, 3), np.array(T, dtype=np.int64)
    if len(T) > cap:
        keep = np.sort(rng.choice(len(T), cap, replace=False))
        O, D, T = O[keep], D[keep], T[keep]
    t, rep, some = bc.text_distances(objs, O, D, T)
    return {"name": label, "regime": "centre", "objs": objs, "o": O, "d": D, "target": T, "t": t, "reported": rep, "some": some}


@functools.lru_cache(maxsize=None)
def centre_case(name):
    objs, centre, _, _, _ = geometry(name)
    return centre_tangents(name, objs, centre)


def stride_of(name, regime):
    """the CPU part looks at about 1000 pairs per cell (a seeded random share), as tests/test_walk_bounds.py does"""
    n = {"spheres200": 20000, "tris300": 20000, "nan200": 20000, "s1030": 20000}.get(name, 6000) * (2 if regime == "surface" else 1)
    return max(1, n // 1000)


def geometry(name):
    """(objs, centre, cmax, tri_extent, pack) of a scene as the upload derives them (bounds_model.pack)"""
    objs = scenes()[name]
    pk = bm.pack_for(objs)
    return objs, pk["centre"], pk["cmax"], pk["tri_extent"], pk


# ---- limb cameras --------------------------------------------------------------------------------------------------------------------------
LIMB_SIZE = 32
LIMB_REGIMES = ("inside", "edge", "outside", "far10")


def limb_objects(name):
    """the scene with every object's emission a distinct dyadic value (k + 1) / 4096 and base colour 0: a path ends at its first hit,
    and the pixel's value names the object"""
    objs = scenes()[name].copy()
    objs["base_color"] = 0.0
    objs["emission_color"] = ((np.arange(len(objs)) + 1.0) / 4096.0)[:, None]
    objs["roughness"] = 1.0
    return objs


def limb_emission(k):
    return (k + 1.0) / 4096.0


@functools.lru_cache(maxsize=None)
def limb_cameras(name, n_targets=20):
    """[(position, direction, fov, target, regime)]: for n_targets spheres / triangles of the scene (seeded) and each distance of
    LIMB_REGIMES a camera that looks ALONG the target's silhouette -- at a sphere's tangent point, along a tangent; at a triangle's
    edge midpoint, from the front -- so that the limb runs through the middle of a LIMB_SIZE^2 frame; the field of view makes
    neighbouring pixel rays pass the tangent point one f32 ulp of the scene's scale apart (no lens jitter: focal_offset =
    non_focal_offset = 0, 1 spp).  The finite spheres and the qualified triangles are the targets."""
    objs = scenes()[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 3571)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    kind = np.asarray(objs["kind"]).astype(int)
    fin = np.isfinite(geom[:, :4]).all(axis=1)
    ids = np.nonzero(((kind == 0) & fin) | (kind == 2))[0]
    ids = ids[np.sort(rng.choice(len(ids), min(n_targets, len(ids)), replace=False))]
    ok = objs[((kind == 0) & fin) | (kind != 0)]
    scale = bc._scale_of(ok)
    limit, extent = 4.0 * scale + 1.0, 2.0 * scale
    ulp = float(np.spacing(np.float32(scale)))
    everyone = np.arange(len(objs))

    def first_hit(o, d):
        t, rep, _ = bc.text_distances(objs, np.tile(o, (len(objs), 1)), np.tile(d, (len(objs), 1)), everyone)
        return int(np.argmin(np.where(rep, t, np.inf))) if rep.any() else -1

    cams = []
    for j in ids:
        for regime in LIMB_REGIMES:
            for attempt in range(40):                       # a view of the limb that no other shape stands in (the text decides)
                if kind[j] == 0:
                    c, r = geom[j, :3], abs(geom[j, 3])
                    d = bc._unit(rng.normal(size=3))
                    w = _perp(rng, d[None, :])[0]
                    Q, inward = c + r * w, -0.1 * r * w
                else:
                    v = geom[j, :9].reshape(3, 3)
                    nrm = bc._unit(np.cross(v[1] - v[0], v[2] - v[0]))
                    if np.dot(nrm, v[0]) < 0.0:
                        nrm = -nrm
                    Q = 0.5 * (v[0] + v[1])
                    inward = 0.1 * (v[2] - Q)
                    d = bc._unit(-nrm + 0.5 * rng.normal(size=3))
                P = bc._place(Q[None, :], d[None, :], regime, limit, extent, rng)[0]
                if first_hit(P + inward, d) != j:
                    continue
                # ... and across which the TEXT's own limb runs: far away its f64 roundings move the limb by more than the frame is
                # wide, so nine rays across the frame are asked, and a third to two thirds of them must report the target
                across = np.linspace(-14.0, 14.0, 9)[:, None] * ulp * bc._unit(inward)[None, :]
                dirs = bc._unit(Q[None, :] + across - P[None, :])
                seen = int(bc.text_distances(objs, np.tile(P, (9, 1)), dirs, np.full(9, j))[1].sum())
                if 3 <= seen <= 6:
                    break
            else:
                continue
            L = float(np.linalg.norm(Q - P))
            cams.append((tuple(P), tuple(d), LIMB_SIZE * ulp / L, int(j), regime))
    return cams


# ---- the adversarial search ------------------------------------------------------------------------------------------------------------------
def _perp(rng, d):
    w = rng.normal(size=d.shape)
    w -= np.sum(w * d, axis=1, keepdims=True) * d
    return bc._unit(w)


def _search_dirs(rng, n):
    """a third each: three components of similar size, one dominant component, generic"""
    kind = np.arange(n) % 3
    sim = bc._unit(rng.choice([-1.0, 1.0], (n, 3)) * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, (n, 3))))
    dom = 10.0 ** rng.uniform(-3.0, -1.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    dom[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    gen = rng.normal(size=(n, 3))
    d = np.where((kind == 0)[:, None], sim, np.where((kind == 1)[:, None], bc._unit(dom), bc._unit(gen)))
    return d


def disc_f64(objs, target, o, d):
    """D = ((c - o) . d)^2 - (|c - o|^2 - r^2) of the f64 inputs in f64, centred on the sphere (well conditioned: the search's ruler;
    the reported figures are re-made exactly by exact_disc)"""
    g = np.asarray(objs["geom"], dtype=np.float64)[target]
    v = g[:, :3] - o
    b = np.sum(v * d, axis=1)
    l = v - b[:, None] * d
    return g[:, 3] * g[:, 3] - np.sum(l * l, axis=1)


def exact_disc(c, r, o, d):
    """the same D of ONE pair in exact rational arithmetic on the f64 inputs (fractions.Fraction) -> float"""
    from fractions import Fraction as Fr
    c, o, d = [[Fr(float(x)) for x in v] for v in (c, o, d)]
    v = [a - b for a, b in zip(c, o)]
    b = sum(x * y for x, y in zip(v, d))
    return float(b * b - (sum(x * x for x in v) - Fr(float(r)) ** 2))


def exact_disc32(rec, f):
    """D of filter_disc1's expression on ONE record and one FilterParams (f32 operands) in exact rational arithmetic -> float"""
    from fractions import Fraction as Fr
    x, y, z, w = [Fr(float(v)) for v in rec]
    p = [Fr(float(v)) for v in f]
    b = x * p[0] + y * p[1] + z * p[2] + p[3]
    return float(b * b + (x * p[4] + y * p[5] + z * p[6] + p[7] - w))


@functools.lru_cache(maxsize=None)
def adversarial_spheres(name, n=N_SEARCH):
    """-> dict o, d, target (KEEP worst by evaluation error, then KEEP worst by share of E among the probable hits), err (the error in
    u M^2 of every kept ray, f64 ruler), and `searched`"""
    objs, centre, cmax, _, pk = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + 1)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    sph = np.nonzero(np.asarray(objs["kind"]) == 0)[0]
    far = sph[np.argsort(-np.linalg.norm(geom[sph, :3] - centre, axis=1))[:8]]
    tg = np.where(np.arange(n) % 2 == 0, far[rng.integers(0, len(far), n)], sph[rng.integers(0, len(sph), n)])
    c, r = geom[tg, :3], np.abs(geom[tg, 3])
    d = _search_dirs(rng, n)
    d = np.where((np.sum((c - centre) * d, axis=1) < 0.0)[:, None], -d, d)          # the sphere lies beyond the centre
    scale = bc._scale_of(objs)
    dv = np.stack([bc._delta_values(scale, ri)[0] for ri in np.unique(r)])          # (per distinct radius: its secants)
    row = np.searchsorted(np.unique(r), r)
    delta = dv[row, rng.integers(0, dv.shape[1], n)]
    Q = c + (r + delta)[:, None] * _perp(rng, d)
    f = np.array([1.0, 3.0, 10.0, 1000.0])[rng.integers(0, 4, n)]
    L = f * cmax + np.sum((Q - centre) * d, axis=1)
    o = Q - d * L[:, None]
    words, off, M = bm.sweep_params(o, d, centre, cmax, bm.WEAKENED["E"])
    rec = bm.sweep_record(objs, centre)[np.searchsorted(sph, tg)]
    D0 = bm.sweep_disc(rec, words).astype(np.float64)
    D = disc_f64(objs, tg, o, d)
    with np.errstate(all="ignore"):
        err = np.where(off, 0.0, np.abs(D - D0) / (U * M * M))
        need = np.where(off | (D < 0.0), -np.inf, -D0 / (U * M * M))
    keep = np.unique(np.concatenate([np.argsort(-err)[:KEEP], np.argsort(-need)[:KEEP]]))
    return {"o": o[keep], "d": d[keep], "target": tg[keep], "err": err[keep], "searched": n}


@functools.lru_cache(maxsize=None)
def adversarial_triangles(name, n=N_SEARCH):
    """-> dict o, d, target: the KEEP rays with the largest share of A among those the footprint rectangle should pass"""
    objs, centre, _, tri_extent, pk = geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + 2)
    geom = np.asarray(objs["geom"], dtype=np.float64)
    tri = np.nonzero((pk["free"] == 2))[0]                                          # (x, y) records: the ones with a real rectangle
    if not len(tri):
        return {"o": np.zeros((0, 3)), "d": np.zeros((0, 3)), "target": np.zeros(0, dtype=np.int64), "searched": 0}
    reach = np.abs(geom[tri, :9].reshape(-1, 3, 3) - centre).max(axis=(1, 2))
    far = tri[np.argsort(-reach)[:8]]
    tg = np.where(np.arange(n) % 2 == 0, far[rng.integers(0, len(far), n)], tri[rng.integers(0, len(tri), n)])
    v = geom[tg, :9].reshape(n, 3, 3)
    cen = v.mean(axis=1)
    nrm = bc._unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    k = rng.integers(0, 6, n)
    pts = np.stack([v[:, 0], v[:, 1], v[:, 2], 0.5 * (v[:, 0] + v[:, 1]), 0.5 * (v[:, 1] + v[:, 2]), 0.5 * (v[:, 0] + v[:, 2])], axis=1)[np.arange(n), k]
    size = np.linalg.norm(v - cen[:, None, :], axis=2).max(axis=1)
    scale = bc._scale_of(objs)
    dv = bc._delta_values(scale, 1.0)[0]
    pick = rng.integers(0, len(dv), n)
    delta = np.where(pick >= len(bc.DELTAS), dv[pick] * size, dv[pick])
    P = pts + delta[:, None] * bc._unit(pts - cen)
    t1 = bc._unit(v[:, 1] - v[:, 0])
    near1 = np.arange(n) % 2 == 0
    s = np.where(near1, 1.0 - 10.0 ** rng.uniform(-7.0, -3.0, n), 32.0 * U * rng.choice([0.5, 1.0 - 2.0 ** -20, 1.0, 1.0 + 2.0 ** -20, 2.0], n))
    s = -s * np.where(np.sum(nrm * v[:, 0], axis=1) >= 0.0, 1.0, -1.0)              # from the front: the cull passes
    d = s[:, None] * nrm + np.sqrt(1.0 - s * s)[:, None] * t1
    f = np.array([1.0, 3.0, 10.0, 1000.0])[rng.integers(0, 4, n)]
    o = P - d * (f * max(tri_extent, 1.0))[:, None]
    rec = pk["rec"][tg]
    tp = bm.tri_params(o, d, centre, tri_extent, bm.WEAKENED["A"])
    sx, sy = bm.tri_filter_sxy(rec[:, 0:4], rec[:, 4:8], tp)
    A = bm.tri_params(o, d, centre, tri_extent)["A"].astype(np.float64)
    with np.errstate(all="ignore"):
        share = np.maximum(-sx.astype(np.float64), -sy.astype(np.float64)) / A
    share = np.where(delta <= 0.0, share, -np.inf)                                 # aimed inside or on the edge: should pass
    keep = np.argsort(-share)[:KEEP]
    return {"o": o[keep], "d": d[keep], "target": tg[keep], "searched": n}


@functools.lru_cache(maxsize=None)
def adversarial_case(name, what):
    """the kept rays of one search with the text's answers, in case()'s layout"""
    rays = (adversarial_spheres if what == "spheres" else adversarial_triangles)(name)
    objs = scenes()[name]
    t, rep, some = bc.text_distances(objs, rays["o"], rays["d"], rays["target"])
    n = len(t)
    return {"name": name, "regime": "adversarial " + what, "objs": objs, "o": rays["o"], "d": rays["d"], "target": rays["target"],
            "sign": np.zeros(n), "what": np.full(n, 6), "aimed": np.ones(n, dtype=bool), "t": t, "reported": rep, "some": some}
