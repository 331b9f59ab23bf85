"""Scenes whose rendered values follow from the TEXT of the reference alone -- no oracle, no RNG stream involved -- so
that the device path and the CPU oracle are each pinned against the reference independently of one another (VERDICT r02:
every RNG-dependent check went through oracle/rtx_oracle.c, written by the author of the kernels).

Each builder returns (objects, camera, config kwargs, width, height, expected) where `expected` is the exact f64 value of
every channel of every pixel, or a per-pixel array."""
import math

import numpy as np


def _obj(dtype, n):
    return np.zeros(n, dtype=dtype)


def closed_box(dtype, n_spheres=0, seed=5):
    """Six inward one-sided planes (plane.rs:25: a plane is hit only from the side its normal points to) around the camera,
    optionally with spheres inside; EVERY object: emission 1, base colour 1/2, roughness 1.  The ray can never leave, every
    iteration of render_ray's loop hits something, and ray_hit adds light * 1 BEFORE it halves light (scene.rs:276-277), so
    every sample is sum_{k=0}^{max_bounces} 2^-k exactly, whatever the seed, the directions drawn or the object hit; the
    loop runs max_bounces + 1 times (scene.rs:227).  A sphere is never re-hit from its own surface (near root negative,
    sphere.rs:29 + the is_sign_positive filter scene.rs:249), a plane never from a point on it (plane.rs:25)."""
    o = _obj(dtype, 6 + n_spheres)
    h = 9.0
    walls = [((h, 0, 0), (-1, 0, 0)), ((-h, 0, 0), (1, 0, 0)), ((0, h, 0), (0, -1, 0)), ((0, -h, 0), (0, 1, 0)),
             ((0, 0, h), (0, 0, -1)), ((0, 0, -h), (0, 0, 1))]
    for k, (p, n) in enumerate(walls):
        o[k]["kind"] = 1
        o[k]["geom"][:6] = (*p, *n)
    if n_spheres:
        rng = np.random.default_rng(seed)
        c = rng.uniform(-7.0, 7.0, (n_spheres, 3))
        c[:, 0] = np.abs(c[:, 0]) + 1.5                       # in front of the camera, which stays outside every sphere
        o["kind"][6:] = 0
        o["geom"][6:, :3] = c
        o["geom"][6:, 3] = rng.uniform(0.1, 0.6, n_spheres)
    o["emission_color"] = 1.0
    o["base_color"] = 0.5
    o["roughness"] = 1.0
    return o


def closed_box_value(max_bounces):
    return sum(2.0 ** -k for k in range(max_bounces + 1))       # 1.9990234375 for the default 10, 1.875 for 3


def inside_a_sphere(dtype):
    """The camera inside a sphere sees nothing of it: Sphere::distance returns the NEAR root (sphere.rs:29), negative from
    inside, and closest_object drops non-positive distances (scene.rs:249) -> render_ray returns resulting_color = 0 (black),
    however bright the sphere.  Five more spheres behind the camera (never in view) give the tree kernels a tree."""
    o = _obj(dtype, 6)
    o["kind"] = 0
    o[0]["geom"][:4] = (0.5, 0.2, -0.1, 3.0)
    for k in range(1, 6):
        o[k]["geom"][:4] = (-10.0 - 3.0 * k, 2.0 * k - 6.0, 1.0, 1.0)
    o["emission_color"] = 4.0
    o["base_color"] = 0.5
    o["roughness"] = 1.0
    return o


TRI = (5.0, -1.0, -1.0, 5.0, 1.0, -1.0, 5.0, 0.0, 1.0)           # the plane x = 5, seen from the origin
TRI_EMIT, SPH_EMIT = (0.25, 0.5, 0.75), (2.0, 0.125, 1.0)


def triangle_distance_bracket(dtype, direction, distance, delta):
    """Triangle::distance takes |t| of the plane distance and `contains` solves two rows only (triangle.rs:108-127, :37-101):
    from the origin the triangle TRI is reported at 5.0 along +x, at 5.0 along -x (a phantom hit BEHIND the ray) and at
    5.007244751357777 along norm(-1, 0.05, 0.02) (phantom).  The device path exposes no distances, so the value is pinned
    through closest_object's ordering (scene.rs:250): a sphere whose near root is `distance + delta` along the same ray wins
    for delta < 0 and loses for delta > 0.  One pixel, no jitter, a 1e-12 rad field of view: the pixel is the winner's
    emission exactly (0 + 1 * e, base colour 0 ends the path).  Filler shapes far off the ray give the tree kernels trees."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / math.sqrt(float(d @ d))
    o = _obj(dtype, 2 + 6 + 6)
    o[0]["kind"] = 2
    o[0]["geom"] = TRI
    o[0]["emission_color"] = TRI_EMIT
    r = 1.0
    o[1]["kind"] = 0
    o[1]["geom"][:3] = d * (distance + delta + r)               # near root = |c| - r = distance + delta (to ~1e-15)
    o[1]["geom"][3] = r
    o[1]["emission_color"] = SPH_EMIT
    for k in range(6):                                           # filler spheres: beside the ray, never on it
        o[2 + k]["kind"] = 0
        o[2 + k]["geom"][:4] = (3.0 * k - 7.0, 40.0 + k, 25.0, 1.0)
        o[2 + k]["emission_color"] = (9.0, 9.0, 9.0)
    for k in range(6):                                           # filler triangles: tiny, far away in y (no phantom hit on this ray)
        o[8 + k]["kind"] = 2
        base = np.array([2.0 + k, 900.0 + 3.0 * k, 0.3 * k])
        o[8 + k]["geom"] = np.concatenate([base, base + (0.5, 0.1, 0.0), base + (0.1, 0.6, 0.2)])
        o[8 + k]["emission_color"] = (7.0, 7.0, 7.0)
    o["base_color"] = 0.0
    o["roughness"] = 1.0
    cam = ((0.0, 0.0, 0.0), tuple(d), 1e-12)
    cfg = dict(rays_per_pixel=3, focal_offset=0.0, non_focal_offset=0.0, seed=1)
    expected = SPH_EMIT if delta < 0 else TRI_EMIT
    return o, cam, cfg, expected


TRIANGLE_CASES = [((1.0, 0.0, 0.0), 5.0), ((-1.0, 0.0, 0.0), 5.0), ((-1.0, 0.05, 0.02), 5.007244751357777)]


# ---- the bounce direction (scene.rs:279-292, vector.rs:36-45), pinned without the oracle ------------------------------------
# The scenes above are direction-independent by construction.  These two are not: a wrong reflection formula, blend weight,
# hemisphere flip or direction distribution changes their pixels.
MIRROR_BASE, MIRROR_EMIT, LIGHT_EMIT = (0.5, 0.25, 0.75), (0.125, 0.0, 0.25), (4.0, 2.0, 1.0)


def _norm(v):
    v = np.asarray(v, dtype=np.float64)
    return v / math.sqrt(float(v @ v))


def _fillers(dtype, centre, below):
    """Six black spheres and six black triangles that no path of these scenes can reach before it ends -- `below` a floor, or far
    behind everything -- so that the tree kernels get their trees.  (A phantom triangle hit, triangle.rs:118, would add 0 like the
    miss it replaces: base colour and emission are 0.)"""
    o = _obj(dtype, 12)
    c = np.asarray(centre, dtype=np.float64)
    for k in range(6):
        o[k]["kind"] = 0
        o[k]["geom"][:4] = (*(c + np.asarray(below) * (40.0 + 3.0 * k) + (2.0 * k, 0.0, 0.0)), 1.0)
        o[6 + k]["kind"] = 2
        base = c + np.asarray(below) * 50.0 + (0.3 * k, 900.0 + 3.0 * k, 0.0)
        o[6 + k]["geom"] = np.concatenate([base, base + (0.5, 0.1, 0.0), base + (0.1, 0.6, 0.0)])
    o["roughness"] = 1.0
    return o


def mirror_cases(dtype):
    """ROUGHNESS 0: random_bounce_dir returns norm(w + (refl - w) * 1) = the mirror direction refl = d - (n * 2) * (d . n) up to
    rounding, whatever w was drawn (scene.rs:281-285), flipped to the normal's side when refl . n <= 0 (scene.rs:287-291).  One
    pixel, no jitter, a 1e-12 rad field of view: the primary ray leaves the origin along +x, hits the mirror (base MIRROR_BASE,
    emission MIRROR_EMIT) at P, and the bounced ray either meets a light sphere (emission LIGHT_EMIT, base 0, radius 1) centred
    10 units along the expected direction -- pixel = MIRROR_EMIT + MIRROR_BASE * LIGHT_EMIT exactly (dyadic values; the light's
    base colour 0 ends the path, scene.rs:228) -- or, with the light displaced by 2.5 > its radius, nothing: pixel = MIRROR_EMIT.
    Mirrors: an axis-aligned plane, a plane with an oblique un-normalised normal (object.rs:37-39 normalises it), a sphere
    (normal = norm(P - c)), and a triangle seen from BEHIND (its normal is never turned towards the ray, triangle.rs:29: refl
    points behind it and the flip sends the ray on through it -- along +x again for this incidence).
    Yields (name, objects, camera, config kwargs, expected rgb)."""
    d = np.array([1.0, 0.0, 0.0])
    cases = []
    # (name, mirror kind, geom, hit point P, unit normal as the reference computes it, direction the fillers hide in)
    cases.append(("plane x=4 facing the camera", 1, (4.0, 0.0, 0.0, -1.0, 0.0, 0.0), (4.0, 0.0, 0.0), (-1.0, 0.0, 0.0), None))
    cases.append(("oblique plane, normal (-3, 0, 1.5)", 1, (4.0, 0.0, 0.0, -3.0, 0.0, 1.5), (4.0, 0.0, 0.0), _norm((-3.0, 0.0, 1.5)), None))
    cases.append(("oblique plane, normal (-1, 2, 0.5) through (6, 1, 1)", 1, (6.0, 1.0, 1.0, -1.0, 2.0, 0.5), None, _norm((-1.0, 2.0, 0.5)), None))
    cases.append(("sphere (5, 0.6, 0) r 1", 0, (5.0, 0.6, 0.0, 1.0), (4.2, 0.0, 0.0), (-0.8, -0.6, 0.0), None))
    cases.append(("triangle in x = 5 seen from behind", 2, TRI, (5.0, 0.0, 0.0), (1.0, 0.0, 0.0), None))
    out = []
    for name, kind, geom, P, n, _ in cases:
        n = np.asarray(n, dtype=np.float64)
        if P is None:                                            # plane through `pos`: the point of the x-axis on it
            pos, nn = np.asarray(geom[:3]), np.asarray(geom[3:6])
            P = (float(pos @ nn) / nn[0], 0.0, 0.0)
        P = np.asarray(P, dtype=np.float64)
        refl = d - (n * 2.0) * float(d @ n)                      # scene.rs:281
        f = _norm(refl)
        if not float(f @ n) > 0.0:                               # scene.rs:287-291
            f = -f
        side = _norm(np.cross(f, (0.0, 0.3, 1.0)))               # a direction perpendicular to the bounced ray
        for displaced in (False, True):
            o = _obj(dtype, 2)
            o[0]["kind"] = kind
            o[0]["geom"][:len(geom)] = geom
            o[0]["base_color"], o[0]["emission_color"], o[0]["roughness"] = MIRROR_BASE, MIRROR_EMIT, 0.0
            o[1]["kind"] = 0
            o[1]["geom"][:3] = P + f * 10.0 + (side * 2.5 if displaced else 0.0)
            o[1]["geom"][3] = 1.0
            o[1]["base_color"], o[1]["emission_color"], o[1]["roughness"] = 0.0, LIGHT_EMIT, 1.0
            # fillers behind the camera, off the x-axis and away from every bounced ray of these cases
            fill = _fillers(dtype, (-60.0, 35.0, 20.0), (-1.0, 0.0, 0.0))
            objs = np.concatenate([o, fill])
            want = tuple(m + (0.0 if displaced else b * e) for m, b, e in zip(MIRROR_EMIT, MIRROR_BASE, LIGHT_EMIT))
            cfg = dict(rays_per_pixel=3, focal_offset=0.0, non_focal_offset=0.0, seed=5)
            out.append((name + (" (light displaced)" if displaced else ""), objs, ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1e-12), cfg, want))
    return out


HEMI_BASE, HEMI_EMIT, HEMI_R, HEMI_D = 0.5, 4.0, 3.0, 5.0


def hemisphere_light(dtype):
    """ROUGHNESS 1: random_bounce_dir returns norm(w + (refl - w) * 0) = w, the direction Vector3::random_direction drew --
    z = 2u - 1, theta = 2 pi u', (sqrt(1 - z^2) cos, sqrt(1 - z^2) sin, z): uniform on the sphere (vector.rs:36-45) -- flipped to the
    normal's side: uniform on the hemisphere.  A floor plane z = -1 (base HEMI_BASE, emission 0, roughness 1) under a light
    sphere (emission HEMI_EMIT, base 0) of radius HEMI_R whose centre is HEMI_D above the point P the primary rays hit; fillers
    hide below the floor.  A bounced ray meets the light iff it lies in the cone of half angle asin(r / d) about the normal:
    probability 1 - sqrt(1 - (r/d)^2) (the cap's share of the hemisphere's solid angle) = 0.2 for r/d = 0.6; each sample is
    HEMI_BASE * HEMI_EMIT = 2 with that probability and 0 otherwise (the light's base colour 0 ends the path; a ray that misses
    leaves the scene).  A cosine-weighted hemisphere would give (r/d)^2 = 0.36, a sphere without the flip 0.1.
    Returns (objects, camera, config kwargs without seed / rays_per_pixel, p, sample value)."""
    d = _norm((1.0, 0.0, -1.0))
    P = np.array([1.0, 0.0, -1.0])
    o = _obj(dtype, 2)
    o[0]["kind"] = 1
    o[0]["geom"][:6] = (0.0, 0.0, -1.0, 0.0, 0.0, 1.0)
    o[0]["base_color"], o[0]["roughness"] = HEMI_BASE, 1.0
    o[1]["kind"] = 0
    o[1]["geom"][:4] = (P[0], P[1], P[2] + HEMI_D, HEMI_R)
    o[1]["emission_color"], o[1]["roughness"] = HEMI_EMIT, 1.0
    fill = _fillers(dtype, (0.0, 0.0, -1.0), (0.0, 0.0, -1.0))
    p = 1.0 - math.sqrt(1.0 - (HEMI_R / HEMI_D) ** 2)
    cam = ((0.0, 0.0, 0.0), tuple(d), 1e-12)
    return np.concatenate([o, fill]), cam, dict(focal_offset=0.0, non_focal_offset=0.0), p, HEMI_BASE * HEMI_EMIT


def hemisphere_check(mean, n_samples, p, value, sigmas=5.0):
    """(|mean - mu|, bound): the grand mean of n_samples Bernoulli(p) * value samples lies within sigmas * sigma / sqrt(N) of
    mu = p * value (5 sigma: a false alarm once in 1.7e6 runs; the alternatives named above are > 100 sigma away)."""
    mu = p * value
    bound = sigmas * value * math.sqrt(p * (1.0 - p) / n_samples)
    return abs(mean - mu), bound


# ---- the first part of Scene::render (scene.rs:144-170, :194-222; camera.rs:42-49), pinned without the oracle ------------------
# Every scene above is a 1 x 1 image with a 1e-12 rad field of view and no jitter.  The scenes below are not: a half-pixel shift
# of the pixel -> angle map, vfov = fov, a flipped row order, another camera basis, a centred or halved lens jitter or one draw
# serving both offsets changes their pixels.
MARK_DISTANCE, MARK_SHARE, MARK_MARGIN = 50.0, 0.3, 2.0
PIXEL_MAP_CAMERAS = [("default", ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), math.pi / 2)),
                     ("z in the direction", ((0.0, 0.0, 0.0), (1.0, 0.2, 0.5), 1.2)),               # |right| = 0.90
                     ("off the origin, looking down", ((0.3, -0.2, 0.1), (0.6, -0.3, -0.7), 0.9))]  # |right| = 0.69
PIXEL_MAP_FRAMES = [(24, 10), (17, 16), (9, 20)]                 # non-square, partial 8 x 8 tiles, h > w (vfov > fov)
PIXEL_MAP_BIG = 1024                                             # 2^20 primary rays: AUTO runs two stages and builds tile lists


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])     # vector.rs:89-95


def camera_basis(direction):
    """Camera::derive_to_world_space_mat (camera.rs:42-49), in the reference's operation order: cam_forward = direction.norm()
    (vector.rs:101-107: self / sqrt(x x + y y + z z)), cam_right = cam_forward x (0, 0, -1) and cam_up = cam_forward x cam_right,
    NEITHER normalised: |right| = |up| = sqrt(1 - forward.z^2).  The matrix' columns are (right, up, forward), so a camera-space
    vector (a, b, c) becomes right * a + up * b + forward * c (mat/mul.rs:42-50 sums in that order)."""
    x, y, z = (float(c) for c in direction)
    n = math.sqrt(x * x + y * y + z * z)
    fwd = (x / n, y / n, z / n)
    right = _cross(fwd, (0.0, 0.0, -1.0))
    up = _cross(fwd, right)
    return np.array(right), np.array(up), np.array(fwd)


def pixel_ray(cam, w, h, x, y):
    """The un-normalised direction Scene::render gives pixel (x, y) of a w x h frame: u = x / w, v = y / h -- the pixel's CORNER,
    not its centre (scene.rs:153,157) --, vertical_fov = h / w * fov (scene.rs:145), angle_x = fov * (u - 0.5), angle_y =
    vertical_fov * (v - 0.5), camera-space (sin angle_x, sin angle_y, cos angle_x * cos angle_y) rotated to world space
    (scene.rs:213-221).  x and y may lie outside the frame (a pixel's neighbours)."""
    _, _, fov = cam
    right, up, fwd = camera_basis(cam[1])
    ax = fov * (x / w - 0.5)
    ay = (h / w * fov) * (y / h - 0.5)
    return right * math.sin(ax) + up * math.sin(ay) + fwd * (math.cos(ax) * math.cos(ay))


def _all_pixel_rays(cam, w, h):
    """[h][w] unit ray directions of the whole frame (the same formulas, vectorised: for the margin checks only)."""
    _, _, fov = cam
    right, up, fwd = camera_basis(cam[1])
    ax = fov * (np.arange(w) / w - 0.5)
    ay = (h / w * fov) * (np.arange(h) / h - 0.5)
    D = (right * np.sin(ax)[None, :, None] + up * np.sin(ay)[:, None, None]
         + fwd * (np.cos(ax)[None, :, None] * np.cos(ay)[:, None, None]))
    return D / np.sqrt((D * D).sum(axis=2))[:, :, None]


def _angle(a, b):
    """angle between unit vectors a [..., 3] and b [3] (atan2 of |a x b| and a . b: exact enough at 1e-4 rad and at pi / 2)"""
    c = np.cross(a, b)
    return np.arctan2(np.sqrt((c * c).sum(axis=-1)), a @ b)


def _tri_rows(v0, v1, v2):
    """The two rows of a r + b s = p that Triangle::contains ends up solving (triangle.rs:55-96): (x, y) unless a zero pivot
    swaps rows (r.x == 0: the y row first, or the z row; then a zero in the eliminated second row: the third).  None: "can't
    handle LGS" (never contains)."""
    r, s = v1 - v0, v2 - v0
    rows = [0, 1, 2]
    if r[0] == 0.0:
        if r[1] == 0.0:
            if r[2] == 0.0:
                return None
            rows = [2, 1, 0]
        else:
            rows = [1, 0, 2]
    i0, i1, i2 = rows
    q = s[i0] / r[i0]
    if s[i1] - q * r[i1] == 0.0:
        if s[i2] - q * r[i2] == 0.0:
            return None
        i1 = i2
    return i0, i1


def _tri_min_barycentric(v0, v1, v2, pos, dirs):
    """Triangle::distance as the text has it (triangle.rs:108-127), for unit directions dirs [..., 3] from pos: the plane distance
    t = n . (v0 - pos) / (dir . n), its ABSOLUTE value, hit point pos + dir * |t| (in front of the ray also when the plane is
    behind it), and `contains` solving two rows for (a, b).  Returns min(a, b, 1 - a - b) per direction: >= 0 where the triangle
    is hit, < (1 - k) / 3 where the hit point lies outside the triangle enlarged k times about its centroid; -inf where the text
    reports no distance (dir . n == 0, or an unsolvable system).  (The cull of triangle.rs:115 is left to the caller.)"""
    n = _norm(np.cross(v1 - v0, v2 - v0))
    rows = _tri_rows(v0, v1, v2)
    out = np.full(dirs.shape[:-1], -np.inf)
    if rows is None:
        return out
    dn = dirs @ n
    ok = dn != 0.0
    t = np.abs(float(n @ (v0 - pos)) / np.where(ok, dn, 1.0))
    p = (pos - v0) + dirs * t[..., None]
    r, s = v1 - v0, v2 - v0
    i0, i1 = rows
    det = r[i0] * s[i1] - s[i0] * r[i1]
    a = (p[..., i0] * s[i1] - s[i0] * p[..., i1]) / det
    b = (r[i0] * p[..., i1] - p[..., i0] * r[i1]) / det
    return np.where(ok, np.minimum(np.minimum(a, b), 1.0 - a - b), out)


def pixel_map_marks(w, h):
    """The pixels that get a mark: the four corners ((0, 0) is where a pixel-CENTRE convention goes dark: its mark would sit half
    a pixel outside the frame), the centre and its neighbours, and pixels on both sides of the borders of the 8 x 8 ray tiles --
    there a mark's ray is the extreme ray of its tile's beam and the mark straddles into the next tile's."""
    cand = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (w // 2 - 1, h // 2), (w // 2, h // 2 - 2),
            (8, 8), (7, 8), (16, 7), (15, 16), (w - 1 - 7, 7), (w - 1 - 8, 8), (7, h - 1 - 7), (8, h - 1 - 8),
            (w // 8 * 8, h // 8 * 8), (w // 8 * 8 - 1, h // 8 * 8 - 1), ((w - 1) // 8 * 8, 3), (3, (h - 1) // 8 * 8),
            (w - 1, h // 2 + 1), (w // 2 + 3, h - 1)]
    out = []
    for x, y in cand:
        if 0 <= x < w and 0 <= y < h and (x, y) not in out:
            out.append((x, y))
    return out


def mark_emission(k):
    """distinct dyadic emissions (k < 63), every channel in (0, 1]: exact under any sum and average, and nonzero as u8"""
    return ((k + 1) / 64.0, ((7 * k) % 64 + 1) / 64.0, ((13 * k) % 64 + 1) / 64.0)


_pixel_map_cache = {}


def pixel_map_case(dtype, cam, w, h, marks=None, shape="sphere", fillers=0):
    """One emissive shape (base colour 0: the path ends there; emission mark_emission(k)) per marked pixel, MARK_DISTANCE along
    that pixel's ray D = norm(pixel_ray(...)) (scene.rs:207 normalises; no lens: focal_offset = non_focal_offset = 0), of angular
    radius rho = MARK_SHARE x the smallest angle between the pixel's ray and any of its eight neighbours':
      "sphere":   centre pos + 50 D, radius 50 sin rho (near root 50 - r, sphere.rs:29);
      "triangle": equilateral, circumradius 50 tan rho about pos + 50 D in the plane perpendicular to D, rotated in that plane by a
                  generic angle so that `contains` solves the (x, y) rows (triangle.rs:55-56), wound so that n . v0 > 1 in absolute
                  coordinates: triangle.rs:115's n . (v0 - dir) < 0 then never culls it, whatever unit dir.  Two exceptions, both
                  on the middle row of an even-height frame of a camera with forward.z = 0, where D.z = 0: (i) D = +x exactly
                  (the centre pixel of an even-width frame): the mark lies in x = const and the zero-pivot swaps solve (y, z)
                  (triangle.rs:60-71,81-87); (ii) any other such D: the perpendicular plane contains the z direction, its (x, y)
                  projection is a segment and the two rows the text solves are singular but for rounding (Triangle::contains is
                  noise there) -- the triangle is tilted by 0.3 rad about its horizontal in-plane axis, inside the same
                  sphere of radius 50 tan rho (the margin below is asserted on the tilted triangle).  The same tilt, or half a
                  radian more of in-plane rotation, is taken wherever the two rows would otherwise be badly conditioned (the
                  (x, y) projection under 5 % of the area, or the first pivot r.x under 0.2 % of its edge).
    Expected image ([y][x], scene.rs:136: row 0 is v = 0): the mark's emission at its pixel -- every sample is 0 + 1 * e and the
    average of n equal dyadic values is that value --, exactly 0 everywhere else; closest_object is called once per ray.
    The closed form's margin is ASSERTED here, in f64: every other pixel's ray (marked or not) misses a sphere mark by at least
    MARK_MARGIN x its angular radius, and for a triangle mark the hit point the text computes (|t|: also for a plane behind the ray)
    lies outside the triangle enlarged MARK_MARGIN x about its centroid; the construction gives 1 / MARK_SHARE = 3.3.
    `fillers` > 0 (the two-stage frame; needs fov < pi): that many more black shapes of the same kind BEHIND the camera, so that the
    tree is a real one (and, for triangles, large enough for AUTO to take the wavefront form).  A black shape changes nothing
    where it replaces a miss; that no MARKED pixel's ray meets one is asserted (spheres: they lie in the half space behind
    the camera, which no ray with D . forward = cos angle_x cos angle_y > 0 enters; triangles: Triangle::distance's text per
    marked ray, phantom hits included).
    Returns (objects, config kwargs, expected [h][w][3], info) -- info: marks, the un-normalised D per mark, rho and sphere radius."""
    marks = list(marks) if marks is not None else pixel_map_marks(w, h)
    key = (str(dtype), cam, w, h, tuple(marks), shape, fillers)
    if key in _pixel_map_cache:
        objs, cfg, expected, info = _pixel_map_cache[key]
        return objs.copy(), dict(cfg), expected.copy(), info
    assert shape in ("sphere", "triangle") and len(marks) < 63 and len(set(marks)) == len(marks)
    pos = np.asarray(cam[0], dtype=np.float64)
    right, up, fwd = camera_basis(cam[1])
    rays = _all_pixel_rays(cam, w, h)
    o = _obj(dtype, len(marks) + fillers)
    o["roughness"] = 1.0
    expected = np.zeros((h, w, 3))
    info = dict(marks=marks, D=[], rho=[], radius=[])
    for k, (x, y) in enumerate(marks):
        D = pixel_ray(cam, w, h, x, y)
        d = _norm(D)
        rho = MARK_SHARE * min(float(_angle(_norm(pixel_ray(cam, w, h, x + i, y + j)), d))
                               for i in (-1, 0, 1) for j in (-1, 0, 1) if (i, j) != (0, 0))
        assert 1e-5 < rho < 0.2
        centre = pos + d * MARK_DISTANCE
        own = np.zeros((h, w), dtype=bool)
        own[y, x] = True
        if shape == "sphere":
            r = MARK_DISTANCE * math.sin(rho)
            o[k]["kind"] = 0
            o[k]["geom"][:4] = (*centre, r)
            assert float(_angle(rays, d)[~own].min()) >= MARK_MARGIN * rho and float(_angle(rays[y, x], d)) < 1e-9
            info["radius"].append(r)
        else:
            e1 = _norm(np.cross(d, (0.0, 0.0, 1.0) if abs(d[2]) < 0.9 else (0.0, 1.0, 0.0)))
            e2 = np.cross(d, e1)
            R, phi = MARK_DISTANCE * math.tan(rho), 0.37 + 0.61 * k
            for tilt, turn in ((0.0, 0.0), (0.0, 0.5), (0.3, 0.0), (0.3, 0.5)):
                f2 = math.cos(tilt) * e2 + math.sin(tilt) * d
                v = [centre + R * (math.cos(phi + turn + j * 2.0 * math.pi / 3.0) * e1 + math.sin(phi + turn + j * 2.0 * math.pi / 3.0) * f2) for j in range(3)]
                if float(_norm(np.cross(v[1] - v[0], v[2] - v[0])) @ v[0]) < 0.0:
                    v[1], v[2] = v[2], v[1]
                nz = abs(float(_norm(np.cross(v[1] - v[0], v[2] - v[0]))[2]))
                pivot = abs(v[1][0] - v[0][0]) / float(np.linalg.norm(v[1] - v[0]))
                if _tri_rows(v[0], v[1], v[2]) != (0, 1) or (nz >= 0.05 and pivot >= 0.002):
                    break
            # the two rows solved are a well-conditioned system: the (x, y) projection keeps >= 5 % of the area, the first pivot >= 0.2 % of its edge
            # (elimination without pivoting then loses at most three of f64's sixteen digits; the margin needs one)
            assert _tri_rows(v[0], v[1], v[2]) != (0, 1) or (nz >= 0.05 and pivot >= 0.002)
            assert float(_norm(np.cross(v[1] - v[0], v[2] - v[0])) @ v[0]) > 1.0                    # never culled (triangle.rs:115)
            o[k]["kind"] = 2
            o[k]["geom"] = np.concatenate(v)
            m = _tri_min_barycentric(v[0], v[1], v[2], pos, rays)
            assert float(m[~own].max()) < (1.0 - MARK_MARGIN) / 3.0 and float(m[y, x]) > 0.3        # (its own ray: the centroid, 1/3 each)
            info["radius"].append(R)
        o[k]["emission_color"] = mark_emission(k)
        expected[y, x] = mark_emission(k)
        info["D"].append(D)
        info["rho"].append(rho)
    if fillers:
        assert cam[2] < math.pi and h / w * cam[2] < math.pi
        ru, uu = _norm(right), _norm(up)
        mark_dirs = np.array([_norm(D) for D in info["D"]])
        for i in range(fillers):
            k = len(marks) + i
            c = pos - fwd * (20.0 + 0.013 * i) + ru * (i % 35 - 17.0) + uu * (i // 35 - 17.0)
            if shape == "sphere":
                o[k]["kind"] = 0
                o[k]["geom"][:4] = (*c, 0.4)
                assert float((c - pos) @ fwd) + 0.4 < 0.0
            else:
                # its normal within ~30 degrees of c's direction (varied, and with a z component: an (x, y) footprint), so that
                # n . v0 > 1: never culled (triangle.rs:115) -- the upload would drop a triangle that always is
                for sign in (1.0, -1.0):
                    n = _norm(_norm(c) + sign * 0.5 * np.array([math.sin(1.0 + i), math.cos(2.0 + 0.7 * i), 0.8]))
                    if abs(n[2]) >= 0.05:
                        break
                a1 = _norm(np.cross(n, (math.sin(0.3 * i), 0.4, 1.0)))
                a2 = np.cross(n, a1)
                v = [c, c + 0.3 * a1, c + 0.3 * a2]
                assert abs(n[2]) >= 0.05 and float(_norm(np.cross(v[1] - v[0], v[2] - v[0])) @ v[0]) > 1.0
                o[k]["kind"] = 2
                o[k]["geom"] = np.concatenate(v)
                assert float(_tri_min_barycentric(v[0], v[1], v[2], pos, mark_dirs).max()) < (1.0 - MARK_MARGIN) / 3.0
    cfg = dict(rays_per_pixel=1 if w * h >= 1 << 20 else 2, focal_offset=0.0, non_focal_offset=0.0, seed=7)
    _pixel_map_cache[key] = (o, cfg, expected, info)
    return o.copy(), dict(cfg), expected.copy(), info


def pixel_map_cases(dtype, big=False):
    """(name, objects, camera, config kwargs, w, h, expected, info, shape): every camera x every small frame x both shapes; big:
    the two-stage frame instead, sphere and triangle marks from two cameras each, with fillers behind the camera."""
    for cname, cam in (PIXEL_MAP_CAMERAS[::2] if big else PIXEL_MAP_CAMERAS):
        for w, h in ([(PIXEL_MAP_BIG, PIXEL_MAP_BIG)] if big else PIXEL_MAP_FRAMES):
            for shape in ("sphere", "triangle"):
                objs, cfg, expected, info = pixel_map_case(dtype, cam, w, h, None, shape, fillers=(200 if shape == "sphere" else 1190) if big else 0)
                yield "%s, %dx%d, %s marks" % (cname, w, h, shape), objs, cam, cfg, w, h, expected, info, shape


def quantized(expected):
    """render_to_image (scene.rs:173-178) of an image with values in [0, 1]: x 256, `as u8` (truncating, saturating), image row y
    = render row height - y - 1."""
    return np.minimum(np.floor(expected * 256.0), 255.0).astype(np.uint8)[::-1]


# ---- the lens (scene.rs:202-207) ------------------------------------------------------------------------------------------------------
LENS_EMIT = (4.0, 2.0, 1.0)
LENS_W, LENS_H, LENS_SPP = 24, 16, 5                             # the exact cases' frame


def _occluder(dtype, X, axis, edge, side):
    """A black triangle (emission 0, base colour 0) in the plane x = X that covers coordinate[axis] >= edge (side +1) or <= edge
    (side -1) wherever a ray of these scenes can pass (|other coordinate| <= 999, up to 1 beyond the edge), wound so that its
    normal is +x: n . v0 = X > 1 and triangle.rs:115 never culls it.  All three x are X: `contains` takes the zero-pivot swaps and
    solves the (y, z) rows; its coefficient along the axis is (hit[axis] - edge) / (+-1000), and a difference has the sign of the
    exact one -- the edge is sharp."""
    other = 3 - axis
    H = 1000.0
    v = np.zeros((3, 3))
    v[:, 0] = X
    v[0, axis], v[0, other] = edge, -H
    v[1, axis], v[1, other] = edge, H
    v[2, axis], v[2, other] = edge + side * H, 0.0
    if np.cross(v[1] - v[0], v[2] - v[0])[0] < 0.0:
        v[[1, 2]] = v[[2, 1]]
    assert X > 1.0 and set(_tri_rows(v[0], v[1], v[2])) == {1, 2}
    o = _obj(dtype, 1)
    o[0]["kind"] = 2
    o[0]["geom"] = v.reshape(9)
    return o


def _lens_scene(dtype, occluders, light_x):
    light = _obj(dtype, 1)
    light[0]["kind"] = 1
    light[0]["geom"][:6] = (light_x, 0.0, 0.0, -1.0, 0.0, 0.0)   # faces the camera (plane.rs:25), behind everything
    light[0]["emission_color"] = LENS_EMIT
    o = np.concatenate([light] + list(occluders) + [_fillers(dtype, (-60.0, 35.0, 20.0), (-1.0, 0.0, 0.0))])
    o["roughness"] = 1.0
    return o


def lens_cases(dtype):
    """scene.rs:202-207: ray_position = position + U * non_focal_offset, target = position + direction * focal_length + U' *
    focal_offset, direction = norm(target - ray_position), with U and U' = Vector3::random() (vector.rs:29-35): SIX independent
    draws, each uniform on [0, 1) -- not centred.  The camera sits at the origin and looks along +x with a 1e-12 rad field of view
    (right = +y, up = +z; every pixel's direction is +x to 1e-12); a light plane (emission LENS_EMIT, base colour 0) faces the camera
    behind everything, and one black occluder (a triangle in a plane x = X with a sharp edge, _occluder; or a one-sided plane)
    covers one side: a sample is LENS_EMIT if its ray passes and 0 if not.  Fillers behind the camera give the tree kernels trees.
    With a = non_focal_offset, b = focal_offset, L = focal_length:
      * b = 0, L = 1e12: the ray runs parallel to +x at lateral offset a U_y, a U_z (its slope is below (a + 1) / L: 1e-11 at x = 5);
      * a = 0, L = 10: at x = 5 the ray is at 5 (10 d + b U')_yz / (10 d_x + b U'_x), inside [-3e-12, b / 2);
      * a = b, an occluder at x = L / 2: y = a (U_y + U'_y) / 2 + e with |e| <= a^2 / (L - a) + 1e-8 (the coupling through U_x, U'_x
        and the pixel's 1e-12 rad).
    EXACT cases (the occluder is never hit: the image is LENS_EMIT bit for bit, for any seed): an occluder over axis <= -1e-9 (a
    centred jitter hits it half the time) and one over axis >= a (1 + 1e-9) resp. b / 2 (1 + 1e-9) (the support's far end), for the
    origin's and the target's jitter, in y and in z; and for the origin's x a black plane at x = -a / 4 that faces AWAY from the
    camera's view (normal -x: plane.rs:25 lets only a ray that starts behind it and heads +x hit it) -- an origin that can
    fall behind it sees black, the reference's never does.
    STATISTICAL cases (Bernoulli; lit share p): a = 1, L = 1e12, occluder over axis >= a / 2 resp. a / 4: p = 1/2 resp. 1/4
    (uniformity and scale: U / 2 gives 1 resp. 1/2); and a = b = 1, L = 2e4, occluder at x = L / 2 over axis >= a / 4: p =
    P(U + U' < 1/2) = 1/8 where ONE draw serving both offsets gives P(2U < 1/2) = 1/4.
    Yields (name, objects, camera, config kwargs, p, exact, systematic) -- systematic: a bound on |lit share - p| from the terms
    neglected above, for lens_check."""
    cam = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1e-12)
    a = b = 1.0
    tiny = 1e-11                                                 # lateral drift of a "parallel" ray at x = 5: 5 (a + 1/2) / (1e12 - a)
    for axis, ax in ((1, "y"), (2, "z")):
        par = dict(non_focal_offset=a, focal_offset=0.0, focal_length=1e12)
        foc = dict(non_focal_offset=0.0, focal_offset=b, focal_length=10.0)
        yield ("origin jitter never below 0, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, -1e-9, -1)], 20.0), cam, par, 1.0, True, 0.0)
        yield ("origin jitter never reaches a, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, a * (1.0 + 1e-9), +1)], 20.0), cam, par, 1.0, True, 0.0)
        yield ("target jitter never below 0, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, -1e-9, -1)], 20.0), cam, foc, 1.0, True, 0.0)
        yield ("target jitter never reaches b, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, 0.5 * b * (1.0 + 1e-9), +1)], 20.0), cam, foc, 1.0, True, 0.0)
        # P(a U < a / 2 + drift): U is k / 2^52, so the share is 1/2 resp. 1/4 exactly but for the drift
        yield ("origin jitter uniform: half, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, a / 2, +1)], 20.0), cam, par, 0.5, False, tiny / a)
        yield ("origin jitter uniform: quarter, " + ax, _lens_scene(dtype, [_occluder(dtype, 5.0, axis, a / 4, +1)], 20.0), cam, par, 0.25, False, tiny / a)
        # lit iff (U + U') / 2 + e / a < 1/4, i.e. S = U + U' < 1/2 + eta with |eta| <= 2 |e| / a; P(S < s) = s^2 / 2 for s <= 1
        L = 2.0e4
        eta = 2.0 * (a * a / (L - a) + 1e-8) / a
        yield ("the two jitters are independent, " + ax, _lens_scene(dtype, [_occluder(dtype, L / 2, axis, a / 4, +1)], 4.0 * L), cam,
               dict(non_focal_offset=a, focal_offset=a, focal_length=L), 0.125, False, ((0.5 + eta) ** 2 - 0.25) / 2.0)
    back = _obj(dtype, 1)
    back[0]["kind"] = 1
    back[0]["geom"][:6] = (-a / 4, 0.0, 0.0, -1.0, 0.0, 0.0)
    yield ("origin jitter never below 0, x", _lens_scene(dtype, [back], 20.0), cam, dict(non_focal_offset=a, focal_offset=0.0, focal_length=1e12), 1.0, True, 0.0)


def lens_check(mean, n_samples, p, systematic, sigmas=5.0):
    """(|mean - p|, bound) for the lit share `mean` (the image divided by LENS_EMIT, averaged) of n_samples samples: hemisphere_check's
    5 sigma of a Bernoulli(p), plus the case's systematic term."""
    err, bound = hemisphere_check(mean, n_samples, p, 1.0, sigmas)
    return err, bound + systematic


# ---- ray_hit's two colour updates and avg (scene.rs:276-277, :253-259; iter_ops.rs:4-8; div.rs:11-20) on values that are NOT dyadic ---------
# Dyadic values come out the same under any summation order, any fused multiply-add and any `* (1 / n)`; these do not.
# (0.1, 0.7, 1/3) as emission would do for the summation, but with these base colours a fused `res = fma(light, e, res)` happens to
# round to the same values as the two-rounding form at every step up to 10 bounces, in all three channels; with the emission below it
# differs in every channel at 3 and at 10 bounces (tests/test_text_shapes.py checks that).
COLOUR_EMIT, COLOUR_BASE = (0.13, 0.6, 1.0 / 7.0), (0.9, 0.3, 0.77)
COLOUR_BOUNCES, COLOUR_SPP = (0, 3, 10), (1, 3, 7, 10, 64)
LENS_COLOUR_SPP, LENS_COLOUR_FRAME = (7, 10, 64, 257), 64


def closed_box_coloured(dtype, n_spheres=0, seed=5):
    """closed_box with emission COLOUR_EMIT and base colour COLOUR_BASE on EVERY object: every ray still hits something at every
    iteration, so every sample is the same value whatever the seed, the directions or the objects hit."""
    o = closed_box(dtype, n_spheres, seed)
    o["emission_color"] = COLOUR_EMIT
    o["base_color"] = COLOUR_BASE
    return o


def coloured_sample(max_bounces, emit=COLOUR_EMIT, base=COLOUR_BASE):
    """render_ray's value per channel, plain Python floats: resulting_color = 0, light_color = 1 (ray.rs:18-19), then max_bounces + 1
    times (scene.rs:227) resulting_color += light_color * emission; light_color *= base_color (scene.rs:276-277) -- a product, then
    a sum: two roundings, nothing fused."""
    out = []
    for e, b in zip(emit, base):
        res, light = 0.0, 1.0
        for _ in range(max_bounces + 1):
            res = res + light * e
            light = light * b
        out.append(res)
    return tuple(out)


def fold(value, k):
    """`value` added k times from zero, left to right (iter_ops.rs:4-8)"""
    total = 0.0
    for _ in range(k):
        total = total + value
    return total


def coloured_pixel(max_bounces, n):
    """avg of n equal samples (scene.rs:253-259): the fold, then / (n as f64) (div.rs:11-20)"""
    return tuple(fold(v, n) / float(n) for v in coloured_sample(max_bounces))


def lens_coloured_cases(dtype):
    """The "origin jitter uniform: half, y" scene of lens_cases with the light's emission COLOUR_EMIT: a sample is E = 0 + 1 * e or 0
    (the occluder is black), adding 0 is exact, so a pixel is fold(E, k) / n in all three channels for ONE k in 0..n -- the number
    of lit samples, Binomial(n, 1/2).  A binomial count with p = 1/2 stays within a few sqrt(n) / 2 of n / 2, so on its own it
    cannot reach half of 0..n for n >= 64: the quarter scene (z) and the same scene with the edge moved to 3/4 (lit share 3/4) cover the
    rest of the range.  Yields (name, objects, camera, config kwargs without seed / rays_per_pixel)."""
    cases = {name: (objs, cam, cfg) for name, objs, cam, cfg, _, _, _ in lens_cases(dtype)}
    objs, cam, cfg = cases["origin jitter uniform: half, y"]
    out = [("half, y", objs, cam, cfg)]
    objs, cam, cfg = cases["origin jitter uniform: quarter, z"]
    out.append(("quarter, z", objs, cam, cfg))
    out.append(("three quarters, z", _lens_scene(dtype, [_occluder(dtype, 5.0, 2, 0.75, +1)], 20.0), cam, cfg))
    for name, objs, cam, cfg in out:
        objs = objs.copy()
        assert tuple(objs[0]["emission_color"]) == LENS_EMIT
        objs[0]["emission_color"] = COLOUR_EMIT
        yield name, objs, cam, dict(cfg)


def lens_allowed(n, emit=COLOUR_EMIT):
    """[n + 1][3]: row k is the pixel with k lit samples, (fold(E_c, k) / n for the three channels)"""
    return np.array([[fold(e, k) / float(n) for e in emit] for k in range(n + 1)])


def lens_lit_counts(img, n):
    """per pixel the k whose row of lens_allowed equals the pixel in ALL THREE channels bit for bit, -1 where there is none"""
    allowed = lens_allowed(n)
    px = np.asarray(img, dtype=np.float64).reshape(-1, 3)
    k = np.clip(np.searchsorted(allowed[:, 0], px[:, 0]), 0, n)
    ok = (allowed[k].view(np.uint64) == np.ascontiguousarray(px).view(np.uint64)).all(axis=1)
    return np.where(ok, k, -1).reshape(np.asarray(img).shape[:-1])
