"""Inputs of tests/test_upsample.py and tests/test_upsample_gpu.py: fuzzed hostile low frames with the guides of both sizes, the option
sets every test walks, the check that the cases reach every branch of the header's text ("Guided upsampling", include/rtx_hip.h), and the
conversion between guide arrays and the library's records."""
import json
import os
import zlib

import numpy as np

import upsample_model as um
from upsample_model import DEMODULATE, NO_NORMAL, Params

INF = float("inf")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_CAM = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), np.pi / 2)              # tests/helpers.DEFAULT_CAM
# the golden scenes whose sizes the factor divides: (scene, s) of the quality condition, of the defaults' grid and of the dumped frames
QUALITY = [("c1_three_spheres_32x32", 2), ("c1_three_spheres_32x32", 4), ("mixed_40x24", 2), ("mixed_40x24", 4), ("tris300_32x18", 2)]
GUIDES = ("albedo", "emission", "normal", "depth")
BRANCHES = ("lattice", "last column", "last row", "h == 0", "guided", "tent", "no usable tap", "dark at p only", "dark at a tap only",
            "dark at both", "missed p among hit taps", "hit p among missed taps")


def fuzz_case(rng, hl, wl, s, hostile=True):
    """(lo, hi): hi = dict(albedo, emission, normal [H][W][3], depth [H][W]) of the hl * s x wl * s output frame -- three "surfaces"
    in patches -- and lo = dict(rgb, var, albedo, emission, normal, depth) of the hl x wl frame: hi's lattice pixels with a little noise
    (another lens jitter), an irradiance times the albedo plus the emission plus noise.  hostile: NaN, +-inf and -0.0 colours and
    variances, zero and sub-threshold albedo per channel, zero normals, +inf, NaN and zero depth, and missed pixels (a = e = n = 0, z =
    +inf, c = 0), on both sizes independently."""
    H, W = hl * s, wl * s
    shape = (H, W)
    patch = rng.integers(0, 3, ((H + 2) // 3, (W + 2) // 3)).repeat(3, axis=0).repeat(3, axis=1)[:H, :W]
    base = np.array([[0.8, 0.3, 0.2], [0.2, 0.7, 0.9], [0.5, 0.5, 0.5]])
    hi = dict(albedo=base[patch] * rng.uniform(0.9, 1.0, shape + (1,)),
              emission=np.where(rng.random(shape + (1,)) < 0.2, rng.uniform(0.0, 2.0, shape + (3,)), 0.0),
              normal=np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])[patch] + rng.normal(0, 0.05, shape + (3,)),
              depth=np.array([2.0, 5.0, 9.0])[patch] * rng.uniform(0.95, 1.05, shape))
    lshape = (hl, wl)
    lo = {k: hi[k][::s, ::s].copy() for k in GUIDES}
    lo["albedo"] = lo["albedo"] * rng.uniform(0.98, 1.0, lshape + (1,))
    lo["normal"] = lo["normal"] + rng.normal(0, 0.02, lshape + (3,))
    lo["depth"] = lo["depth"] * rng.uniform(0.99, 1.01, lshape)
    lo["rgb"] = lo["albedo"] * rng.uniform(0.2, 1.5, lshape + (1,)) + lo["emission"] + rng.normal(0, 0.05, lshape + (3,))
    lo["var"] = rng.uniform(0.0, 0.05, lshape + (3,))
    if hostile:
        def some(shp, frac):
            return rng.random(shp) < max(frac, 1.2 / (shp[0] * shp[1]))
        for g, shp in ((hi, shape), (lo, lshape)):
            g["depth"][some(shp, 0.06)] = INF
            g["normal"][some(shp, 0.08)] = 0.0
            g["albedo"][some(shp, 0.06)] = 0.0
            g["albedo"][some(shp, 0.08), 1] = 5e-4                        # below albedo_min 1e-3 on one channel
            g["albedo"][some(shp, 0.05), 2] = 0.0
            g["emission"][some(shp, 0.05)] = -0.0
            g["emission"][some(shp, 0.02), 0] = INF
            g["albedo"][some(shp, 0.02), 0] = np.nan
            g["normal"][some(shp, 0.02), 0] = np.nan
            g["depth"][some(shp, 0.02)] = np.nan
            g["depth"][some(shp, 0.02)] = 0.0
            miss = some(shp, 0.08)
            g["albedo"][miss], g["emission"][miss], g["normal"][miss], g["depth"][miss] = 0.0, 0.0, 0.0, INF
            if g is lo:
                g["rgb"][miss] = 0.0
        lo["var"][some(lshape, 0.1)] = 0.0
        lo["rgb"][some(lshape, 0.05), 0] = -0.0
        lo["rgb"][some(lshape, 0.05), 2] = np.nan
        lo["rgb"][some(lshape, 0.05), 1] = INF
        lo["rgb"][some(lshape, 0.03)] = -INF
        lo["var"][some(lshape, 0.04), 0] = np.nan
        lo["var"][some(lshape, 0.04), 1] = INF
    return lo, hi


def branches_reached(lo, hi, p):
    """the names of BRANCHES that some pixel (and channel) of this case takes under p, read off the array model's trace.  The three
    "dark" branches and the two "missed" ones look at ONE tap of a pixel, (X0, Y0) -- always inside the frame and, off the lattice,
    taken unless its tent weight is zero -- not at every tap the pixel takes: a sufficient sign that the branch occurs, which the
    fuzzed density of dark and missed pixels gives on every option set (cases() asserts it), not an exact account of "a tap"."""
    tr = {}
    um.upsample(lo, hi, p, trace=tr)
    s = p.factor
    hl, wl = lo["depth"].shape
    H, W = hi["depth"].shape
    got = set()
    nl = ~tr["lattice"]
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    if tr["lattice"].any():
        got.add("lattice")
    if (tr["outside"] & (x // s == wl - 1)).any():
        got.add("last column")
    if (tr["outside"] & (y // s == hl - 1)).any():
        got.add("last row")
    if tr["h_zero"].any():
        got.add("h == 0")
    for name, key in (("guided", "guided"), ("tent", "tent"), ("no usable tap", "none")):
        if tr[key].any():
            got.add(name)
    if p.flags & DEMODULATE:
        dark_p = hi["albedo"] <= p.albedo_min
        dark_q = (lo["albedo"] <= p.albedo_min)[tr["Y0"], tr["X0"]]
        for name, m in (("dark at p only", dark_p & ~dark_q), ("dark at a tap only", ~dark_p & dark_q), ("dark at both", dark_p & dark_q)):
            if (m & nl[..., None]).any():
                got.add(name)
    miss_p = np.isinf(hi["depth"]) & (hi["albedo"] == 0.0).all(axis=2)
    miss_q = (np.isinf(lo["depth"]) & (lo["albedo"] == 0.0).all(axis=2))[tr["Y0"], tr["X0"]]
    if (miss_p & ~miss_q & nl).any():
        got.add("missed p among hit taps")
    if (~miss_p & miss_q & nl).any():
        got.add("hit p among missed taps")
    return got


def option_sets():
    """(name, Params fields without the factor, with variance?): every flag and term on and off, NO_NORMAL and the ends of the power's
    range, min_weight zero and large"""
    full = dict(sigma_depth=0.3, sigma_albedo=0.5, albedo_min=1e-3, normal_power_log2=2, flags=DEMODULATE, min_weight=1e-2)
    return [("all terms", dict(full), True),
            ("no variance", dict(full), False),
            ("no demodulation", dict(full, flags=0), True),
            ("no demodulation, no variance", dict(full, flags=0), False),
            ("no normal term", dict(full, normal_power_log2=NO_NORMAL), True),
            ("normal power 2^0", dict(full, normal_power_log2=0), True),
            ("normal power 2^8", dict(full, normal_power_log2=8), False),
            ("no depth term", dict(full, sigma_depth=INF), True),
            ("no albedo term", dict(full, sigma_albedo=INF), True),
            ("no term at all", dict(full, sigma_depth=INF, sigma_albedo=INF, normal_power_log2=NO_NORMAL), True),
            ("min_weight 0, albedo_min 0", dict(full, min_weight=0.0, albedo_min=0.0), True),
            ("min_weight 0.5", dict(full, min_weight=0.5), True)]


def cases(low_sizes, factors, name, fields, with_var):
    """[(lo, hi, Params)] over low_sizes [(hl, wl)] x factors for one option set, from a seed the name gives; lo["var"] is None without
    a variance.  Asserts, as the cases are made, that together they reach every branch the option set can reach."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out, got = [], set()
    for (hl, wl) in low_sizes:
        for s in factors:
            lo, hi = fuzz_case(rng, hl, wl, s)
            if not with_var:
                lo["var"] = None
            p = Params(factor=s, **fields)
            got |= branches_reached(lo, hi, p)
            out.append((lo, hi, p))
    want = set(BRANCHES)
    if not fields["flags"] & DEMODULATE:
        want -= {"dark at p only", "dark at a tap only", "dark at both"}
    if all(s == 1 for s in factors):
        want = {"lattice"}
    elif max(hl * wl for hl, wl in low_sizes) > 1 and (math_isinf(fields["sigma_depth"]) and math_isinf(fields["sigma_albedo"]) and
                                                         fields["normal_power_log2"] == NO_NORMAL):
        want -= {"tent"}                                                  # w = h > 0 on every tap: the guided sum is the tent sum
    assert want <= got, (name, sorted(want - got))
    return out


def math_isinf(x):
    return x == INF or x == -INF


def oracle_guides(oracle, rtx, objs_raw, cam, w, h, **cfg):
    """the guides of a w x h frame from the oracle's closest_object on every pixel's zero-offset ray (rtxo_get_ray_dir): the hit
    object's base and emission colour, its normal at the hit point and the distance; a miss has a = e = n = 0 and z = +inf, as
    RtxPixelFeatures.  Also returns the ray directions [h][w][3]."""
    import ctypes as C
    objs = np.frombuffer(objs_raw.tobytes(), dtype=rtx.OBJECT_DTYPE)
    sc = oracle.make_scene(np.frombuffer(objs_raw.tobytes(), dtype=oracle.OBJECT_DTYPE), cam, **cfg)
    L = oracle.lib()
    vfov = h / w * cam[2]
    g = dict(albedo=np.zeros((h, w, 3)), emission=np.zeros((h, w, 3)), normal=np.zeros((h, w, 3)), depth=np.full((h, w), INF))
    dirs = np.zeros((h, w, 3))
    o = np.array(cam[0], dtype=np.float64)
    for y in range(h):
        for x in range(w):
            rd = np.array(L.rtxo_get_ray_dir(C.byref(sc), x / w, y / h, vfov).tuple())
            dirs[y, x] = rd
            i, dist = oracle.closest_object(sc, cam[0], tuple(rd))
            if i < 0:
                continue
            P = o + rd * dist
            geom = objs[i]["geom"]
            if objs[i]["kind"] == rtx.RTX_SPHERE:
                n = (P - geom[:3]) / np.linalg.norm(P - geom[:3])
            elif objs[i]["kind"] == rtx.RTX_PLANE:
                n = geom[3:6] / np.linalg.norm(geom[3:6])
            else:
                n = np.array(oracle.triangle_normal(geom[0:3], geom[3:6], geom[6:9]))
            g["albedo"][y, x], g["emission"][y, x] = objs[i]["base_color"], objs[i]["emission_color"]
            g["normal"][y, x], g["depth"][y, x] = n, dist
    return g, dirs


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["objects"], int(z["width"]), int(z["height"]), json.loads(str(z["config"]))


def model_params(rtx, s, **fields):
    """the library's defaults as a model Params"""
    d = rtx.upsample_params(factor=s, **fields)
    return Params(**{k: d[k].item() for k in ("factor", "flags", "normal_power_log2", "sigma_depth", "sigma_albedo", "albedo_min", "min_weight")})


def quality_inputs(oracle, rtx, name, s):
    """(lo, hi, ref): the oracle's frame of the golden scene at 1 / s of its golden size and 4 s^2 spp with the guides of both sizes
    from the oracle pick, and the 256-spp frame at the golden size"""
    objs_raw, w, h, cfg = golden(name)
    assert w % s == 0 and h % s == 0
    objs = np.frombuffer(objs_raw.tobytes(), dtype=oracle.OBJECT_DTYPE)
    wl, hl = w // s, h // s
    lo, _ = oracle_guides(oracle, rtx, objs_raw, DEFAULT_CAM, wl, hl, **cfg)
    hi, _ = oracle_guides(oracle, rtx, objs_raw, DEFAULT_CAM, w, h, **cfg)
    lo["rgb"] = oracle.render(oracle.make_scene(objs, DEFAULT_CAM, **dict(cfg, rays_per_pixel=4 * s * s, seed=11)), wl, hl)
    lo["var"] = None
    ref = oracle.render(oracle.make_scene(objs, DEFAULT_CAM, **dict(cfg, rays_per_pixel=256, seed=999)), w, h)
    return lo, hi, ref


def bilinear_params(s):
    """the same model with both sigmas +inf, no normal term, not demodulated: the tent weights alone"""
    return Params(factor=s, flags=0, normal_power_log2=NO_NORMAL, sigma_depth=INF, sigma_albedo=INF, albedo_min=0.0, min_weight=0.0)


def rmse(a, b):
    d = a - b
    return float(np.sqrt(np.mean(d * d)))


def to_records(dtype, guides):
    """RtxPixelFeatures records [h][w] of a frame's guides (coverage 1, object 0: the call reads neither)"""
    h, w = guides["depth"].shape
    f = np.zeros((h, w), dtype=dtype)
    f["albedo"], f["emission"], f["normal"], f["depth"] = guides["albedo"], guides["emission"], guides["normal"], guides["depth"]
    f["coverage"] = 1.0
    return f


def params_record(dtype, p):
    """the RtxUpsampleParams record of a model Params"""
    r = np.zeros((), dtype=dtype)
    for k in ("factor", "flags", "normal_power_log2", "sigma_depth", "sigma_albedo", "albedo_min", "min_weight"):
        r[k] = getattr(p, k)
    return r


def bits_equal(a, b):
    """the same f64 patterns, every NaN counted as one pattern (the device and numpy may differ in a NaN's payload and sign)"""
    a, b = np.array(a, dtype=np.float64, copy=True), np.array(b, dtype=np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
