"""Fuzzed inputs for the temporal accumulation tests (CPU and GPU): a previous frame that saw the inside of a spherical shell around its camera, cut into vertical bands of
object ids, through a camera with a random orthonormal to_cam_space, and a current frame whose surface points are aimed at chosen
coordinates of the previous one -- so most pixels find their history -- with every way of losing it, and hostile values, planted on
chosen pixels.  Every case is checked on the CPU when it is made (check_case), so no way goes untested and no case is vacuous."""
import math

import numpy as np

import temporal_model as tm

NAN, INF = float("nan"), float("inf")
PARAMS = tm.Params(alpha_min=0.05, max_history=32.0, plane_tolerance=0.02, normal_min=0.9, min_weight=0.1)
HOSTILE = (NAN, INF, -INF, -0.0)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[2] = -q[2]
    return q                                                 # rows: the camera's right, up, forward in world space


def _shell_points(cam_pos, R, fov, w, h, fx, fy, dist):
    """the points at distance dist that the camera (cam_pos, rows R) sees at the continuous pixel coordinates (fx, fy): a spherical shell
    around the camera, seen from inside"""
    vfov = h / w * fov
    ax, ay = fov * (fx / w - 0.5), vfov * (fy / h - 0.5)
    dc = np.stack([np.sin(ax), np.sin(ay), np.cos(ax) * np.cos(ay)], axis=-1)
    dw = dc @ R                                              # camera space -> world (R orthonormal)
    return cam_pos + dist * dw / np.linalg.norm(dw, axis=-1, keepdims=True)


def fuzz_case(seed, w, h, fov=math.pi / 2, with_var=True, planted=True):
    """-> dict(cur, hist, params, w, h).  planted=False (frames too small to hold the planted pixels): only the aimed surface"""
    rng = np.random.default_rng(seed)
    R = _rotation(rng)
    cam_pos = rng.normal(0, 2, 3)
    dist = 6.0
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    bands = lambda fx: np.clip(np.floor(fx * 3.0 / w), 0, 2).astype(np.int64) + 4
    aim = lambda fx, fy: _shell_points(cam_pos, R, fov, w, h, fx, fy, dist)
    inward = lambda pos: (cam_pos - pos) / np.linalg.norm(cam_pos - pos, axis=-1, keepdims=True)       # the shell's normal, towards the camera
    hist = dict(cam_pos=cam_pos, to_cam=R.reshape(9).copy(), tables=tm.tables(fov, w, h), fov=fov,
                rgb=rng.uniform(0, 2, (h, w, 3)), var=rng.uniform(0, 0.1, (h, w, 3)) if with_var else None,
                len=np.floor(rng.uniform(1, 40, (h, w))) + rng.choice([0.0, 0.25, 0.5], (h, w)),
                position=aim(xs, ys), object=bands(xs))
    hist["normal"] = inward(hist["position"]) * rng.choice([1.0, 0.5, 3.0], (h, w, 1))
    # the current frame: every pixel's point is where the previous camera saw (x + sx, y + sy)
    tx_, ty_ = xs + rng.uniform(-0.9, 0.9, (h, w)), ys + rng.uniform(-0.9, 0.9, (h, w))
    whole = rng.random((h, w)) < 0.15                        # some land on a pixel's own ray (one tap of weight ~1)
    tx_, ty_ = np.where(whole, np.round(tx_), tx_), np.where(whole, np.round(ty_), ty_)
    tx_, ty_ = np.clip(tx_, -0.4, w - 0.6), np.clip(ty_, -0.4, h - 0.6)
    if w * h == 1:
        tx_, ty_ = np.zeros((1, 1)), np.zeros((1, 1))       # (one pixel spans the whole fov: only its own ray finds the same surface)
    cur = dict(rgb=rng.uniform(0, 2, (h, w, 3)), var=rng.uniform(0, 0.4, (h, w, 3)) if with_var else None, position=aim(tx_, ty_),
               object=bands(np.clip(np.round(tx_), 0, w - 1)))
    cur["normal"] = inward(cur["position"]) * rng.choice([1.0, 0.25, 2.0], (h, w, 1))
    if planted:
        assert w >= 12 and h >= 10, "planted cases need room"
        picks = rng.permutation(w * h)
        take = iter(picks)
        px = lambda: divmod(int(next(take)), w)              # (y, x) of a fresh pixel
        # -- the current frame's own ways of losing history
        for _ in range(2):
            y, x = px(); cur["object"][y, x] = -1; cur["position"][y, x] = NAN; cur["normal"][y, x] = NAN          # a miss
            y, x = px(); cur["position"][y, x, rng.integers(3)] = rng.choice([NAN, INF, -INF])                     # a hostile position
            y, x = px(); cur["position"][y, x] = cam_pos - 3.0 * R[2] + 0.3 * R[0]                                 # behind the camera
            y, x = px(); cur["object"][y, x] = 9                                                                   # another object
            y, x = px(); cur["position"][y, x] += cur["normal"][y, x] / np.linalg.norm(cur["normal"][y, x]) * 0.5 * dist   # off the plane
            y, x = px(); cur["normal"][y, x] = R[0]                                                                # turned normal
            y, x = px(); cur["normal"][y, x] = 0.0                                                                 # zero normal
            y, x = px(); cur["rgb"][y, x, rng.integers(3)] = rng.choice(HOSTILE)                                   # hostile colour (kept)
            if with_var:
                y, x = px(); cur["var"][y, x, rng.integers(3)] = rng.choice(HOSTILE)
        ways = [tm.MISS, tm.BEHIND]
        outside = [(tm.LEFT, -1.0, h / 2), (tm.RIGHT, float(w), h / 2), (tm.ABOVE, w / 2, -1.0), (tm.BELOW, w / 2, float(h))]
        for way, fx, fy in outside:                          # outside the previous frame on each side, aimed without the scale --
            pt = aim(np.float64(fx), np.float64(fy))
            if (pt - cam_pos) @ R[2] > 1e-3:                 # -- where such a ray exists: at fov = pi the frame's sides are the horizon
                y, x = px(); cur["position"][y, x] = pt
                ways.append(way)
        # -- the history's: blocks of 2 x 2 previous pixels, with a current pixel aimed into the middle of each
        used = np.zeros((h, w), dtype=bool)
        def block():                                         # (disjoint blocks, one band's object id in each)
            while True:
                y, x = px()
                if x < w - 1 and y < h - 1 and not used[y:y + 2, x:x + 2].any():
                    used[y:y + 2, x:x + 2] = True
                    hist["object"][y:y + 2, x:x + 2] = hist["object"][y, x]
                    return y, x
        for kind in ("nan", "inf", "len0", "lennan", "posnan", "posoff", "normal", "var", "object", "zero"):
            y, x = block()
            sl = (slice(y, y + 2), slice(x, x + 2))
            if kind == "nan": hist["rgb"][sl + (1,)] = NAN
            elif kind == "inf": hist["rgb"][sl + (2,)] = -INF
            elif kind == "len0": hist["len"][sl] = 0.0
            elif kind == "lennan": hist["len"][sl] = NAN
            elif kind == "posnan": hist["position"][sl + (0,)] = NAN
            elif kind == "posoff": hist["position"][sl] += 3.0 * inward(hist["position"][sl])
            elif kind == "normal":                           # turned: a fifth along the shell's normal, the rest across it
                n_in = inward(hist["position"][sl])
                across = np.cross(n_in, R[1])
                hist["normal"][sl] = across / np.linalg.norm(across, axis=-1, keepdims=True) + 0.2 * n_in
            elif kind == "var" and with_var: hist["var"][sl + (0,)] = INF
            cur["position"][y, x] = aim(np.float64(x + 0.5), np.float64(y + 0.5))
            cur["object"][y, x] = hist["object"][y, x]
            cur["normal"][y, x] = inward(cur["position"][y, x])
            if kind == "object": cur["object"][y, x] = 9
            elif kind == "zero": cur["normal"][y, x] = 0.0
        # -- too little weight: the heavy tap has no history, the other three weigh 0.0975 <= min_weight
        y, x = block()
        hist["len"][y, x] = 0.0
        cur["position"][y, x] = aim(np.float64(x + 0.05), np.float64(y + 0.05))
        cur["object"][y, x] = hist["object"][y, x]
        cur["normal"][y, x] = inward(cur["position"][y, x])
        hist["rgb"][tuple(divmod(int(next(take)), w))] = -0.0
    case = dict(cur=cur, hist=hist, params=PARAMS, w=w, h=h, planted=planted, ways=ways if planted else [])
    check_case(case)
    return case


def check_case(case):
    """no case is vacuous: enough pixels blend two or more taps, and every way of losing history occurs"""
    out, _, ln, _, info = tm.accumulate(case["cur"], case["hist"], case["params"], info=True)
    why, taps, kept = info["why"], info["taps"], info["kept"]
    blended = why == tm.BLENDED
    if not case["planted"]:
        assert blended.any()
        return
    assert ((blended & (kept >= 2)).sum() * 4 >= why.size), "fewer than a quarter of the pixels blend two taps or more"
    lost = why == tm.LOW_WEIGHT
    assert len(case["ways"]) >= 4                             # (all six but at fov = pi, which has no left and right outside)
    for way in case["ways"]:
        assert (why == way).any(), way
    for bit in (tm.TAP_OBJECT, tm.TAP_LEN, tm.TAP_NOT_FINITE, tm.TAP_NORMAL, tm.TAP_PLANE):
        assert (lost & (taps == bit)).any(), bit             # a pixel that lost its history to this test alone
    assert (lost & (kept > 0)).any(), "no pixel with 0 < sw <= min_weight"
    assert (ln[blended] > 1).all() and (ln[~blended] == 1).all()


def _ulp_search(T_i, want):
    """(x, z) with y = 0 for which the header's arithmetic gives sx == want exactly (the identity camera at the origin), or None"""
    x0 = T_i
    z0 = math.sqrt(max(1.0 - x0 * x0, 0.0))
    for dz in range(-40, 41):
        z = z0
        for _ in range(abs(dz)):
            z = math.nextafter(z, INF if dz > 0 else -INF)
        for dx in range(-6, 7):
            x = x0
            for _ in range(abs(dx)):
                x = math.nextafter(x, INF if dx > 0 else -INF)
            a = x * x
            L = (a + 0.0) + z * z
            q = L * L - 4.0 * (a * 0.0)
            m = 2.0 / (L + math.sqrt(q if q > 0 else 0.0))
            if x * math.sqrt(m) == want:
                return x, z
    return None


def table_edge_case(w=16, h=8, fov=math.pi / 2):
    """sx exactly on a table entry, and one ulp to either side, through the identity camera at the origin (y = 0: sy = 0 = Ty[h / 2]
    exactly).  -> the case, and how many of the 3 * (w + 1) aims were found"""
    T = tm.tables(fov, w, h)
    aims = []
    for i in range(w + 1):
        for want in (T[i], math.nextafter(T[i], -INF), math.nextafter(T[i], INF)):
            got = _ulp_search(float(T[i]), float(want))
            if got is not None:
                aims.append((i, got))
    n = len(aims)
    assert n >= 2 * (w + 1), "the search found too few exact aims"
    hh, ww = h, w
    reps = -(-n // ww)
    assert reps <= hh
    rng = np.random.default_rng(5)
    flat = dict(rgb=rng.uniform(0, 1, (hh, ww, 3)), var=rng.uniform(0, 0.1, (hh, ww, 3)), position=np.full((hh, ww, 3), NAN),
                normal=np.broadcast_to(np.array([0.0, 0.0, -1.0]), (hh, ww, 3)).copy(), object=np.full((hh, ww), -1, dtype=np.int64))
    for k, (i, (x, z)) in enumerate(aims):
        flat["position"][k // ww, k % ww] = (x, 0.0, z)
        flat["object"][k // ww, k % ww] = 0
    hist = dict(cam_pos=np.zeros(3), to_cam=np.eye(3).reshape(9), tables=T, fov=fov, rgb=rng.uniform(0, 1, (hh, ww, 3)),
                var=rng.uniform(0, 0.1, (hh, ww, 3)), len=np.full((hh, ww), 3.0), position=np.zeros((hh, ww, 3)),
                normal=np.broadcast_to(np.array([0.0, 0.0, -1.0]), (hh, ww, 3)).copy(), object=np.zeros((hh, ww), dtype=np.int64))
    # the history's points: far from every plane test's edge is not the point here -- accept everything (a huge tolerance)
    case = dict(cur=flat, hist=hist, params=PARAMS.replace(plane_tolerance=1e3, min_weight=0.0), w=ww, h=hh, planted=False)
    _, _, _, motion, info = tm.accumulate(flat, hist, case["params"], info=True)
    fx = motion[..., 0].ravel()[:n]
    on = sum(1 for k, (i, _) in enumerate(aims) if fx[k] == float(i))
    assert on >= w // 2, "no aim landed exactly on its entry"
    assert (motion[..., 1].ravel()[:n][np.isfinite(fx)] == h // 2).all()
    return case, n


def tiny_fov_case(w=16, h=8):
    """a fov so small that neighbouring table entries are equal (den == 0): the identity camera, points on and beside the axis"""
    fov = 2e-323
    T = tm.tables(fov, w, h)
    assert (np.diff(T[:w + 1]) == 0).any() and (np.diff(T[w + 1:]) == 0).any()
    rng = np.random.default_rng(6)
    xs = rng.choice([0.0, -0.0, 5e-324, -5e-324, 1e-323, -1e-323, 1.5e-323, 1e-300], (h, w))
    ysv = rng.choice([0.0, 5e-324, -5e-324, -0.0], (h, w))
    pos = np.stack([xs, ysv, np.ones((h, w))], axis=-1)      # z = 1: L == 1, so sx == x and sy == y exactly
    nrm = np.broadcast_to(np.array([0.0, 0.0, -1.0]), (h, w, 3)).copy()
    cur = dict(rgb=rng.uniform(0, 1, (h, w, 3)), var=rng.uniform(0, 0.1, (h, w, 3)), position=pos, normal=nrm, object=np.zeros((h, w), dtype=np.int64))
    hist = dict(cam_pos=np.zeros(3), to_cam=np.eye(3).reshape(9), tables=T, fov=fov, rgb=rng.uniform(0, 1, (h, w, 3)), var=rng.uniform(0, 0.1, (h, w, 3)),
                len=np.full((h, w), 2.0), position=pos.copy(), normal=nrm.copy(), object=np.zeros((h, w), dtype=np.int64))
    case = dict(cur=cur, hist=hist, params=PARAMS.replace(min_weight=0.0), w=w, h=h, planted=False)
    _, _, _, motion, info = tm.accumulate(cur, hist, case["params"], info=True)
    assert (info["why"] == tm.BLENDED).sum() * 2 >= w * h
    return case


def params_record(dtype, p):
    """the RtxTemporalParams record of a model Params"""
    r = np.zeros((), dtype=dtype)
    for k in ("alpha_min", "max_history", "plane_tolerance", "normal_min", "min_weight"):
        r[k] = getattr(p, k)
    return r


def hit_records(dtype, frame):
    """RtxHit records [h][w] of a frame's pick buffer (distance 1: the accumulation does not read it)"""
    h, w = frame["object"].shape
    r = np.zeros((h, w), dtype=dtype)
    r["position"], r["normal"], r["object"], r["distance"] = frame["position"], frame["normal"], frame["object"], 1.0
    return r


def bits_equal(a, b):
    """the same f64 patterns, every NaN counted as one pattern (the device and numpy may differ in a NaN's payload and sign)"""
    a, b = np.array(a, dtype=np.float64, copy=True), np.array(b, dtype=np.float64, copy=True)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
