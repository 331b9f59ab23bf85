"""The tile-list builder (build_mesh_tile_lists_kernel, rtx_wavefront.hip) held to the f64 text on the extreme rays of every tile.

Once per 8 x 8 tile the builder decides which shapes any primary ray of the tile may ever see, with a lower bound t_lb of the distance
that the packet kernels trust to stop early.  Frames show a wrong list only when one of their few random samples needs exactly the
missing entry; here the lists themselves are read back (rtx_debug_tile_lists: the handle's own buffer, carved as the launch carved
it) and held to the rays of tests/tile_list_cases.py -- lens draws at the corners of their boxes, corner and edge pixels, partial
tiles, a band of blocks, offsets of both signs, phantom triangles -- in scenes aimed at exactly those rays.  The CPU conditions the
generator must meet are tests/test_tile_lists.py's.

THE PROPERTY, no tolerance: for every pair the text reports -- a ray of tile T, an object j of the tree, the distance t, the origin
inside the walks' range -- T has no list (its packets walk), or j is in T's list with t_lb <= t (the f32 as an f64 value against
the f64 distance).  In the aimed cases no tile may answer "walk": the scenes are under every cap and every beam is non-degenerate.
Structure: count <= cap, t_lb finite, >= 0 and non-decreasing, objects distinct, sphere entries' records equal the independent pack
of tests/bounds_model.py bit for bit, filter records map to triangles that pack puts in the tree.  (Every tile of these frames owns a
pixel: "a tile without pixels has count 0" has no instance here and is asserted through the tile count alone.)

Mutations of the builder, one scratch build and one run of this module each (values only -- no index, address or loop bound):

  mutation                                                    turns red
  the origin box collapsed to cam (non_focal_offset ignored)   the property, 17 of the first 21 cases ("absent from the list"; not the
                                                               pinhole, not where the aimed shapes' boxes cover the 0.1 offset),
                                                               the fallback frames, both resident-scene tests, the 4 spp frames
  focal_offset left out of tmax                                the property on the three wide_focal cases (absent), the 4 spp frames;
                                                               NOT on the issue's own cameras -- the first finding below
  the hull taken over lanes 0 ... 62                           the property on pinhole-spheres-band and pinhole-mesh-whole (absent:
                                                               the shape aimed at the tile's last pixel), the 4 spp frames
  fmin(0, nfo) / fmax(0, nfo) swapped                          the property on every case but the pinhole's
  A2 = 0                                                       nothing -- the second finding
  t_lb with lmax for lmin                                      the property on 20 of the first 21 cases ("t_lb overshoots")
  t_lb divided by the smallest |n.D|                           the property on every mesh and joint case (overshoots)
  the sort's comparison reversed                               the structure check of every case (t_lb not non-decreasing)
  the 1e-12 widenings set to 0                                 nothing -- expected, the third finding
  the 1e-9 widenings set to 0                                  nothing -- expected, the third finding

Findings of the first run.  The shipped builder has the property on all 24 cases, every fallback and every resident-scene step: no
pair is absent, the smallest (t - t_lb) / t seen is 2.1e-2 (profiles/tile_list_property.txt).
  1. The beam is LOOSE: one parameter interval [u0, u1] serves all its rays and the direction box is axis-aligned, so at a shape's
     depth it is wider than the ray family by 1 / (cos angle_x cos angle_y) of the tile -- by that reckoning at least 3.5 % of its
     width in every tile of these frames.  A focal_offset of 1e-4 (the default), 0.05 at focal length 30 or -0.3 (which tmax does not see at all) moves the
     family's edge by far less; only a target box that is a good part of a tile wide (wide_focal: 2.0 at focal length 10) shows
     focal_offset missing from tmax.  That camera was added for it.
  2. A2, the filter's own allowance (2 * 64 u S, "whatever the f32 filter passes is in the list"), is not needed for what the TEXT
     reports: the records' rectangles are packed grown by 1 + 2^-20 and rounded up, which already covers their f32 rounding, and the
     exact tests reject what only the allowance admits.  It keeps the list a superset of the f32 FILTER's passes -- a statement about
     equal counters with the walks, not about frames -- and no test of this module can see it go.
  3. The 1e-12 and 1e-9 widenings guard f64 roundings of the builder's own arithmetic: 10^4 to 10^7 times below the smallest secant
     depth aimed here (2^-20 of a radius) and far below finding 1's looseness.  Not caught, as expected."""
import numpy as np
import pytest

import bounds_model as bm
import tile_list_cases as tc
from helpers import hip_scene


@pytest.fixture(scope="module")
def gpu(rtx):
    if rtx.device_count() < 1:
        pytest.fail("no gfx950 device: the gpu tests must run on an MI355X (there is no CPU fallback to test)")
    return rtx


def _config(gpu, kind, lens, spp=1, tuning=0, kernel=None):
    fl, fo, nfo = lens
    if kernel is None:
        kernel, base = (gpu.RTX_KERNEL_AUTO, gpu.RTX_TUNE_TWO_STAGE) if kind == "spheres" else (gpu.RTX_KERNEL_WAVEFRONT, 0)
    else:
        base = 0
    return dict(kernel=kernel, rays_per_pixel=spp, seed=11, tuning=base | tuning, focal_length=fl, focal_offset=fo, non_focal_offset=nfo)


def _frame(hnd, frame):
    """one frame (or band) on a resident handle: (pixels, stats)"""
    import torch
    w, h, band = frame
    rows = tc.band_rows(h, band)
    buf = torch.zeros((len(rows), w, 3), dtype=torch.float64, device="cuda:0")
    if band is None:
        st = hnd.render_rows(w, h, 0, 1, h, buf.data_ptr())
    else:
        st = hnd.render_blocks(w, h, band[0], band[1], band[2], buf.data_ptr())
    return buf.cpu().numpy(), st


def _packets_ran(gpu, kind, st):
    if kind == "spheres":
        return st.kernel == gpu.RTX_KERNEL_BVH and st.stage1_ms > 0
    return st.kernel == gpu.RTX_KERNEL_WAVEFRONT


def _render(gpu, objs, cam, lens, frame, kind, spp=1, tuning=0, kernel=None, want_lists=True):
    hnd = hip_scene(gpu, objs, cam=cam, **_config(gpu, kind, lens, spp, tuning, kernel)).upload(0, lab=True)
    try:
        img, st = _frame(hnd, frame)
        return img, st, (hnd.debug_tile_lists() if want_lists else None)
    finally:
        hnd.close()


def check_structure(gpu, L, kind, frame, pk):
    w, h, band = frame
    tx, ty, _ = tc.tile_grid(w, h, band)
    assert L["form"] == (1 if kind == "spheres" else 2) and L["tiles_x"] == tx and L["n_tiles"] == tx * ty
    assert L["cap"] == (tc.SPHERE_CAP if kind == "spheres" else tc.MESH_CAP)
    for t in range(L["n_tiles"]):
        c = int(L["count"][t])
        if c == gpu.TILE_LIST_WALK:
            continue
        assert c <= L["cap"], (t, c)
        tl, ob = L["t_lb"][t, :c], L["object"][t, :c]
        assert np.isfinite(tl).all() and (tl >= 0).all() and (np.diff(tl) >= 0).all(), (t, tl)
        assert (ob >= 0).all() and len(set(ob.tolist())) == c, (t, ob)
        assert pk["in_tree"][ob].all(), t
        rec = L["is_record"][t, :c]
        assert ((pk["kind"][ob] == 2) == rec).all(), t                       # filter records are triangles, the others spheres
        if kind == "spheres":                                                # {c - centre, |r| rounded up}: the independent pack's bits
            assert np.array_equal(L["raw"][t, :c, :4], pk["rec"][ob][:, :4].view(np.uint32)), t
            assert np.array_equal(L["raw"][t, :c, 5].view(np.float32), tl) and not L["raw"][t, :c, 6:].any()


def check_property(gpu, L, ep, label, must_list):
    """the property over the reported pairs ep; returns the figures profiles/tile_list_property.txt records"""
    count = L["count"]
    walk = count == gpu.TILE_LIST_WALK
    if must_list:
        assert not walk.any(), (label, np.nonzero(walk)[0])
    where = [{int(o): k for k, o in enumerate(L["object"][t, :int(count[t])])} if not walk[t] else None for t in range(L["n_tiles"])]
    looked, slack = 0, np.inf
    for tile, obj, t in zip(ep["tile"].tolist(), ep["object"].tolist(), ep["t"].tolist()):
        if where[tile] is None:
            continue
        k = where[tile].get(obj)
        assert k is not None, "%s: tile %d, object %d, t = %r: absent from the list" % (label, tile, obj, t)
        t_lb = float(L["t_lb"][tile, k])
        assert t_lb <= t, "%s: tile %d, object %d, t = %r: t_lb = %r overshoots" % (label, tile, obj, t, t_lb)
        looked += 1
        slack = min(slack, (t - t_lb) / t)
    assert looked > 0 or not must_list, label
    have = ~walk
    fig = dict(case=label, tiles=int(L["n_tiles"]), with_lists=int(have.sum()), entries_min=int(count[have].min()) if have.any() else 0,
               entries_max=int(count[have].max()) if have.any() else 0, entries_mean=float(count[have].mean()) if have.any() else 0.0,
               pairs=looked, min_slack=float(slack))
    print("TILE_LIST_PROPERTY %(case)s tiles %(tiles)d with_lists %(with_lists)d entries %(entries_min)d..%(entries_max)d mean %(entries_mean).1f "
          "pairs %(pairs)d min_(t-t_lb)/t %(min_slack).3e" % fig)
    return fig


@pytest.mark.gpu
@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_lists_hold_every_shape_the_text_reports(gpu, case):
    camera, kind, frame = case
    objs, _ = tc.scene(*case)
    cam, lens = tc.CAMERAS[camera]
    _, st, L = _render(gpu, objs, cam, lens, tc.FRAMES[frame], kind)
    assert _packets_ran(gpu, kind, st), (st.kernel, st.stage1_ms)
    check_structure(gpu, L, kind, tc.FRAMES[frame], bm.pack_for(objs))
    check_property(gpu, L, tc.expected_pairs(*case), "-".join(case), must_list=True)


def _row_of_shapes(gpu, what, n, tile=4):
    """n small shapes along the central ray of one tile of the 24 x 16 bench frame"""
    cam, lens = tc.CAMERAS["bench"]
    w, h, band = tc.FRAMES["whole"]
    X, Y = tc.tile_pixels(w, h, band, tile)
    half = np.full((1, 3), 0.5)
    o, d, _ = tc.lens_rays(cam, lens, w, h, [0.5 * (X.min() + X.max())], [0.5 * (Y.min() + Y.max())], half, half)
    objs = np.zeros(n, dtype=gpu.OBJECT_DTYPE)
    m = tc._tilted_normal(d[0])
    e1 = tc._perp(m)
    for k, s in enumerate(np.linspace(6.0, 40.0, n)):
        P = o[0] + s * d[0]
        if what == "spheres":
            objs[k]["kind"] = 0
            objs[k]["geom"][:4] = (*P, 0.05)
        else:
            objs[k]["kind"] = 2
            objs[k]["geom"][:9] = tc._orient(tc._vertex_triangle(P, e1, np.cross(m, e1), 0.3, 0.3), d[0]).ravel()
    objs["base_color"] = 0.7
    objs["emission_color"][::3] = (1.0, 0.8, 0.6)
    return objs


def _fallback_cases(gpu):
    """(label, kind, objects, camera, lens, the tiles that must walk (None: every tile whose beam is degenerate))"""
    bench_cam, bench_lens = tc.CAMERAS["bench"]
    spheres, _ = tc.scene("bench", "spheres", "whole")
    mesh, _ = tc.scene("bench", "mesh", "partial")
    far = ((-1.0e15, 10.0, 5.0), (1.0, 0.0, 0.0), 1e-14)
    out = [("80 spheres behind one tile", "spheres", _row_of_shapes(gpu, "spheres", 80), bench_cam, bench_lens, [4]),
           ("600 records behind one tile", "mesh", _row_of_shapes(gpu, "mesh", 600), bench_cam, bench_lens, [4])]
    for kind, objs in (("spheres", spheres), ("mesh", mesh)):
        out += [("focal_length 0, " + kind, kind, objs, bench_cam, (0.0, 1e-4, 0.1), None),
                ("|focal_length| < non_focal_offset, " + kind, kind, objs, bench_cam, (0.3, 1e-4, 1.0), None),
                ("a camera 1e15 away, " + kind, kind, objs, far, bench_lens, "all")]
    return out


@pytest.mark.gpu
def test_fallbacks_happen_and_are_harmless(gpu):
    """Where the builder must give up -- a list over its cap (64 spheres, 512 records), a degenerate beam (the origin box meets the
    target box), a camera beyond the range its allowance was derived for (S >= 1e14) -- the tile answers WALK, and the frame equals the
    exhaustive kernel's and the packets' own walks' (RTX_TUNE_NO_TILE_LISTS) bit for bit."""
    frame = tc.FRAMES["whole"]
    w, h, band = frame
    for label, kind, objs, cam, lens, walkers in _fallback_cases(gpu):
        img, st, L = _render(gpu, objs, cam, lens, frame, kind, spp=2)
        assert _packets_ran(gpu, kind, st) and L["form"] != 0, label
        gaps = np.array([tc.beam_boxes(cam, lens, w, h, band, t)[4] for t in range(L["n_tiles"])])
        if walkers is None:
            walkers = np.nonzero(gaps == 0.0)[0].tolist()
            assert walkers, label
        elif walkers == "all":
            walkers = list(range(L["n_tiles"]))
        else:
            assert (gaps > 0).all(), label                   # (the cap is the only reason to give up)
        for t in walkers:
            assert L["count"][t] == gpu.TILE_LIST_WALK, (label, t, int(L["count"][t]))
        print("TILE_LIST_FALLBACK %s: %d of %d tiles walk" % (label, int((L["count"] == gpu.TILE_LIST_WALK).sum()), L["n_tiles"]))
        for other, kern, tune in (("exact", gpu.RTX_KERNEL_EXACT, 0), ("walks", None, gpu.RTX_TUNE_NO_TILE_LISTS)):
            ref, rst, _ = _render(gpu, objs, cam, lens, frame, kind, spp=2, tuning=tune, kernel=kern, want_lists=False)
            assert np.array_equal(img, ref, equal_nan=True) and st.segments == rst.segments, (label, other)


def _moved(objs, j, geom):
    new = np.array(objs[[j]], copy=True)
    new["geom"][0, :len(geom)] = geom
    now = np.array(objs, copy=True)
    now[j] = new[0]
    return new, now


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spheres", "joint"])
def test_resident_scenes_keep_the_property(gpu, kind):
    """Every render call rebuilds its lists from the scene as it is NOW: after set_camera, after update_objects moves an aimed sphere
    into another tile's margin (the refit path), after RTX_UPDATE_DEFORM of an aimed triangle (the joint scene; a sphere scene holds
    none), after hide and after show, the next render's lists have the property for the current scene and camera."""
    case = ("bench", kind, "whole" if kind == "spheres" else "band")
    frame = tc.FRAMES[case[2]]
    objs, aimed = tc.scene(*case)
    cam, lens = tc.CAMERAS["bench"]
    pk = bm.pack_for(objs)                                   # (in-place updates keep origin_limit and the in-tree flags)
    hnd = hip_scene(gpu, objs, cam=cam, **_config(gpu, kind, lens)).upload(0, lab=True)
    try:
        def step(label, now, camera):
            _, st = _frame(hnd, frame)
            assert _packets_ran(gpu, kind, st), label
            L = hnd.debug_tile_lists()
            assert L["form"] == (1 if kind == "spheres" else 2)
            check_property(gpu, L, tc.pairs_for(now, camera, lens, *frame, pk=pk), "%s, %s" % (kind, label), must_list=True)

        step("as uploaded", objs, cam)
        cam2 = ((0.4, -0.3, 0.2), (1.0, 0.15, -0.1), 1.3)
        hnd.set_camera(gpu.Camera(*cam2))
        step("set_camera", objs, cam2)
        hnd.set_camera(gpu.Camera(*cam))
        # an aimed sphere of one tile moves to the place of an aimed sphere of another tile, a little smaller
        sph = [a for a in aimed if a["cls"] == "sphere"]
        a, b = sph[0], next(s for s in sph if s["tile"] != sph[0]["tile"])
        g = np.array(objs["geom"][b["object"]][:4])
        g[3] *= 0.9
        new, now = _moved(objs, a["object"], g)
        assert hnd.update_objects([a["object"]], new) == "refit"
        step("update_objects (refit)", now, cam)
        if kind == "joint":
            tri = next(t for t in aimed if t["cls"] == "vertex")
            v = now["geom"][tri["object"]][:9].reshape(3, 3)
            new, now = _moved(now, tri["object"], (v[0] + 0.8 * (v - v[0])).ravel())      # shrunk towards its right-angle vertex
            assert hnd.update_objects([tri["object"]], new, mode="deform") == "refit"
            step("RTX_UPDATE_DEFORM", now, cam)
        gone = [sph[1]["object"], sph[2]["object"]]
        hidden = np.array(now, copy=True)
        hidden["geom"][gone] = np.nan                        # (include/rtx_hip.h: a hidden object is its list entry with NaN geometry)
        hnd.hide(gone)
        step("hide", hidden, cam)
        hnd.show(gone)
        step("show", now, cam)
    finally:
        hnd.close()


@pytest.mark.gpu
def test_aimed_scenes_through_the_real_path(gpu):
    """The aimed scenes at 4 spp: with lists == the packets' own walks == the exhaustive kernel, image and segment count; and the
    lists were USED: fewer box tests than the walks."""
    for case in tc.CASES:
        camera, kind, frame = case
        objs, _ = tc.scene(*case)
        cam, lens = tc.CAMERAS[camera]
        a, sa, _ = _render(gpu, objs, cam, lens, tc.FRAMES[frame], kind, spp=4, want_lists=False)
        b, sb, _ = _render(gpu, objs, cam, lens, tc.FRAMES[frame], kind, spp=4, tuning=gpu.RTX_TUNE_NO_TILE_LISTS, want_lists=False)
        e, se, _ = _render(gpu, objs, cam, lens, tc.FRAMES[frame], kind, spp=4, kernel=gpu.RTX_KERNEL_EXACT, want_lists=False)
        assert _packets_ran(gpu, kind, sa) and _packets_ran(gpu, kind, sb), case
        assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, e, equal_nan=True), case
        assert sa.segments == sb.segments == se.segments, case
        if kind == "spheres":
            assert sa.stage1_box_tests < sb.stage1_box_tests, (case, sa.stage1_box_tests, sb.stage1_box_tests)
        else:
            assert sa.box_tests < sb.box_tests, (case, sa.box_tests, sb.box_tests)
