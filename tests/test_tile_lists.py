"""The conditions the tile-list property test (tests/test_tile_lists_gpu.py) rests on, on the reference alone: no device.

tests/tile_list_cases.py generates, per camera and scene kind, the rays of every tile's family at its extremes and scenes whose
shapes only such rays reach.  For that to test anything the generator itself must be right:
  * every generated ray IS in the family (scene.rs:196-207): origin and target inside their boxes, the draws in [0, 1), the closed
    corner 1 - 2^-53 strictly inside;
  * the aimed shapes are reached: in every case at least half of them are reported by the f64 text for a generated ray of their own
    tile, and at least one reported shape has its centre (a triangle: every vertex) OUTSIDE the hull of the tile's pixel-centre rays
    -- the case is about the builder's margins (lens boxes, the widenings), not about its pixel hull alone;
  * the scenes stay under every cap, and every tile's beam is non-degenerate (gap > 0): the builder has no legitimate reason to give
    up, so "the tile walks" is not an answer in these cases;
  * the expected set {(tile, object, t)} is deterministic.  COUNTS holds, per case: objects, aimed shapes, aimed shapes reported,
    reported shapes outside the hull, rays generated, pairs reported:

      case                          objects aimed reported outside   rays  pairs
      bench-spheres-whole               41    36       36      36   4020   1037
      bench-mesh-partial                89    84       84      50   4020   7531
      bench-joint-band                  62    52       52      31   3350   2576
      inside-spheres-partial            44    36       36      35   4020   1128
      inside-mesh-band                  78    70       70      44   3350   4060
      inside-joint-whole                80    64       64      41   4020   4158
      down_z-spheres-band               45    40       40      39   3350  16955
      down_z-mesh-whole                 89    84       84      84   4020  69545
      down_z-joint-partial              52    42       42      42   4020  27400
      neg_focal-spheres-whole           41    36       36      36   4020    838
      neg_focal-mesh-partial            89    84       84      41   4020   8351
      neg_focal-joint-band              64    54       54      40   3350   3078
      neg_offsets-spheres-partial       41    36       36      36   4020    502
      neg_offsets-mesh-band             75    70       70      62   3350   3536
      neg_offsets-joint-whole           75    65       65      51   4020   3904
      pinhole-spheres-band              45    40       40      40     50     50
      pinhole-mesh-whole                89    84       78      25     60    160
      pinhole-joint-partial             73    63       58      21     60     97
      wide-spheres-whole                41    36       36      36   4020    547
      wide-mesh-partial                 89    84       84      71   4020   4873
      wide-joint-band                   63    53       53      50   3350   1582
      wide_focal-spheres-partial        41    36       36      36   4020    332
      wide_focal-mesh-band              75    70       70      70   3350   1677
      wide_focal-joint-whole            73    63       63      57   4020   2136

    (down_z: the camera's right and up vectors vanish, every pixel has the same ray and every tile the same beam -- each shape is
    seen from every tile.  pinhole: one ray per pixel; the shapes it misses have delta = 1/2, which puts a triangle's hit point at
    a = b = 1/2, ON the hypotenuse -- the text's rounding makes a + b a few ulps more than 1.  With a lens another draw of the same pixel
    hits.)"""
import numpy as np
import pytest

import bounds_model as bm
import closed_form as cf
import tile_list_cases as tc

COUNTS = {
    "bench-spheres-whole": (41, 36, 36, 36, 4020, 1037), "bench-mesh-partial": (89, 84, 84, 50, 4020, 7531),
    "bench-joint-band": (62, 52, 52, 31, 3350, 2576), "inside-spheres-partial": (44, 36, 36, 35, 4020, 1128),
    "inside-mesh-band": (78, 70, 70, 44, 3350, 4060), "inside-joint-whole": (80, 64, 64, 41, 4020, 4158),
    "down_z-spheres-band": (45, 40, 40, 39, 3350, 16955), "down_z-mesh-whole": (89, 84, 84, 84, 4020, 69545),
    "down_z-joint-partial": (52, 42, 42, 42, 4020, 27400), "neg_focal-spheres-whole": (41, 36, 36, 36, 4020, 838),
    "neg_focal-mesh-partial": (89, 84, 84, 41, 4020, 8351), "neg_focal-joint-band": (64, 54, 54, 40, 3350, 3078),
    "neg_offsets-spheres-partial": (41, 36, 36, 36, 4020, 502), "neg_offsets-mesh-band": (75, 70, 70, 62, 3350, 3536),
    "neg_offsets-joint-whole": (75, 65, 65, 51, 4020, 3904), "pinhole-spheres-band": (45, 40, 40, 40, 50, 50),
    "pinhole-mesh-whole": (89, 84, 78, 25, 60, 160), "pinhole-joint-partial": (73, 63, 58, 21, 60, 97),
    "wide-spheres-whole": (41, 36, 36, 36, 4020, 547), "wide-mesh-partial": (89, 84, 84, 71, 4020, 4873),
    "wide-joint-band": (63, 53, 53, 50, 3350, 1582), "wide_focal-spheres-partial": (41, 36, 36, 36, 4020, 332),
    "wide_focal-mesh-band": (75, 70, 70, 70, 3350, 1677), "wide_focal-joint-whole": (73, 63, 63, 57, 4020, 2136),
}


def _points(objs, j):
    g = objs["geom"][j]
    return g[:3].reshape(1, 3) if objs["kind"][j] == 0 else g[:9].reshape(3, 3)


def _reached(case):
    """(aimed shapes the text reports for a ray of their own tile, those of them wholly outside the tile's pixel-centre hull)"""
    objs, aimed = tc.scene(*case)
    ep = tc.expected_pairs(*case)
    cam, lens = tc.CAMERAS[case[0]]
    w, h, band = tc.FRAMES[case[2]]
    hit = set(zip(ep["tile"].tolist(), ep["object"].tolist()))
    rep = [a for a in aimed if (a["tile"], a["object"]) in hit]
    return rep, [a for a in rep if tc.outside_hull(cam, lens, w, h, band, a["tile"], _points(objs, a["object"]))]


def test_the_cases_cover_every_camera_kind_and_frame():
    assert len(tc.CASES) == 24 and set(COUNTS) == set(tc.IDS)
    for c in tc.CAMERAS:
        assert {k for cc, k, _ in tc.CASES if cc == c} == set(tc.KINDS)
        assert {f for cc, _, f in tc.CASES if cc == c} == set(tc.FRAMES)
    for k in tc.KINDS:
        assert {f for _, kk, f in tc.CASES if kk == k} == set(tc.FRAMES)
    # the frames: whole tiles, partial tiles on the right and at the bottom, a band of blocks whose local rows are not image rows
    assert tc.tile_grid(24, 16, None)[:2] == (3, 2) and tc.tile_grid(20, 12, None)[:2] == (3, 2)
    tx, ty, rows = tc.tile_grid(*tc.FRAMES["band"])
    assert (tx, ty) == (5, 1) and rows.tolist() == list(range(8, 16))
    assert len(tc.tile_pixels(20, 12, None, 5)[0]) == 4 * 4 and len(tc.tile_pixels(20, 12, None, 0)[0]) == 64


def test_every_generated_ray_is_in_the_family():
    assert tc.ONE_M < 1.0 and np.nextafter(1.0, 0.0) == tc.ONE_M
    for camera, (cam, lens) in tc.CAMERAS.items():
        fl, fo, nfo = lens
        for off in (fo, nfo):
            assert off == 0.0 or abs(tc.ONE_M * off) < abs(off)          # the closed corner stays strictly inside the box
        pos = np.asarray(cam[0])
        for frame, (w, h, band) in tc.FRAMES.items():
            tx, ty, rows = tc.tile_grid(w, h, band)
            for tile in range(tx * ty):
                r = tc.beam_rays(cam, lens, w, h, band, tile)
                X, Y = tc.tile_pixels(w, h, band, tile)
                mine = set(zip(X.tolist(), Y.tolist()))
                assert set(zip(r["px"].tolist(), r["py"].tolist())) <= mine          # the tile's own, existing pixels
                for x, y, _ in tc.boundary_pixels(w, h, band, tile):
                    assert (x, y) in mine
                assert {(int(X.min()), int(Y.min())), (int(X.max()), int(Y.max()))} <= set(zip(r["px"].tolist(), r["py"].tolist()))
                assert ((r["u1"] >= 0) & (r["u1"] < 1) & (r["u2"] >= 0) & (r["u2"] < 1)).all()
                omin, omax, tmin, tmax, _ = tc.beam_boxes(cam, lens, w, h, band, tile)
                assert ((r["o"] >= omin) & (r["o"] <= omax)).all() and ((r["target"] >= tmin) & (r["target"] <= tmax)).all()
                assert np.abs(np.linalg.norm(r["d"], axis=1) - 1.0).max() < 4e-16
                # the text's own lines, one ray at a time (closed_form.pixel_ray is the suite's restatement of get_ray_dir)
                for k in (0, len(r["px"]) // 2, len(r["px"]) - 1):
                    o = pos + r["u1"][k] * nfo
                    t = (pos + cf.pixel_ray(cam, w, h, float(r["px"][k]), float(r["py"][k])) * fl) + r["u2"][k] * fo
                    assert np.array_equal(o, r["o"][k]) and np.allclose(t, r["target"][k], rtol=0, atol=1e-14 * (1 + abs(fl)))
                if fo != 0.0 or nfo != 0.0:                   # all 64 corners of the two lens boxes, at every boundary pixel
                    c1, c2 = tc.lens_corners()
                    assert len({(tuple(a), tuple(b)) for a, b in zip(c1, c2)}) == 64
                    first = (r["px"] == r["px"][0]) & (r["py"] == r["py"][0])
                    assert first.sum() >= 64 + tc.N_INTERIOR


@pytest.mark.parametrize("case", tc.CASES, ids=tc.IDS)
def test_aimed_scenes_meet_the_generators_conditions(case):
    objs, aimed = tc.scene(*case)
    cam, lens = tc.CAMERAS[case[0]]
    w, h, band = tc.FRAMES[case[2]]
    pk = bm.pack_for(objs)
    n_sph, n_tri = int((objs["kind"] == 0).sum()), int((objs["kind"] == 2).sum())
    # the caps: a sphere list holds 64 entries, a mesh or joint list 512; the builder's budget (records + 4 per node visit) and its
    # 512-entry stack are out of reach of a tree over 300 records
    if case[1] == "spheres":
        assert n_tri == 0 and 4 < n_sph <= tc.MAX_SPHERES < tc.SPHERE_CAP
    else:
        assert n_sph + n_tri <= tc.MAX_RECORDS < tc.MESH_CAP and 5 * (n_sph + n_tri) < tc.MESH_BUDGET and n_sph + n_tri < tc.MESH_STACK
    if case[1] == "mesh":                                    # a pure (x, y)-footprint tree
        assert n_sph == 0 and pk["in_tree"].all() and (pk["free"] == 2).all()
    if case[1] == "joint":
        assert (pk["in_tree"] & (pk["kind"] == 0)).sum() > 4 and (pk["in_tree"] & (pk["free"] == 2)).sum() > 4
        if case[0] != "down_z":                              # (its rays are parallel to the planes x = const and y = const: no such faces)
            assert (pk["in_tree"] & (pk["free"] == 0)).sum() > 4 and (pk["in_tree"] & (pk["free"] == 1)).sum() > 4
    assert pk["in_tree"][[a["object"] for a in aimed]].all()
    tx, ty, _ = tc.tile_grid(w, h, band)
    for tile in range(tx * ty):                              # a non-degenerate beam in every tile: WALK is not a legitimate answer
        assert tc.beam_boxes(cam, lens, w, h, band, tile)[4] > 0.0, tile
    rep, out = _reached(case)
    assert 2 * len(rep) >= len(aimed) and len(out) >= 1, (len(aimed), len(rep), len(out))
    classes = {a["cls"] for a in aimed}
    assert classes <= {a["cls"] for a in rep}                # every class of aimed shape is reached
    if case[1] != "spheres":
        assert "phantom" in classes
        for a in aimed:                                      # the ray a phantom was aimed with meets its plane BEHIND the origin, at -s
            if a["cls"] == "phantom":
                o, d, _ = tc.lens_rays(cam, lens, w, h, [a["px"]], [a["py"]], a["u1"][None], a["u2"][None])
                v = objs["geom"][a["object"]][:9].reshape(3, 3)
                n = np.cross(v[1] - v[0], v[2] - v[0])
                t = (n @ (v[0] - o[0])) / (n @ d[0])
                assert t < 0 and abs(t + a["s"]) < 1e-9 * a["s"]
                if case[0] == "down_z":                      # (looking down the footprints' free axis the whole triangle lies behind it)
                    assert (((v - o[0]) @ d[0]) < 0).all()
    ep = tc.expected_pairs(*case)
    assert len(ep["t"]) > 0 and np.isfinite(ep["t"]).all() and (ep["t"] > 0).all()
    got = (len(objs), len(aimed), len(rep), len(out), ep["n_rays"], len(ep["t"]))
    assert got == COUNTS["%s-%s-%s" % case], got


def test_the_expected_pairs_are_deterministic():
    case = tc.CASES[1]
    a = tc.expected_pairs(*case)
    tc.expected_pairs.cache_clear(); tc.scene.cache_clear()
    b = tc.expected_pairs(*case)
    for k in ("tile", "object", "ray", "t"):
        assert np.array_equal(a[k], b[k]), k
