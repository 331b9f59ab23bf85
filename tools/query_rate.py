#!/usr/bin/env python3
"""Closest-hit, any-hit, path, feature, sample and refinement query rates (rtx_scene_closest_hits / rtx_scene_primary_hits / rtx_scene_any_hits /
rtx_scene_trace_paths / rtx_scene_pixel_features / rtx_scene_trace_samples / rtx_render_blocks_accumulate / rtx_render_blocks_refine), in Mrays/s (the path legs: Msegments/s) from RtxStats.trace_ms, on the scenes of the
benchmark's C2 (10k spheres), C3 (100k triangles) and J1 (5k spheres + 50k triangles: a joint tree), built with scenes.py's
generators and the same parameters:

  incoherent   2^24 rays, origins uniform in the scene's box, unit directions uniform on the sphere (the tree walk)
  pick         the 1920x1080 pick buffer (rtx_scene_primary_hits)
  exact        the incoherent set with RTX_KERNEL_EXACT (every shape of every ray in f64)
  any          rtx_scene_any_hits on the incoherent set, t_max = +inf (any hit at all)
  any_short    the same with t_max = 1.0 (the median closest distance in these boxes is ~25)
  any_aimed    t_max = +inf on rays with the incoherent set's origins, each aimed at a random sphere centre / triangle centroid
  paths        rtx_scene_trace_paths on the incoherent set at the scene's config (max_bounces = 10), ids (i, 0)
  paths_1seg   the same rays at max_bounces = 0: one segment per path -- against `incoherent`, the price of the shade and the refill
  paths_pick   the 1920x1080 zero-offset primary rays (built on the host from the camera) with ids (pixel, 0)
  render_pick  rtx_render_rows of the same frame at 1 spp with both offsets 0: paths_pick's segments, with the render's tile packets
  paths_primary  paths_pick's rays and ids at max_bounces = 0: one segment per pixel -- what a `features` sample does, plus reading a
               48-byte ray and writing 24 bytes per ray
  features     rtx_scene_pixel_features of the 1920x1080 frame with the bench camera and the default offsets, at 1 and at 16 samples
               per pixel (two lines): one segment per (pixel, sample), the ray built on the device, one 96-byte record per pixel
  accumulate   the 1920x1080 frame at --spp samples (the benchmark's 64): rtx_render_blocks, then rtx_render_blocks_accumulate in one
               call with and without d_sum_sq and in four calls of a quarter each (four lines; trace_ms and resolve_ms summed over the
               calls) -- the same launches minus the division, and the price of splitting
  samples_frame  rtx_scene_trace_samples, sample 0 of every pixel of the 1920x1080 frame with the default offsets, at max_bounces = 10
               and at 0 (two lines; the second is what `features` at 1 spp and `paths_primary` trace), and rtx_render_rows of the frame
               at 1 spp (the same samples through the render's tiles and packets)
  samples_sparse  a random tenth of the frame's pixels, samples 0..7 of each, sample-major: per sample against samples_frame
  multi1, multi4, multi16   rtx_scene_multi_hits on the incoherent set at k = 1, 4, 16: the k nearest objects of each ray, sorted (no limit)
  multi4_pick  rtx_scene_primary_multi_hits of the 1920x1080 pick buffer at k = 4
  peel4        the same four layers the old way, for 32 rays: hide(winners so far) + closest_hits + show per layer and ray -- wall time
  refine       the 1920x1080 frame with the bench camera: rtx_render_blocks_accumulate of 8 samples, then ONE rtx_render_blocks_refine
               call to max_samples = 64 (8 samples per round, 7 rounds, threshold 0.5, floor 0.01: on C2 the oracle's samples of twelve
               rows of the frame leave 14 % of the pixels selected after the base; 0.4 leaves 15 %, 0.6 6 %), against
               the same refinement as 7 calls of one round each and
               rtx_scene_trace_samples over the identical (pixel, sample) list, sample-major -- alternating, two runs each, each the best
               of --reps after a warm-up: pixels refined, samples traced, ms and ns per sample

    tools/query_rate.py [--rays 24] [--scenes C2,C3,J1] [--reps 3] [--exact-rays 20] [--legs incoherent,pick,...]

The library is the package's (RTX_HIP_LIB selects another build, e.g. one of the parent commit: the legs it lacks are then skipped).

The exact leg runs 2^--exact-rays of the rays (the sweep is ~n_objects tests per ray) and reports its rate on those.  One JSON line per
scene and leg; the best of --reps timed runs after one warm-up.  Every line of a query leg also carries the timed call's raw counters
(segments, exact_tests, filter_tests, box_tests) and the sha256 of the buffers it wrote: equal between two builds of the library that
compute the same thing, since a lane's work depends only on its own ray.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SCENES = {                                   # (bench.py CONFIGS: the same generators, seeds and boxes)
    "C2": lambda s: s.random_spheres(10000, 1, box=1.0),
    "C3": lambda s: s.random_triangles(100000, 2, box=1.0),
    "J1": lambda s: np.concatenate([s.random_spheres(5000, 4, box=1.0), s.random_triangles(50000, 5, box=1.0)]),
}


def incoherent(objs, n, seed=1):
    rng = np.random.default_rng(seed)
    g = objs["geom"]
    pts = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3)])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    o = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d


def aimed(objs, o, seed=2):
    """unit directions from the origins o toward a random sphere centre or triangle centroid each"""
    rng = np.random.default_rng(seed)
    g = objs["geom"]
    targets = np.concatenate([g[objs["kind"] == 0][:, :3], g[objs["kind"] == 2][:, :9].reshape(-1, 3, 3).mean(axis=1)])
    d = targets[rng.integers(0, len(targets), len(o))] - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return d


def primary_rays(rtx, cam, width, height):
    """the zero-offset primary ray of every pixel (scene.rs:196-222 with focal_offset = non_focal_offset = 0), row-major"""
    c = rtx.Camera(*cam)
    m = np.array(c._to_world, dtype=np.float64).reshape(3, 3)
    ax = c.fov * (np.arange(width) / width - 0.5)
    ay = (height / width * c.fov) * (np.arange(height) / height - 0.5)
    v = np.stack([np.broadcast_to(np.sin(ax)[None, :], (height, width)), np.broadcast_to(np.sin(ay)[:, None], (height, width)),
                  np.cos(ax)[None, :] * np.cos(ay)[:, None]], axis=2).reshape(-1, 3)
    d = v @ m.T                                                        # mat/mul.rs:42-50: rhs.dot(row)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.broadcast_to(np.array(list(c.position), dtype=np.float64), d.shape), d


def raw_counts(st):
    """the launch counters of the timed call as they are, for comparing two builds of the library: a lane's work depends only on its ray"""
    return {"segments": int(st.segments), "exact_tests": int(st.exact_tests), "filter_tests": int(st.filter_tests), "box_tests": int(st.box_tests)}


def digest(*tensors):
    """sha256 of what the timed call wrote: the bytes of the device tensors in the order given, read back in 256 MiB pieces.
    Outside the timed call, but every byte crosses to the host: 1 GiB per line of the 2^24-ray closest-hit legs, 4 GiB for multi4 and
    16 GiB for multi16 -- seconds per line, most of these legs' wall time."""
    h = hashlib.sha256()
    for t in tensors:
        b = t.contiguous().view(torch.uint8).reshape(-1)
        for at in range(0, b.numel(), 1 << 28):
            h.update(b[at:at + (1 << 28)].cpu().numpy())
    return h.hexdigest()


LEGS = ("incoherent", "pick", "exact", "any", "any_short", "any_aimed", "paths", "paths_1seg", "paths_pick", "render_pick", "paths_primary",
        "features", "accumulate", "samples_frame", "samples_sparse", "refine", "multi1", "multi4", "multi16", "multi4_pick", "peel4")
REFINE = dict(base=8, step=8, cap=64, threshold=0.5, floor=0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=24, help="log2 of the incoherent set's size")
    ap.add_argument("--exact-rays", type=int, default=20, help="log2 of the rays the exact leg runs")
    ap.add_argument("--scenes", default="C2,C3,J1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--spp", type=int, default=64, help="samples per pixel of the accumulate leg's frame")
    args = ap.parse_args()

    import rust_raytracing_amd as rtx
    from rust_raytracing_amd import scenes
    dev = torch.device("cuda", 0)
    n = 1 << args.rays
    legs = [l for l in args.legs.split(",") if l]
    assert all(l in LEGS for l in legs), legs
    if os.environ.get("RTX_HIP_LIB"):           # maybe a build of an older commit: bind what it exports, skip the legs it lacks
        import ctypes
        rtx.abi._share_hip_runtime_with_torch()
        probe = ctypes.CDLL(rtx.abi.LIB_PATH)
        rtx.abi.SYMBOLS[:] = [sym for sym in rtx.abi.SYMBOLS if hasattr(probe, sym[0])]
        if not hasattr(probe, "rtx_scene_any_hits"):
            legs = [l for l in legs if not l.startswith("any")]
        if not hasattr(probe, "rtx_scene_trace_paths"):
            legs = [l for l in legs if not l.startswith("paths")]
        if not hasattr(probe, "rtx_scene_pixel_features"):
            legs = [l for l in legs if l != "features"]
        if not hasattr(probe, "rtx_scene_trace_samples"):
            legs = [l for l in legs if not l.startswith("samples")]
        if not hasattr(probe, "rtx_render_blocks_refine"):
            legs = [l for l in legs if l != "refine"]
        if not hasattr(probe, "rtx_scene_multi_hits"):
            legs = [l for l in legs if not l.startswith("multi") and l != "peel4"]
        have_accumulate = hasattr(probe, "rtx_render_blocks_accumulate")
    else:
        have_accumulate = True
    for name in args.scenes.split(","):
        objs = SCENES[name](scenes)
        o, d = incoherent(objs, n)
        rays = rtx.make_rays(o, d)
        d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
        W, H = 1920, 1080
        d_hits = torch.empty(max(n * 64, W * H * 96), dtype=torch.uint8, device=dev)      # (the frame legs' records fit whatever --rays)
        d_aimed = d_lim = d_prim = d_prim_ids = None
        if "paths_pick" in legs or "paths_primary" in legs:
            d_prim = torch.from_numpy(rtx.make_rays(*primary_rays(rtx, scenes.CAMERA, W, H)).view(np.uint8)).to(dev)
            d_prim_ids = torch.stack([torch.arange(W * H, dtype=torch.int64, device=dev), torch.zeros(W * H, dtype=torch.int64, device=dev)], dim=1).contiguous()
        if "any_aimed" in legs:
            d_aimed = torch.from_numpy(rtx.make_rays(o, aimed(objs, o)).view(np.uint8)).to(dev)
        if "any_short" in legs:
            d_lim = torch.full((n,), 1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)

        def best(fn):
            fn()
            runs = [fn() for _ in range(args.reps)]
            return min(runs, key=lambda s: s.trace_ms)

        for leg in legs:
            kernel = rtx.RTX_KERNEL_EXACT if leg == "exact" else rtx.RTX_KERNEL_AUTO
            cfg = rtx.Config(rays_per_pixel=1, kernel=kernel, max_bounces=0 if leg in ("paths_1seg", "paths_primary") else 10)
            if leg == "features":
                k = W * H
                for spp in (1, 16):
                    hnd = rtx.Scene.from_packed(cfg.with_rays_per_pixel(spp), rtx.Camera(*scenes.CAMERA), objs).upload(0)
                    st = best(lambda: hnd.pixel_features(W, H, d_hits.data_ptr()))           
                    f = d_hits[:k * 96].cpu().numpy().view(rtx.FEATURE_DTYPE)
                    print(json.dumps({"scene": name, "leg": leg, "spp": spp, "rays": int(st.segments), "trace_ms": round(st.trace_ms, 3),
                                      "mrays_per_s": round(st.segments / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                      "exact_tests_per_ray": round(st.exact_tests / st.segments, 2),
                                      "box_tests_per_ray": round(st.box_tests / st.segments, 2),
                                      "coverage": round(float(f["coverage"].mean()), 4), **raw_counts(st), "sha256": digest(d_hits[:k * 96])}), flush=True)
                    hnd.close()
                continue
            if leg == "accumulate":
                hnd = rtx.Scene.from_packed(cfg.with_rays_per_pixel(args.spp), rtx.Camera(*scenes.CAMERA), objs).upload(0)
                d_sum = d_hits.view(torch.float64)[:3 * W * H]
                d_sq = d_hits.view(torch.float64)[3 * W * H:6 * W * H]

                def calls(parts, moments):
                    """one frame's samples in `parts` calls: the stats of the calls added up"""
                    d_sum.zero_()
                    d_sq.zero_()
                    torch.cuda.synchronize(dev)
                    tot = None
                    for q in range(parts):
                        a, b = args.spp * q // parts, args.spp * (q + 1) // parts
                        st = hnd.render_accumulate(W, H, a, b - a, d_sum.data_ptr(), d_sq.data_ptr() if moments else None)
                        if tot is None:
                            tot = st
                        else:
                            tot.trace_ms += st.trace_ms; tot.resolve_ms += st.resolve_ms; tot.trace_launches += st.trace_launches
                            tot.segments += st.segments; tot.primary_rays += st.primary_rays
                    return tot

                forms = [("render_blocks", lambda: hnd.render_blocks(W, H, 8, 0, 1, d_sum.data_ptr()))]
                if have_accumulate:
                    forms += [("one call", lambda: calls(1, True)), ("one call, no d_sum_sq", lambda: calls(1, False)),
                              ("four calls", lambda: calls(4, True))]
                for form, fn in forms:
                    fn()
                    st = min((fn() for _ in range(args.reps)), key=lambda s: s.trace_ms + s.resolve_ms)
                    print(json.dumps({"scene": name, "leg": leg, "form": form, "spp": args.spp, "rays": int(st.primary_rays),
                                      "trace_ms": round(st.trace_ms, 3), "resolve_ms": round(st.resolve_ms, 3),
                                      "mrays_per_s": round(st.primary_rays / ((st.trace_ms + st.resolve_ms) * 1e-3) / 1e6, 1),
                                      "launches": int(st.trace_launches), "kernel": int(st.kernel)}), flush=True)
                hnd.close()
                continue
            if leg.startswith("samples"):
                d_rgb = d_hits.view(torch.float64)
                if leg == "samples_frame":
                    k = W * H
                    d_ids = torch.stack([torch.arange(k, dtype=torch.int64, device=dev), torch.zeros(k, dtype=torch.int64, device=dev)], dim=1).contiguous()
                else:
                    pix = torch.from_numpy(np.sort(np.random.default_rng(9).permutation(W * H)[:W * H // 10])).to(dev)
                    k = 8 * int(pix.numel())
                    d_ids = torch.stack([pix.repeat(8), torch.arange(8, dtype=torch.int64, device=dev).repeat_interleave(pix.numel())], dim=1).contiguous()
                torch.cuda.synchronize(dev)
                for bounces in ((10, 0) if leg == "samples_frame" else (10,)):
                    hnd = rtx.Scene.from_packed(cfg.with_max_bounces(bounces), rtx.Camera(*scenes.CAMERA), objs).upload(0)
                    st = best(lambda: hnd.trace_samples(W, H, d_ids.data_ptr(), k, d_rgb.data_ptr()))
                    print(json.dumps({"scene": name, "leg": leg, "max_bounces": bounces, "samples": k, "segments": int(st.segments),
                                      "trace_ms": round(st.trace_ms, 3), "msamples_per_s": round(k / (st.trace_ms * 1e-3) / 1e6, 1),
                                      "msegments_per_s": round(st.segments / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                      "segments_per_sample": round(st.segments / k, 3),
                                      "lit_fraction": round(float((d_rgb[:3 * k].view(-1, 3) != 0).any(dim=1).float().mean().item()), 4),
                                      **raw_counts(st), "sha256": digest(d_rgb[:3 * k])}), flush=True)
                    if leg == "samples_frame" and bounces == 10:
                        st = best(lambda: hnd.render_rows(W, H, 0, 1, H, d_rgb.data_ptr()))
                        print(json.dumps({"scene": name, "leg": leg, "form": "render_rows at 1 spp", "samples": k, "segments": int(st.segments),
                                          "trace_ms": round(st.trace_ms, 3), "resolve_ms": round(st.resolve_ms, 3),
                                          "msamples_per_s": round(k / (st.trace_ms * 1e-3) / 1e6, 1),
                                          "msegments_per_s": round(st.segments / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel)}), flush=True)
                    hnd.close()
                continue
            if leg == "refine":
                k, r = W * H, REFINE
                hnd = rtx.Scene.from_packed(cfg, rtx.Camera(*scenes.CAMERA), objs).upload(0)
                d_sums = d_hits.view(torch.float64)[:6 * k]                          # d_sum, then d_sum_sq
                d_extra = torch.zeros(k, dtype=torch.int32, device=dev)
                d_sums.zero_()
                torch.cuda.synchronize(dev)
                st_base = hnd.render_accumulate(W, H, 0, r["base"], d_sums.data_ptr(), d_sums[3 * k:].data_ptr())
                d_base = d_sums.clone()
                rounds = (r["cap"] - r["base"] + r["step"] - 1) // r["step"]
                counts = [None]

                def refine():
                    d_sums.copy_(d_base)
                    d_extra.zero_()
                    torch.cuda.synchronize(dev)
                    counts[0], st = hnd.render_refine(W, H, r["base"], r["step"], r["cap"], r["threshold"], r["floor"], d_sums.data_ptr(),
                                                      d_sums[3 * k:].data_ptr(), d_extra.data_ptr(), rounds=rounds)
                    return st

                def refine_calls():
                    """the same refinement as `rounds` calls of one round each: a launch per round"""
                    d_sums.copy_(d_base)
                    d_extra.zero_()
                    torch.cuda.synchronize(dev)
                    tot = None
                    for _ in range(rounds):
                        c, st = hnd.render_refine(W, H, r["base"], r["step"], r["cap"], r["threshold"], r["floor"], d_sums.data_ptr(),
                                                  d_sums[3 * k:].data_ptr(), d_extra.data_ptr(), rounds=1)
                        if tot is None:
                            tot = st
                        else:
                            tot.trace_ms += st.trace_ms; tot.segments += st.segments; tot.primary_rays += st.primary_rays
                            tot.trace_launches += st.trace_launches
                            tot.exact_tests += st.exact_tests; tot.filter_tests += st.filter_tests; tot.box_tests += st.box_tests
                    assert tot.primary_rays == counts[0][1] and c[2] == 0, (tot.primary_rays, c)
                    return tot

                refine()
                extra = d_extra.cpu().numpy()
                top = int(extra.max())
                pix = [np.nonzero(extra > s)[0] for s in range(top)]                 # sample-major: the pixels that got sample base + s
                ids = np.concatenate([np.stack([p_, np.full(len(p_), r["base"] + s)], axis=1) for s, p_ in enumerate(pix)]).astype(np.int64)
                d_ids = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
                d_rgb = torch.empty(3 * len(ids), dtype=torch.float64, device=dev)
                torch.cuda.synchronize(dev)
                assert len(ids) == counts[0][1], (len(ids), counts[0])
                print(json.dumps({"scene": name, "leg": leg, "form": "base", "samples": int(st_base.primary_rays),
                                  "trace_ms": round(st_base.trace_ms, 3), "resolve_ms": round(st_base.resolve_ms, 3),
                                  "selected_after_base": round(float((extra > 0).mean()), 4), **r}), flush=True)
                for run in (1, 2):
                    for form, fn, wrote in (("rtx_render_blocks_refine", refine, (d_sums, d_extra)),
                                            ("rtx_render_blocks_refine, a call per round", refine_calls, (d_sums, d_extra)),
                                            ("rtx_scene_trace_samples", lambda: hnd.trace_samples(W, H, d_ids.data_ptr(), len(ids), d_rgb.data_ptr()),
                                             (d_rgb,))):
                        st = best(fn)
                        print(json.dumps({"scene": name, "leg": leg, "form": form, "run": run, "pixels": counts[0][0], "samples": len(ids),
                                          "still_selected": counts[0][2], "segments": int(st.segments), "trace_ms": round(st.trace_ms, 3),
                                          "ns_per_sample": round(st.trace_ms * 1e6 / len(ids), 3),
                                          "msegments_per_s": round(st.segments / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                          **raw_counts(st), "sha256": digest(*wrote)}), flush=True)
                hnd.close()
                continue
            if leg == "render_pick":
                cfg = cfg.with_focal_offset(0.0).with_non_focal_offset(0.0)
            hnd = rtx.Scene.from_packed(cfg, rtx.Camera(*scenes.CAMERA), objs).upload(0)
            if leg.startswith("paths") or leg == "render_pick":
                d_rgb = d_hits.view(torch.float64)                       # (n * 8 doubles: room for 3 per ray or pixel)
                if leg in ("paths_pick", "paths_primary"):
                    k = W * H
                    st = best(lambda: hnd.trace_paths(d_prim.data_ptr(), d_prim_ids.data_ptr(), k, d_rgb.data_ptr()))
                elif leg == "render_pick":
                    k = W * H
                    st = best(lambda: hnd.render_rows(W, H, 0, 1, H, d_rgb.data_ptr()))
                else:
                    k = n
                    st = best(lambda: hnd.trace_paths(d_rays.data_ptr(), None, k, d_rgb.data_ptr()))
                print(json.dumps({"scene": name, "leg": leg, "rays": k, "segments": int(st.segments), "trace_ms": round(st.trace_ms, 3),
                                  "msegments_per_s": round(st.segments / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                  "segments_per_ray": round(st.segments / k, 3), "exact_tests_per_ray": round(st.exact_tests / k, 2),
                                  "box_tests_per_ray": round(st.box_tests / k, 2),
                                  "lit_fraction": round(float((d_rgb[:3 * k].view(-1, 3) != 0).any(dim=1).float().mean().item()), 4),
                                  **raw_counts(st), "sha256": digest(d_rgb[:3 * k])}), flush=True)
                hnd.close()
                continue
            if leg.startswith("any"):
                k = n
                src = d_aimed if leg == "any_aimed" else d_rays
                lim = d_lim.data_ptr() if leg == "any_short" else None
                st = best(lambda: hnd.any_hits(src.data_ptr(), lim, k, d_hits.data_ptr()))
                print(json.dumps({"scene": name, "leg": leg, "rays": k, "trace_ms": round(st.trace_ms, 3),
                                  "mrays_per_s": round(k / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                  "exact_tests_per_ray": round(st.exact_tests / k, 2), "box_tests_per_ray": round(st.box_tests / k, 2),
                                  "occluded_fraction": round(float(d_hits[:k].float().mean().item()), 4),
                                  **raw_counts(st), "sha256": digest(d_hits[:k])}), flush=True)
                hnd.close()
                continue
            if leg.startswith("multi"):
                kk = int(leg[5:].split("_")[0])
                k = W * H if leg.endswith("_pick") else n
                d_multi = torch.empty(k * kk * 64, dtype=torch.uint8, device=dev)           # (multi16 of 2^24 rays: 16 GiB)
                d_cnt = torch.empty(k, dtype=torch.int32, device=dev)
                if leg.endswith("_pick"):
                    st = best(lambda: hnd.primary_multi_hits(W, H, kk, d_multi.data_ptr(), d_cnt.data_ptr()))
                else:
                    st = best(lambda: hnd.multi_hits(d_rays.data_ptr(), None, k, kk, d_multi.data_ptr(), d_cnt.data_ptr()))
                cnt = d_cnt.cpu().numpy()
                print(json.dumps({"scene": name, "leg": leg, "k": kk, "rays": k, "trace_ms": round(st.trace_ms, 3),
                                  "mrays_per_s": round(k / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                                  "exact_tests_per_ray": round(st.exact_tests / k, 2), "box_tests_per_ray": round(st.box_tests / k, 2),
                                  "entries_per_ray": round(float(cnt.mean()), 3), "full_fraction": round(float((cnt == kk).mean()), 4),
                                  "empty_fraction": round(float((cnt == 0).mean()), 4), **raw_counts(st), "sha256": digest(d_multi, d_cnt)}), flush=True)
                del d_multi, d_cnt
                hnd.close()
                continue
            if leg == "peel4":
                # what a caller did before multi-hit queries: per ray and layer hide(the winners so far) + closest_hits + show -- a scene
                # edit and a launch per layer, one ray at a time (visibility is per scene).  Wall time, 32 rays that have 4 layers
                import time
                dist, obj, _, _, cnt = hnd.query_all(o[:4096], d[:4096], 4)
                rows = np.nonzero(cnt == 4)[0][:32]
                one = torch.empty(64, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for r in rows:
                    won = []
                    for layer in range(4):
                        if won:
                            hnd.hide(won)
                        hnd.closest_hits(d_rays.data_ptr() + 48 * int(r), 1, one.data_ptr())
                        if won:
                            hnd.show(won)
                        won.append(int(one.cpu().numpy().view(rtx.HIT_DTYPE)["object"][0]))
                    assert won == [int(v) for v in obj[r]], (r, won, obj[r])
                dt = time.perf_counter() - t0
                print(json.dumps({"scene": name, "leg": leg, "k": 4, "rays": int(len(rows)), "wall_ms": round(dt * 1e3, 3),
                                  "ms_per_ray": round(dt * 1e3 / max(len(rows), 1), 4)}), flush=True)
                hnd.close()
                continue
            if leg == "pick":
                k = 1920 * 1080
                st = best(lambda: hnd.primary_hits(1920, 1080, d_hits.data_ptr()))
            else:
                k = n if leg == "incoherent" else min(n, 1 << args.exact_rays)
                st = best(lambda: hnd.closest_hits(d_rays.data_ptr(), k, d_hits.data_ptr()))
            hits = d_hits[:k * 64].cpu().numpy().view(rtx.HIT_DTYPE)
            print(json.dumps({"scene": name, "leg": leg, "rays": k, "trace_ms": round(st.trace_ms, 3),
                              "mrays_per_s": round(k / (st.trace_ms * 1e-3) / 1e6, 1), "kernel": int(st.kernel),
                              "exact_tests_per_ray": round(st.exact_tests / k, 2), "box_tests_per_ray": round(st.box_tests / k, 2),
                              "hit_fraction": round(float((hits["object"] >= 0).mean()), 4), **raw_counts(st), "sha256": digest(d_hits[:k * 64])}), flush=True)
            hnd.close()


if __name__ == "__main__":
    main()
