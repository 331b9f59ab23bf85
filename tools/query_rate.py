#!/usr/bin/env python3
"""Closest-hit query rates (rtx_scene_closest_hits / rtx_scene_primary_hits), in Mrays/s from RtxStats.trace_ms, on the scenes of the
benchmark's C2 (10k spheres), C3 (100k triangles) and J1 (5k spheres + 50k triangles: a joint tree), built with scenes.py's
generators and the same parameters:

  incoherent   2^24 rays, origins uniform in the scene's box, unit directions uniform on the sphere (the tree walk)
  pick         the 1920x1080 pick buffer (rtx_scene_primary_hits)
  exact        the incoherent set with RTX_KERNEL_EXACT (every shape of every ray in f64)

    tools/query_rate.py [--rays 24] [--scenes C2,C3,J1] [--reps 3] [--exact-rays 20]

The exact leg runs 2^--exact-rays of the rays (the sweep is ~n_objects tests per ray) and reports its rate on those.  One JSON line per
scene and leg; the best of --reps timed runs after one warm-up.
"""
import argparse
import json
import os
import sys

import numpy as np

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=24, help="log2 of the incoherent set's size")
    ap.add_argument("--exact-rays", type=int, default=20, help="log2 of the rays the exact leg runs")
    ap.add_argument("--scenes", default="C2,C3,J1")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    import rust_raytracing_amd as rtx
    from rust_raytracing_amd import scenes
    dev = torch.device("cuda", 0)
    n = 1 << args.rays
    for name in args.scenes.split(","):
        objs = SCENES[name](scenes)
        o, d = incoherent(objs, n)
        rays = rtx.make_rays(o, d)
        d_rays = torch.from_numpy(rays.view(np.uint8)).to(dev)
        d_hits = torch.empty(n * 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)

        def best(fn):
            fn()
            runs = [fn() for _ in range(args.reps)]
            return min(runs, key=lambda s: s.trace_ms)

        for leg, kernel in (("incoherent", rtx.RTX_KERNEL_AUTO), ("pick", rtx.RTX_KERNEL_AUTO), ("exact", rtx.RTX_KERNEL_EXACT)):
            hnd = rtx.Scene.from_packed(rtx.Config(rays_per_pixel=1, kernel=kernel), rtx.Camera(*scenes.CAMERA), objs).upload(0)
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
                              "hit_fraction": round(float((hits["object"] >= 0).mean()), 4)}), flush=True)
            hnd.close()


if __name__ == "__main__":
    main()
