#!/usr/bin/env python3
"""What rewinding a pick buffer costs (rtx_rewind_hits_device, include/rtx_hip.h "Rewinding a pick buffer").

  rate     the 1920 x 1080 pick buffer (rtx_scene_primary_hits) of C2 (scenes.random_spheres(10000, 1)), device buffers throughout:
           milliseconds per call (device events around --reps calls after --warmup calls) with no sphere, 1 % of the spheres (every
           hundredth) and all of them moved by a third of a unit.  A call must move 128 B per hit -- the record in, the record out --
           so each is given as a share of the rate of a plain device copy (torch's copy kernel) of the same 128 B per hit between the
           SAME two buffers in the same run; the share of the hits that were rewound is reported with it.

    tools/rewind_rate.py [--reps 30] [--warmup 3] [--width 1920 --height 1080]

One JSON line per measurement.  Needs a gfx950 device; nothing falls back.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, reps, warmup):
    """milliseconds per call: device events around `reps` calls, after `warmup` calls"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def leg_rate(rtx, args):
    import torch
    from rust_raytracing_amd import scenes
    w, h = args.width, args.height
    n = w * h
    packed = scenes.random_spheres(10000, 1)
    hnd = rtx.Scene.from_packed(rtx.Config(rays_per_pixel=1, seed=scenes.RENDER_SEED), rtx.Camera(*scenes.CAMERA), packed).upload(0)
    dev = torch.device("cuda", 0)
    d_hits = torch.empty(n * rtx.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_out = torch.empty_like(d_hits)
    torch.cuda.synchronize()
    hnd.primary_hits(w, h, d_hits.data_ptr(), want_stats=True)
    hit_objects = d_hits.cpu().numpy().view(rtx.HIT_DTYPE)["object"]
    nbytes = 2 * n * rtx.HIT_DTYPE.itemsize
    copy_ms = timed(lambda: d_out.copy_(d_hits), args.reps, args.warmup)
    copy_gbs = nbytes / copy_ms / 1e6
    print(json.dumps(dict(leg="rate", what="device copy of the same buffers (torch)", width=w, height=h, bytes=nbytes, ms=round(copy_ms, 4),
                          gb_per_s=round(copy_gbs, 1), pixels_with_a_hit=round(float((hit_objects >= 0).mean()), 4))), flush=True)
    for what, idx in (("no sphere moved", np.zeros(0, dtype=np.int64)), ("1 % of the spheres moved", np.arange(0, len(packed), 100)),
                      ("all spheres moved", np.arange(len(packed)))):
        now = packed[idx].copy()
        now["geom"][:, 1] += 1.0 / 3.0
        objects, motions = rtx.object_motions(idx, packed[idx], now)
        m = len(objects)
        d_obj = torch.from_numpy(objects).to(dev) if m else None
        d_mot = torch.from_numpy(motions.view(np.uint8).reshape(-1)).to(dev) if m else None
        torch.cuda.synchronize()
        call = lambda: hnd.rewind_hits_device(n, d_hits.data_ptr(), d_out.data_ptr(), d_obj.data_ptr() if m else None,
                                              d_mot.data_ptr() if m else None, m)
        ms = timed(call, args.reps, args.warmup)
        out = d_out.cpu().numpy().view(rtx.HIT_DTYPE)
        moved = float((out["position"] != d_hits.cpu().numpy().view(rtx.HIT_DTYPE)["position"]).any(axis=-1)[hit_objects >= 0].sum()) / n
        print(json.dumps(dict(leg="rate", what=what, width=w, height=h, moved_objects=m, list_in_lds=bool(0 < m * 8 <= 32768),
                              ms_per_call=round(ms, 4), hits_rewound=round(moved, 4), bytes_least=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1),
                              share_of_copy_rate=round(nbytes / ms / 1e6 / copy_gbs, 4))), flush=True)
    hnd.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import rust_raytracing_amd as rtx
    if rtx.device_count() < 1:
        raise SystemExit("rewind_rate: no gfx950 device (nothing is measured without one)")
    leg_rate(rtx, args)


if __name__ == "__main__":
    main()
