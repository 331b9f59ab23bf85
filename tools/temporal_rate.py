#!/usr/bin/env python3
"""What temporal accumulation costs (rtx_temporal_accumulate_device, include/rtx_hip.h "Temporal accumulation").

  rate     a 1920 x 1080 frame pair of tests/temporal_cases.fuzz_case (no planted pixels), device buffers throughout, the default
           parameters: milliseconds per call (device events around --reps calls after --warmup calls) with the history fully valid
           and with half of it rejected (hist_len = 0 on a checkerboard of 16 x 16 blocks), with and without a variance, and as a
           first frame.  Against the bytes a call must move at least -- every input and every output once: 304 B per pixel with a
           variance, 232 B without, d_motion included; a first frame 120 B and 72 B -- as achieved GB/s, next to a plain device copy (torch's copy kernel) that
           moves the same number of bytes on the same device.
  render   the same frame size on C2 (scenes.random_spheres(10000, 1)): one sample of every pixel through
           rtx_render_blocks_accumulate, device time (RtxStats trace_ms + resolve_ms) -- what a call is to be held against.

    tools/temporal_rate.py [--legs rate,render] [--reps 30] [--warmup 3] [--width 1920 --height 1080]

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
    from temporal_cases import fuzz_case, hit_records
    w, h = args.width, args.height
    npix = w * h
    case = fuzz_case(1, w, h, with_var=True, planted=False)
    cur, hist = case["cur"], case["hist"]
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d = dict(rgb=up(cur["rgb"]), var=up(cur["var"]), hits=up(hit_records(rtx.HIT_DTYPE, cur)), hist_rgb=up(hist["rgb"]), hist_var=up(hist["var"]),
             hist_len=up(hist["len"]), hist_hits=up(hit_records(rtx.HIT_DTYPE, hist)), tables=up(hist["tables"]))
    ys, xs = np.mgrid[0:h, 0:w]
    half = hist["len"].copy()
    half[((ys // 16) + (xs // 16)) % 2 == 0] = 0.0
    d["hist_len_half"] = up(half)
    out = {k: torch.empty(n * npix, dtype=torch.uint8, device=dev) for k, n in (("rgb", 24), ("var", 24), ("len", 8), ("motion", 16))}
    cam = rtx.abi.RtxCamera()
    cam.fov = float(hist["fov"])
    cam.position[:] = [float(x) for x in hist["cam_pos"]]
    cam.to_cam_space[:] = [float(x) for x in hist["to_cam"]]
    p = rtx.temporal_params()
    lib = rtx.load_library()
    for with_var in (True, False):
        moved = npix * (304 if with_var else 232)
        a, b = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_ms = timed(lambda: b.copy_(a), args.reps, args.warmup)
        copy_gbs = moved / copy_ms / 1e6
        print(json.dumps(dict(leg="rate", what="device copy moving the same bytes (torch)", variance=with_var, width=w, height=h,
                              bytes=moved, ms=round(copy_ms, 4), gb_per_s=round(copy_gbs, 1))), flush=True)
        for what, len_key, first in (("history fully valid", "hist_len", False), ("half of the history rejected", "hist_len_half", False),
                                     ("first frame", "hist_len", True)):
            hp = (lambda k: None) if first else (lambda k: d[k].data_ptr())

            def call():
                rtx.abi.check(lib.rtx_temporal_accumulate_device(
                    d["rgb"].data_ptr(), d["var"].data_ptr() if with_var else None, d["hits"].data_ptr(), hp("hist_rgb"),
                    hp("hist_var") if with_var else None, hp(len_key), hp("hist_hits"), None if first else rtx.abi.C.addressof(cam), hp("tables"),
                    w, h, p.ctypes.data, out["rgb"].data_ptr(), out["var"].data_ptr() if with_var else None, out["len"].data_ptr(),
                    out["motion"].data_ptr(), 0, None), lib)
            ms = timed(call, args.reps, args.warmup)
            kept = float((out["len"].view(torch.float64) > 1).double().mean())
            # (a first frame reads only the frame and its variance -- no pick buffer -- and writes every output)
            nbytes = npix * ((24 + 24 + 8 + 16 + (48 if with_var else 0)) if first else (304 if with_var else 232))
            print(json.dumps(dict(leg="rate", what=what, variance=with_var, width=w, height=h, ms_per_call=round(ms, 4), pixels_with_history=round(kept, 4),
                                  bytes_least=nbytes, gb_per_s=round(nbytes / ms / 1e6, 1), share_of_copy_rate=round(nbytes / ms / 1e6 / copy_gbs, 4))),
                  flush=True)


def leg_render(rtx, args):
    import torch
    from rust_raytracing_amd import scenes
    w, h = args.width, args.height
    hnd = rtx.Scene.from_packed(rtx.Config(rays_per_pixel=1, seed=scenes.RENDER_SEED), rtx.Camera(*scenes.CAMERA), scenes.random_spheres(10000, 1)).upload(0)
    s = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    q = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    times = []
    for k in range(args.warmup + 5):
        st = hnd.render_accumulate(w, h, k, 1, s.data_ptr(), q.data_ptr())
        times.append(st.trace_ms + st.resolve_ms)
    hnd.close()
    t = times[args.warmup:]
    print(json.dumps(dict(leg="render", what="C2, one sample per pixel, rtx_render_blocks_accumulate, trace_ms + resolve_ms", width=w, height=h,
                          ms_best=round(min(t), 4), ms_worst=round(max(t), 4))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="rate,render")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import rust_raytracing_amd as rtx
    if rtx.device_count() < 1:
        raise SystemExit("temporal_rate: no gfx950 device (nothing is measured without one)")
    d = rtx.temporal_params()
    print(json.dumps(dict(leg="defaults", **{k: d[k].item() for k in d.dtype.names})), flush=True)
    for leg in args.legs.split(","):
        {"rate": leg_rate, "render": leg_render}[leg](rtx, args)


if __name__ == "__main__":
    main()
