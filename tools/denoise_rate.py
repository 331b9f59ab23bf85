#!/usr/bin/env python3
"""What the denoiser costs and what it buys (rtx_denoise_device, include/rtx_hip.h "Denoising").

  rate     a 1920 x 1080 frame of seeded noise on three "surfaces" (tests/denoise_cases.fuzz_frame without its hostile values), device
           buffers throughout, the default parameters with passes = 1 .. 5, with and without a variance: milliseconds per call (device
           events around --reps calls after --warmup calls) and per pass (the call with p passes minus the call with p - 1; the
           first row also holds the preparation launch).  Against the bytes a pass must move -- one 128-byte record read and one
           written per pixel, the last pass writing the 24-byte pixel (48 with a variance) instead -- as achieved GB/s, next to the
           rate of a plain device copy of the same frame's records (torch's copy kernel: epilogue_kernel's form 8 has no entry point
           that launches it on a caller's device buffer, so its own rate is NOT measured here).
  render   the same frame size on C2 (scenes.random_spheres(10000, 1)): one sample of every pixel through
           rtx_render_blocks_accumulate, device time (RtxStats trace_ms + resolve_ms) -- what a denoise call is to be held against.
  quality  the golden scenes at their golden sizes and seeds, 4 / 8 / 16 spp, the default parameters: RMSE of the noisy and of the
           denoised frame against the same handle's 256-spp frame.

    tools/denoise_rate.py [--legs rate,render,quality] [--reps 30] [--warmup 3] [--width 1920 --height 1080]

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

GOLDEN = ("c1_three_spheres_32x32", "spheres200_48x27", "mixed_40x24", "tris300_32x18")


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
    from denoise_cases import fuzz_frame, to_records
    w, h = args.width, args.height
    npix = w * h
    fr = fuzz_frame(np.random.default_rng(1), h, w, hostile=False)
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_rgb, d_var, d_feat = up(fr["rgb"]), up(fr["var"]), up(to_records(rtx.FEATURE_DTYPE, fr))
    d_out, d_vout = torch.empty(24 * npix, dtype=torch.uint8, device=dev), torch.empty(24 * npix, dtype=torch.uint8, device=dev)
    d_work = torch.empty(256 * npix, dtype=torch.uint8, device=dev)
    lib = rtx.load_library()
    src, dst = d_work[:128 * npix], d_work[128 * npix:]
    copy_ms = timed(lambda: dst.copy_(src), args.reps, args.warmup)
    copy_gbs = 2 * 128 * npix / copy_ms / 1e6
    print(json.dumps(dict(leg="rate", what="device copy of the frame's records (torch)", width=w, height=h, ms=round(copy_ms, 4),
                          gb_per_s=round(copy_gbs, 1))), flush=True)
    for with_var in (True, False):
        prev = 0.0
        for passes in range(1, 6):
            p = rtx.denoise_params(passes=passes)

            def call():
                rtx.abi.check(lib.rtx_denoise_device(d_rgb.data_ptr(), d_var.data_ptr() if with_var else None, d_feat.data_ptr(), w, h,
                                                     p.ctypes.data, d_out.data_ptr(), d_vout.data_ptr() if with_var else None,
                                                     d_work.data_ptr(), 0, None), lib)
            ms = timed(call, args.reps, args.warmup)
            pass_ms = ms - prev
            prev = ms
            # what the marginal pass moves: its records in, and records out (the call's last pass writes pixels instead, so the
            # marginal cost of pass p is one more record-to-record pass)
            moved = npix * (128 + (128 if passes > 1 else (48 if with_var else 24))) + (npix * (24 + 96 + (24 if with_var else 0) + 128) if passes == 1 else 0)
            print(json.dumps(dict(leg="rate", variance=with_var, passes=passes, width=w, height=h, ms_per_call=round(ms, 4),
                                  ms_marginal_pass=round(pass_ms, 4), bytes_marginal=moved, gb_per_s=round(moved / pass_ms / 1e6, 1),
                                  share_of_copy_rate=round(moved / pass_ms / 1e6 / copy_gbs, 4))), flush=True)


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


def leg_quality(rtx, args):
    from helpers import hip_scene

    def rmse(a, b):
        m = np.isfinite(a).all(axis=2) & np.isfinite(b).all(axis=2)
        d = (a - b)[m]
        return float(np.sqrt(np.mean(d * d)))
    for name in GOLDEN:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        objs = np.frombuffer(z["objects"].tobytes(), dtype=rtx.OBJECT_DTYPE)
        cfg, w, h = json.loads(str(z["config"])), int(z["width"]), int(z["height"])
        ref = None
        for spp in (4, 8, 16):
            hnd = hip_scene(rtx, objs, **dict(cfg, rays_per_pixel=spp)).upload(0)
            prog = hnd.progressive(w, h)
            prog.add(spp)
            noisy, den = prog.mean(), prog.denoise()
            if ref is None:
                prog.add(256 - spp)
                ref = prog.mean()
            hnd.close()
            a, b = rmse(noisy, ref), rmse(den, ref)
            print(json.dumps(dict(leg="quality", scene=name, spp=spp, rmse_noisy=round(a, 6), rmse_denoised=round(b, 6), ratio=round(b / a, 5))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="rate,render,quality")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import rust_raytracing_amd as rtx
    if rtx.device_count() < 1:
        raise SystemExit("denoise_rate: no gfx950 device (nothing is measured without one)")
    d = rtx.denoise_params()
    print(json.dumps(dict(leg="defaults", **{k: d[k].item() for k in d.dtype.names})), flush=True)
    for leg in args.legs.split(","):
        {"rate": leg_rate, "render": leg_render, "quality": leg_quality}[leg](rtx, args)


if __name__ == "__main__":
    main()
