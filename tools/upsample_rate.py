#!/usr/bin/env python3
"""What guided upsampling costs and what it buys (rtx_upsample_device, include/rtx_hip.h "Guided upsampling").

  rate     seeded frames on three "surfaces" (tests/upsample_cases.fuzz_case without its hostile values), device buffers throughout,
           the default parameters: milliseconds per call (device events around --reps calls after --warmup calls) for 960 x 540 ->
           1920 x 1080 and 1920 x 1080 -> 3840 x 2160 at s = 2 and 960 x 540 -> 3840 x 2160 at s = 4, with and without a variance,
           demodulated and not.  Against the least bytes a call must move -- per output pixel its 96-byte guide record and the 24-byte
           pixel written (48 with a variance), per low pixel its record and its 24 (48) bytes read once -- as achieved GB/s, next to a
           device copy (torch's copy kernel) that reads and writes the same number of bytes on the same device.
  buys     C2 (scenes.random_spheres(10000, 1)) at 1920 x 1080 and --spp samples: the low frame at 960 x 540 through
           rtx_render_blocks_accumulate + rtx_scene_pixel_features at both sizes + the upsample call, against the full frame at the same
           samples per pixel through rtx_render_blocks_accumulate.  Device events around each stage (asynchronous calls).
  dump     --dump DIR: the device frames of the golden scene / factor pairs (low mean and variance at 4 s^2 spp, the features of both
           sizes, the 256-spp frame at full size) as .npz, for running the model over parameter grids on the CPU.

    tools/upsample_rate.py [--legs rate,buys] [--reps 30] [--warmup 3] [--spp 4] [--dump DIR]

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

SHAPES = ((960, 540, 2), (1920, 1080, 2), (960, 540, 4))                   # (wl, hl, s)


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
    from upsample_cases import fuzz_case, to_records
    dev = torch.device("cuda", 0)
    lib = rtx.load_library()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    for wl, hl, s in SHAPES:
        w, h = wl * s, hl * s
        npix, nlo = w * h, wl * hl
        lo, hi = fuzz_case(np.random.default_rng(1), hl, wl, s, hostile=False)
        d_lo, d_var = up(lo["rgb"]), up(lo["var"])
        d_lo_feat, d_feat = up(to_records(rtx.FEATURE_DTYPE, lo)), up(to_records(rtx.FEATURE_DTYPE, hi))
        del lo, hi
        d_out, d_vout = torch.empty(24 * npix, dtype=torch.uint8, device=dev), torch.empty(24 * npix, dtype=torch.uint8, device=dev)
        for with_var in (True, False):
            px = 48 if with_var else 24
            moved = npix * (96 + px) + nlo * (96 + px)
            src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            copy_ms = timed(lambda: dst.copy_(src), args.reps, args.warmup)
            del src, dst
            for demod in (True, False):
                p = rtx.upsample_params(factor=s, demodulate=demod)

                def call():
                    rtx.abi.check(lib.rtx_upsample_device(d_lo.data_ptr(), d_var.data_ptr() if with_var else None, d_lo_feat.data_ptr(),
                                                          d_feat.data_ptr(), w, h, p.ctypes.data, d_out.data_ptr(),
                                                          d_vout.data_ptr() if with_var else None, 0, None), lib)
                ms = timed(call, args.reps, args.warmup)
                print(json.dumps(dict(leg="rate", low="%dx%d" % (wl, hl), out="%dx%d" % (w, h), factor=s, variance=with_var, demodulate=demod,
                                      ms_per_call=round(ms, 4), least_bytes=moved, gb_per_s=round(moved / ms / 1e6, 1),
                                      copy_ms_same_bytes=round(copy_ms, 4), copy_gb_per_s=round(moved / copy_ms / 1e6, 1),
                                      share_of_copy_rate=round(copy_ms / ms, 4))), flush=True)


def leg_buys(rtx, args):
    import torch
    from rust_raytracing_amd import scenes
    w, h, s, spp = 1920, 1080, 2, args.spp
    wl, hl = w // s, h // s
    dev = torch.device("cuda", 0)
    hnd = rtx.Scene.from_packed(rtx.Config(rays_per_pixel=spp, seed=scenes.RENDER_SEED), rtx.Camera(*scenes.CAMERA), scenes.random_spheres(10000, 1)).upload(0)
    frame = lambda ww, hh: torch.zeros((hh, ww, 3), dtype=torch.float64, device=dev)
    full_s, full_q, lo_s, lo_q, out = frame(w, h), frame(w, h), frame(wl, hl), frame(wl, hl), frame(w, h)
    f_lo = torch.empty(wl * hl * 96, dtype=torch.uint8, device=dev)
    f_hi = torch.empty(w * h * 96, dtype=torch.uint8, device=dev)
    p = rtx.upsample_params(factor=s)
    reps, warm = max(args.reps // 6, 3), 2
    stages = {
        "full frame, %d spp (rtx_render_blocks_accumulate)" % spp:
            lambda: hnd.render_accumulate(w, h, 0, spp, full_s.data_ptr(), full_q.data_ptr(), want_stats=False),
        "low frame, %d spp" % spp: lambda: hnd.render_accumulate(wl, hl, 0, spp, lo_s.data_ptr(), lo_q.data_ptr(), want_stats=False),
        "features, low size": lambda: hnd.pixel_features(wl, hl, f_lo.data_ptr(), want_stats=False),
        "features, full size": lambda: hnd.pixel_features(w, h, f_hi.data_ptr(), want_stats=False),
        "upsample (sums as the frame: the arithmetic is the same)":
            lambda: hnd.upsample_device(w, h, lo_s.data_ptr(), f_lo.data_ptr(), f_hi.data_ptr(), out.data_ptr(), d_lo_var_ptr=lo_q.data_ptr(), params=p),
    }
    got = {}
    for name, fn in stages.items():
        got[name] = timed(fn, reps, warm)
        print(json.dumps(dict(leg="buys", scene="C2", out="%dx%d" % (w, h), factor=s, spp=spp, stage=name, ms=round(got[name], 4))), flush=True)
    names = list(stages)
    chain = sum(got[n] for n in names[1:])
    print(json.dumps(dict(leg="buys", scene="C2", spp=spp, full_ms=round(got[names[0]], 4), low_features_upsample_ms=round(chain, 4),
                          ratio=round(chain / got[names[0]], 4))), flush=True)
    hnd.close()


def dump(rtx, path):
    from helpers import hip_scene
    from upsample_cases import QUALITY
    os.makedirs(path, exist_ok=True)
    for name, s in QUALITY:
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        objs = np.frombuffer(z["objects"].tobytes(), dtype=rtx.OBJECT_DTYPE)
        cfg, w, h = json.loads(str(z["config"])), int(z["width"]), int(z["height"])
        wl, hl, spp = w // s, h // s, 4 * s * s
        hnd = hip_scene(rtx, objs, **dict(cfg, rays_per_pixel=spp)).upload(0)
        prog = hnd.progressive(wl, hl)
        prog.add(spp)
        out = dict(lo_rgb=prog.mean(), lo_var=prog.variance())
        for k, a in zip(("albedo", "emission", "normal", "depth"), hnd.features(wl, hl)[:4]):
            out["lo_" + k] = a
        for k, a in zip(("albedo", "emission", "normal", "depth"), hnd.features(w, h)[:4]):
            out["hi_" + k] = a
        full = hnd.progressive(w, h, moments=False)
        full.add(256)
        out["ref"] = full.mean()
        hnd.close()
        np.savez(os.path.join(path, "%s_s%d.npz" % (name, s)), **out)
        print(json.dumps(dict(leg="dump", scene=name, factor=s)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="rate,buys")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    import rust_raytracing_amd as rtx
    if rtx.device_count() < 1:
        raise SystemExit("upsample_rate: no gfx950 device (nothing is measured without one)")
    d = rtx.upsample_params()
    print(json.dumps(dict(leg="defaults", **{k: d[k].item() for k in d.dtype.names})), flush=True)
    if args.dump:
        dump(rtx, args.dump)
    for leg in [x for x in args.legs.split(",") if x]:
        {"rate": leg_rate, "buys": leg_buys}[leg](rtx, args)


if __name__ == "__main__":
    main()
