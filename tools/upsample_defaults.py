"""How rtx_upsample_default_params was chosen: the model of tests/upsample_model.py on oracle frames of the golden
scenes whose sizes the factor divides -- the low frame at 4 s^2 spp, the guides from the oracle pick, RMSE against 256 spp at the golden
size -- over a grid of parameters; prints every set's ratios against bilinear and the set with the lowest mean ratio.  CPU only.

    python tools/upsample_defaults.py [--frames DIR]

--frames DIR: the same grid on device frames that `tools/upsample_rate.py --dump DIR` wrote (the handle's lens-jittered features of
both sizes, the low frame's variance, the same handle's 256-spp frame) instead of oracle frames.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import rust_raytracing_amd as rtx                      # noqa: E402
import upsample_model as um                            # noqa: E402
from oracle import rtx_oracle                          # noqa: E402
from upsample_cases import QUALITY, bilinear_params, quality_inputs, rmse      # noqa: E402


def dumped(path, name, s):
    """(lo, hi, ref) from the .npz that tools/upsample_rate.py --dump wrote on a device: lens-jittered features, a variance"""
    z = np.load(os.path.join(path, "%s_s%d.npz" % (name, s)))
    keys = ("albedo", "emission", "normal", "depth")
    lo = dict({k: z["lo_" + k] for k in keys}, rgb=z["lo_rgb"], var=z["lo_var"])
    return lo, {k: z["hi_" + k] for k in keys}, z["ref"]


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--frames":
        inputs = [(name, s) + dumped(sys.argv[2], name, s) for name, s in QUALITY]
    else:
        rtx_oracle.build()
        inputs = [(name, s) + quality_inputs(rtx_oracle, rtx, name, s) for name, s in QUALITY]
    bil = [rmse(um.upsample(lo, hi, bilinear_params(s))[0], ref) for _, s, lo, hi, ref in inputs]
    print("pairs: " + ", ".join("%s s=%d" % (n.split("_")[0], s) for n, s, *_ in inputs))
    print("bilinear RMSE: " + " ".join("%.4f" % b for b in bil))
    grid = itertools.product((0.05, 0.1, 0.2), (0.25, 0.5, 1.0), (0, 1, 2), (1e-3,), (0.0, 1e-3, 1e-2, 0.1))
    best = None
    for sd, sa, power, amin, mw in grid:
        ratios = []
        for (_, s, lo, hi, ref), b in zip(inputs, bil):
            p = um.Params(factor=s, flags=um.DEMODULATE, normal_power_log2=power, sigma_depth=sd, sigma_albedo=sa, albedo_min=amin, min_weight=mw)
            ratios.append(rmse(um.upsample(lo, hi, p)[0], ref) / b)
        mean = sum(ratios) / len(ratios)
        print("sigma_depth %-5g sigma_albedo %-5g power 2^%d albedo_min %g min_weight %-6g: %s  mean %.4f" %
              (sd, sa, power, amin, mw, " ".join("%.3f" % r for r in ratios), mean))
        if best is None or mean < best[0]:
            best = (mean, sd, sa, power, amin, mw)
    print("lowest mean ratio %.4f: sigma_depth %g, sigma_albedo %g, power 2^%d, albedo_min %g, min_weight %g" % best)


if __name__ == "__main__":
    main()
