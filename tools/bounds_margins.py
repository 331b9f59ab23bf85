#!/usr/bin/env python3
"""How much of each f32 margin of the tree walks the worst aimed ray uses ("What holds the bounds").

Runs rtx_debug_path_bounds (the lab library, on the GPU) on tests/bounds_cases.py's scenes and rays and prints, per bound, margin and
origin regime, the worst observed share

    share = (b0 - t) / (b0 - b1)        for a lower bound (the entry distance, t_lo)
    share = (t - b0) / (b1 - b0)        for an upper bound (t_hi of a certain hit)

where t is the f64 text's distance of a reported pair, b1 the shipped bound and b0 the same bound with the named margin(s) at zero
(tests/bounds_model.py: every operation exact and rounded once).  share <= 0: the ray did not need the margin; 1.0 would be the
edge; above 1.0 the bound is violated.  `n` counts the reported pairs in which the margin loosened the bound (b0 > b1 for a lower bound, b0 < b1 for an upper one: without
the second abs_pad the 64-byte node's grid itself changes, and a few boxes come out LARGER; those pairs say nothing about the margin).

Two kinds of rows:
  "device ..."  b1 is the DEVICE's word (the largest entry distance of the whole resident path; t_lo; t_hi), b0 the model with ALL the
      margins of that bound at zero on the object's own unpadded box.  The path's ancestors have looser boxes than the own box, so the
      medians of the entry rows are large and negative; the worst share is the figure.
  "<margin> alone"  b0 and b1 are both the model's, on the object's own one-node path, with only that margin at zero -- the share a
      single margin has of itself.  (tests/test_walk_bounds.py holds the device to the model bit for bit on these paths.)  The row
      "abs_pad2 alone" is the 64-byte sphere visit's entry distance on the model's two-child node: the device's visit returns none.

    tools/bounds_margins.py [--scenes s6,spheres200,...] [--out profiles/bounds_margin_use.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bounds_cases as bc            # noqa: E402
import bounds_model as bm            # noqa: E402
import rust_raytracing_amd as rtx    # noqa: E402
from helpers import hip_scene        # noqa: E402

ZERO_SLAB = bm.Margins(widen=0.0, abs_pad=0.0, abs_pad2=0.0, slack=0.0)
ZERO_LEAF = bm.Margins(K=0.0, G=0.0, e_nv=0.0, e_dn=0.0)


def single(rows, label, b0, b1, lower, mask, t):
    b0, b1 = np.asarray(b0, dtype=np.float64), np.asarray(b1, dtype=np.float64)
    with np.errstate(all="ignore"):
        m = mask & np.isfinite(b0) & np.isfinite(b1) & ((b0 > b1) if lower else (b0 < b1))
        if m.any():
            sh = ((b0 - t) / (b0 - b1) if lower else (t - b0) / (b1 - b0))[m]
            rows[label] = (int(m.sum()), float(np.max(sh)), float(np.median(sh)))


def shares(name, regime, hnd, objs):
    cs = bc.case(name, regime)
    pk0 = bm.pack_for(objs, ZERO_SLAB)
    pk = bm.pack_for(objs)
    o, d, tg, t, rep = cs["o"], cs["d"], cs["target"], cs["t"], cs["reported"]
    best = np.where(rep, bm.round_up32(np.where(rep, t, 0.0)), bm.INF32).astype(np.float32)
    out = hnd.debug_path_bounds(o, d, tg, best, form=0)
    flags = out[:, 0]
    act = rep & ((flags & 3) != 3) & ((flags & 4) != 0)
    f = lambda w: np.ascontiguousarray(w).view(np.float32).astype(np.float64)
    _, in32 = bm.ray_form(o, d, pk["limit32"])
    rows = {}
    with np.errstate(all="ignore"):
        q0 = bm.make_ray32(o, d, pk["inv_max32"], in32, ZERO_SLAB)
        _, e0 = bm.walk_steps(bm.own_steps(pk0, tg, 0), q0, np.float32(np.inf), ZERO_SLAB)
        leaf0 = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], np.float32(np.inf), ZERO_LEAF)
        tri = pk["kind"][tg] == 2
        for label, b0, b1, lower, mask in (
                ("entry distance (widen, abs_pad, slack)", e0.astype(np.float64), f(out[:, 3]), True, act),
                ("sphere t_lo (K, G)", leaf0["tlo_hi"].astype(np.float64), f(out[:, 4]), True, act & ~tri & ((flags & 8) != 0)),
                ("sphere t_hi (K, G)", leaf0["thi_lo"].astype(np.float64), f(out[:, 5]), False, act & ~tri & ((flags & 16) != 0)),
                ("triangle t_lo (e_nv, e_dn)", leaf0["tlo_hi"].astype(np.float64), f(out[:, 4]), True, act & tri & ((flags & 8) != 0)),
                ("triangle t_hi (e_nv, e_dn)", leaf0["thi_lo"].astype(np.float64), f(out[:, 5]), False, act & tri & ((flags & 16) != 0))):
            m = mask & np.isfinite(b0) & np.isfinite(b1) & ((b0 > b1) if lower else (b0 < b1))
            if not m.any():
                continue
            sh = ((b0 - t) / (b0 - b1) if lower else (t - b0) / (b1 - b0))[m]
            rows["device " + label] = (int(m.sum()), float(np.max(sh)), float(np.median(sh)))
        # one margin alone, model against model on the own one-node path
        inf = np.float32(np.inf)
        q1 = bm.make_ray32(o, d, pk["inv_max32"], in32)
        _, e1 = bm.walk_steps(bm.own_steps(pk, tg, 0), q1, inf)
        leaf1 = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], inf)
        for name in ("widen", "abs_pad", "slack"):
            mm = bm.WEAKENED[name]
            pkm = bm.pack_for(objs, mm)
            _, em = bm.walk_steps(bm.own_steps(pkm, tg, 0, mm), bm.make_ray32(o, d, pk["inv_max32"], in32, mm), inf, mm)
            single(rows, name + " alone: entry distance", em, e1, True, act, t)
        st1 = bm.own_steps(pk, tg, 2)
        if st1 is not None and st1[0][0] == "q3":
            mm = bm.WEAKENED["abs_pad2"]
            stm = bm.own_steps(pk, tg, 2, mm)
            _, tn1 = bm.q3_entry(st1[0][1], st1[0][2], st1[0][3], st1[0][4], q1, inf)
            _, tnm = bm.q3_entry(stm[0][1], stm[0][2], stm[0][3], stm[0][4], q1, inf, mm)
            single(rows, "abs_pad2 alone: 64-byte entry distance", tnm, tn1, True, act & st1[0][5] & stm[0][5], t)
        for name, kinds in (("K", ~tri), ("G", ~tri), ("e_nv", tri), ("e_dn", tri)):
            lm = bm.leaf_bounds(pk["kind"][tg], pk["rec"][tg], o, d, pk["centre"], pk["cmax"], pk["tri_extent"], inf, bm.WEAKENED[name])
            single(rows, name + " alone: t_lo", lm["tlo_hi"], leaf1["tlo_hi"], True, act & kinds & leaf1["cand"] & lm["cand"], t)
            single(rows, name + " alone: t_hi", lm["thi_lo"], leaf1["thi_lo"], False, act & kinds & leaf1["certain_any"] & lm["certain_any"], t)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(n for n, _ in bc.scenes(rtx.OBJECT_DTYPE)))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# worst share of each margin used by a reported (ray, object) pair: tools/bounds_margins.py (MI355X, the lab library's",
             "# rtx_debug_path_bounds on tests/bounds_cases.py's rays; share 1.0 = the edge, <= 0 = the margin was not needed)",
             "# 'device ...': the device's bound against the model with all that bound's margins at zero on the object's OWN unpadded box",
             "#   (the resident path's ancestors are looser: large negative medians);  '<margin> alone': model against model on the own",
             "#   one-node path with only that margin at zero; 'abs_pad2 alone': the 64-byte sphere visit, which returns no distance on the device",
             "%-12s %-8s %-50s %8s %12s %12s" % ("scene", "regime", "bound (margins)", "n", "worst", "median")]
    scenes = dict(bc.scenes(rtx.OBJECT_DTYPE))
    for name in a.scenes.split(","):
        hnd = hip_scene(rtx, scenes[name], rays_per_pixel=1).upload(0, lab=True)
        for regime in bc.regimes_of(name):
            if regime == "nowalk":
                continue
            for label, (n, worst, med) in shares(name, regime, hnd, scenes[name]).items():
                lines.append("%-12s %-8s %-50s %8d %12.4g %12.4g" % (name, regime, label, n, worst, med))
                print(lines[-1], flush=True)
        hnd.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
