#!/usr/bin/env python3
"""What the round code AROUND the walk of stage 2 costs in the ISA, without a GPU (the sibling of tools/isa_visit_count.py, whose
compile step and control-flow helpers it uses).

A round of trace_bvh_spheres_kernel is one iteration of its outer loop: idle lanes are refilled from the survivors' queue, the walk's
f32 ray is set up, the walk runs (tools/isa_visit_count.py counts that), the candidates get their exact f64 tests, the hit is shaded
and a finished path stores its sample.  This tool follows the control flow of the outer loop and reports, per region, what a wave
issues when it passes through every block of the region once:

    outer loop    the OUTERMOST loop around the block that fetches the 64-byte node (found as isa_visit_count.py finds it)
    walk          the outermost loop inside it around the same block: not counted here
    refill        the blocks in front of the walk (from which the walk is still ahead within the iteration) from which a vector access
                  to global memory is still ahead or in the block itself: the queue's atomic, the survivor's and the material's record
    set-up        the other blocks in front of the walk: make_rayx, sphere_ray_from, make_ray32, the walk's reset
    exact loop    behind the walk, the first loop (in layout order) that reads LDS and computes in f64: one iteration of it
    shading       the blocks behind the walk that lie in no loop: hit_init, the counters, advance_and_shade, store_sample
    other loops   behind the walk: the sweep of every sphere (no walk / overflow), the planes, the triangles -- listed, not summed

Per region: VALU instructions; of those the f64 ones, the quarter-rate class (v_rcp / v_rsq / v_sqrt _f64, v_mul_lo / v_mul_hi _u32,
v_mad_u64_u32) and the v_mov copies; SALU instructions (branches, s_waitcnt, s_nop and scalar loads apart); scalar loads; vector-memory
instructions by prefix (global_, flat_, scratch_); LDS instructions; s_waitcnt.  And of the kernel: VGPRs, spilled VGPRs, SGPRs,
spilled SGPRs, scratch bytes per lane.  Instructions are classified by the prefix of their mnemonic, nothing else is looked for.

These are static counts of straight-line code: a lane-divergent region is issued whole by a wave with lanes on both sides, which is
the usual case of a round; the exact loop runs once per candidate of the wave's longest list.

    tools/isa_round_count.py [--json] [--blocks] [--kernel MANGLED_SUBSTRING] [--asm FILE.s] [-DMACRO=..]...
"""
import importlib.util
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("_isa_visit_count", os.path.join(HERE, "isa_visit_count.py"))
ivc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ivc)

KERNEL = ivc.KERNEL
REGIONS = ("refill", "setup", "exact_iter", "shading")
QUARTER = ("v_rcp_f64", "v_rsq_f64", "v_sqrt_f64", "v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32")
FIELDS = ("valu", "f64", "quarter", "v_mov", "salu", "s_load", "global", "flat", "scratch", "lds", "waitcnt", "branches")


def classify(ins, out):
    """Adds the instructions `ins` (stripped lines) to the counts in `out`."""
    for l in ins:
        mn = l.split()[0]
        if mn.startswith("v_"):
            out["valu"] += 1
            if "_f64" in mn:
                out["f64"] += 1
            if mn.startswith(QUARTER):
                out["quarter"] += 1
            if mn.startswith("v_mov_") or mn.startswith("v_accvgpr_"):
                out["v_mov"] += 1
        elif mn.startswith("s_cbranch") or mn in ("s_branch", "s_endpgm"):
            out["branches"] += 1
        elif mn == "s_waitcnt":
            out["waitcnt"] += 1
        elif mn.startswith("s_load_") or mn.startswith("s_buffer_load_"):
            out["s_load"] += 1
        elif mn.startswith("s_"):
            if mn != "s_nop":
                out["salu"] += 1
        elif mn.startswith("global_"):
            out["global"] += 1
        elif mn.startswith("flat_"):
            out["flat"] += 1
        elif mn.startswith("scratch_") or mn.startswith("buffer_"):
            out["scratch"] += 1
        elif mn.startswith("ds_"):
            out["lds"] += 1


def outermost_loop(succ, k):
    """(blocks, header blocks) of the outermost loop around block k."""
    c = ivc.component(succ, k, set(range(len(succ))))
    return c, {b for b in c if any(b in succ[a] for a in range(len(succ)) if a not in c)}


def kernel_resources(lines, key):
    """VGPRs, spills, SGPRs and scratch bytes of the kernel from the code object's metadata."""
    at = next(i for i, l in enumerate(lines) if l.strip().startswith(".name:") and key in l)
    lo = max(j for j in range(at + 1) if lines[j].lstrip().startswith("- .") and lines[j].startswith("  - "))
    hi = next((j for j in range(at + 1, len(lines)) if lines[j].startswith("  - ") or lines[j].startswith("amdhsa.")), len(lines))
    out = {}
    for l in lines[lo:hi]:
        m = re.match(r"^\s+(?:- )?\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", l)
        if m:
            out[m.group(1)] = int(m.group(2))
    return out


def round_counts(asm, key=KERNEL):
    """Counts of the round code; `asm` is the assembly text (isa_visit_count.compile_asm) or the path of a .s file."""
    lines = (asm if "\n" in asm else open(asm).read()).splitlines()
    body = ivc.kernel_body(lines, key)
    blocks = ivc.blocks_of(body)
    succ = ivc.successors(body, blocks)
    ins_of = lambda k: [l.strip() for l in body[blocks[k][0]:blocks[k][1] + 1] if ivc.is_instr(l)]
    fetch = [i for i, l in enumerate(body) if "global_load_dwordx4" in l]
    node_fetch = next(i for k, i in enumerate(fetch) if k + 3 < len(fetch) and fetch[k + 3] - i <= 8 and
                      len({re.search(r"(v\[\d+:\d+\]), off", body[j]).group(1) for j in fetch[k:k + 4]}) == 1 and
                      any("v_cvt_f32_ubyte" in l for l in body[i:i + 40]))
    main = next(k for k, (s, e) in enumerate(blocks) if s <= node_fetch <= e)
    outer, heads = outermost_loop(succ, main)
    walk = ivc.component(succ, main, outer - heads)
    # one iteration of the outer loop: the edges back into its header taken out
    once = [[n for n in succ[k] if n not in heads] for k in range(len(succ))]
    pred = [[] for _ in succ]
    for a in outer:
        for n in once[a]:
            if n in outer:
                pred[n].append(a)
    rest = outer - walk
    before = set()
    for w in walk:
        for a in pred[w]:
            if a in rest:
                before |= ivc.reach(pred, a, rest)
    after = rest - before
    # loops nested in the round code
    nested, loops = set(), []
    for k in sorted(rest - heads):
        if k not in nested:
            c = ivc.component(succ, k, rest - heads)
            if c:
                loops.append(c)
                nested |= c
    is_mem = lambda k: any(l.split()[0].startswith(("global_", "flat_")) for l in ins_of(k))
    refill = set()
    for k in before:
        if is_mem(k):
            refill |= ivc.reach(pred, k, before)
    exact = next((c for c in loops if c <= after and any(l.startswith("ds_") for k in c for l in ins_of(k)) and
                  any("_f64" in l.split()[0] for k in c for l in ins_of(k))), set())
    region = {}
    for k in rest:
        if k in exact:
            region[k] = "exact_iter"
        elif k in nested:
            region[k] = "other_loops"
        elif k in refill:
            region[k] = "refill"
        elif k in before:
            region[k] = "setup"
        else:
            region[k] = "shading"
    out = {r: dict.fromkeys(FIELDS, 0) for r in REGIONS + ("other_loops",)}
    out["blocks"] = []
    for k in sorted(rest):
        ins = ins_of(k)
        classify(ins, out[region[k]])
        s, e = blocks[k]
        out["blocks"].append((body[s].split()[0] if body[s].strip() else "", s, e, len(ins), region[k]))
    out["round"] = {f: sum(out[r][f] for r in REGIONS) for f in FIELDS}
    out["walk_blocks"] = len(walk)
    out["other_loop_count"] = len([c for c in loops if c != exact])
    out["kernel"] = kernel_resources(lines, key)
    out["kernel"]["instructions"] = sum(1 for l in body if ivc.is_instr(l))
    return out


def summary(c):
    """The figures a test pins: the regions' counts and the kernel's resources, without the block list."""
    return {k: c[k] for k in REGIONS + ("round", "kernel")}


def main():
    extra = [a for a in sys.argv[1:] if a.startswith("-D")]
    key = sys.argv[sys.argv.index("--kernel") + 1] if "--kernel" in sys.argv else KERNEL
    path = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else ivc.compile_asm(extra)
    c = round_counts(path, key)
    if "--json" in sys.argv:
        print(json.dumps(summary(c)))
        return
    print("%s, the round code around the walk%s" % (key, (" (" + " ".join(extra) + ")") if extra else ""))
    print("  %-12s" % "region" + "".join("%9s" % f for f in FIELDS))
    for r in REGIONS + ("round", "other_loops"):
        print("  %-12s" % r + "".join("%9d" % c[r][f] for f in FIELDS))
    kr = c["kernel"]
    print("  kernel: %d instructions, %d VGPRs (%d spilled), %d SGPRs (%d spilled), %d B scratch per lane, %d B LDS" % (
        kr["instructions"], kr.get("vgpr_count", -1), kr.get("vgpr_spill_count", -1), kr.get("sgpr_count", -1),
        kr.get("sgpr_spill_count", -1), kr.get("private_segment_fixed_size", -1), kr.get("group_segment_fixed_size", -1)))
    if "--blocks" in sys.argv:
        print("  blocks of the outer loop outside the walk (label, lines, instructions, region):")
        for lab, s, e, n, r in c["blocks"]:
            print("    %-12s %5d-%-5d %4d %s" % (lab, s, e, n, r))


if __name__ == "__main__":
    main()
