#!/usr/bin/env python3
"""What one node visit of stage 2 costs in the ISA, without a GPU.

Compiles rust-raytracing_amd/csrc/rtx_bvh_spheres.hip for gfx950 with the flags of build.py (device code only, to assembly), takes
trace_bvh_spheres_kernel<false, 2, 2> (stage 2 of the sphere path) and counts the node-visit path of its walk loop:

    walk loop     the innermost loop around the block that fetches the 64-byte node (four global_load_dwordx4): the blocks from which
                  the loop's header is reached again, found in the control-flow graph (a block's branches and its fall-through) --
                  NOT the lines between the header and the last back-branch: with the node visits in an inner loop of their own
                  (sphere_walk_phased<.., INNER>) the compiler lays the block with the pushes behind the back-branch
    the path      the blocks of that loop, without
                    - the leaf visit (the two-arm form of the loop, -DRTX_WALK_INNER=0; the inner loop holds none): the blocks on a
                      way from the block that decodes a leaf link (its record index: v_and_b32 .., 0x1fffffff, ..) to the block that
                      pops the stack (the nearest ds_read_b32 behind it outside a nested loop), nested loops included
                    - the pushes of a lane without room for three rows: the visit's main block (the one with the node fetch) ends
                      in a branch on the exec mask; of the blocks that only one of its two sides reaches, the side that writes to
                      LDS under further branches (one push per entered child, each under its own test)
                  -- what a wave issues in an iteration in which it visits nodes and every lane has room on its LDS stack

The two exclusions are recognised by what this compiler (AMD clang 22) emits for them -- the mask that decodes a leaf link, the branch
on exec that ends the main block.  Where the blocks lie no longer matters, but a compiler that shapes the control flow differently can
still move the counts without any change of the source.  The tests that pin them check that the path found holds one node fetch, the
pushes and the pop; when they fail after a toolchain change, look at --blocks before looking at the kernel.

It prints the VALU instructions on the path, how many of them read an SGPR, an SGPR pair or a literal (or write an SGPR pair: the
v_cmp e64 forms), the SALU and LDS instructions, and the per-mnemonic table (VALU and LDS).

    tools/isa_visit_count.py [--json] [--blocks] [--asm FILE.s] [-DMACRO=..]...
"""
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "trace_bvh_spheres_kernelILb0ELi2ELi2E"


def compile_asm(extra=()):
    """The assembly text of rtx_bvh_spheres.hip's device code (nothing is left on disk)."""
    spec = importlib.util.spec_from_file_location("_rtx_build", os.path.join(ROOT, "rust-raytracing_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    with tempfile.TemporaryDirectory(prefix="rtx_isa_") as tmp:
        out = os.path.join(tmp, "rtx_bvh_spheres.s")
        cmd = [b.hipcc()] + b.FLAGS + list(extra) + ["-S", "--cuda-device-only", os.path.join(b.CSRC, "rtx_bvh_spheres.hip"), "-o", out]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def is_instr(l):
    s = l.strip()
    return bool(s) and not s.startswith((";", ".", "//")) and not s.endswith(":")


def kernel_body(lines, key=KERNEL):
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


BRANCH = re.compile(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)")


def blocks_of(body):
    """[(first line, last line)] of the basic blocks of a kernel body: a block starts at a label or a '; %bb.N:' line."""
    starts = [i for i, l in enumerate(body) if re.match(r"^\.LBB\d+_\d+:", l) or re.match(r"^; %bb\.\d+:", l)]
    if not starts or starts[0] != 0:
        starts = [0] + starts
    return [(s, (starts[k + 1] - 1 if k + 1 < len(starts) else len(body) - 1)) for k, s in enumerate(starts)]


def successors(body, blocks):
    """The control-flow graph: block -> the blocks its branches name, and the next block unless it ends in an unconditional transfer."""
    at = {}
    for k, (s, e) in enumerate(blocks):
        m = re.match(r"^(\.LBB\d+_\d+):", body[s])
        if m:
            at[m.group(1)] = k
    succ = []
    for k, (s, e) in enumerate(blocks):
        ins = [l.strip() for l in body[s:e + 1] if is_instr(l)]
        out = [at[m.group(1)] for l in ins for m in [BRANCH.search(l)] if m and m.group(1) in at]
        if k + 1 < len(blocks) and not (ins and ins[-1].split()[0] in ("s_branch", "s_endpgm", "s_setpc_b64")):
            out.append(k + 1)
        succ.append(sorted(set(out)))
    return succ


def reach(succ, start, inside, stop=()):
    """The blocks of `inside` reached from `start` (a block of `inside`: counted in) without passing through a block of `stop`."""
    seen, todo = set(), [start]
    while todo:
        k = todo.pop()
        if k in seen or k not in inside:
            continue
        seen.add(k)
        if k not in stop:
            todo.extend(succ[k])
    return seen


def component(succ, k, inside):
    """The blocks of `inside` on a cycle through block k (its strongly connected component), empty when there is none."""
    fwd = set()
    for n in succ[k]:
        fwd |= reach(succ, n, inside)
    pred = [[] for _ in succ]
    for a, outs in enumerate(succ):
        for n in outs:
            pred[n].append(a)
    back = set()
    for n in pred[k]:
        back |= reach(pred, n, inside)
    return fwd & back


def innermost_loop(succ, k):
    """(blocks, header blocks) of the innermost loop around block k: the cycles through k that are left when the headers of the loops
    around it are taken away, outermost first.  A loop is the set of blocks from which its header is reached again -- wherever the
    compiler has laid them out, behind the back-branch included."""
    inside = set(range(len(succ)))
    loop, heads = None, None
    while True:
        c = component(succ, k, inside)
        if not c:
            return loop, heads
        entries = {b for b in c if any(b in succ[a] for a in range(len(succ)) if a not in c)}
        loop, heads = c, entries
        if k in entries or not entries:
            return loop, heads
        inside = c - entries


SGPR = re.compile(r"\bs\d+\b|\bs\[\d+:\d+\]|\b0x[0-9a-f]+\b|\bexec\b")


def visit_counts(asm):
    """Counts of the node-visit path; `asm` is the assembly text (compile_asm) or the path of a .s file."""
    body = kernel_body((asm if "\n" in asm else open(asm).read()).splitlines())
    fetch = [i for i, l in enumerate(body) if "global_load_dwordx4" in l]
    # the node fetch: four loads off one base register within a few lines
    node_fetch = next(i for k, i in enumerate(fetch) if k + 3 < len(fetch) and fetch[k + 3] - i <= 8 and
                      len({re.search(r"(v\[\d+:\d+\]), off", body[j]).group(1) for j in fetch[k:k + 4]}) == 1 and
                      any("v_cvt_f32_ubyte" in l for l in body[i:i + 40]))
    all_blocks = blocks_of(body)
    succ = successors(body, all_blocks)
    text = lambda k: body[all_blocks[k][0]:all_blocks[k][1] + 1]
    main = next(k for k, (s, e) in enumerate(all_blocks) if s <= node_fetch <= e)
    loop, heads = innermost_loop(succ, main)
    # one iteration: the loop's blocks with the edges back into its header taken out
    once = [[n for n in succ[k] if n not in heads] for k in range(len(succ))]
    skip = set()
    # the pushes of a lane without room: the main block ends in a branch on the exec mask, and of the blocks that only one of its two
    # sides reaches, the side with the pushes under further branches (one ds_write per entered child, each under its own test)
    ins = [l.strip() for l in text(main) if is_instr(l)]
    if len(succ[main]) == 2 and re.match(r"s_cbranch_exec", ins[-1]):
        x, y = succ[main]
        rx, ry = reach(once, x, loop), reach(once, y, loop)
        sides = []
        for only in (rx - ry, ry - rx):
            t = [l.strip() for k in only for l in text(k) if is_instr(l)]
            sides.append((sum(l.startswith("ds_write") for l in t) > 0, sum(bool(BRANCH.search(l)) for l in t), only))
        sides = [sd for sd in sides if sd[0] and sd[1]]
        if sides:
            skip |= max(sides, key=lambda sd: sd[1])[2]
    # the leaf visit: the blocks on a way from the block that decodes a leaf link (its record index: v_and_b32 .., 0x1fffffff, ..) to
    # the block that pops the stack (the nearest ds_read_b32 behind it outside a nested loop), that block not included
    nested = set()
    for k in loop - heads:
        if k not in nested:
            nested |= component(succ, k, loop - heads)
    leaf0 = next((k for k in sorted(loop - skip) if k != main and any(re.search(r"v_and_b32_e32 v\d+, 0x1fffffff, ", l) for l in text(k))), None)
    if leaf0 is not None:
        after = reach(once, leaf0, loop)
        pops = [k for k in after if k not in nested and any("ds_read_b32" in l for l in text(k))]
        if pops:
            dist, todo = {leaf0: 0}, [leaf0]
            for k in todo:
                for n in once[k]:
                    if n in loop and n not in dist:
                        dist[n] = dist[k] + 1
                        todo.append(n)
            pop = min(pops, key=lambda k: dist[k])
            back = [[] for _ in succ]
            for k in loop:
                for n in once[k]:
                    back[n].append(k)
            skip |= (reach(once, leaf0, loop, stop={pop}) & reach(back, pop, loop)) - {pop}
    blocks = all_blocks
    out = {"valu": 0, "valu_sgpr_or_literal": 0, "salu": 0, "lds": 0, "global": 0, "branches": 0, "mnemonics": {}, "blocks": []}
    for k, (s, e) in enumerate(blocks):
        if k not in loop:
            continue
        ins = [l.strip() for l in body[s:e + 1] if is_instr(l)]
        v = [l for l in ins if l.startswith("v_")]
        out["blocks"].append((body[s].split()[0] if body[s].strip() else "", s, e, len(ins), len(v), k in skip))
        if k in skip:
            continue
        for l in ins:
            mn = l.split()[0]
            if mn.startswith("v_"):
                out["valu"] += 1
                ops = l[len(mn):]
                scal = bool(SGPR.search(ops))
                out["valu_sgpr_or_literal"] += scal
                key = re.sub(r"_e(32|64)$", "", mn) + (" [s]" if scal else "")
                out["mnemonics"][key] = out["mnemonics"].get(key, 0) + 1
            elif mn.startswith("s_c") and "branch" in mn or mn == "s_branch":
                out["branches"] += 1
            elif mn.startswith("s_") and mn not in ("s_waitcnt", "s_nop"):
                out["salu"] += 1
            elif mn.startswith("ds_"):
                out["lds"] += 1
                out["mnemonics"][mn] = out["mnemonics"].get(mn, 0) + 1
            elif mn.startswith("global_"):
                out["global"] += 1
    return out


def main():
    extra = [a for a in sys.argv[1:] if a.startswith("-D")]
    path = sys.argv[sys.argv.index("--asm") + 1] if "--asm" in sys.argv else compile_asm(extra)
    c = visit_counts(path)
    if "--json" in sys.argv:
        print(json.dumps({k: c[k] for k in ("valu", "valu_sgpr_or_literal", "salu", "lds", "global", "branches")}))
        return
    print("%s, node-visit path of the walk loop%s" % (KERNEL, (" (" + " ".join(extra) + ")") if extra else ""))
    print("  VALU instructions                       %d" % c["valu"])
    print("  ... reading an SGPR (pair) or a literal %d" % c["valu_sgpr_or_literal"])
    print("  SALU %d   branches %d   LDS %d   global loads %d" % (c["salu"], c["branches"], c["lds"], c["global"]))
    for k, n in sorted(c["mnemonics"].items(), key=lambda kv: (-kv[1], kv[0])):
        print("    %-28s %3d" % (k, n))
    if "--blocks" in sys.argv:
        print("  blocks of the walk loop (label, lines, instructions, VALU, skipped):")
        for lab, s, e, n, v, sk in c["blocks"]:
            print("    %-12s %5d-%-5d %4d %4d %s" % (lab, s, e, n, v, "-" if sk else "+"))


if __name__ == "__main__":
    main()
