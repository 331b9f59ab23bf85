#!/usr/bin/env python3
"""What one node visit of stage 2 costs in the ISA, without a GPU.

Compiles rust-raytracing_amd/csrc/rtx_bvh_spheres.hip for gfx950 with the flags of build.py (device code only, to assembly), takes
trace_bvh_spheres_kernel<false, 2, 2> (stage 2 of the sphere path) and counts the node-visit path of its walk loop:

    walk loop     the innermost loop around the block that fetches the 64-byte node (four global_load_dwordx4)
    the path      the blocks of that loop in layout order, without
                    - the leaf visit: from the block that decodes a leaf link (v_lshrrev_b32 .., 29, ..) up to the block that pops
                      the stack (the first ds_read_b32 outside a nested loop after it), nested loops included
                    - the pushes of a lane without room for three rows: the blocks between the visit's main block (the one with
                      the v_cvt_f32_ubyte) and the target of the s_cbranch_execz that ends it, as far as they are reached from
                      the main block's fall-through
                  -- what a wave issues in an iteration in which it visits nodes and every lane has room on its LDS stack

The two exclusions are recognised by what this compiler (AMD clang 22) emits for them -- the shift by 29 that decodes a leaf link, the
s_cbranch_execz that ends the main block -- and the blocks are taken in layout order: a compiler that lays the loop out differently can
move the counts without any change of the source.  The test that pins them checks that the path found holds one node fetch, the pushes
and the pop; when it fails after a toolchain change, look at --blocks before looking at the kernel.

It prints the VALU instructions on the path, how many of them read an SGPR, an SGPR pair or a literal (or write an SGPR pair: the
v_cmp e64 forms), the SALU and LDS instructions, and the per-mnemonic table.

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


def loops_of(body):
    label_at = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    by_head = {}
    for i, l in enumerate(body):
        m = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] <= i:
            a = label_at[m.group(1)]
            by_head[a] = max(by_head.get(a, a), i)
    return sorted(by_head.items()), label_at


def blocks_of(body, a, b):
    """[(first line, last line)] of the basic blocks inside body[a..b]: a block starts at a label or a '; %bb.N:' line."""
    starts = [i for i in range(a, b + 1) if re.match(r"^\.LBB\d+_\d+:", body[i]) or re.match(r"^; %bb\.\d+:", body[i])]
    if not starts or starts[0] != a:
        starts = [a] + starts
    return [(s, (starts[k + 1] - 1 if k + 1 < len(starts) else b)) for k, s in enumerate(starts)]


SGPR = re.compile(r"\bs\d+\b|\bs\[\d+:\d+\]|\b0x[0-9a-f]+\b|\bexec\b")


def visit_counts(asm):
    """Counts of the node-visit path; `asm` is the assembly text (compile_asm) or the path of a .s file."""
    body = kernel_body((asm if "\n" in asm else open(asm).read()).splitlines())
    loops, label_at = loops_of(body)
    fetch = [i for i, l in enumerate(body) if "global_load_dwordx4" in l]
    # the node fetch: four loads off one base register within a few lines
    node_fetch = next(i for k, i in enumerate(fetch) if k + 3 < len(fetch) and fetch[k + 3] - i <= 8 and
                      len({re.search(r"(v\[\d+:\d+\]), off", body[j]).group(1) for j in fetch[k:k + 4]}) == 1 and
                      any("v_cvt_f32_ubyte" in l for l in body[i:i + 40]))
    a, b = min(((a, b) for a, b in loops if a <= node_fetch <= b), key=lambda ab: ab[1] - ab[0])
    nested = [(c, d) for c, d in loops if a < c and d <= b]
    blocks = blocks_of(body, a, b)
    main = next(k for k, (s, e) in enumerate(blocks) if s <= node_fetch <= e)
    skip = set()
    # the pushes of a lane without room: what the branch at the end of the main block jumps over
    last = next(l for l in reversed(body[blocks[main][0]:blocks[main][1] + 1]) if is_instr(l))
    m = re.search(r"s_cbranch_execz\s+(\.LBB\d+_\d+)", last)
    if m and label_at[m.group(1)] > blocks[main][1]:
        # ... followed through the branches, so that glue blocks that merely lie in between stay on the path
        stop = label_at[m.group(1)]
        block_at = lambda i: next(k for k, (s, e) in enumerate(blocks) if s <= i <= e)
        todo = [main + 1]
        while todo:
            k = todo.pop()
            if k in skip or k >= len(blocks) or not (blocks[main][1] < blocks[k][0] < stop):
                continue
            skip.add(k)
            ins = [l.strip() for l in body[blocks[k][0]:blocks[k][1] + 1] if is_instr(l)]
            for l in ins:
                t = re.search(r"\bs_c?branch\w*\s+(\.LBB\d+_\d+)", l)
                if t and a <= label_at.get(t.group(1), -1) <= b:
                    todo.append(block_at(label_at[t.group(1)]))
            if not (ins and ins[-1].startswith("s_branch")):
                todo.append(k + 1)
    # the leaf visit
    in_nested = lambda i: any(c <= i <= d for c, d in nested)
    leaf0 = next((k for k, (s, e) in enumerate(blocks) if k > main and k not in skip and
                  any(re.search(r"v_lshrrev_b32_e32 v\d+, 29, ", l) for l in body[s:e + 1])), None)
    if leaf0 is not None:
        last_nested = max(d for c, d in nested) if nested else blocks[leaf0][1]
        pop = next((k for k, (s, e) in enumerate(blocks) if s > last_nested and
                    any("ds_read_b32" in l for l in body[s:e + 1])), len(blocks))
        skip.update(range(leaf0, pop))
    out = {"valu": 0, "valu_sgpr_or_literal": 0, "salu": 0, "lds": 0, "global": 0, "branches": 0, "mnemonics": {}, "blocks": []}
    for k, (s, e) in enumerate(blocks):
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
