"""The packet kernel's pool of primary hits (rust-raytracing_amd/csrc/rtx_spk_pool.h) and its place in the product library, without a GPU.

spk_pool_lane / spk_pool_next / spk_pool_flush_lane are the functions that say which lane shades which hit and when: the header is
compiled as it stands into a small host program that walks sequences of hit masks through them and prints every lane's action.  A
model of the 64 slots then follows the transcript: every hit must be shaded exactly once, the count must stay below 64, a slot must
be written before it is read and not written again while it is live, every pass before the flush must run with all 64 lanes, and the
flush must empty the pool.  A second build of the same program with -fsanitize=address,undefined runs the same sequences stand-alone.
"""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytracing_amd", "csrc")

# argv: hexadecimal hit masks, "-" ends a sequence (a wave's life).  Per packet: "p <pool before> <shades> <pool after>" and 64
# "<action> <slot>" pairs on one line; per flush "f <pool before>" and the same.
MAIN = r"""
#include "rtx_spk_pool.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
int main(int argc, char **argv)
{
    uint32_t pool = 0;
    std::printf("seq\n");
    for (int a = 1; a < argc; ++a) {
        if (std::strcmp(argv[a], "-") == 0) {
            std::printf("f %u", pool);
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const rtx::SpkPoolStep s = rtx::spk_pool_flush_lane(lane, pool);
                std::printf(" %u %u", (unsigned)s.action, s.slot);
            }
            std::printf("\nseq\n");
            pool = 0;
            continue;
        }
        const uint64_t m = std::strtoull(argv[a], nullptr, 16);
        std::printf("p %u %d %u", pool, rtx::spk_pool_shades(m, pool) ? 1 : 0, rtx::spk_pool_next(m, pool));
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const rtx::SpkPoolStep s = rtx::spk_pool_lane(m, lane, pool);
            std::printf(" %u %u", (unsigned)s.action, s.slot);
        }
        std::printf("\n");
        pool = rtx::spk_pool_next(m, pool);
    }
    return 0;
}
"""

KEEP, PUSH, PULL, IDLE = 0, 1, 2, 3
ALL = (1 << 64) - 1


def _sequences():
    rng = random.Random(0x5EED)
    low = lambda n: (1 << n) - 1
    seqs = [
        [],                                                   # a wave that met nothing
        [0],
        [0] * 5,
        [ALL],
        [ALL] * 3,
        [1], [1 << 63], [1 << 31],                            # one lane, the flush alone
        [low(63), 1],                                         # 63 then 1: the pool is full to its last slot, then one pass
        [low(63), 1 << 63],
        [low(63), low(63), low(63)],
        [low(63) << 1, 1, 0, ALL, 1],
        [low(31)] * 40,                                       # long runs of 31: 31, 62, then a pass leaves 29, ...
        [low(31) << 33] * 40,
        [low(31) << 16, low(31)] * 20,
        [low(32)] * 9,                                        # exactly 64 at every second packet: a pass that leaves 0
        [0x5555555555555555, 0xAAAAAAAAAAAAAAAA] * 7,
        [1 << (k % 64) for k in range(200)],                  # one hit per packet: 63 packets fill, the 64th shades
        [ALL ^ (1 << (k % 64)) for k in range(70)],           # 63 per packet
    ]
    for density in (0.02, 0.2, 0.5, 0.645, 0.9, 0.99):
        for _ in range(4):
            seqs.append([sum(1 << b for b in range(64) if rng.random() < density) for _ in range(rng.randrange(1, 120))])
    for _ in range(8):                                        # a frame's mix: empty tiles, full tiles, edges
        seqs.append([rng.choice((0, ALL, low(rng.randrange(1, 64)), rng.getrandbits(64), rng.getrandbits(64) & rng.getrandbits(64)))
                     for _ in range(rng.randrange(1, 150))])
    return seqs


def _follow(seq, lines):
    """One wave's transcript against a model of its 64 slots; hits are named (packet, lane)."""
    assert len(lines) == len(seq) + 1, (len(lines), len(seq))
    slots = [None] * 64                                       # the hit a slot holds while it is live
    pool, shaded, passes = 0, {}, 0
    every = set()
    for p, (m, line) in enumerate(zip(seq, lines)):
        f = line.split()
        assert f[0] == "p" and int(f[1]) == pool, (p, line)
        shades, nxt = int(f[2]), int(f[3])
        steps = [(int(f[4 + 2 * k]), int(f[5 + 2 * k])) for k in range(64)]
        n = bin(m).count("1")
        assert shades == (1 if pool + n >= 64 else 0)
        lanes_shading = 0
        pushes, pulls = [], []
        for lane, (action, slot) in enumerate(steps):
            hit = (m >> lane) & 1
            if hit:
                every.add((p, lane))
            if shades:
                assert action == (KEEP if hit else PULL), (p, lane, action)
            else:
                assert action == (PUSH if hit else IDLE), (p, lane, action)
            if action == KEEP:
                shaded[(p, lane)] = shaded.get((p, lane), 0) + 1
                lanes_shading += 1
            elif action == PUSH:
                pushes.append((slot, (p, lane)))
            elif action == PULL:
                pulls.append(slot)
                lanes_shading += 1
        # pulls come first in the kernel's order only in a packet that shades, pushes only in one that does not: never both
        assert not (pushes and pulls)
        for slot in pulls:
            assert 0 <= slot < 64 and slots[slot] is not None, "slot %d read before it was written (packet %d)" % (slot, p)
            assert slot < pool
            shaded[slots[slot]] = shaded.get(slots[slot], 0) + 1
            slots[slot] = None
        for slot, who in pushes:
            assert 0 <= slot < 64 and slots[slot] is None, "slot %d written while live (packet %d)" % (slot, p)
            assert slot >= pool
            slots[slot] = who
        if shades:
            passes += 1
            assert lanes_shading == 64, "a pass before the flush runs with 64 lanes (packet %d: %d)" % (p, lanes_shading)
        pool = pool + n - 64 if shades else pool + n
        assert nxt == pool and 0 <= pool < 64, (p, nxt, pool)
        assert sum(s is not None for s in slots) == pool and all(s is not None for s in slots[:pool]), "the live slots are [0, pool)"
    f = lines[-1].split()
    assert f[0] == "f" and int(f[1]) == pool
    for lane in range(64):
        action, slot = int(f[2 + 2 * lane]), int(f[3 + 2 * lane])
        if lane < pool:
            assert action == PULL and slot == lane and slots[slot] is not None
            shaded[slots[slot]] = shaded.get(slots[slot], 0) + 1
            slots[slot] = None
        else:
            assert action == IDLE
    assert all(s is None for s in slots), "the flush empties the pool"
    assert shaded == {h: 1 for h in every}, "every hit is shaded exactly once"
    return passes


def _build(tmp_path, name, extra):
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I" + CSRC, str(src), "-o", str(exe)])
    return exe


def _run(exe, seqs):
    args = []
    for s in seqs:
        args += ["%x" % m for m in s] + ["-"]
    text = subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout
    blocks = text.split("seq\n")[1:]
    assert blocks[-1] == "" and len(blocks) == len(seqs) + 1
    return [b.strip().split("\n") for b in blocks[:-1]]


def test_every_hit_is_shaded_once_and_full_passes_only_before_the_flush(tmp_path):
    seqs = _sequences()
    blocks = _run(_build(tmp_path, "pool", []), seqs)
    total_hits = total_passes = 0
    for seq, lines in zip(seqs, blocks):
        passes = _follow(seq, lines)
        hits = sum(bin(m).count("1") for m in seq)
        assert passes == hits // 64, "a pass per 64 hits, the rest in the flush"
        total_hits += hits
        total_passes += passes
    assert total_passes > 100 and total_hits > 64 * total_passes


def test_the_same_walk_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone program alone is built with the sanitizers; its transcript must be the plain build's"""
    seqs = _sequences()
    plain = _run(_build(tmp_path, "pool", []), seqs)
    san = _run(_build(tmp_path, "pool_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), seqs)
    assert san == plain


def test_the_pool_fits_the_packet_kernel_into_four_workgroups_per_cu():
    """tools/kernel_instances.py on the built product library: at most 25 kernel instances, one trace_sph_packet_kernel with at most
    128 VGPRs, no spilled VGPR and no scratch, and its static LDS (the candidate queues + the pool) at most 40 KB: four workgroups
    share a CU's 160 KB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_instances
    lib = os.path.join(ROOT, "rust-raytracing_amd", "librtx_hip.so")
    if not os.path.exists(lib):
        pytest.fail("librtx_hip.so is not built (python rust-raytracing_amd/build.py)")
    rows = kernel_instances.kernels(lib)
    assert len(rows) <= 25, len(rows)
    pk = [r for r in rows if r["name"] == "trace_sph_packet_kernel"]
    assert len(pk) == 1, [r["name"] for r in rows]
    print(pk[0])
    assert pk[0]["vgpr"] <= 128 and pk[0]["vgpr_spill"] == 0 and pk[0]["scratch"] == 0, pk[0]
    assert pk[0]["lds"] <= 40 * 1024, pk[0]
