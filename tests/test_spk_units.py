"""The packet kernel's work units (rust-raytracing_amd/csrc/rtx_spk_units.h) and its place in the product library, without a GPU.

spk_unit is the one function that says which wave meets which (tile, sample): the header is compiled as it stands into a small host
program that walks every unit of a launch and prints (tile, first sample, count); every (tile, sample) of the launch must then be
visited exactly once, runs must not cross a tile, and only a tile's last run may be short.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-raytracing_amd", "csrc")

MAIN = r"""
#include "rtx_spk_units.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv)
{
    for (int a = 1; a + 2 < argc; a += 3) {
        const uint32_t tiles = (uint32_t)atoi(argv[a]), samples = (uint32_t)atoi(argv[a + 1]), group = (uint32_t)atoi(argv[a + 2]);
        const uint64_t n = rtx::spk_unit_count(tiles, samples, group);
        std::printf("launch %u %u %u %llu\n", tiles, samples, group, (unsigned long long)n);
        for (uint64_t u = 0; u < n; ++u) {
            const rtx::SpkUnit w = rtx::spk_unit((uint32_t)u, tiles, samples, group);
            std::printf("%u %u %u\n", w.tile, w.first, w.count);
        }
    }
    return 0;
}
"""


def _launches():
    out = []
    for g in range(1, 17):
        for samples in sorted({1, g - 1, g, g + 1, 2 * g + 1} - {0}):
            for tiles in (1, 2, 7):
                out.append((tiles, samples, g))
    return out


def test_every_tile_and_sample_of_a_launch_is_visited_exactly_once(tmp_path):
    src, exe = tmp_path / "units.cpp", tmp_path / "units"
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    launches = _launches()
    text = subprocess.run([str(exe)] + [str(v) for l in launches for v in l], capture_output=True, text=True, check=True).stdout
    blocks = text.split("launch ")[1:]
    assert len(blocks) == len(launches)
    for (tiles, samples, g), block in zip(launches, blocks):
        lines = block.strip().split("\n")
        assert [int(v) for v in lines[0].split()] == [tiles, samples, g, tiles * ((samples + g - 1) // g)], lines[0]
        units = [tuple(int(v) for v in l.split()) for l in lines[1:]]
        assert len(units) == tiles * ((samples + g - 1) // g)
        seen = {}
        for tile, first, count in units:
            assert tile < tiles and 1 <= count <= g and first % g == 0 and first + count <= samples, (tiles, samples, g, tile, first, count)
            assert count == g or first + count == samples, "only a tile's last run is short"
            for s in range(first, first + count):
                seen[(tile, s)] = seen.get((tile, s), 0) + 1
        assert seen == {(t, s): 1 for t in range(tiles) for s in range(samples)}, (tiles, samples, g)
        assert units == sorted(units, key=lambda w: (w[1], w[0])), "run by run, a run's tiles in order"


def test_the_packet_kernel_stays_at_four_workgroups_per_cu():
    """tools/kernel_instances.py on the built product library: at most 25 kernel instances; trace_sph_packet_kernel at most 128 VGPRs, no
    spilled VGPR, no scratch (so none inside its list loop or its sample loop), which is what 4 workgroups of 256 per CU need."""
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
