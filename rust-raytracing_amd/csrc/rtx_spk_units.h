// rtx_spk_units.h -- the work units of the packet kernel (trace_sph_packet_kernel, rtx_bvh_spheres.hip).
//
// A launch holds n_tiles 8x8 tiles x n_samples samples, one packet of 64 rays each.  A unit is a run of at most `group`
// consecutive samples of ONE tile, so that what a packet derives from its tile alone is derived once per unit.  The units are
// numbered run by run: first every tile's samples [0, group), then every tile's [group, 2 group), ...; the last run of a tile holds
// what is left.  Consecutive units are therefore neighbouring tiles, as consecutive packets were before: the launch still
// sweeps the frame once per run of samples.  Nothing here but integer arithmetic, and no header of the project: the host
// compiles it as it stands (tests/test_spk_units.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_SPK_HD __host__ __device__ inline
#else
#define RTX_SPK_HD inline
#endif

namespace rtx {

struct SpkUnit { uint32_t tile, first, count; };          // samples [first, first + count) of the launch (local: 0 = rv.sample_begin)

// runs per tile (group >= 1)
RTX_SPK_HD uint32_t spk_runs_per_tile(uint32_t n_samples, uint32_t group) { return (n_samples + group - 1u) / group; }

// units of a launch (64 bits: the counter they are drawn from is a u64; a launch's packets, hence its units, stay below 2^26)
RTX_SPK_HD uint64_t spk_unit_count(uint32_t n_tiles, uint32_t n_samples, uint32_t group)
{
    return (uint64_t)n_tiles * spk_runs_per_tile(n_samples, group);
}

// unit u < spk_unit_count(n_tiles, n_samples, group) -> its tile and samples
RTX_SPK_HD SpkUnit spk_unit(uint32_t u, uint32_t n_tiles, uint32_t n_samples, uint32_t group)
{
    const uint32_t run = u / n_tiles;
    SpkUnit w;
    w.tile = u - run * n_tiles;
    w.first = run * group;
    w.count = n_samples - w.first < group ? n_samples - w.first : group;
    return w;
}

}  // namespace rtx
