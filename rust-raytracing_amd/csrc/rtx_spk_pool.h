// rtx_spk_pool.h -- the wave-local pool of primary hits of the packet kernel (trace_sph_packet_kernel, rtx_bvh_spheres.hip).
//
// Behind a packet's exact tests some lanes hold a hit and the others (misses, the padding of a partial tile) hold nothing; the
// shading block behind them costs the same with one lane as with 64.  So a wave keeps up to 63 hits in 64 slots of its own and
// runs the block only when it can fill every lane: with P hits pooled and n new ones (the set bits of the ballot m),
//   P + n >= 64   the 64 - n lanes without a hit pull one pooled hit each (rank k among them: slot P - 1 - k), all 64 lanes shade,
//                 P -= 64 - n
//   otherwise     the lanes with a hit push it (rank k among them: slot P + k), nobody shades, P += n
// and when the wave leaves, lanes k < P pull slot k and shade once (the flush).  A hit is shaded exactly once, a slot is read only
// while it is live (the pool is a stack: pushes above P, pulls from below it), and P stays below 64.
// Nothing here but integer arithmetic, and no header of the project: the host compiles it as it stands (tests/test_spk_pool.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_SPK_POOL_HD __host__ __device__ inline
#else
#define RTX_SPK_POOL_HD inline
#endif

namespace rtx {

constexpr uint32_t kSpkPoolSlots = 64;        // per wave; at most 63 are ever live

enum SpkPoolAction : uint32_t {
    kSpkPoolKeep = 0,                         // the lane shades the hit it holds
    kSpkPoolPush = 1,                         // the lane writes its hit to `slot` and does not shade
    kSpkPoolPull = 2,                         // the lane reads the hit of `slot` and shades it
    kSpkPoolIdle = 3                          // the lane holds nothing and does nothing
};

struct SpkPoolStep { uint32_t action, slot; };

RTX_SPK_POOL_HD uint32_t spk_pool_popcount(uint64_t m)
{
    return (uint32_t)__builtin_popcountll((unsigned long long)m);
}

// does the shading block run for a packet whose lanes with a hit are `m`, with `pool` hits pooled (pool < 64)?
RTX_SPK_POOL_HD bool spk_pool_shades(uint64_t m, uint32_t pool) { return pool + spk_pool_popcount(m) >= kSpkPoolSlots; }

// the pool's count behind that packet
RTX_SPK_POOL_HD uint32_t spk_pool_next(uint64_t m, uint32_t pool)
{
    const uint32_t n = spk_pool_popcount(m);
    return pool + n >= kSpkPoolSlots ? pool + n - kSpkPoolSlots : pool + n;
}

// what `lane` (< 64) does in that packet
RTX_SPK_POOL_HD SpkPoolStep spk_pool_lane(uint64_t m, uint32_t lane, uint32_t pool)
{
    const bool hit = ((m >> lane) & 1ull) != 0ull;
    const uint32_t hits_below = spk_pool_popcount(m & ((1ull << lane) - 1ull));     // the lane's rank among the lanes with a hit ...
    const uint32_t idle_below = lane - hits_below;                                   // ... and among those without one
    SpkPoolStep s;
    if (spk_pool_shades(m, pool)) {
        s.action = hit ? kSpkPoolKeep : kSpkPoolPull;
        s.slot = hit ? 0u : pool - 1u - idle_below;             // (64 - n <= pool: every idle lane finds a slot)
    } else {
        s.action = hit ? kSpkPoolPush : kSpkPoolIdle;
        s.slot = hit ? pool + hits_below : 0u;                  // (pool + n < 64)
    }
    return s;
}

// the flush of a leaving wave: lanes below the count pull their own slot, the count falls to zero
RTX_SPK_POOL_HD SpkPoolStep spk_pool_flush_lane(uint32_t lane, uint32_t pool)
{
    SpkPoolStep s;
    s.action = lane < pool ? kSpkPoolPull : kSpkPoolIdle;
    s.slot = lane < pool ? lane : 0u;
    return s;
}

}  // namespace rtx
