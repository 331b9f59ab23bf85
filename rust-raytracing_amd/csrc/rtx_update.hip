// rtx_update.hip -- scene_update_kernel: rtx_scene_update_objects and rtx_scene_set_visible on the device (include/rtx_hip.h, DESIGN.md
// "Moving objects", "Hidden objects").
// One kernel, a launch-uniform mode (UpdateArgs, rtx_refit.h); the arithmetic is rtx_refit.h's, which the host reference
// refit_packed (rtx_pack.hip) compiles too.  No spin-waits, no dependence between the blocks of one launch; threads write
// disjoint words (mode B reads the nodes the previous launch wrote: the host enqueues the levels deepest first on one stream).
#include "rtx_launch.h"

namespace rtx {

__global__ __launch_bounds__(256) void scene_update_kernel(UpdateArgs u)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (u.mode == 0u) {                                   // A: one entry's records
        if (i < u.n) update_record(u, i);
        return;
    }
    if (u.mode == 1u) {                                   // B: one wide node of this level
        if (i < u.n) { const unsigned long long bad = refit_level_entry(u, u.level[i]); if (bad) atomicOr(u.status, bad); }
        return;
    }
    if (u.mode == 4u) {                                   // E: the kept words of one wide node (the first visibility call after a pack)
        if (i < u.n) capture_keep(u, u.level[i]);
        return;
    }
    // C: sphere_cmax = max of reach;  D: tri_extent = max of tri_reach.  Grid-stride, then the 64-lane wave, then one atomicMax per wave on the bit pattern
    // (non-negative doubles order like their bits; a launch of mode C only runs when every reach is finite).
    const double *src = u.mode == 2u ? u.reach : u.tri_reach;
    double m = 0.0;
    for (uint64_t k = i; k < u.n; k += (uint64_t)gridDim.x * blockDim.x) { const double r = src[k]; m = r > m ? r : m; }
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(m, off, 64); m = o > m ? o : m; }
    if ((threadIdx.x & 63u) == 0u) atomicMax(u.status + (u.mode == 2u ? 1 : 2), (unsigned long long)__double_as_longlong(m));
}

hipError_t launch_scene_update(const UpdateArgs &u, hipStream_t stream)
{
    if (u.n == 0) return hipSuccess;
    uint32_t blocks = (uint32_t)(((uint64_t)u.n + 255u) / 256u);
    if ((u.mode == 2u || u.mode == 3u) && blocks > 1024u) blocks = 1024u;
    hipLaunchKernelGGL(scene_update_kernel, dim3(blocks), dim3(256), 0, stream, u);
    return hipGetLastError();
}

}  // namespace rtx
