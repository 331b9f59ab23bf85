// rtx_kernels.hip -- gfx950 (MI355X, CDNA4) kernels of the Scene::render hot path.
//
//   trace_exact_kernel  one thread per ray (pixel, sample); every shape test in f64 in the
//                       reference's operation order.  The parity kernel.
//   trace_mixed_kernel  persistent workgroups; each lane owns S ray slots whose f64 state lives in
//                       HBM structure-of-arrays; the sphere list is staged through LDS in chunks as
//                       16-byte f32 records and swept with a conservative f32 discriminant filter
//                       (9 VALU ops per sphere per ray, one broadcast ds_read_b128 shared by 64*S
//                       rays); candidates the filter cannot exclude are queued per slot in LDS and
//                       re-evaluated exactly in f64, so the result has the same bits as
//                       trace_exact_kernel.  Dead slots are refilled from a global ray queue with a
//                       wave ballot + mbcnt prefix sum (one atomic per workgroup per round).
//   resolve_kernel      left fold of a pixel's samples in sample order, then / rays_per_pixel.
//   epilogue_kernel     render_to_image's quantize, the multi-device gather, the two forms of the denoiser (rtx_denoise.h), the
//                       temporal accumulation (rtx_temporal.h), the rewind of a pick buffer (rtx_rewind.h) and the guided upsampling
//                       (rtx_upsample.h), by a launch-uniform form.
//
// Compiled with -ffp-contract=off; the f32 filter uses explicit fmaf.
#include "rtx_launch.h"
#include "rtx_traverse.h"
#include "rtx_denoise.h"
#include "rtx_temporal.h"
#include "rtx_rewind.h"
#include "rtx_upsample.h"

#include <cstdlib>

namespace rtx {

// ------------------------------------------------------------------------------------------
// wave helpers (wave = 64 lanes on gfx950)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ uint32_t mbcnt(unsigned long long mask)      // # set bits of mask below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ void flush_counters(Counters *ctr, unsigned long long segs, unsigned long long exact,
                                               unsigned long long filt)
{
    segs = wave_sum_u64(segs);
    exact = wave_sum_u64(exact);
    filt = wave_sum_u64(filt);
    if (lane_id() == 0) {
        uint32_t shard = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (kCounterShards - 1);
        if (segs) atomicAdd(&ctr[shard].segments, segs);
        if (exact) atomicAdd(&ctr[shard].exact_tests, exact);
        if (filt) atomicAdd(&ctr[shard].filter_tests, filt);
    }
}

// closest_object (scene.rs:243-251) over every shape of one type, exact f64.
__device__ __forceinline__ void closest_spheres_exact(const SceneView &sv, const RayX &rx, Hit &h)
{
    for (uint32_t k = 0; k < sv.n_spheres; ++k) {
        double t;
        if (sphere_distance(sv.spheres[k], rx, &t)) hit_consider(h, t, sv.sphere_id[k], 0, k);
    }
}

__device__ __forceinline__ void closest_planes_exact(const SceneView &sv, const RayX &rx, Hit &h)
{
    for (uint32_t k = 0; k < sv.n_planes; ++k) {
        double t;
        if (plane_distance(sv.planes[k], rx, &t)) hit_consider(h, t, sv.planes[k].id, 1, k);
    }
}

__device__ __forceinline__ void closest_tris_exact(const SceneView &sv, const RayX &rx, Hit &h)
{
    for (uint32_t k = 0; k < sv.n_tris; ++k) {
        double t;
        if (triangle_distance(sv.tris[k], rx, &t)) hit_consider(h, t, sv.tris[k].id, 2, k);
    }
}

// ------------------------------------------------------------------------------------------
// EXACT kernel
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_exact_kernel(const SceneView *__restrict__ svp, const RowsView *__restrict__ rvp,
                                                          double *__restrict__ samples, Counters *__restrict__ ctr,
                                                          uint64_t ray_offset)
{
    // scene and launch descriptors live in device memory (not in the kernarg segment): fields are
    // (re)loaded where they are used instead of pinning ~100 SGPRs for the whole kernel
    const SceneView &sv = *svp;
    const RowsView &rv = *rvp;
    uint64_t i = ray_offset + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long segs = 0;
    if (i < rv.n_rays) {
        uint32_t pl, s_local;
        ray_index_to_pixel(rv, i, pl, s_local);
        RayState r;
        gen_primary(sv, rv, pl, rv.sample_begin + s_local, r);
        if (sv.n_objects != 0) {                                          // scene.rs:224-226
            const uint64_t limit = sv.max_bounces + 1;                    // scene.rs:227
            for (uint64_t b = 0; b < limit; ++b) {
                if (light_is_zero(r)) break;                              // scene.rs:228
                RayX rx = make_rayx(r.pos, r.dir);
                Hit h;
                hit_init(h);
                ++segs;
                closest_spheres_exact(sv, rx, h);
                closest_planes_exact(sv, rx, h);
                closest_tris_exact(sv, rx, h);
                if (h.id == 0xFFFFFFFFu) break;                           // scene.rs:238
                advance_and_shade(sv, h, r);
            }
        }
        store_sample(samples, rv, i, r.result);
    }
    flush_counters(ctr, segs, segs * sv.n_objects, 0);
}

#ifdef RTX_LAB
// The EXACT kernel's loop once more, writing every segment down (rtx_debug_paths): step b of the path of local pixel pl, sample s
// goes to steps[(pl * n_samples + s) * max_steps + b] while b < max_steps; counts[] takes the path's number of segments.
__global__ __launch_bounds__(256) void trace_transcript_kernel(const SceneView *__restrict__ svp, const RowsView *__restrict__ rvp,
                                                               PathStep *__restrict__ steps, uint32_t *__restrict__ counts, uint32_t max_steps)
{
    const SceneView &sv = *svp;
    const RowsView &rv = *rvp;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rv.n_rays) return;
    uint32_t pl, s_local;
    ray_index_to_pixel(rv, i, pl, s_local);
    RayState r;
    gen_primary(sv, rv, pl, rv.sample_begin + s_local, r);
    PathStep *out = steps + ((size_t)pl * rv.n_samples + s_local) * max_steps;
    uint32_t n = 0;
    if (sv.n_objects != 0) {
        const uint64_t limit = sv.max_bounces + 1;
        for (uint64_t b = 0; b < limit; ++b) {
            if (light_is_zero(r)) break;
            RayX rx = make_rayx(r.pos, r.dir);
            Hit h;
            hit_init(h);
            closest_spheres_exact(sv, rx, h);
            closest_planes_exact(sv, rx, h);
            closest_tris_exact(sv, rx, h);
            const bool miss = h.id == 0xFFFFFFFFu;
            if (n < max_steps) {
                PathStep st;
                st.pos[0] = r.pos.x; st.pos[1] = r.pos.y; st.pos[2] = r.pos.z;
                st.dir[0] = r.dir.x; st.dir[1] = r.dir.y; st.dir[2] = r.dir.z;
                st.t = miss ? __builtin_inf() : h.t;
                st.object = miss ? -1ll : (long long)h.id;
                out[n] = st;
            }
            ++n;
            if (miss) break;
            advance_and_shade(sv, h, r);
        }
    }
    counts[(size_t)pl * rv.n_samples + s_local] = n;
}

hipError_t launch_trace_transcript(const SceneView *d_sv, const RowsView *d_rv, const RowsView &rv, PathStep *steps, uint32_t *counts,
                                   uint32_t max_steps, hipStream_t stream)
{
    if (rv.n_rays == 0) return hipSuccess;
    if (rv.n_rays > (1ull << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(trace_transcript_kernel, dim3((uint32_t)((rv.n_rays + 255) / 256)), dim3(256), 0, stream, d_sv, d_rv, steps, counts, max_steps);
    return hipGetLastError();
}
#endif

// ------------------------------------------------------------------------------------------
// MIXED kernel
// ------------------------------------------------------------------------------------------
constexpr uint32_t kInvalid = 0xFFFFFFFFu;

// The f32 filter evaluates  D = ((c-p).d)^2 - (|c-p|^2 - r^2)  (a quarter of the reference's
// discriminant for |d| = 1, sphere.rs:22-25) in the expanded form
//     b = c.d - p.d            q = 2 c.p - p.p + E            D = b*b + (q - (c.c - r*r))
// with all points relative to the scene centre.  E bounds the f32 evaluation error, so a sphere the
// reference could report (discriminant > 1e-100) always has D_f32 >= 0 and is queued (held by tests/test_sweep_filters.py on rays
// aimed at the filter; the measured use of E is in rtx_device.h, filter_from_ray).
// Two spheres are evaluated per instruction (v_pk_fma_f32): LDS holds the records pair-interleaved,
//     float4 A = {x0, x1, y0, y1}   float4 B = {z0, z1, w0, w1},   w = |c|^2 - r^2
// and the slot holds {d.xyz, -p.d, 2p.xyz, -p.p + E}.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// D for the two spheres of one LDS pair record
__device__ __forceinline__ f32x2 filter_disc2(const float4 A, const float4 B, const FilterParams &f)
{
    const f32x2 x = {A.x, A.y}, y = {A.z, A.w}, z = {B.x, B.y}, w = {B.z, B.w};
    f32x2 b = __builtin_elementwise_fma(z, (f32x2){f.dz, f.dz}, (f32x2){f.npd, f.npd});
    b = __builtin_elementwise_fma(y, (f32x2){f.dy, f.dy}, b);
    b = __builtin_elementwise_fma(x, (f32x2){f.dx, f.dx}, b);
    f32x2 q = __builtin_elementwise_fma(z, (f32x2){f.p2z, f.p2z}, (f32x2){f.nppE, f.nppE});
    q = __builtin_elementwise_fma(y, (f32x2){f.p2y, f.p2y}, q);
    q = __builtin_elementwise_fma(x, (f32x2){f.p2x, f.p2x}, q);
    return __builtin_elementwise_fma(b, b, q - w);
}

// Per-slot data that lives between rounds, structure-of-arrays in HBM (slot = lane_gid + s * n_lanes):
//   state  [12][n_slots] f64   ray.position, ray.direction, resulting_color, light_color  (ray.rs:4-21)
//   fstate [16][n_slots] f32   the slot's sphere-filter (0-7) and triangle-filter (8-15) parameters
//   istate [ 3][n_slots] u32   local pixel, batch-local sample, bounce count
//   oflow  [24][n_slots] u32   candidates beyond the Q-entry LDS queue (a ray that collects more than Q + 24
//                              candidates falls back to the exhaustive exact sweep)
// Only a one-bit-per-slot `live` mask stays in registers across rounds, so the heavy f64 code (primary ray
// generation, exact tests, shading) exists once and loops over the slots instead of being unrolled S times.
constexpr int kOverflowQ = 24;             // candidates per slot beyond the LDS queue, kept in HBM (rare)
constexpr size_t kSlotBytes = 12 * sizeof(double) + 16 * sizeof(float) + (3 + kOverflowQ) * sizeof(uint32_t);

#ifdef RTX_LAB
// rtx_debug_sweep_filter: the sweep's two f32 filters for single rays, by the functions the sweep itself calls (filter_from_ray /
// tri_filter_from_ray as the refill calls them, filter_disc2 on the resident pair records, filter_disc1, tri_filter_sign), one thread
// per entry.  pairs (a.entries != null): 24 words per entry (include/rtx_hip.h), entry i = ray i and the record a.entries[i] -- a
// sphere's index, or bit 31 | a triangle filter record, or ~0: the object has no filter record.  counts (a.entries == null): 4 words
// per ray -- the records of the whole padded sphere array and of the n_tri_filter triangle records whose sign bit is clear: what the
// sweep queues for that ray -- and the two pass-all flags.
__global__ __launch_bounds__(256) void debug_sweep_filter_kernel(const SceneView *__restrict__ svp, SweepFilterArgs a)
{
    const SceneView &sv = *svp;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const QueryRay ray = a.rays[i];
    const V3 pos = mk(ray.position[0], ray.position[1], ray.position[2]), dir = mk(ray.direction[0], ray.direction[1], ray.direction[2]);
    FilterParams f;
    filter_from_ray(sv, pos, dir, f);
    TriFilterParams tf;
    if (sv.n_tri_filter != 0) tri_filter_from_ray(sv, pos, dir, tf); else tri_filter_idle(tf);
    const bool s_all = f.nppE == 1.0e30f, t_all = tf.A == 1.0e30f;      // (inside the range gates |nppE| and A stay below 1e24)
    if (!a.entries) {
        uint32_t *o = a.out + i * 4;
        uint32_t n_s = 0, n_t = 0;
        const uint32_t ns4 = (sv.n_spheres + 3u) & ~3u;
        for (uint32_t j = 0; j < ns4; j += 2) {
            const f32x2 d = filter_disc2(sv.sphere_f32[j], sv.sphere_f32[j + 1], f);
            n_s += ((int)__float_as_uint(d.x) >= 0) + ((int)__float_as_uint(d.y) >= 0);
        }
        for (uint32_t r = 0; r < sv.n_tri_filter; ++r)
            n_t += (int)tri_filter_sign(sv.tri_f32[2 * (size_t)r], sv.tri_f32[2 * (size_t)r + 1], tf) >= 0;
        o[0] = n_s; o[1] = n_t; o[2] = (s_all ? 4u : 0u) | (t_all ? 16u : 0u); o[3] = 0u;
        return;
    }
    uint32_t *o = a.out + i * 24;
    for (int w = 0; w < 24; ++w) o[w] = 0u;
    const uint32_t e = a.entries[i];
    if (e == 0xFFFFFFFFu) return;
    if (e & 0x80000000u) {
        const uint32_t r = e & 0x7FFFFFFFu;
        const float4 A = sv.tri_f32[2 * (size_t)r], B = sv.tri_f32[2 * (size_t)r + 1];
        const uint32_t sg = tri_filter_sign(A, B, tf);
        o[0] = 1u | 2u | (t_all ? 4u : 0u) | ((int)sg >= 0 ? 8u : 0u);
        const float p[8] = { tf.dx, tf.dy, tf.dz, tf.npx, tf.npy, tf.npz, tf.A, tf.pad };
        const float rec[8] = { A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w };
        for (int w = 0; w < 8; ++w) { o[1 + w] = __float_as_uint(p[w]); o[9 + w] = __float_as_uint(rec[w]); }
        o[17] = sg; o[19] = r;
        return;
    }
    const uint32_t k = e, odd = k & 1u;
    const float4 A = sv.sphere_f32[(size_t)(k & ~1u)], B = sv.sphere_f32[(size_t)(k | 1u)];      // the pair's two float4
    const f32x2 d2 = filter_disc2(A, B, f);
    const float4 s = odd ? make_float4(A.y, A.w, B.y, B.w) : make_float4(A.x, A.z, B.x, B.z);
    const float D2 = odd ? d2.y : d2.x, D1 = filter_disc1(s, f);
    o[0] = 2u | (s_all ? 4u : 0u) | ((int)__float_as_uint(D2) >= 0 ? 8u : 0u);
    const float p[8] = { f.dx, f.dy, f.dz, f.npd, f.p2x, f.p2y, f.p2z, f.nppE };
    for (int w = 0; w < 8; ++w) o[1 + w] = __float_as_uint(p[w]);
    o[9] = __float_as_uint(s.x); o[10] = __float_as_uint(s.y); o[11] = __float_as_uint(s.z); o[12] = __float_as_uint(s.w);
    o[17] = __float_as_uint(D2); o[18] = __float_as_uint(D1); o[19] = k;
}
#endif

template <int S, int THREADS, int CHUNK, int Q, int WAVES_PER_EU>
__global__ __launch_bounds__(THREADS, WAVES_PER_EU) void trace_mixed_kernel(const SceneView *__restrict__ svp,
                                                              const RowsView *__restrict__ rvp, double *__restrict__ samples,
                                                              char *__restrict__ slot_mem, Counters *__restrict__ ctr,
                                                              unsigned long long *__restrict__ work_counter,
                                                              uint32_t verify, unsigned long long max_rounds)
{
    const SceneView &sv = *svp;
    const RowsView &rv = *rvp;
    constexpr int WAVES = THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *lds_sph = reinterpret_cast<float4 *>(smem);                                  // [CHUNK]
    uint32_t *lds_q = reinterpret_cast<uint32_t *>(smem + (size_t)CHUNK * 16);           // [Q][S][THREADS]
    uint32_t *lds_cnt = lds_q + (size_t)Q * S * THREADS;                                 // [S][THREADS]
    uint32_t *lds_misc = lds_cnt + (size_t)S * THREADS;                                  // [WAVES + 4]

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    const uint64_t n_lanes = (uint64_t)gridDim.x * THREADS;         // SoA stride between the slots of one lane
    const uint64_t n_slots = n_lanes * S;                           // SoA stride between fields
    const uint64_t lane_gid = (uint64_t)blockIdx.x * THREADS + tid;
    double *state = reinterpret_cast<double *>(slot_mem);
    float *fstate = reinterpret_cast<float *>(state + 12 * n_slots);
    uint32_t *istate = reinterpret_cast<uint32_t *>(fstate + 16 * n_slots);
    uint32_t *oflow = istate + 3 * n_slots;
    const uint32_t ns = sv.n_spheres;
    const uint32_t bounce_limit = sv.max_bounces >= 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)sv.max_bounces + 1u;

    uint32_t live = 0;                           // bit s: slot s holds a ray
    unsigned long long segs = 0, exact = 0, mism = 0, rounds_swept = 0;

    // Every round either advances every live ray by one segment or finds the queue drained, so a
    // workgroup needs at most (rays / slots + 2) * (max_bounces + 1) rounds; max_rounds is that bound
    // (computed by the launcher).  Hitting it means a logic error: the workgroup leaves and flags it.
    for (unsigned long long round = 0;; ++round) {
        if (round >= max_rounds) {
            if (tid == 0) atomicAdd(&ctr[1].pad_, 1ull);
            break;
        }
        // ---- refill idle slots from the global ray queue: ballot + prefix sum, one atomic per workgroup
        uint32_t wave_need = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) wave_need += (uint32_t)__popcll(__ballot(((live >> s) & 1u) == 0u));
        if (lane == 0) lds_misc[wave] = wave_need;
        __syncthreads();
        if (tid == 0) {
            uint32_t total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) total += lds_misc[w];
            unsigned long long base = 0;
            if (total) base = atomicAdd(work_counter, (unsigned long long)total);
            lds_misc[WAVES] = (uint32_t)base;
            lds_misc[WAVES + 1] = (uint32_t)(base >> 32);
            lds_misc[WAVES + 2] = 0;           // "some slot of this workgroup is live" (set below)
        }
        __syncthreads();
        {
            unsigned long long base = ((unsigned long long)lds_misc[WAVES + 1] << 32) | lds_misc[WAVES];
            for (uint32_t w = 0; w < wave; ++w) base += lds_misc[w];
#pragma unroll 1
            for (int s = 0; s < S; ++s) {
                const bool idle = ((live >> s) & 1u) == 0u;
                const unsigned long long m = __ballot(idle);          // same value as in the count above: bit s unchanged so far
                if (idle) {
                    const unsigned long long my = base + mbcnt(m);
                    if (my < rv.n_rays) {
                        uint32_t p, sl;
                        ray_index_to_pixel(rv, my, p, sl);
                        RayState r;
                        gen_primary(sv, rv, p, rv.sample_begin + sl, r);
                        if (sv.n_objects == 0) {                                  // scene.rs:224-226
                            store_sample(samples, rv, my, mk(0.0, 0.0, 0.0));
                        } else {
                            const uint64_t slot = lane_gid + (uint64_t)s * n_lanes;
                            double *st = state + slot;
                            st[0 * n_slots] = r.pos.x; st[1 * n_slots] = r.pos.y; st[2 * n_slots] = r.pos.z;
                            st[3 * n_slots] = r.dir.x; st[4 * n_slots] = r.dir.y; st[5 * n_slots] = r.dir.z;
                            st[6 * n_slots] = 0.0; st[7 * n_slots] = 0.0; st[8 * n_slots] = 0.0;
                            st[9 * n_slots] = 1.0; st[10 * n_slots] = 1.0; st[11 * n_slots] = 1.0;
                            FilterParams f;
                            filter_from_ray(sv, r.pos, r.dir, f);
                            float *fs = fstate + slot;
                            fs[0 * n_slots] = f.dx; fs[1 * n_slots] = f.dy; fs[2 * n_slots] = f.dz; fs[3 * n_slots] = f.npd;
                            fs[4 * n_slots] = f.p2x; fs[5 * n_slots] = f.p2y; fs[6 * n_slots] = f.p2z; fs[7 * n_slots] = f.nppE;
                    {
                        TriFilterParams tf;
                        if (sv.n_tri_filter != 0) tri_filter_from_ray(sv, r.pos, r.dir, tf); else tri_filter_idle(tf);
                        fs[8 * n_slots] = tf.dx; fs[9 * n_slots] = tf.dy; fs[10 * n_slots] = tf.dz; fs[11 * n_slots] = tf.npx;
                        fs[12 * n_slots] = tf.npy; fs[13 * n_slots] = tf.npz; fs[14 * n_slots] = tf.A;
                    }
                            uint32_t *is = istate + slot;
                            is[0 * n_slots] = p; is[1 * n_slots] = sl; is[2 * n_slots] = 0u;
                            live |= 1u << s;
                        }
                    }
                }
                base += (unsigned long long)__popcll(m);
            }
        }
        // ---- workgroup-uniform exit: nothing live here and the queue handed out nothing
        if (__ballot(live != 0u) != 0ull && lane == 0) lds_misc[WAVES + 2] = 1;
        __syncthreads();
        // the flag is cleared by thread 0 between the two refill barriers of the NEXT round, i.e. after
        // every wave has passed this read
        if (lds_misc[WAVES + 2] == 0) break;

        // ---- sweep the sphere list through LDS with the f32 filter
        FilterParams fp[S];
        uint32_t cnt[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            cnt[s] = 0;
            filter_idle(fp[s]);
            if ((live >> s) & 1u) {
                const float *fs = fstate + (lane_gid + (uint64_t)s * n_lanes);
                fp[s].dx = fs[0 * n_slots]; fp[s].dy = fs[1 * n_slots]; fp[s].dz = fs[2 * n_slots]; fp[s].npd = fs[3 * n_slots];
                fp[s].p2x = fs[4 * n_slots]; fp[s].p2y = fs[5 * n_slots]; fp[s].p2z = fs[6 * n_slots]; fp[s].nppE = fs[7 * n_slots];
            }
        }
        for (uint32_t c0 = 0; c0 < ns; c0 += CHUNK) {
            const uint32_t n = (ns - c0 < (uint32_t)CHUNK) ? ns - c0 : (uint32_t)CHUNK;
            const uint32_t n4 = (n + 3u) & ~3u;            // the device array is padded to a multiple of 4
            if (c0 != 0) __syncthreads();                  // everyone is done with the previous chunk
            for (uint32_t j = tid; j < n4; j += THREADS) lds_sph[j] = sv.sphere_f32[c0 + j];
            __syncthreads();
#pragma unroll 1
            for (uint32_t j = 0; j < n4; j += 4) {
                const float4 A0 = lds_sph[j], B0 = lds_sph[j + 1], A1 = lds_sph[j + 2], B1 = lds_sph[j + 3];
                f32x2 d[S][2];
                uint32_t sign_and = 0xFFFFFFFFu;
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    d[s][0] = filter_disc2(A0, B0, fp[s]);
                    d[s][1] = filter_disc2(A1, B1, fp[s]);
                    sign_and &= __float_as_uint(d[s][0].x) & __float_as_uint(d[s][0].y) &
                                __float_as_uint(d[s][1].x) & __float_as_uint(d[s][1].y);
                }
                if ((int)sign_and >= 0) {                  // some D has its sign bit clear: D >= 0
#pragma unroll
                    for (int s = 0; s < S; ++s) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float dk = (k & 1) ? d[s][k >> 1].y : d[s][k >> 1].x;
                            if ((int)__float_as_uint(dk) >= 0) {
                                if (cnt[s] < (uint32_t)Q) lds_q[((size_t)cnt[s] * S + s) * THREADS + tid] = c0 + j + k;
                                else if (cnt[s] < (uint32_t)(Q + kOverflowQ))
                                    oflow[(size_t)(cnt[s] - Q) * n_slots + lane_gid + (uint64_t)s * n_lanes] = c0 + j + k;
                                cnt[s] += 1;                       // > Q + kOverflowQ marks overflow
                            }
                        }
                    }
                }
            }
        }
        // ---- the same for the triangles that can be hit at all: 32-byte records {n, n.(v0-c)} {cx, cy, hx, hy}
        if (sv.n_tri_filter != 0) {
            const uint32_t nt = sv.n_tri_filter;
            constexpr uint32_t TCHUNK = CHUNK / 2;                  // records per LDS load (2 float4 each)
            TriFilterParams tp[S];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                tri_filter_idle(tp[s]);
                if ((live >> s) & 1u) {
                    const float *fs = fstate + (lane_gid + (uint64_t)s * n_lanes);
                    tp[s].dx = fs[8 * n_slots]; tp[s].dy = fs[9 * n_slots]; tp[s].dz = fs[10 * n_slots]; tp[s].npx = fs[11 * n_slots];
                    tp[s].npy = fs[12 * n_slots]; tp[s].npz = fs[13 * n_slots]; tp[s].A = fs[14 * n_slots];
                }
            }
            for (uint32_t c0 = 0; c0 < nt; c0 += TCHUNK) {
                const uint32_t n = (nt - c0 < TCHUNK) ? nt - c0 : TCHUNK;
                if (c0 != 0 || ns != 0) __syncthreads();           // everyone is done with the previous LDS contents
                for (uint32_t j = tid; j < 2 * n; j += THREADS) lds_sph[j] = sv.tri_f32[2 * (size_t)c0 + j];
                __syncthreads();
#pragma unroll 1
                for (uint32_t j = 0; j < n; j += 2) {
                    const bool two = j + 1 < n;
                    const float4 A0 = lds_sph[2 * j], B0 = lds_sph[2 * j + 1];
                    const float4 A1 = two ? lds_sph[2 * j + 2] : A0, B1 = two ? lds_sph[2 * j + 3] : B0;
                    uint32_t sg[S][2];
                    uint32_t sign_and = 0xFFFFFFFFu;
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        sg[s][0] = tri_filter_sign(A0, B0, tp[s]);
                        sg[s][1] = two ? tri_filter_sign(A1, B1, tp[s]) : 0x80000000u;
                        sign_and &= sg[s][0] & sg[s][1];
                    }
                    if ((int)sign_and >= 0) {
#pragma unroll
                        for (int s = 0; s < S; ++s) {
#pragma unroll
                            for (int k = 0; k < 2; ++k) {
                                if ((int)sg[s][k] >= 0) {
                                    if (cnt[s] < (uint32_t)Q)
                                        lds_q[((size_t)cnt[s] * S + s) * THREADS + tid] = 0x80000000u | sv.tri_fidx[c0 + j + k];
                                    else if (cnt[s] < (uint32_t)(Q + kOverflowQ))
                                        oflow[(size_t)(cnt[s] - Q) * n_slots + lane_gid + (uint64_t)s * n_lanes] =
                                            0x80000000u | sv.tri_fidx[c0 + j + k];
                                    cnt[s] += 1;
                                }
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) lds_cnt[s * THREADS + tid] = cnt[s];
        rounds_swept += 1;

        // ---- exact f64 re-evaluation of the candidates, other shapes, shading (one code instance, loop over slots)
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            if (((live >> s) & 1u) == 0u) continue;
            const uint64_t slot = lane_gid + (uint64_t)s * n_lanes;
            double *st = state + slot;
            uint32_t *is = istate + slot;
            const uint32_t pl = is[0 * n_slots], smp = is[1 * n_slots], bnc = is[2 * n_slots];
            const uint32_t ncand = lds_cnt[s * THREADS + tid];
            RayState r;
            r.pos = mk(st[0 * n_slots], st[1 * n_slots], st[2 * n_slots]);
            r.dir = mk(st[3 * n_slots], st[4 * n_slots], st[5 * n_slots]);
            const RayX rx = make_rayx(r.pos, r.dir);
            Hit h;
            hit_init(h);
            ++segs;
            if (ncand > (uint32_t)(Q + kOverflowQ)) {
                // more candidates than the queue holds (many shapes along one line, or a pass-all filter): exact sweep
                closest_spheres_exact(sv, rx, h);
                closest_tris_exact(sv, rx, h);
                exact += ns + sv.n_tris;
            } else {
                for (uint32_t k = 0; k < ncand; ++k) {
                    const uint32_t idx = k < (uint32_t)Q ? lds_q[((size_t)k * S + s) * THREADS + tid]
                                                         : oflow[(size_t)(k - Q) * n_slots + slot];
                    double t;
                    if (idx & 0x80000000u) {                                  // a triangle candidate
                        const uint32_t ti = idx & 0x7FFFFFFFu;
                        if (ti < sv.n_tris && triangle_distance(sv.tris[ti], rx, &t)) hit_consider(h, t, sv.tris[ti].id, 2, ti);
                    } else if (idx < ns) {
                        if (sphere_distance(sv.spheres[idx], rx, &t)) hit_consider(h, t, sv.sphere_id[idx], 0, idx);
                    }
                }
                exact += ncand;
                if (verify) {            // debug: the filters must never lose the exact winner
                    Hit hv;
                    hit_init(hv);
                    closest_spheres_exact(sv, rx, hv);
                    closest_tris_exact(sv, rx, hv);
                    if (hv.id != h.id || (hv.id != kInvalid && hv.t != h.t)) {
                        ++mism;
                        if (verify > 1 && mism < 3)
                            printf("MISMATCH round %llu bnc %u pl %u blk %u tid %u s %d ncand %u h(%u,%g) hv(%u,%g) pos(%g,%g,%g) "
                                   "dir(%g,%g,%g)\n", round, bnc, pl, blockIdx.x, tid, s, ncand, h.id, h.t, hv.id, hv.t, r.pos.x,
                                   r.pos.y, r.pos.z, r.dir.x, r.dir.y, r.dir.z);
                    }
                }
            }
            closest_planes_exact(sv, rx, h);
            exact += sv.n_planes;

            r.result = mk(st[6 * n_slots], st[7 * n_slots], st[8 * n_slots]);
            bool done = true;
            if (h.id != kInvalid) {                                            // scene.rs:233-236
                r.light = mk(st[9 * n_slots], st[10 * n_slots], st[11 * n_slots]);
                const uint32_t k = fastdiv(pl, rv.div_width);
                const uint32_t x = pl - k * rv.width;
                const uint64_t pix = (uint64_t)image_row(rv, k) * rv.width + x;
                r.key = rng_key(sv.seed, pix, rv.sample_begin + smp);
                r.draw = 6u + 2u * bnc;
                r.bounce = bnc;
                advance_and_shade(sv, h, r);
                done = (r.bounce >= bounce_limit) || light_is_zero(r);         // scene.rs:227-228
                if (!done) {
                    st[0 * n_slots] = r.pos.x; st[1 * n_slots] = r.pos.y; st[2 * n_slots] = r.pos.z;
                    st[3 * n_slots] = r.dir.x; st[4 * n_slots] = r.dir.y; st[5 * n_slots] = r.dir.z;
                    st[6 * n_slots] = r.result.x; st[7 * n_slots] = r.result.y; st[8 * n_slots] = r.result.z;
                    st[9 * n_slots] = r.light.x; st[10 * n_slots] = r.light.y; st[11 * n_slots] = r.light.z;
                    is[2 * n_slots] = r.bounce;
                    FilterParams f;
                    filter_from_ray(sv, r.pos, r.dir, f);
                    float *fs = fstate + slot;
                    fs[0 * n_slots] = f.dx; fs[1 * n_slots] = f.dy; fs[2 * n_slots] = f.dz; fs[3 * n_slots] = f.npd;
                    fs[4 * n_slots] = f.p2x; fs[5 * n_slots] = f.p2y; fs[6 * n_slots] = f.p2z; fs[7 * n_slots] = f.nppE;
                    {
                        TriFilterParams tf;
                        if (sv.n_tri_filter != 0) tri_filter_from_ray(sv, r.pos, r.dir, tf); else tri_filter_idle(tf);
                        fs[8 * n_slots] = tf.dx; fs[9 * n_slots] = tf.dy; fs[10 * n_slots] = tf.dz; fs[11 * n_slots] = tf.npx;
                        fs[12 * n_slots] = tf.npy; fs[13 * n_slots] = tf.npz; fs[14 * n_slots] = tf.A;
                    }
                }
            }
            if (done) {
                store_sample(samples, rv, (uint64_t)smp * rv.npix + pl, r.result);      // = the ray's queue index (ray_index_to_pixel)
                live &= ~(1u << s);
            }
        }
    }
    flush_counters(ctr, segs, exact, rounds_swept * ((unsigned long long)ns + sv.n_tri_filter) * S);
    if (verify) {
        mism = wave_sum_u64(mism);
        if (lane == 0 && mism) atomicAdd(&ctr[0].pad_, mism);
    }
}

// ------------------------------------------------------------------------------------------
// resolve: avg() (scene.rs:253-259) = left fold from zeros (iter_ops.rs:4-8), then / len
// One thread per slot of a sample's queue order (tiles_x != 0: 8x8 pixel tiles, padding slots skipped); consecutive
// threads read consecutive 32-byte records {r, g, b, 0}, sample after sample.
// Zero samples are skipped: store_sample (rtx_device.h) writes no record for them and leaves their bit of `nonzero` clear, and
// a record is read only where the bit is set.  Why the sum keeps its bits:
//   The left fold starts at +0.0 and never becomes -0.0.
//   Round-to-nearest gives +0.0 for x + (-x) and for +0.0 + -0.0.
//   So s + 0.0 == s bit for bit for every addend of either sign.
// (The running sum of an earlier batch, acc, is such a fold's value too.)  The bits of a sample's slots are read a word per
// thread, eight samples ahead of the records, so that the records of those samples are in flight together.
// sq (launch-uniform; null for every render): the second moments' accumulator of rtx_render_blocks_accumulate, in acc's layout --
// where a record's bit is set, sq += c * c per component (a rounded multiply, then a rounded add: -ffp-contract=off).  The same
// proof: c * c of a zero sample is +0.0, and a sum of squares from +0.0 is >= +0.0 or NaN, so the skipped samples change nothing.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resolve_kernel(const double *__restrict__ samples, const uint32_t *__restrict__ nonzero,
                                                      double *__restrict__ acc,
                                                      double *__restrict__ out, uint32_t width, uint32_t n_rows, uint32_t tiles_x,
                                                      uint32_t per_sample, uint32_t n_samples,
                                                      double divisor, int first, int last, double *__restrict__ sq)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= per_sample) return;
    uint32_t p = t;                                   // local pixel k * width + x
    if (tiles_x != 0u) {
        const uint32_t tile = t >> 6, j = t & 63u;
        const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const uint32_t x = tx * 8u + (j & 7u), k = ty * 8u + (j >> 3);
        if (x >= width || k >= n_rows) return;
        p = k * width + x;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (!first) { sx = acc[3 * (uint64_t)p]; sy = acc[3 * (uint64_t)p + 1]; sz = acc[3 * (uint64_t)p + 2]; }
    double qx = 0.0, qy = 0.0, qz = 0.0;
    if (sq) { qx = sq[3 * (uint64_t)p]; qy = sq[3 * (uint64_t)p + 1]; qz = sq[3 * (uint64_t)p + 2]; }
    constexpr uint32_t kAhead = 8;
    for (uint32_t s0 = 0; s0 < n_samples; s0 += kAhead) {
        const uint32_t n = n_samples - s0 < kAhead ? n_samples - s0 : kAhead;
        uint32_t set = 0;                             // bit j: sample s0 + j of this slot has a record
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            if (j < n) {
                const uint64_t slot = (uint64_t)(s0 + j) * per_sample + t;
                set |= ((nonzero[slot >> 5] >> (uint32_t)(slot & 31u)) & 1u) << j;
            }
        }
        if (set == 0u) continue;
        double4 c[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            c[j] = make_double4(0.0, 0.0, 0.0, 0.0);
            if ((set >> j) & 1u) c[j] = reinterpret_cast<const double4 *>(samples)[(uint64_t)(s0 + j) * per_sample + t];
        }
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j)
            if ((set >> j) & 1u) { sx = sx + c[j].x; sy = sy + c[j].y; sz = sz + c[j].z; }
        if (sq) {
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j)
                if ((set >> j) & 1u) { qx = qx + c[j].x * c[j].x; qy = qy + c[j].y * c[j].y; qz = qz + c[j].z * c[j].z; }
        }
    }
    if (sq) { sq[3 * (uint64_t)p] = qx; sq[3 * (uint64_t)p + 1] = qy; sq[3 * (uint64_t)p + 2] = qz; }
    if (last) {
        double *o = out + 3 * (uint64_t)p;
        o[0] = sx / divisor; o[1] = sy / divisor; o[2] = sz / divisor;
    } else {
        acc[3 * (uint64_t)p] = sx; acc[3 * (uint64_t)p + 1] = sy; acc[3 * (uint64_t)p + 2] = sz;
    }
}

// ------------------------------------------------------------------------------------------
// render_to_image epilogue (scene.rs:175-178): img[height-1-y][x] * 256, Rust `as u8`
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t rust_as_u8(double v)
{
    if (!(v == v)) return 0;
    if (v <= 0.0) return 0;
    if (v >= 255.0) return 255;
    return (uint8_t)v;
}

// The epilogues: one kernel, a launch-uniform `form` (memory-bound movers of one value or one pixel per thread).
//
// form 0 -- quantize (render_to_image's `* 256`, Rust's saturating `as u8`), one pixel per thread.
//   flip = 1: render_to_image's rows, output row y from row height - 1 - y (scene.rs:176) -- the whole-frame epilogue.
//   flip = 0: the rows of a band in place order (before it travels over xGMI: 3 bytes per pixel instead of 24; the gather
//   epilogue puts rows where they belong).
// form 8 / 1 -- the multi-device gather epilogue on values of that many bytes (8: the f64 frame, 1: the quantised one), one value
//   per thread, moved as one load and one store: parts[p] (cap_rows rows each) holds band p of n: the blocks of `block` image rows
//   b = p, p + n, ... in order.  flip: output row height - 1 - y (render_to_image, scene.rs:176).
// form 16 / 17 -- rtx_denoise_device's preparation and one of its passes (rtx_denoise.h): everything they read is in `dn`, which the
//   other forms pass zeroed; of the two only form 17 is launched with dynamic LDS (kDnLdsBytes), so the movers' occupancy pays none for it.
// form 18 -- rtx_temporal_accumulate_device (rtx_temporal.h): everything it reads is in `ta`, which the other forms pass zeroed; it is
//   launched with dynamic LDS for its two sine tables when they fit kTemporalLdsBytes, else with none.
// form 19 -- rtx_rewind_hits_device (rtx_rewind.h): everything it reads is in `rw`, which the other forms pass zeroed; it is launched
//   with dynamic LDS for its list of moved objects when that fits kTemporalLdsBytes, else with none.
// form 20 -- rtx_upsample_device (rtx_upsample.h): everything it reads is in `up`, which the other forms pass zeroed; it is launched
//   with no LDS.
constexpr uint32_t kEpilogueDenoisePrepare = 16u, kEpilogueDenoisePass = 17u, kEpilogueTemporal = 18u, kEpilogueRewind = 19u;
constexpr uint32_t kEpilogueUpsample = 20u;
extern __shared__ double epilogue_lds[];
__global__ __launch_bounds__(256) void epilogue_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                       uint32_t width, uint32_t height, uint32_t n, uint32_t cap_rows,
                                                       uint32_t block, uint32_t flip, uint32_t form, DenoiseArgs dn, TemporalArgs ta,
                                                       RewindArgs rw, UpsampleArgs up)
{
    if (form == kEpilogueUpsample) { upsample_pixel(up); return; }
    if (form == kEpilogueRewind) { rewind_hits(rw, epilogue_lds); return; }
    if (form == kEpilogueTemporal) { temporal_accumulate(ta, epilogue_lds); return; }
    if (form == kEpilogueDenoisePass) { denoise_pass(dn, epilogue_lds); return; }
    if (form == kEpilogueDenoisePrepare) { denoise_prepare(dn); return; }
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (form == 0u) {
        const uint64_t npix = (uint64_t)width * height;
        if (i >= npix) return;
        const uint32_t y = (uint32_t)(i / width);
        const uint32_t x = (uint32_t)(i - (uint64_t)y * width);
        const double *c = reinterpret_cast<const double *>(in) + 3 * ((uint64_t)(flip ? height - y - 1 : y) * width + x);
        uint8_t *o = out + 3 * i;
        o[0] = rust_as_u8(c[0] * 256.0);
        o[1] = rust_as_u8(c[1] * 256.0);
        o[2] = rust_as_u8(c[2] * 256.0);
        return;
    }
    const uint64_t row_vals = (uint64_t)width * 3;
    if (i >= row_vals * height) return;
    const uint32_t yo = (uint32_t)(i / row_vals);
    const uint64_t c = i - (uint64_t)yo * row_vals;
    const uint32_t y = flip ? height - 1u - yo : yo;
    const uint32_t b = y / block, p = b % n, k = (b / n) * block + (y - b * block);
    const uint64_t src = ((uint64_t)p * cap_rows + k) * row_vals + c;
    if (form == 8u) reinterpret_cast<unsigned long long *>(out)[i] = reinterpret_cast<const unsigned long long *>(in)[src];
    else out[i] = in[src];
}

#ifdef RTX_LAB
// ops 11-16: a ray index -> pixel arithmetic of the trace kernels (rtx_device.h) on the RowsView the host built for the op, passed
// by value as the renders pass their divisors: out[i] for the index / numerator (uint32_t)a[i]
__global__ void debug_math_kernel(int op, const double *a, const double *b, double *out, uint64_t n, RowsView rv)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r;
    switch (op) {
        case 0: r = a[i] / b[i]; break;
        case 1: r = sqrt(a[i]); break;
        case 2: r = sin(a[i]); break;
        case 3: r = cos(a[i]); break;
        case 4: case 5: { double sn, cs; sincos(a[i], &sn, &cs); r = (op == 4) ? sn : cs; } break;
        case 6:                                          // rtx_writelane (rtx_traverse.h): lane (int)b[1] of every wave takes (int)b[0]
            r = (double)rtx_writelane(__builtin_amdgcn_readfirstlane((int)b[0]), __builtin_amdgcn_readfirstlane((int)b[1]), (int)a[i]);
            break;
        case 9: case 10: { double sn, cs; sincos_2pi(a[i], &sn, &cs); r = (op == 9) ? sn : cs; } break;     // random_direction's sin / cos (rtx_math.h)
        case 11: r = (double)fastdiv((uint32_t)a[i], rv.div_npix); break;
        case 12: case 13: {                              // ray_index_to_pixel: the local pixel / the sample
            uint32_t pl, s_local;
            ray_index_to_pixel(rv, (uint64_t)a[i], pl, s_local);
            r = (double)(op == 12 ? pl : s_local);
        } break;
        case 14: case 15: case 16: {                     // ray_index_to_pixel_tiled: the local pixel / the sample / 1.0 unless the lane is padding
            uint32_t pl, s_local;
            const bool live = ray_index_to_pixel_tiled(rv, (uint64_t)a[i], pl, s_local);
            r = op == 14 ? (double)pl : (op == 15 ? (double)s_local : (live ? 1.0 : 0.0));
        } break;
        default: {                                       // 7 / 8: the child sort's v_min_f64 / v_max_f64 on raw bit patterns
            double lo, hi;
            rtx_minmax_f64_bits(a[i], b[i], lo, hi);
            r = (op == 7) ? lo : hi;
        } break;
    }
    out[i] = r;
}

// rtx_debug_store_samples: entry i is the sample rgb[3 i .. 3 i + 2] of ray-queue slot slots[i], stored by the trace kernels' own
// store_sample (rtx_device.h) under the RowsView the host built for the call (nonzero, nonzero_base), passed by value
__global__ void debug_store_samples_kernel(const double *rgb, const uint64_t *slots, uint64_t n, double *samples, RowsView rv)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_sample(samples, rv, slots[i], mk(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
}
#endif

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
hipError_t launch_trace_exact(const SceneView *d_sv, const RowsView *d_rv, const RowsView &rv, double *samples,
                              Counters *counters, hipStream_t stream)
{
    const uint64_t per_launch = 1ull << 30;                 // rays per launch (grid.x stays < 2^31)
    for (uint64_t off = 0; off < rv.n_rays; off += per_launch) {
        uint64_t n = rv.n_rays - off < per_launch ? rv.n_rays - off : per_launch;
        uint32_t blocks = (uint32_t)((n + 255) / 256);
        hipLaunchKernelGGL(trace_exact_kernel, dim3(blocks), dim3(256), 0, stream, d_sv, d_rv, samples, counters, off);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace {

// Launch shape of the MIXED kernel: 4 workgroups x 4 waves per CU, 2 slots per lane, 128 VGPRs, 34 KB LDS each.
// Other shapes (8 waves per workgroup, 1/3/4 slots per lane, 2048-record chunks, ...) were measured in round 1 and were
// all slower on C2 (0.67x - 0.95x); they are compiled only with -DRTX_MIXED_TUNING (then RTX_HIP_MIXED_VARIANT=n picks
// one, and tests/test_gpu_parity.py::test_mixed_tuning_variants checks each against the exact kernel), so the product
// binary holds no kernel the test-suite does not run.
struct MixVariant {
    int s, threads, chunk, q, blocks_per_cu;
    size_t lds;
    const void *fn;
};

template <int S, int T, int CH, int Q, int WPE, int BPC>
MixVariant make_variant()
{
    MixVariant v;
    v.s = S; v.threads = T; v.chunk = CH; v.q = Q; v.blocks_per_cu = BPC;
    v.lds = (size_t)CH * 16 + (size_t)Q * S * T * 4 + (size_t)S * T * 4 + (T / 64 + 4) * 4;
    v.fn = reinterpret_cast<const void *>(&trace_mixed_kernel<S, T, CH, Q, WPE>);
    return v;
}

const MixVariant &mix_variant()
{
    static const MixVariant table[] = {
        make_variant<2, 256, 1024, 8, 4, 4>(),      // 0: production
#ifdef RTX_MIXED_TUNING
        make_variant<2, 512, 2048, 8, 4, 2>(),      // 1: 2 workgroups x 8 waves per CU
        make_variant<3, 256, 1024, 8, 3, 3>(),      // 2: 3 slots per lane, 12 waves/CU
        make_variant<4, 256, 2048, 8, 2, 2>(),      // 3: 4 slots per lane, 8 waves/CU, 256 VGPRs
        make_variant<1, 512, 1024, 8, 8, 4>(),      // 4: 1 slot per lane, 32 waves/CU
        make_variant<2, 1024, 2048, 8, 4, 1>(),     // 5: one 1024-thread workgroup per CU
        make_variant<4, 256, 2048, 8, 4, 2>(),      // 6: as 3, 128 VGPRs
        make_variant<2, 256, 2048, 8, 4, 3>(),      // 7: as 0 with 2048-record chunks, 3 workgroups per CU
        make_variant<2, 128, 1024, 8, 4, 8>(),      // 8: 128-thread workgroups
#endif
    };
#ifdef RTX_MIXED_TUNING
    static const int idx = [] {                           // tuning builds only: the production binary holds one shape
        const char *e = getenv("RTX_HIP_MIXED_VARIANT");
        int i = e ? atoi(e) : 0;
        return (i < 0 || i >= (int)(sizeof(table) / sizeof(table[0]))) ? 0 : i;
    }();
    return table[idx];
#else
    return table[0];
#endif
}

}  // namespace

size_t mixed_state_bytes(int n_cus)
{
    const MixVariant &v = mix_variant();
    return (size_t)n_cus * v.blocks_per_cu * v.threads * v.s * kSlotBytes;
}

hipError_t launch_trace_mixed(const SceneView *d_sv, const SceneView &sv, const RowsView *d_rv, const RowsView &rv,
                              double *samples, double *state, Counters *counters, unsigned long long *work_counter,
                              int n_cus, bool verify, hipStream_t stream)
{
    const MixVariant &v = mix_variant();
    {   // per launch: the attribute is per device and this call may come from any thread / device
        hipError_t e = hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds);
        if (e != hipSuccess) return e;
    }
    const uint64_t slots_per_block = (uint64_t)v.threads * v.s;
    uint64_t want = (rv.n_rays + slots_per_block - 1) / slots_per_block;
    uint64_t cap = (uint64_t)n_cus * v.blocks_per_cu;
    uint32_t blocks = (uint32_t)(want < cap ? want : cap);
    if (blocks == 0) return hipSuccess;
    const unsigned long long limit = sv.max_bounces >= 0xFFFFFFF0ull ? 0xFFFFFFF0ull : sv.max_bounces + 1ull;
    unsigned long long max_rounds = (rv.n_rays / slots_per_block + 2ull) * limit + 4ull;
#ifdef RTX_MIXED_TUNING
    uint32_t verify_u = verify ? (getenv("RTX_HIP_DEBUG_PRINT") ? 2u : 1u) : 0u;
#else
    uint32_t verify_u = verify ? 1u : 0u;
#endif
    void *args[] = { (void *)&d_sv, (void *)&d_rv, (void *)&samples, (void *)&state, (void *)&counters, (void *)&work_counter,
                     (void *)&verify_u, (void *)&max_rounds };
    return hipLaunchKernel(v.fn, dim3(blocks), dim3(v.threads), args, v.lds, stream);
}

hipError_t launch_resolve(const double *samples, double *acc, double *out, const RowsView &rv, uint32_t per_sample,
                          uint64_t rays_per_pixel, bool first, bool last, hipStream_t stream, double *sq)
{
    if (per_sample == 0) return hipSuccess;
    hipLaunchKernelGGL(resolve_kernel, dim3((per_sample + 255) / 256), dim3(256), 0, stream, samples, rv.nonzero, acc, out, rv.width, rv.n_rows,
                       rv.tiles_x, per_sample, rv.n_samples, (double)rays_per_pixel, first ? 1 : 0, last ? 1 : 0, sq);
    return hipGetLastError();
}

hipError_t launch_quantize(const double *rgb, uint8_t *rgb8, uint32_t width, uint32_t height, hipStream_t stream)
{
    uint64_t npix = (uint64_t)width * height;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint8_t *>(rgb), rgb8, width, height, 1u, 0u, 1u, 1u, 0u, DenoiseArgs{}, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_quantize_values(const double *rgb, uint8_t *rgb8, uint32_t width, uint32_t n_rows, hipStream_t stream)
{
    uint64_t npix = (uint64_t)width * n_rows;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint8_t *>(rgb), rgb8, width, n_rows, 1u, 0u, 1u, 0u, 0u, DenoiseArgs{}, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_deinterleave(const double *parts, double *full, uint32_t width, uint32_t height, uint32_t n, uint32_t cap_rows,
                               uint32_t block, hipStream_t stream)
{
    const uint64_t total = (uint64_t)width * height * 3;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream,
                       reinterpret_cast<const uint8_t *>(parts), reinterpret_cast<uint8_t *>(full), width, height, n, cap_rows, block, 0u, 8u, DenoiseArgs{}, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_deinterleave_u8(const uint8_t *parts, uint8_t *full, uint32_t width, uint32_t height, uint32_t n, uint32_t cap_rows,
                                  uint32_t block, bool flip, hipStream_t stream)
{
    const uint64_t total = (uint64_t)width * height * 3;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, parts, full, width,
                       height, n, cap_rows, block, flip ? 1u : 0u, 1u, DenoiseArgs{}, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_denoise_prepare(const DenoiseArgs &d, hipStream_t stream)
{
    const uint64_t npix = (uint64_t)d.width * d.height;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, stream, nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u,
                       kEpilogueDenoisePrepare, d, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_denoise_pass(const DenoiseArgs &d_, hipStream_t stream)
{
    DenoiseArgs d = d_;
    if (d.width == 0 || d.height == 0 || d.step == 0) return hipSuccess;
    // the sub-lattices that exist (offsets below the step AND inside the frame), each cut into 16 x 16 tiles of the largest one
    d.sub_x = d.step < d.width ? d.step : d.width;
    const uint32_t sub_y = d.step < d.height ? d.step : d.height;
    const uint64_t lw = ((uint64_t)d.width + d.step - 1u) / d.step, lh = ((uint64_t)d.height + d.step - 1u) / d.step;
    d.tiles_x = (uint32_t)((lw + kDnTile - 1u) / kDnTile);
    const uint64_t tiles = (uint64_t)d.tiles_x * ((lh + kDnTile - 1u) / kDnTile);
    const uint64_t blocks = tiles * d.sub_x * sub_y;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    d.tiles = (uint32_t)tiles;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)blocks), dim3(256), kDnLdsBytes, stream, nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u,
                       kEpilogueDenoisePass, d, TemporalArgs{}, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_temporal(const TemporalArgs &t_, hipStream_t stream)
{
    TemporalArgs t = t_;
    const uint64_t npix = (uint64_t)t.width * t.height;
    if (npix == 0) return hipSuccess;
    const size_t table_bytes = ((size_t)t.width + 1u + (size_t)t.height + 1u) * sizeof(double);
    t.tables_in_lds = ((t.flags & kTaHistory) != 0u && table_bytes <= kTemporalLdsBytes) ? 1u : 0u;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), t.tables_in_lds ? table_bytes : 0, stream, nullptr,
                       nullptr, 0u, 0u, 0u, 0u, 0u, 0u, kEpilogueTemporal, DenoiseArgs{}, t, RewindArgs{}, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_rewind(const RewindArgs &r_, hipStream_t stream)
{
    RewindArgs r = r_;
    if (r.n == 0) return hipSuccess;
    const size_t list_bytes = (size_t)r.m * sizeof(long long);
    r.list_in_lds = (r.m != 0u && list_bytes <= kTemporalLdsBytes) ? 1u : 0u;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)(((uint64_t)r.n + 255) / 256)), dim3(256), r.list_in_lds ? list_bytes : 0, stream, nullptr,
                       nullptr, 0u, 0u, 0u, 0u, 0u, 0u, kEpilogueRewind, DenoiseArgs{}, TemporalArgs{}, r, UpsampleArgs{});
    return hipGetLastError();
}

hipError_t launch_upsample(const UpsampleArgs &u, hipStream_t stream)
{
    const uint64_t npix = (uint64_t)u.width * u.height;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(epilogue_kernel, dim3((uint32_t)((npix + 255) / 256)), dim3(256), 0, stream, nullptr, nullptr, 0u, 0u, 0u, 0u, 0u, 0u,
                       kEpilogueUpsample, DenoiseArgs{}, TemporalArgs{}, RewindArgs{}, u);
    return hipGetLastError();
}

#ifdef RTX_LAB
// The RowsView of the index ops, sized as render_band sizes a launch's: 11-13 take the divisor / npix from b[0], 14-16 a band of
// b[0] columns x b[1] rows whose ray queue runs over 8x8 tiles.
static RowsView debug_index_view(int op, const double *b_host, uint64_t n)
{
    RowsView rv{};
    const uint32_t b0 = b_host ? (uint32_t)b_host[0] : 0u, b1 = (b_host && n > 1) ? (uint32_t)b_host[1] : 0u;
    if (op >= 11 && op <= 13) {
        rv.npix = b0;
        rv.div_npix = make_fastdiv(b0);
    } else if (op >= 14 && op <= 16) {
        rv.width = b0; rv.n_rows = b1; rv.npix = b0 * b1;
        rv.tiles_x = (b0 + 7u) / 8u;
        rv.div_width = make_fastdiv(b0); rv.div_npix = make_fastdiv(rv.npix); rv.div_tiles_x = make_fastdiv(rv.tiles_x);
        rv.div_per_sample = make_fastdiv((uint32_t)((uint64_t)rv.tiles_x * ((b1 + 7u) / 8u) * 64u));
    }
    return rv;
}

hipError_t launch_debug_math(int op, const double *a, const double *b, double *out, uint64_t n, const double *b_host, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(debug_math_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, op, a, b, out, n,
                       debug_index_view(op, b_host, n));
    return hipGetLastError();
}

hipError_t launch_debug_store_samples(const double *rgb, const uint64_t *slots, uint64_t n, double *samples, const RowsView &rv,
                                      hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(debug_store_samples_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, rgb, slots, n, samples, rv);
    return hipGetLastError();
}

hipError_t launch_debug_sweep_filter(const SceneView *d_sv, const SweepFilterArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(debug_sweep_filter_kernel, dim3((uint32_t)((a.n + 255) / 256)), dim3(256), 0, stream, d_sv, a);
    return hipGetLastError();
}

void mixed_queue_sizes(uint32_t *q, uint32_t *overflow)
{
    *q = (uint32_t)mix_variant().q;
    *overflow = (uint32_t)kOverflowQ;
}

// ops 17-21 need no kernel: the HOST forms (RTX_HD) that size launches and fill the row tables.  17: fastdiv(a[i], make_fastdiv(b[0]));
// 18: image_row of local row a[i] in a band with row_begin, row_stride, row_block = b[0], b[1], b[2]; 19 / 20 / 21: m, s1, s2 of
// make_fastdiv(a[i])
bool debug_math_host(int op, const double *a, const double *b, double *out, uint64_t n)
{
    if (op < 17 || op > 21) return false;
    RowsView rv{};
    if (op == 18) {
        if (n < 3) return false;
        rv.row_begin = (uint32_t)b[0]; rv.row_stride = (uint32_t)b[1]; rv.row_block = (uint32_t)b[2];
        rv.div_row_block = make_fastdiv(rv.row_block);
    }
    const FastDiv f17 = make_fastdiv((uint32_t)b[0]);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t v = (uint32_t)a[i];
        const FastDiv f = make_fastdiv(v);
        out[i] = op == 17 ? (double)fastdiv(v, f17) : op == 18 ? (double)image_row(rv, v) : op == 19 ? (double)f.m : op == 20 ? (double)f.s1 : (double)f.s2;
    }
    return true;
}
#endif

}  // namespace rtx
