// rtx_rewind.h -- the device text of rtx_rewind_hits_device (include/rtx_hip.h, "Rewinding a pick buffer"): the rewind form of
// epilogue_kernel (rtx_kernels.hip).  The header comment of rtx_rewind_hits_device is the specification; every f64 operation here is
// written in its order and bracketing (the build never fuses: -ffp-contract=off).  Host side: rtx_rewind.hip.
#pragma once

#include "rtx_launch.h"

namespace rtx {

typedef unsigned long long rw_u2 __attribute__((ext_vector_type(2)));          // 16 bytes of a record, moved as bits

__device__ __forceinline__ bool rw_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
__device__ __forceinline__ double rw_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void rw_norm(double *a)           // vector.rs:97-107: three true divisions by the length
{
    const double len = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
    a[0] = a[0] / len;  a[1] = a[1] / len;  a[2] = a[2] / len;
}

// the header's fixed search of the ascending list L[0 .. m) (m >= 1) for o -> its entry, or m when it is not there
__device__ __forceinline__ uint32_t rw_find(const long long *L, uint32_t m, long long o)
{
    uint32_t lo = 0, hi = m;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (L[mid] <= o) lo = mid; else hi = mid;
    }
    return L[lo] == o ? lo : m;
}

// form kEpilogueRewind: one hit per thread.  A workgroup first stages the list of moved objects in LDS (when it fits: r.list_in_lds),
// so the search's ~log2(m) dependent reads are LDS reads; the record is loaded and stored as four 16-byte vectors; only a hit on a
// moved object reads its 152-byte motion record (the lanes of a wave mostly share a few of them) and does arithmetic.
__device__ __forceinline__ void rewind_hits(const RewindArgs &r, double *lds_)
{
    long long *lds = reinterpret_cast<long long *>(lds_);
    const bool in_lds = r.list_in_lds != 0u;
    if (in_lds) {                                           // launch-uniform: every thread of the workgroup reaches the barrier
        for (uint32_t i = threadIdx.x; i < r.m; i += blockDim.x) lds[i] = r.objects[i];
        __syncthreads();
    }
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint64_t)r.n) return;

    const rw_u2 *src = reinterpret_cast<const rw_u2 *>(r.hits + p);
    rw_u2 a0 = src[0], a1 = src[1], a2 = src[2], a3 = src[3];                  // P.x P.y | P.z n.x | n.y n.z | distance object
    const long long o = (long long)a3.y;
    if (r.m != 0u && o >= 0) {
        uint32_t k;                                         // (two calls, so that the staged one compiles to LDS reads, not flat ones)
        if (in_lds) k = rw_find(lds, r.m, o); else k = rw_find(r.objects, r.m, o);
        if (k < r.m) {
            const RewindMotion &M = r.motions[k];
            const uint32_t kind = M.kind;
            const double P[3] = { __longlong_as_double((long long)a0.x), __longlong_as_double((long long)a0.y),
                                  __longlong_as_double((long long)a1.x) };
            double Q[3] = { 0.0, 0.0, 0.0 }, N[3] = { 0.0, 0.0, 0.0 };
            bool lost = true;
            if (rw_finite(P[0]) && rw_finite(P[1]) && rw_finite(P[2])) {
                if (kind == 0u) {                           // RTX_SPHERE
                    const double s = M.before[3] / M.now[3];
                    if (s > 0.0 && s < __builtin_inf()) {
                        lost = false;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const double g = P[j] - M.now[j];
                            Q[j] = M.before[j] + g * s;
                            N[j] = Q[j] - M.before[j];
                        }
                        rw_norm(N);                         // sphere.rs:31-33
                        rw_norm(N);                         // object.rs:37-39
                    }
                } else if (kind == 1u) {                    // RTX_PLANE
                    lost = false;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const double t = M.before[j] - M.now[j];
                        Q[j] = P[j] + t;
                        N[j] = M.before[3 + j];             // plane.rs:33-35
                    }
                    rw_norm(N);                             // object.rs:37-39
                } else if (kind == 2u) {                    // RTX_TRIANGLE
                    double e1[3], e2[3], w[3];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        e1[j] = M.now[3 + j] - M.now[j];  e2[j] = M.now[6 + j] - M.now[j];  w[j] = P[j] - M.now[j];
                    }
                    const double d11 = rw_dot(e1, e1), d12 = rw_dot(e1, e2), d22 = rw_dot(e2, e2), w1 = rw_dot(w, e1), w2 = rw_dot(w, e2);
                    const double det = d11 * d22 - d12 * d12;
                    if (det > 0.0 && det < __builtin_inf()) {
                        lost = false;
                        const double u = (d22 * w1 - d12 * w2) / det;
                        const double v = (d11 * w2 - d12 * w1) / det;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            e1[j] = M.before[3 + j] - M.before[j];  e2[j] = M.before[6 + j] - M.before[j];
                            Q[j] = (M.before[j] + u * e1[j]) + v * e2[j];
                        }
                        N[0] = e1[1] * e2[2] - e1[2] * e2[1];   // vector.rs:89-95
                        N[1] = e1[2] * e2[0] - e1[0] * e2[2];
                        N[2] = e1[0] * e2[1] - e1[1] * e2[0];
                        rw_norm(N);                         // triangle.rs:104-107
                        rw_norm(N);                         // object.rs:37-39
                    }
                }
            }
            // one select per word after the branches have joined (a record is lost, or all six of its words are replaced)
            const bool good = !lost && rw_finite(Q[0]) && rw_finite(Q[1]) && rw_finite(Q[2]);
            a0.x = good ? (unsigned long long)__double_as_longlong(Q[0]) : a0.x;
            a0.y = good ? (unsigned long long)__double_as_longlong(Q[1]) : a0.y;
            a1.x = good ? (unsigned long long)__double_as_longlong(Q[2]) : a1.x;
            a1.y = good ? (unsigned long long)__double_as_longlong(N[0]) : a1.y;
            a2.x = good ? (unsigned long long)__double_as_longlong(N[1]) : a2.x;
            a2.y = good ? (unsigned long long)__double_as_longlong(N[2]) : a2.y;
            a3.y = good ? a3.y : ~0ull;                     // LOST: object = -1, every other byte as it came
        }
    }
    rw_u2 *dst = reinterpret_cast<rw_u2 *>(r.out + p);
    dst[0] = a0;  dst[1] = a1;  dst[2] = a2;  dst[3] = a3;
}

}  // namespace rtx
