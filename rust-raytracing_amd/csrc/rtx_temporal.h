// rtx_temporal.h -- the device text of rtx_temporal_accumulate_device (include/rtx_hip.h, "Temporal accumulation"): the temporal form
// of epilogue_kernel (rtx_kernels.hip).  The header comment of rtx_temporal_accumulate_device is the specification; every f64 operation
// here is written in its order and bracketing (the build never fuses: -ffp-contract=off).  Host side: rtx_temporal.hip.
#pragma once

#include "rtx_launch.h"

namespace rtx {

__device__ __forceinline__ bool ta_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
__device__ __forceinline__ double ta_dot(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the header's fixed search of a sine table T[0 .. n] for s, and the position in its interval (the first and last extrapolate)
__device__ __forceinline__ double ta_unmap(const double *T, uint32_t n, double s)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T[mid] <= s) lo = mid; else hi = mid;
    }
    const double t0 = T[lo], den = T[lo + 1] - t0;
    return (double)lo + (den > 0.0 ? (s - t0) / den : 0.0);
}

// form kEpilogueTemporal: one pixel per thread.  A workgroup first stages both tables in LDS (when they fit: t.tables_in_lds), so the
// two searches' ~11 dependent reads each are LDS reads; the four taps are gathers of the previous frame's 64-byte hit records and 7
// doubles of history; the pixel's own loads and stores are coalesced.
__device__ __forceinline__ void temporal_accumulate(const TemporalArgs &t, double *lds)
{
    const uint32_t W = t.width, H = t.height;
    const bool history = (t.flags & kTaHistory) != 0u, has_var = (t.flags & kTaVariance) != 0u;
    const bool in_lds = history && t.tables_in_lds != 0u;
    if (in_lds) {                                           // launch-uniform: every thread of the workgroup reaches the barrier
        const uint32_t n = (W + 1u) + (H + 1u);
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lds[i] = t.tables[i];
        __syncthreads();
    }
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint64_t)W * H) return;

    const double c[3] = { t.rgb[3 * p], t.rgb[3 * p + 1], t.rgb[3 * p + 2] };
    double v[3] = { 0.0, 0.0, 0.0 };
    if (has_var) { v[0] = t.var[3 * p]; v[1] = t.var[3 * p + 1]; v[2] = t.var[3 * p + 2]; }
    const double nan = __builtin_nan("");
    double o[3] = { c[0], c[1], c[2] }, ov[3] = { v[0], v[1], v[2] }, olen = 1.0, mx = nan, my = nan;

    if (history) {
        const QueryHit &hit = t.hits[p];
        const double P[3] = { hit.position[0], hit.position[1], hit.position[2] };
        const double n[3] = { hit.normal[0], hit.normal[1], hit.normal[2] };
        const long long obj = hit.object;
        if (obj >= 0 && ta_finite(P[0]) && ta_finite(P[1]) && ta_finite(P[2])) {
            const double e[3] = { P[0] - t.cam_pos[0], P[1] - t.cam_pos[1], P[2] - t.cam_pos[2] };
            const double ccx = ta_dot(e, t.to_cam), ccy = ta_dot(e, t.to_cam + 3), ccz = ta_dot(e, t.to_cam + 6);
            if (ccz > 0.0) {
                const double a = ccx * ccx, b = ccy * ccy, L = (a + b) + ccz * ccz;
                double q = L * L - 4.0 * (a * b);
                q = q > 0.0 ? q : 0.0;
                const double m = 2.0 / (L + sqrt(q));
                const double k = sqrt(m), sx = ccx * k, sy = ccy * k;
                double fx, fy;                              // (two calls, so that the staged one compiles to LDS reads, not flat ones)
                if (in_lds) { fx = ta_unmap(lds, W, sx); fy = ta_unmap(lds + (W + 1u), H, sy); }
                else { fx = ta_unmap(t.tables, W, sx); fy = ta_unmap(t.tables + (W + 1u), H, sy); }
                if (fx >= -0.5 && fx <= (double)W - 0.5 && fy >= -0.5 && fy <= (double)H - 0.5) {
                    mx = fx; my = fy;
                    const double fi = floor(fx), fj = floor(fy);
                    const double tx = fx - fi, ty = fy - fj;
                    const long long i0 = (long long)fi, j0 = (long long)fj;
                    const double nn = ta_dot(n, n), ee = ta_dot(e, e);
                    const double plane_rhs = (t.plane_tol2 * ee) * nn;
                    double sw = 0.0, hs[3] = { 0.0, 0.0, 0.0 }, hv[3] = { 0.0, 0.0, 0.0 }, hn = 0.0;
#pragma unroll
                    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                        for (int dx = 0; dx < 2; ++dx) {
                            const long long qx = i0 + dx, qy = j0 + dy;
                            if (qx < 0 || qx >= (long long)W || qy < 0 || qy >= (long long)H) continue;
                            const double w = (dx ? tx : 1.0 - tx) * (dy ? ty : 1.0 - ty);
                            if (!(w > 0.0)) continue;
                            const uint64_t qi = (uint64_t)qy * W + (uint64_t)qx;
                            const QueryHit &prev = t.hist_hits[qi];
                            if (prev.object != obj) continue;
                            const double ql = t.hist_len[qi];
                            if (!(ql >= 1.0)) continue;
                            const double hc[3] = { t.hist_rgb[3 * qi], t.hist_rgb[3 * qi + 1], t.hist_rgb[3 * qi + 2] };
                            if (!(ta_finite(hc[0]) && ta_finite(hc[1]) && ta_finite(hc[2]))) continue;
                            double hq[3] = { 0.0, 0.0, 0.0 };
                            if (has_var) {
                                hq[0] = t.hist_var[3 * qi]; hq[1] = t.hist_var[3 * qi + 1]; hq[2] = t.hist_var[3 * qi + 2];
                                if (!(ta_finite(hq[0]) && ta_finite(hq[1]) && ta_finite(hq[2]))) continue;
                            }
                            const double Q[3] = { prev.position[0], prev.position[1], prev.position[2] };
                            const double nq[3] = { prev.normal[0], prev.normal[1], prev.normal[2] };
                            const double tt = ta_dot(n, nq);
                            if (!(tt > 0.0)) continue;
                            if (!(tt * tt >= t.normal_min2 * (nn * ta_dot(nq, nq)))) continue;
                            const double g[3] = { Q[0] - P[0], Q[1] - P[1], Q[2] - P[2] };
                            const double d = ta_dot(g, n);
                            if (!(d * d <= plane_rhs)) continue;
                            sw = sw + w;
                            hs[0] = hs[0] + w * hc[0];  hs[1] = hs[1] + w * hc[1];  hs[2] = hs[2] + w * hc[2];
                            if (has_var) { hv[0] = hv[0] + w * hq[0];  hv[1] = hv[1] + w * hq[1];  hv[2] = hv[2] + w * hq[2]; }
                            hn = hn + w * ql;
                        }
                    }
                    if (sw > t.min_weight) {
                        const double N = hn / sw;
                        double alpha = 1.0 / (N + 1.0);
                        alpha = alpha > t.alpha_min ? alpha : t.alpha_min;
                        const double beta = 1.0 - alpha;
#pragma unroll
                        for (int k2 = 0; k2 < 3; ++k2) {
                            o[k2] = beta * (hs[k2] / sw) + alpha * c[k2];
                            if (has_var) ov[k2] = (beta * beta) * (hv[k2] / sw) + (alpha * alpha) * v[k2];
                        }
                        const double len = N + 1.0;
                        olen = len < t.max_history ? len : t.max_history;
                    }
                }
            }
        }
    }
    t.out_rgb[3 * p] = o[0];  t.out_rgb[3 * p + 1] = o[1];  t.out_rgb[3 * p + 2] = o[2];
    if (t.out_var) { t.out_var[3 * p] = ov[0];  t.out_var[3 * p + 1] = ov[1];  t.out_var[3 * p + 2] = ov[2]; }
    t.out_len[p] = olen;
    if (t.motion) { t.motion[2 * p] = mx;  t.motion[2 * p + 1] = my; }
}

}  // namespace rtx
