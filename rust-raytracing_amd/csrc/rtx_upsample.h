// rtx_upsample.h -- the device text of rtx_upsample_device (include/rtx_hip.h, "Guided upsampling"): form 20 of epilogue_kernel
// (rtx_kernels.hip).  The header comment of rtx_upsample_device is the specification; every f64 operation here is written in its order
// and bracketing (the build never fuses: -ffp-contract=off).  The three guide weights are the denoiser's own functions (rtx_denoise.h).
// Host side: rtx_upsample.hip.
//
// One output pixel per thread, consecutive threads consecutive pixels of a row: the output pixel's record (96 B) and the stores (24 +
// 24 B) are contiguous across a wave.  The four low taps are gathered through the cache: the 64 pixels of a wave lie on one output row
// (or two), so they share 64 / s + 1 low pixels of at most two low rows per tap row -- the same few lines, read by every lane (DESIGN.md
// 3.17 says why the patch is not staged in LDS).
#pragma once

#include "rtx_denoise.h"

namespace rtx {

// a tap's values per channel and which channels are usable: (c, var, a, e) of low pixel q -> (u, v), bit k of the result = channel k
__device__ __forceinline__ uint32_t upsample_tap(const UpsampleArgs &a, uint64_t q, const QueryFeatures &fq, bool demod, bool has_var,
                                                 double u[3], double v[3])
{
    uint32_t usable = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = a.lo_rgb[3 * q + k], al = fq.albedo[k];
        double var = has_var ? a.lo_var[3 * q + k] : 0.0;
        bool ok = true;
        if (demod) {
            const double t = c - fq.emission[k];
            ok = al > a.albedo_min;
            u[k] = ok ? t / al : t;
            if (has_var && ok) var = var / (al * al);
        } else {
            u[k] = c;
        }
        v[k] = var;
        if (ok && dn_finite(u[k])) usable |= 1u << k;
    }
    return usable;
}

__device__ __forceinline__ void upsample_pixel(const UpsampleArgs &a)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint64_t)a.width * a.height) return;
    const uint32_t s = a.factor, wl = a.lo_width, hl = a.lo_height;
    const uint32_t y = (uint32_t)(p / a.width), x = (uint32_t)(p - (uint64_t)y * a.width);
    const uint32_t X0 = x / s, Y0 = y / s, rx = x - s * X0, ry = y - s * Y0;
    const bool demod = (a.flags & kDnDemodulate) != 0u, has_var = (a.flags & kDnVariance) != 0u;
    const QueryFeatures f = a.feat[p];
    double u[3] = { 0.0, 0.0, 0.0 }, v[3] = { 0.0, 0.0, 0.0 };
    if (rx == 0u && ry == 0u) {                           // a lattice pixel: the low pixel itself
        const uint64_t q = (uint64_t)Y0 * wl + X0;
        const QueryFeatures fq = a.lo_feat[q];
        double uq[3], vq[3];
        const uint32_t usable = upsample_tap(a, q, fq, demod, has_var, uq, vq);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (usable & (1u << k)) { u[k] = uq[k]; v[k] = vq[k]; }
    } else {
        const double fx = (double)rx / (double)s, fy = (double)ry / (double)s;
        const double np[3] = { f.normal[0], f.normal[1], f.normal[2] }, ap[3] = { f.albedo[0], f.albedo[1], f.albedo[2] };
        const double zp = f.depth;
        const bool zp_fin = dn_finite(zp);
        double tc[3] = { 0.0, 0.0, 0.0 }, tw[3] = { 0.0, 0.0, 0.0 }, tv[3] = { 0.0, 0.0, 0.0 };
        double sc[3] = { 0.0, 0.0, 0.0 }, sw[3] = { 0.0, 0.0, 0.0 }, sv[3] = { 0.0, 0.0, 0.0 };
#pragma unroll 1
        for (uint32_t t = 0; t < 4u; ++t) {
            const uint32_t i = t & 1u, j = t >> 1;
            const uint32_t X = X0 + i, Y = Y0 + j;
            if (X >= wl || Y >= hl) continue;
            const double h = (i ? fx : 1.0 - fx) * (j ? fy : 1.0 - fy);
            if (h == 0.0) continue;
            const uint64_t q = (uint64_t)Y * wl + X;
            const QueryFeatures fq = a.lo_feat[q];
            double wn = 1.0, wz = 1.0, wa = 1.0;
            if (a.flags & kDnNormal) wn = dn_weight_normal(np, fq.normal[0], fq.normal[1], fq.normal[2], a.normal_power_log2);
            if (a.flags & kDnDepth) wz = dn_weight_depth(zp, zp_fin, fq.depth, a.sigma_depth);
            if (a.flags & kDnAlbedo) wa = dn_weight_albedo(ap, fq.albedo[0], fq.albedo[1], fq.albedo[2], a.sigma_albedo2);
            const double w = ((h * wn) * wz) * wa;
            const bool guided = w > 0.0;
            double uq[3], vq[3];
            const uint32_t usable = upsample_tap(a, q, fq, demod, has_var, uq, vq);
            const double h2 = h * h, w2 = w * w;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (!(usable & (1u << k))) continue;
                tc[k] = tc[k] + h * uq[k];
                tw[k] = tw[k] + h;
                if (has_var) tv[k] = tv[k] + h2 * vq[k];
                if (guided) {
                    sc[k] = sc[k] + w * uq[k];
                    sw[k] = sw[k] + w;
                    if (has_var) sv[k] = sv[k] + w2 * vq[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (sw[k] > a.min_weight * tw[k]) {
                u[k] = sc[k] / sw[k];
                if (has_var) v[k] = sv[k] / (sw[k] * sw[k]);
            } else if (tw[k] > 0.0) {
                u[k] = tc[k] / tw[k];
                if (has_var) v[k] = tv[k] / (tw[k] * tw[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double o = u[k], vo = v[k];
        if (demod) {
            const double al = f.albedo[k], e = f.emission[k];
            if (al > a.albedo_min) { o = o * al + e; vo = vo * (al * al); }
            else { o = e; vo = 0.0; }
        }
        a.out[3 * p + k] = o;
        if (a.var_out) a.var_out[3 * p + k] = vo;
    }
}

}  // namespace rtx
