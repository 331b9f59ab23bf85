// rtx_denoise.h -- the device text of rtx_denoise_device (include/rtx_hip.h, "Denoising"): the two denoise forms of epilogue_kernel
// (rtx_kernels.hip).  The header comment of rtx_denoise_device is the specification; every f64 operation here is written in its order
// and bracketing (the build never fuses: -ffp-contract=off).  Host side: rtx_denoise.hip.
#pragma once

#include "rtx_launch.h"

namespace rtx {

// A pixel's packed record, 16 doubles = 128 bytes = one cache line: what a tap reads of its pixel lies in one line however large the
// step.  {u.xyz, v.xyz, nv, z, n.xyz, a.xyz, 0, 0}
constexpr uint32_t kDnRecDoubles = 16;
constexpr int kDnTile = 16;                              // a workgroup's tile of one sub-lattice: 16 x 16 pixels, one per thread
constexpr int kDnRim = kDnTile + 4;                      // ... staged with a halo of 2 lattice neighbours on every side
constexpr int kDnStaged = kDnRim * kDnRim;               // records in LDS
constexpr int kDnPlanes = 13;                            // u, v, z, n, a of each (nv is read at step 1, not along the lattice)
constexpr size_t kDnLdsBytes = (size_t)kDnPlanes * kDnStaged * sizeof(double);     // 41,600 B: three workgroups per CU

__device__ __forceinline__ bool dn_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
__device__ __forceinline__ double dn_b3(int i) { return i == 2 ? 0.375 : ((i == 1 || i == 3) ? 0.25 : 0.0625); }

// The three guide weights of a tap q against the centre p, in the header's words; the upsampler (rtx_upsample.h) takes the same three.
__device__ __forceinline__ double dn_weight_normal(const double np[3], double nq0, double nq1, double nq2, uint32_t power_log2)
{
    double t = (np[0] * nq0 + np[1] * nq1) + np[2] * nq2;
    t = t > 0.0 ? t : 0.0;
    for (uint32_t j = 0; j < power_log2; ++j) t = t * t;
    return t;
}
__device__ __forceinline__ double dn_weight_depth(double zp, bool zp_fin, double zq, double sigma_depth)
{
    const bool zq_fin = dn_finite(zq);
    if (zp_fin && zq_fin) {
        const double r = (zp - zq) / (sigma_depth * (zp + zq));
        return 1.0 / (1.0 + r * r);
    }
    return (zp_fin == zq_fin) ? 1.0 : 0.0;
}
__device__ __forceinline__ double dn_weight_albedo(const double ap[3], double aq0, double aq1, double aq2, double sigma_albedo2)
{
    const double d0 = ap[0] - aq0, d1 = ap[1] - aq1, d2 = ap[2] - aq2;
    const double da = (d0 * d0 + d1 * d1) + d2 * d2;
    return 1.0 / (1.0 + da / sigma_albedo2);
}

// form kEpilogueDenoisePrepare: one pixel per thread, (rgb, var, features) -> the record
__device__ __forceinline__ void denoise_prepare(const DenoiseArgs &d)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (uint64_t)d.width * d.height) return;
    const QueryFeatures f = d.feat[p];
    const bool demod = (d.flags & kDnDemodulate) != 0u, has_var = (d.flags & kDnVariance) != 0u;
    double u[3], v[3] = { 0.0, 0.0, 0.0 };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double c = d.rgb[3 * p + k], a = f.albedo[k];
        double var = has_var ? d.var[3 * p + k] : 0.0;
        if (demod) {
            const double t = c - f.emission[k];
            const bool div = a > d.albedo_min;
            u[k] = div ? t / a : t;
            if (has_var && div) var = var / (a * a);
        } else {
            u[k] = c;
        }
        v[k] = var;
    }
    const double nv = (v[0] + v[1]) + v[2];
    double2 *rec = reinterpret_cast<double2 *>(d.dst + kDnRecDoubles * p);
    rec[0] = make_double2(u[0], u[1]);           rec[1] = make_double2(u[2], v[0]);
    rec[2] = make_double2(v[1], v[2]);           rec[3] = make_double2(nv, f.depth);
    rec[4] = make_double2(f.normal[0], f.normal[1]);   rec[5] = make_double2(f.normal[2], f.albedo[0]);
    rec[6] = make_double2(f.albedo[1], f.albedo[2]);   rec[7] = make_double2(0.0, 0.0);
}

// form kEpilogueDenoisePass: one pass of step d.step.  A pass of step s is a dense 5 x 5 stencil on each of the s x s sub-lattices
// {(ox + i s, oy + j s)}; a workgroup takes a 16 x 16 tile of one sub-lattice and stages the tile and its halo in LDS, plane by plane
// (consecutive lanes read consecutive doubles: no bank conflict).  Slots of pixels outside the frame are never written and never read.
__device__ __forceinline__ void denoise_pass(const DenoiseArgs &d, double *lds)
{
    constexpr int R = kDnRim, N = kDnStaged;
    const uint32_t tid = threadIdx.x;
    const uint32_t tile = blockIdx.x % d.tiles, sub = blockIdx.x / d.tiles;
    const long long ox = sub % d.sub_x, oy = sub / d.sub_x, s = d.step, W = d.width, H = d.height;
    const long long tx0 = (long long)(tile % d.tiles_x) * kDnTile, ty0 = (long long)(tile / d.tiles_x) * kDnTile;
    for (int r = (int)tid; r < N; r += 256) {
        const int ty = r / R, tx = r - ty * R;
        const long long qx = ox + (tx0 + tx - 2) * s, qy = oy + (ty0 + ty - 2) * s;
        if (qx >= 0 && qx < W && qy >= 0 && qy < H) {
            const double2 *rec = reinterpret_cast<const double2 *>(d.src + kDnRecDoubles * (uint64_t)(qy * W + qx));
            const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4], r5 = rec[5], r6 = rec[6];
            lds[0 * N + r] = r0.x;  lds[1 * N + r] = r0.y;  lds[2 * N + r] = r1.x;                     // u
            lds[3 * N + r] = r1.y;  lds[4 * N + r] = r2.x;  lds[5 * N + r] = r2.y;                     // v
            lds[6 * N + r] = r3.y;                                                                     // z
            lds[7 * N + r] = r4.x;  lds[8 * N + r] = r4.y;  lds[9 * N + r] = r5.x;                     // n
            lds[10 * N + r] = r5.y; lds[11 * N + r] = r6.x; lds[12 * N + r] = r6.y;                    // a
        }
    }
    __syncthreads();
    const int lx = (int)(tid & 15u), ly = (int)(tid >> 4);
    const long long x = ox + (tx0 + lx) * s, y = oy + (ty0 + ly) * s;
    if (x >= W || y >= H) return;
    const uint64_t p = (uint64_t)(y * W + x);
    const int c0 = (ly + 2) * R + lx + 2;
    const bool has_var = (d.flags & kDnVariance) != 0u;
    const double up[3] = { lds[0 * N + c0], lds[1 * N + c0], lds[2 * N + c0] };
    const double vp[3] = { lds[3 * N + c0], lds[4 * N + c0], lds[5 * N + c0] };
    const double zp = lds[6 * N + c0];
    const double np[3] = { lds[7 * N + c0], lds[8 * N + c0], lds[9 * N + c0] };
    const double ap[3] = { lds[10 * N + c0], lds[11 * N + c0], lds[12 * N + c0] };
    double un[3] = { up[0], up[1], up[2] }, vn[3] = { vp[0], vp[1], vp[2] };
    if (dn_finite(up[0]) && dn_finite(up[1]) && dn_finite(up[2])) {
        double cden = 0.0;
        if (d.flags & kDnColor) {                        // the 3 x 3 mean of nv at step 1, in-frame neighbours only
            double g = 0.0, gw = 0.0;
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const long long qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const double m = (double)((dx == 0 ? 2 : 1) * (dy == 0 ? 2 : 1));
                    g = g + m * d.src[kDnRecDoubles * (uint64_t)(qy * W + qx) + 6];
                    gw = gw + m;
                }
            cden = d.sigma_color2 * (g / gw) + d.epsilon;
        }
        const bool zp_fin = dn_finite(zp);
        double sc[3] = { 0.0, 0.0, 0.0 }, sv[3] = { 0.0, 0.0, 0.0 }, sw = 0.0;
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const double h = dn_b3(dx + 2) * dn_b3(dy + 2);
                const int c = c0 + dy * R + dx;
                double w = h;
                if (dx != 0 || dy != 0) {
                    const long long qx = x + dx * s, qy = y + dy * s;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    double wn = 1.0, wz = 1.0, wa = 1.0, wc = 1.0;
                    if (d.flags & kDnNormal) wn = dn_weight_normal(np, lds[7 * N + c], lds[8 * N + c], lds[9 * N + c], d.normal_power_log2);
                    if (d.flags & kDnDepth) wz = dn_weight_depth(zp, zp_fin, lds[6 * N + c], d.sigma_depth);
                    if (d.flags & kDnAlbedo) wa = dn_weight_albedo(ap, lds[10 * N + c], lds[11 * N + c], lds[12 * N + c], d.sigma_albedo2);
                    if (d.flags & kDnColor) {
                        const double d0 = up[0] - lds[0 * N + c], d1 = up[1] - lds[1 * N + c], d2 = up[2] - lds[2 * N + c];
                        const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
                        wc = 1.0 / (1.0 + dd / cden);
                    }
                    w = (((h * wn) * wz) * wa) * wc;
                    if (!(w > 0.0)) continue;
                }
                const double uq[3] = { lds[0 * N + c], lds[1 * N + c], lds[2 * N + c] };
                if (!(dn_finite(uq[0]) && dn_finite(uq[1]) && dn_finite(uq[2]))) continue;
                sc[0] = sc[0] + w * uq[0];  sc[1] = sc[1] + w * uq[1];  sc[2] = sc[2] + w * uq[2];
                sw = sw + w;
                if (has_var) {
                    const double w2 = w * w;
                    sv[0] = sv[0] + w2 * lds[3 * N + c];  sv[1] = sv[1] + w2 * lds[4 * N + c];  sv[2] = sv[2] + w2 * lds[5 * N + c];
                }
            }
        }
        un[0] = sc[0] / sw;  un[1] = sc[1] / sw;  un[2] = sc[2] / sw;
        if (has_var) {
            const double sw2 = sw * sw;
            vn[0] = sv[0] / sw2;  vn[1] = sv[1] / sw2;  vn[2] = sv[2] / sw2;
        }
    }
    if (d.dst) {                                          // the next pass's input
        const double nv = has_var ? (vn[0] + vn[1]) + vn[2] : 0.0;
        double2 *rec = reinterpret_cast<double2 *>(d.dst + kDnRecDoubles * p);
        rec[0] = make_double2(un[0], un[1]);  rec[1] = make_double2(un[2], vn[0]);
        rec[2] = make_double2(vn[1], vn[2]);  rec[3] = make_double2(nv, zp);
        rec[4] = make_double2(np[0], np[1]);  rec[5] = make_double2(np[2], ap[0]);
        rec[6] = make_double2(ap[1], ap[2]);  rec[7] = make_double2(0.0, 0.0);
        return;
    }
    const bool demod = (d.flags & kDnDemodulate) != 0u;   // the last pass: back to the frame
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double o = un[k], vo = vn[k];
        if (demod) {
            const double e = d.feat[p].emission[k];
            if (ap[k] > d.albedo_min) { o = o * ap[k] + e; vo = vo * (ap[k] * ap[k]); }
            else o = o + e;
        }
        d.out[3 * p + k] = o;
        if (d.var_out) d.var_out[3 * p + k] = vo;
    }
}

}  // namespace rtx
