// rtx_upsample.hip -- rtx_upsample_device, rtx_upsample and their helpers (include/rtx_hip.h "Guided upsampling"): the
// argument checks (made before any device is looked for), the one launch, and the one-shot host form.  The device text is
// rtx_upsample.h, compiled into epilogue_kernel (rtx_kernels.hip) as one more launch-uniform form.
#include "rtx_host.h"

#include <cmath>
#include <cstring>

namespace {

const char *params_error(const RtxUpsampleParams *p)
{
    if (!p) return "null params";
    if (p->factor == 0u || p->factor > RTX_UPSAMPLE_MAX_FACTOR) return "factor is 0 or exceeds RTX_UPSAMPLE_MAX_FACTOR";
    if (p->flags & ~(uint32_t)RTX_UPSAMPLE_DEMODULATE) return "a flag bit include/rtx_hip.h does not name";
    if (p->normal_power_log2 > 8u && p->normal_power_log2 != RTX_DENOISE_NO_NORMAL) return "normal_power_log2 is neither 0..8 nor RTX_DENOISE_NO_NORMAL";
    if (p->reserved != 0u) return "reserved must be 0";
    if (!(p->sigma_depth > 0.0) || !(p->sigma_albedo > 0.0)) return "a sigma is NaN, zero or negative";
    if (!(p->albedo_min >= 0.0) || std::isinf(p->albedo_min)) return "albedo_min is NaN, negative or infinite";
    if (!(p->min_weight >= 0.0) || std::isinf(p->min_weight)) return "min_weight is NaN, negative or infinite";
    return nullptr;
}

// everything rtx_upsample_device refuses, without a device
int32_t check_call(const char *who, const double *lo_rgb, const double *lo_var, const RtxPixelFeatures *lo_features,
                   const RtxPixelFeatures *features, uint32_t width, uint32_t height, const RtxUpsampleParams *params, const double *out,
                   const double *var_out)
{
    const std::string w = std::string(who) + ": ";
    if (const char *e = params_error(params)) return fail(RTX_ERR_INVALID_ARGUMENT, w + e);
    const uint64_t npix = (uint64_t)width * height;
    if (npix == 0 || npix >= 0xFFFFFFF0ull) return fail(RTX_ERR_INVALID_ARGUMENT, w + "width * height is 0, or 2^32 - 16 or more");
    if (width % params->factor != 0u || height % params->factor != 0u)
        return fail(RTX_ERR_INVALID_ARGUMENT, w + "width or height is not a multiple of factor (the low frame's pixels are the output's lattice only then)");
    if (!lo_rgb || !lo_features || !features || !out) return fail(RTX_ERR_INVALID_ARGUMENT, w + "null low frame, features or output");
    if (var_out && !lo_var) return fail(RTX_ERR_INVALID_ARGUMENT, w + "a variance output without a variance input");
    const uint64_t nlo = (uint64_t)(width / params->factor) * (height / params->factor);
    const Range r[6] = { { lo_rgb, (size_t)(nlo * 24) }, { lo_var, (size_t)(nlo * 24) }, { lo_features, (size_t)(nlo * sizeof(RtxPixelFeatures)) },
                         { features, (size_t)(npix * sizeof(RtxPixelFeatures)) }, { out, (size_t)(npix * 24) }, { var_out, (size_t)(npix * 24) } };
    if (ranges_overlap(r, 6)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "input and output buffers overlap");
    return RTX_OK;
}

}  // namespace

extern "C" {

void rtx_upsample_default_params(RtxUpsampleParams *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->factor = 2;
    out->flags = RTX_UPSAMPLE_DEMODULATE;
    out->normal_power_log2 = 2;                            // chosen on the golden scenes: the grid is flat, within
    out->sigma_depth = 0.05;                               // 1.2 % from end to end; a tight depth term and the 4th power of the
    out->sigma_albedo = 0.5;                               // normals' dot product lead it on oracle and on device frames alike
    out->albedo_min = 1e-3;
    out->min_weight = 1e-3;
}

int32_t rtx_upsample_device(const double *d_lo_rgb, const double *d_lo_var, const RtxPixelFeatures *d_lo_features,
                            const RtxPixelFeatures *d_features, uint32_t width, uint32_t height, const RtxUpsampleParams *params,
                            double *d_out, double *d_var_out, int32_t device, void *stream_)
{
    if (int32_t rc = check_call("rtx_upsample_device", d_lo_rgb, d_lo_var, d_lo_features, d_features, width, height, params, d_out, d_var_out)) return rc;
    if (int32_t rc = check_device(device, "rtx_upsample_device")) return rc;
    RTX_HIP_CHECK(hipSetDevice(device));
    const RtxUpsampleParams &p = *params;
    UpsampleArgs u{};
    u.lo_rgb = d_lo_rgb; u.lo_var = d_lo_var;
    u.lo_feat = reinterpret_cast<const QueryFeatures *>(d_lo_features);
    u.feat = reinterpret_cast<const QueryFeatures *>(d_features);
    u.out = d_out; u.var_out = d_var_out;
    u.sigma_depth = p.sigma_depth;
    u.sigma_albedo2 = p.sigma_albedo * p.sigma_albedo;
    u.albedo_min = p.albedo_min; u.min_weight = p.min_weight;
    u.width = width; u.height = height; u.lo_width = width / p.factor; u.lo_height = height / p.factor;
    u.factor = p.factor;
    u.normal_power_log2 = p.normal_power_log2 == RTX_DENOISE_NO_NORMAL ? 0u : p.normal_power_log2;
    u.flags = ((p.flags & RTX_UPSAMPLE_DEMODULATE) ? kDnDemodulate : 0u) | (d_lo_var ? kDnVariance : 0u) |
              (!std::isinf(p.sigma_depth) ? kDnDepth : 0u) | (!std::isinf(p.sigma_albedo) ? kDnAlbedo : 0u) |
              (p.normal_power_log2 != RTX_DENOISE_NO_NORMAL ? kDnNormal : 0u);
    RTX_HIP_CHECK(launch_upsample(u, static_cast<hipStream_t>(stream_)));
    return RTX_OK;
}

int32_t rtx_upsample(const double *lo_rgb, const double *lo_var, const RtxPixelFeatures *lo_features, const RtxPixelFeatures *features,
                     uint32_t width, uint32_t height, const RtxUpsampleParams *params, double *out, double *var_out)
{
    if (int32_t rc = check_call("rtx_upsample", lo_rgb, lo_var, lo_features, features, width, height, params, out, var_out)) return rc;
    if (int32_t rc = check_device(0, "rtx_upsample")) return rc;
    RTX_HIP_CHECK(hipSetDevice(0));
    const uint64_t npix = (uint64_t)width * height, nlo = (uint64_t)(width / params->factor) * (height / params->factor);
    // one allocation: low frame, low variance, low features, features, output, variance output -- each part padded to 128 bytes
    const uint64_t sizes[6] = { nlo * 24, lo_var ? nlo * 24 : 0, nlo * sizeof(RtxPixelFeatures), npix * sizeof(RtxPixelFeatures), npix * 24,
                                var_out ? npix * 24 : 0 };
    uint64_t off[7] = { 0 };
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + ((sizes[i] + 127u) & ~(uint64_t)127u);
    char *base = nullptr;
    RTX_HIP_CHECK(hipMalloc((void **)&base, off[6]));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } guard{ base };
    double *d_lo = reinterpret_cast<double *>(base + off[0]), *d_var = lo_var ? reinterpret_cast<double *>(base + off[1]) : nullptr;
    RtxPixelFeatures *d_lo_feat = reinterpret_cast<RtxPixelFeatures *>(base + off[2]), *d_feat = reinterpret_cast<RtxPixelFeatures *>(base + off[3]);
    double *d_out = reinterpret_cast<double *>(base + off[4]), *d_var_out = var_out ? reinterpret_cast<double *>(base + off[5]) : nullptr;
    RTX_HIP_CHECK(hipMemcpy(d_lo, lo_rgb, sizes[0], hipMemcpyHostToDevice));
    if (lo_var) RTX_HIP_CHECK(hipMemcpy(d_var, lo_var, sizes[1], hipMemcpyHostToDevice));
    RTX_HIP_CHECK(hipMemcpy(d_lo_feat, lo_features, sizes[2], hipMemcpyHostToDevice));
    RTX_HIP_CHECK(hipMemcpy(d_feat, features, sizes[3], hipMemcpyHostToDevice));
    if (int32_t rc = rtx_upsample_device(d_lo, d_var, d_lo_feat, d_feat, width, height, params, d_out, d_var_out, 0, nullptr)) return rc;
    RTX_HIP_CHECK(hipDeviceSynchronize());
    RTX_HIP_CHECK(hipMemcpy(out, d_out, sizes[4], hipMemcpyDeviceToHost));
    if (var_out) RTX_HIP_CHECK(hipMemcpy(var_out, d_var_out, sizes[5], hipMemcpyDeviceToHost));
    return RTX_OK;
}

}  // extern "C"
