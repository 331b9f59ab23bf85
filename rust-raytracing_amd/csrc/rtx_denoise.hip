// rtx_denoise.hip -- rtx_denoise_device, rtx_denoise and their helpers (include/rtx_hip.h "Denoising"): the argument
// checks (made before any device is looked for), the plan of a call -- one preparation launch, one launch per pass, the packed records
// ping-ponging between the two halves of the caller's work buffer, the last pass writing the frame -- and the one-shot host form.  The
// device text is rtx_denoise.h, compiled into epilogue_kernel (rtx_kernels.hip) as two launch-uniform forms.
#include "rtx_host.h"

#include <cmath>
#include <cstring>

namespace {

constexpr uint64_t kRecordBytes = 128;                    // = kDnRecDoubles * 8 (rtx_denoise.h)

const char *params_error(const RtxDenoiseParams *p)
{
    if (!p) return "null params";
    if (p->passes > RTX_DENOISE_MAX_PASSES) return "passes exceeds RTX_DENOISE_MAX_PASSES";
    if (p->flags & ~(uint32_t)RTX_DENOISE_DEMODULATE) return "a flag bit include/rtx_hip.h does not name";
    if (p->normal_power_log2 > 8u && p->normal_power_log2 != RTX_DENOISE_NO_NORMAL) return "normal_power_log2 is neither 0..8 nor RTX_DENOISE_NO_NORMAL";
    if (p->reserved != 0u) return "reserved must be 0";
    if (!(p->sigma_color > 0.0) || !(p->sigma_depth > 0.0) || !(p->sigma_albedo > 0.0)) return "a sigma is NaN, zero or negative";
    if (!(p->epsilon >= 0.0) || std::isinf(p->epsilon)) return "epsilon is NaN, negative or infinite";
    if (!(p->albedo_min >= 0.0) || std::isinf(p->albedo_min)) return "albedo_min is NaN, negative or infinite";
    return nullptr;
}

bool frame_ok(uint32_t width, uint32_t height)
{
    const uint64_t npix = (uint64_t)width * height;
    return npix != 0 && npix < 0xFFFFFFF0ull;
}

uint64_t work_bytes(uint32_t width, uint32_t height, uint32_t passes)
{
    return (uint64_t)width * height * kRecordBytes * (passes == 0 ? 0u : (passes == 1 ? 1u : 2u));
}

// everything rtx_denoise_device refuses, without a device
int32_t check_call(const char *who, const double *rgb, const double *var, const RtxPixelFeatures *features, uint32_t width, uint32_t height,
                   const RtxDenoiseParams *params, const double *out, const double *var_out, const void *work, bool need_work)
{
    const std::string w = std::string(who) + ": ";
    if (const char *e = params_error(params)) return fail(RTX_ERR_INVALID_ARGUMENT, w + e);
    if (!frame_ok(width, height)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "width * height is 0, or 2^32 - 16 or more");
    if (!rgb || !features || !out) return fail(RTX_ERR_INVALID_ARGUMENT, w + "null frame, features or output");
    if (var_out && !var) return fail(RTX_ERR_INVALID_ARGUMENT, w + "a variance output without a variance input");
    const uint64_t npix = (uint64_t)width * height, wb = work_bytes(width, height, params->passes);
    if (need_work && wb && !work) return fail(RTX_ERR_INVALID_ARGUMENT, w + "null work buffer");
    if (need_work && ((uintptr_t)work & 15u)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "the work buffer is not 16-byte aligned");
    const Range r[6] = { { rgb, (size_t)(npix * 24) }, { var, (size_t)(npix * 24) }, { features, (size_t)(npix * sizeof(RtxPixelFeatures)) },
                         { out, (size_t)(npix * 24) }, { var_out, (size_t)(npix * 24) }, { (need_work && wb) ? work : nullptr, (size_t)wb } };
    if (ranges_overlap(r, 6)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "input, output and work buffers overlap");
    return RTX_OK;
}

}  // namespace

extern "C" {

void rtx_denoise_default_params(RtxDenoiseParams *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->passes = 5;
    out->flags = RTX_DENOISE_DEMODULATE;
    out->normal_power_log2 = 0;                            // tuned on the golden scenes: the features' normals are means
    out->sigma_color = 2.0;                                // over a pixel's samples, shorter than 1 on every edge, and a power of
    out->sigma_depth = 0.1;                                // their dot product leaves such pixels with no neighbour at all
    out->sigma_albedo = 0.5;
    out->epsilon = 1e-10;
    out->albedo_min = 1e-3;
}

uint64_t rtx_denoise_work_bytes(uint32_t width, uint32_t height, const RtxDenoiseParams *params)
{
    if (params_error(params) || !frame_ok(width, height)) return 0;
    return work_bytes(width, height, params->passes);
}

int32_t rtx_denoise_device(const double *d_rgb, const double *d_var, const RtxPixelFeatures *d_features, uint32_t width, uint32_t height,
                           const RtxDenoiseParams *params, double *d_out, double *d_var_out, void *d_work, int32_t device, void *stream_)
{
    if (int32_t rc = check_call("rtx_denoise_device", d_rgb, d_var, d_features, width, height, params, d_out, d_var_out, d_work, true)) return rc;
    if (int32_t rc = check_device(device, "rtx_denoise_device")) return rc;
    RTX_HIP_CHECK(hipSetDevice(device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const RtxDenoiseParams &p = *params;
    const uint64_t npix = (uint64_t)width * height;
    if (p.passes == 0) {                                   // byte copies: no arithmetic at all
        RTX_HIP_CHECK(hipMemcpyAsync(d_out, d_rgb, npix * 24, hipMemcpyDeviceToDevice, stream));
        if (d_var_out) RTX_HIP_CHECK(hipMemcpyAsync(d_var_out, d_var, npix * 24, hipMemcpyDeviceToDevice, stream));
        return RTX_OK;
    }
    DenoiseArgs d{};
    d.rgb = d_rgb; d.var = d_var; d.feat = reinterpret_cast<const QueryFeatures *>(d_features);
    d.sigma_color2 = p.sigma_color * p.sigma_color;
    d.sigma_depth = p.sigma_depth;
    d.sigma_albedo2 = p.sigma_albedo * p.sigma_albedo;
    d.epsilon = p.epsilon; d.albedo_min = p.albedo_min;
    d.width = width; d.height = height;
    d.normal_power_log2 = p.normal_power_log2 == RTX_DENOISE_NO_NORMAL ? 0u : p.normal_power_log2;
    d.flags = ((p.flags & RTX_DENOISE_DEMODULATE) ? kDnDemodulate : 0u) | (d_var ? kDnVariance : 0u) |
              ((d_var && !std::isinf(p.sigma_color)) ? kDnColor : 0u) | (!std::isinf(p.sigma_depth) ? kDnDepth : 0u) |
              (!std::isinf(p.sigma_albedo) ? kDnAlbedo : 0u) | (p.normal_power_log2 != RTX_DENOISE_NO_NORMAL ? kDnNormal : 0u);
    double *half[2] = { static_cast<double *>(d_work), static_cast<double *>(d_work) + npix * (kRecordBytes / 8) };
    d.dst = half[0];
    RTX_HIP_CHECK(launch_denoise_prepare(d, stream));
    for (uint32_t i = 0; i < p.passes; ++i) {
        const bool last = i + 1 == p.passes;
        d.step = 1u << i;
        d.src = half[i & 1u];
        d.dst = last ? nullptr : half[(i + 1u) & 1u];
        d.out = last ? d_out : nullptr;
        d.var_out = last ? d_var_out : nullptr;
        RTX_HIP_CHECK(launch_denoise_pass(d, stream));
    }
    return RTX_OK;
}

int32_t rtx_denoise(const double *rgb, const double *var, const RtxPixelFeatures *features, uint32_t width, uint32_t height,
                    const RtxDenoiseParams *params, double *out, double *var_out)
{
    if (int32_t rc = check_call("rtx_denoise", rgb, var, features, width, height, params, out, var_out, nullptr, false)) return rc;
    if (int32_t rc = check_device(0, "rtx_denoise")) return rc;
    RTX_HIP_CHECK(hipSetDevice(0));
    const uint64_t npix = (uint64_t)width * height, wb = work_bytes(width, height, params->passes);
    // one allocation: frame, variance, features, output, variance output, work -- each part a multiple of 8 bytes, the work part first
    const uint64_t sizes[6] = { wb, npix * 24, var ? npix * 24 : 0, npix * sizeof(RtxPixelFeatures), npix * 24, var_out ? npix * 24 : 0 };
    uint64_t off[7] = { 0 };
    for (int i = 0; i < 6; ++i) off[i + 1] = off[i] + ((sizes[i] + 127u) & ~(uint64_t)127u);
    char *base = nullptr;
    RTX_HIP_CHECK(hipMalloc((void **)&base, off[6]));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } guard{ base };
    double *d_rgb = reinterpret_cast<double *>(base + off[1]), *d_var = var ? reinterpret_cast<double *>(base + off[2]) : nullptr;
    RtxPixelFeatures *d_feat = reinterpret_cast<RtxPixelFeatures *>(base + off[3]);
    double *d_out = reinterpret_cast<double *>(base + off[4]), *d_var_out = var_out ? reinterpret_cast<double *>(base + off[5]) : nullptr;
    RTX_HIP_CHECK(hipMemcpy(d_rgb, rgb, sizes[1], hipMemcpyHostToDevice));
    if (var) RTX_HIP_CHECK(hipMemcpy(d_var, var, sizes[2], hipMemcpyHostToDevice));
    RTX_HIP_CHECK(hipMemcpy(d_feat, features, sizes[3], hipMemcpyHostToDevice));
    if (int32_t rc = rtx_denoise_device(d_rgb, d_var, d_feat, width, height, params, d_out, d_var_out, wb ? base : nullptr, 0, nullptr)) return rc;
    RTX_HIP_CHECK(hipDeviceSynchronize());
    RTX_HIP_CHECK(hipMemcpy(out, d_out, sizes[4], hipMemcpyDeviceToHost));
    if (var_out) RTX_HIP_CHECK(hipMemcpy(var_out, d_var_out, sizes[5], hipMemcpyDeviceToHost));
    return RTX_OK;
}

}  // extern "C"
