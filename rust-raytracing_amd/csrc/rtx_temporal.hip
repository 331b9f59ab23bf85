// rtx_temporal.hip -- rtx_temporal_accumulate_device, rtx_temporal_accumulate, rtx_temporal_tables and their helpers (include/rtx_hip.h
// "Temporal accumulation"): the argument checks (made before any device is looked for), the sine tables of the previous
// camera's pixel map, the one launch, and the one-shot host form.  The device text is rtx_temporal.h, compiled into epilogue_kernel
// (rtx_kernels.hip) as one launch-uniform form.
#include "rtx_host.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr double kPi = 3.14159265358979323846;             // the double nearest pi: fov == kPi is the widest camera accepted

const char *params_error(const RtxTemporalParams *p)
{
    if (!p) return "null params";
    if (p->flags != 0u || p->reserved != 0u) return "flags and reserved must be 0";
    if (!(p->alpha_min >= 0.0 && p->alpha_min <= 1.0)) return "alpha_min is not in [0, 1]";
    if (!(p->max_history >= 1.0) || std::isinf(p->max_history)) return "max_history is NaN, below 1 or infinite";
    if (!(p->plane_tolerance >= 0.0) || std::isinf(p->plane_tolerance)) return "plane_tolerance is NaN, negative or infinite";
    if (!(p->normal_min >= 0.0 && p->normal_min <= 1.0)) return "normal_min is not in [0, 1]";
    if (!(p->min_weight >= 0.0 && p->min_weight < 1.0)) return "min_weight is not in [0, 1)";
    return nullptr;
}

bool frame_ok(uint32_t width, uint32_t height)
{
    const uint64_t npix = (uint64_t)width * height;
    return npix != 0 && npix < 0xFFFFFFF0ull;
}

bool fov_ok(double fov) { return fov > 0.0 && fov <= kPi; }

void fill_tables(double fov, uint32_t width, uint32_t height, double *tables)
{
    // host libm's sin(), called by name, of the angles the render's own tables take (table_angle, rtx_host.h); sin() alone: no cosine
    // is wanted here, so no compiler makes a sincos() of it
    const double vertical_fov = table_vertical_fov(fov, width, height);
    for (uint32_t i = 0; i <= width; ++i) tables[i] = ::sin(table_angle(fov, i, width));
    for (uint32_t j = 0; j <= height; ++j) tables[(size_t)width + 1u + j] = ::sin(table_angle(vertical_fov, j, height));
}

// everything the two calls refuse, without a device.  tables: the device form's (the host form builds its own)
int32_t check_call(const char *who, const double *rgb, const double *var, const RtxHit *hits, const double *hist_rgb, const double *hist_var,
                   const double *hist_len, const RtxHit *hist_hits, const RtxCamera *prev_camera, const double *tables, bool need_tables,
                   uint32_t width, uint32_t height, const RtxTemporalParams *params, const double *out_rgb, const double *out_var,
                   const double *out_len, const double *motion)
{
    const std::string w = std::string(who) + ": ";
    if (const char *e = params_error(params)) return fail(RTX_ERR_INVALID_ARGUMENT, w + e);
    if (!frame_ok(width, height)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "width * height is 0, or 2^32 - 16 or more");
    if (!rgb || !hits || !out_rgb || !out_len) return fail(RTX_ERR_INVALID_ARGUMENT, w + "null frame, hits, output or output length");
    if (out_var && !var) return fail(RTX_ERR_INVALID_ARGUMENT, w + "a variance output without a variance input");
    const bool any_hist = hist_rgb || hist_var || hist_len || hist_hits;
    if (any_hist) {
        if (!hist_rgb || !hist_len || !hist_hits) return fail(RTX_ERR_INVALID_ARGUMENT, w + "a history that is only partly given");
        if ((var != nullptr) != (hist_var != nullptr))
            return fail(RTX_ERR_INVALID_ARGUMENT, w + "a variance without the history's variance, or the reverse");
        if (!prev_camera || (need_tables && !tables)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "a history without its camera or tables");
        if (!fov_ok(prev_camera->fov)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "the previous camera's fov is not in (0, pi]");
    }
    const uint64_t npix = (uint64_t)width * height;
    const size_t f = (size_t)(npix * 24), h = (size_t)(npix * sizeof(RtxHit));
    const Range r[12] = { { rgb, f }, { var, f }, { hits, h }, { hist_rgb, f }, { hist_var, f }, { hist_len, (size_t)(npix * 8) }, { hist_hits, h },
                          { (any_hist && need_tables) ? tables : nullptr, ((size_t)width + height + 2u) * 8u },
                          { out_rgb, f }, { out_var, f }, { out_len, (size_t)(npix * 8) }, { motion, (size_t)(npix * 16) } };
    if (ranges_overlap(r, 12)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "input and output buffers overlap");
    return RTX_OK;
}

}  // namespace

extern "C" {

void rtx_temporal_default_params(RtxTemporalParams *out)
{
    if (!out) return;
    std::memset(out, 0, sizeof *out);
    out->alpha_min = 0.5;                                  // DESIGN.md 3.15 records the grid these were taken from: on the golden
    out->max_history = 32.0;                               // scenes' tiny frames a pixel is 3 degrees wide, and repeated bilinear taps
    out->plane_tolerance = 0.005;                          // blur their one-pixel features faster than a lower alpha_min averages noise
    out->normal_min = 0.9;
    out->min_weight = 0.01;
}

int32_t rtx_temporal_tables(double fov, uint32_t width, uint32_t height, double *tables)
{
    if (!tables) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_temporal_tables: null tables");
    if (!fov_ok(fov)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_temporal_tables: fov is not in (0, pi]");
    if (!frame_ok(width, height)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_temporal_tables: width * height is 0, or 2^32 - 16 or more");
    fill_tables(fov, width, height, tables);
    return RTX_OK;
}

int32_t rtx_temporal_accumulate_device(const double *d_rgb, const double *d_var, const RtxHit *d_hits, const double *d_hist_rgb,
                                       const double *d_hist_var, const double *d_hist_len, const RtxHit *d_hist_hits,
                                       const RtxCamera *prev_camera, const double *d_prev_tables, uint32_t width, uint32_t height,
                                       const RtxTemporalParams *params, double *d_out_rgb, double *d_out_var, double *d_out_len,
                                       double *d_motion, int32_t device, void *stream_)
{
    if (int32_t rc = check_call("rtx_temporal_accumulate_device", d_rgb, d_var, d_hits, d_hist_rgb, d_hist_var, d_hist_len, d_hist_hits,
                                prev_camera, d_prev_tables, true, width, height, params, d_out_rgb, d_out_var, d_out_len, d_motion)) return rc;
    if (int32_t rc = check_device(device, "rtx_temporal_accumulate_device")) return rc;
    RTX_HIP_CHECK(hipSetDevice(device));
    const RtxTemporalParams &p = *params;
    TemporalArgs t{};
    t.rgb = d_rgb; t.var = d_var; t.hits = reinterpret_cast<const QueryHit *>(d_hits);
    t.out_rgb = d_out_rgb; t.out_var = d_out_var; t.out_len = d_out_len; t.motion = d_motion;
    t.width = width; t.height = height;
    t.flags = d_var ? kTaVariance : 0u;
    if (d_hist_rgb) {
        t.flags |= kTaHistory;
        t.hist_rgb = d_hist_rgb; t.hist_var = d_hist_var; t.hist_len = d_hist_len;
        t.hist_hits = reinterpret_cast<const QueryHit *>(d_hist_hits);
        t.tables = d_prev_tables;
        for (int k = 0; k < 3; ++k) t.cam_pos[k] = prev_camera->position[k];
        for (int k = 0; k < 9; ++k) t.to_cam[k] = prev_camera->to_cam_space[k];
    }
    t.alpha_min = p.alpha_min; t.max_history = p.max_history; t.min_weight = p.min_weight;
    t.plane_tol2 = p.plane_tolerance * p.plane_tolerance;
    t.normal_min2 = p.normal_min * p.normal_min;
    RTX_HIP_CHECK(launch_temporal(t, static_cast<hipStream_t>(stream_)));
    return RTX_OK;
}

int32_t rtx_temporal_accumulate(const double *rgb, const double *var, const RtxHit *hits, const double *hist_rgb, const double *hist_var,
                                const double *hist_len, const RtxHit *hist_hits, const RtxCamera *prev_camera, uint32_t width,
                                uint32_t height, const RtxTemporalParams *params, double *out_rgb, double *out_var, double *out_len,
                                double *motion)
{
    if (int32_t rc = check_call("rtx_temporal_accumulate", rgb, var, hits, hist_rgb, hist_var, hist_len, hist_hits, prev_camera, nullptr,
                                false, width, height, params, out_rgb, out_var, out_len, motion)) return rc;
    if (int32_t rc = check_device(0, "rtx_temporal_accumulate")) return rc;
    RTX_HIP_CHECK(hipSetDevice(0));
    const uint64_t npix = (uint64_t)width * height;
    const bool hist = hist_rgb != nullptr;
    std::vector<double> tables;
    if (hist) { tables.resize((size_t)width + height + 2u); fill_tables(prev_camera->fov, width, height, tables.data()); }
    // one allocation: the inputs in the call's order, the tables, then the outputs
    const uint64_t f = npix * 24, h = npix * sizeof(RtxHit);
    const void *src[8] = { rgb, var, hits, hist_rgb, hist_var, hist_len, hist_hits, hist ? tables.data() : nullptr };
    void *dst[4] = { out_rgb, out_var, out_len, motion };
    const uint64_t sizes[12] = { f, var ? f : 0, h, hist ? f : 0, hist_var ? f : 0, hist ? npix * 8 : 0, hist ? h : 0,
                                 hist ? (uint64_t)tables.size() * 8 : 0, f, out_var ? f : 0, npix * 8, motion ? npix * 16 : 0 };
    uint64_t off[13] = { 0 };
    for (int i = 0; i < 12; ++i) off[i + 1] = off[i] + ((sizes[i] + 127u) & ~(uint64_t)127u);
    char *base = nullptr;
    RTX_HIP_CHECK(hipMalloc((void **)&base, off[12]));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } guard{ base };
    auto at = [&](int i) -> void * { return sizes[i] ? base + off[i] : nullptr; };
    for (int i = 0; i < 8; ++i)
        if (sizes[i]) RTX_HIP_CHECK(hipMemcpy(at(i), src[i], sizes[i], hipMemcpyHostToDevice));
    if (int32_t rc = rtx_temporal_accumulate_device((const double *)at(0), (const double *)at(1), (const RtxHit *)at(2), (const double *)at(3),
                                                    (const double *)at(4), (const double *)at(5), (const RtxHit *)at(6), prev_camera,
                                                    (const double *)at(7), width, height, params, (double *)at(8), (double *)at(9),
                                                    (double *)at(10), (double *)at(11), 0, nullptr)) return rc;
    RTX_HIP_CHECK(hipDeviceSynchronize());
    for (int i = 0; i < 4; ++i)
        if (sizes[8 + i]) RTX_HIP_CHECK(hipMemcpy(dst[i], at(8 + i), sizes[8 + i], hipMemcpyDeviceToHost));
    return RTX_OK;
}

}  // extern "C"
