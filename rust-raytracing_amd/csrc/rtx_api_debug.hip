// rtx_api_debug.hip -- the rtx_debug_* entry points of include/rtx_hip.h: the hooks the tests and the lab tools read the library
// through.  Most bodies exist in librtx_hip_lab.so only (RTX_LAB); the product library answers RTX_ERR_UNSUPPORTED.
#include "rtx_host.h"

#include <algorithm>
#include <cstring>

extern "C" {

int32_t rtx_debug_host_scene(const RtxScene *scene, uint64_t *stats)
{
    if (!scene || !stats) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_host_scene: null argument");
    if (scene->n_objects && !scene->objects) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_host_scene: objects is null");
    PackedScene p;
    if (int32_t rc = pack_scene(scene, p)) return rc;
    return check_packed(p, scene->objects, stats);
}

#ifdef RTX_LAB
// The resident arrays, downloaded into the shape digest_packed / digest_packed_mesh read.
static int32_t fetch_resident(RtxSceneHandle_ *h, bool mesh, PackedScene &p)
{
    RTX_HIP_CHECK(hipSetDevice(h->device));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    const SceneView &sv = h->sv;
    auto fetch = [](auto &vec, const void *src, size_t count) -> hipError_t {
        vec.resize(count);
        return count && src ? hipMemcpy(vec.data(), src, count * sizeof(vec[0]), hipMemcpyDeviceToHost) : hipSuccess;
    };
    const size_t n_leaf = h->refit.sphere_tree ? h->refit.slot.size() : 0;
    RTX_HIP_CHECK(fetch(p.bvh4.nodes, sv.bvh_nodes, sv.n_bvh_nodes));
    RTX_HIP_CHECK(fetch(p.q3nodes, sv.bvh_q3nodes, sv.bvh_q3nodes ? sv.n_bvh_nodes : 0));
    RTX_HIP_CHECK(fetch(p.leaf32, sv.bvh_leaf_f32, n_leaf));
    RTX_HIP_CHECK(fetch(p.leaf_cr, sv.bvh_leaf_cr, n_leaf));
    RTX_HIP_CHECK(fetch(p.sph32, sv.sphere_f32, ((size_t)sv.n_spheres + 3) & ~(size_t)3));
    RTX_HIP_CHECK(fetch(p.spheres, sv.spheres, sv.n_spheres));
    RTX_HIP_CHECK(fetch(p.planes, sv.planes, sv.n_planes));
    RTX_HIP_CHECK(fetch(p.mats, sv.materials, sv.n_objects));
    p.sv.sphere_cmax = sv.sphere_cmax;
    if (!mesh) return RTX_OK;
    RTX_HIP_CHECK(fetch(p.tris, sv.tris, sv.n_tris));
    RTX_HIP_CHECK(fetch(p.tri32, sv.tri_f32, sv.n_tri_filter ? 2 * ((size_t)sv.n_tri_filter + 1) : 0));      // (+ the pad record)
    RTX_HIP_CHECK(fetch(p.tri_geo, sv.tri_geo, 2 * (size_t)sv.n_tri_tree));
    RTX_HIP_CHECK(fetch(p.qnodes, sv.bvh_qnodes, sv.bvh_qnodes ? sv.n_bvh_nodes : 0));
    p.sv.tri_extent = sv.tri_extent;
    return RTX_OK;
}
#endif

int32_t rtx_debug_host_refit(const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                             uint64_t *stats, uint32_t *how, uint64_t *digests)
{
#ifdef RTX_LAB
    return host_refit("rtx_debug_host_refit", scene, indices, objects, n, mode, stats, how, digests, nullptr);
#else
    (void)scene; (void)indices; (void)objects; (void)n; (void)mode; (void)stats; (void)how; (void)digests;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_host_refit is a hook of the lab library (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_host_refit_mesh(const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                                  uint64_t *stats, uint32_t *how, uint64_t *digests, double *info)
{
#ifdef RTX_LAB
    if (!info) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_host_refit_mesh: null argument");
    return host_refit("rtx_debug_host_refit_mesh", scene, indices, objects, n, mode, stats, how, digests, info);
#else
    (void)scene; (void)indices; (void)objects; (void)n; (void)mode; (void)stats; (void)how; (void)digests; (void)info;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_host_refit_mesh is a hook of the lab library (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_host_set_visible(const RtxScene *scene, const uint32_t *step_kind, const uint64_t *step_begin, uint64_t n_steps,
                                   const uint64_t *indices, const RtxObject *objects, uint32_t *how, uint64_t *stats, uint64_t *digests,
                                   double *info, uint8_t *mask, uint32_t *dump, uint64_t dump_words)
{
#ifdef RTX_LAB
    return host_visibility("rtx_debug_host_set_visible", scene, step_kind, step_begin, n_steps, indices, objects, how, stats, digests, info, mask,
                           dump, dump_words);
#else
    (void)scene; (void)step_kind; (void)step_begin; (void)n_steps; (void)indices; (void)objects; (void)how; (void)stats; (void)digests;
    (void)info; (void)mask; (void)dump; (void)dump_words;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_host_set_visible is a hook of the lab library (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_resident_digests(RtxSceneHandle h, uint64_t *digests)
{
#ifdef RTX_LAB
    if (!h || !digests) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resident_digests: null argument");
    PackedScene p;
    if (int32_t rc = fetch_resident(h, false, p)) return rc;
    digest_packed(p, digests);
    return RTX_OK;
#else
    (void)h; (void)digests;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_resident_digests is a hook of the lab library (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_resident_mesh_digests(RtxSceneHandle h, uint64_t *digests)
{
#ifdef RTX_LAB
    if (!h || !digests) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resident_mesh_digests: null argument");
    PackedScene p;
    if (int32_t rc = fetch_resident(h, true, p)) return rc;
    digest_packed_mesh(p, digests);
    return RTX_OK;
#else
    (void)h; (void)digests;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_resident_mesh_digests is a hook of the lab library (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_paths(RtxSceneHandle h, uint32_t width, uint32_t height, uint32_t row, uint32_t max_steps, RtxPathStep *steps,
                        uint32_t *counts)
{
#ifdef RTX_LAB
    static_assert(sizeof(RtxPathStep) == sizeof(PathStep) && sizeof(PathStep) == 64, "RtxPathStep layout");
    if (!h || !steps || !counts) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_paths: null argument");
    if (width == 0 || row >= height || max_steps == 0) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_paths: bad row / size");
    const uint64_t paths = (uint64_t)width * h->cfg.rays_per_pixel;
    if (paths == 0) return RTX_OK;
    if (paths * max_steps > (1ull << 24)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_paths: more than 2^24 steps asked for");
    RTX_HIP_CHECK(hipSetDevice(h->device));
    struct Bufs {                                   // freed, and the handle's pointers cleared, on every return path
        RtxSceneHandle_ *h; double *rgb = nullptr; uint32_t kernel;
        ~Bufs() {
            (void)hipDeviceSynchronize();
            if (h->transcript) (void)hipFree(h->transcript);
            if (h->transcript_counts) (void)hipFree(h->transcript_counts);
            if (rgb) (void)hipFree(rgb);
            h->transcript = nullptr; h->transcript_counts = nullptr; h->transcript_steps = 0; h->cfg.kernel = kernel;
        }
    } d{h, nullptr, h->cfg.kernel};
    RTX_HIP_CHECK(hipMalloc((void **)&h->transcript, paths * max_steps * sizeof(PathStep)));
    RTX_HIP_CHECK(hipMalloc((void **)&h->transcript_counts, paths * sizeof(uint32_t)));
    RTX_HIP_CHECK(hipMalloc((void **)&d.rgb, (size_t)width * 3 * sizeof(double)));
    RTX_HIP_CHECK(hipMemset(h->transcript, 0, paths * max_steps * sizeof(PathStep)));
    h->transcript_steps = max_steps;
    h->cfg.kernel = RTX_KERNEL_EXACT;
    RtxStats st;
    if (int32_t rc = render_band(h, width, height, row, 1u, 1u, 1u, d.rgb, nullptr, &st)) return rc;
    if (st.trace_launches != 1) return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_paths: the row did not fit one launch");
    RTX_HIP_CHECK(hipMemcpy(steps, h->transcript, paths * max_steps * sizeof(PathStep), hipMemcpyDeviceToHost));
    RTX_HIP_CHECK(hipMemcpy(counts, h->transcript_counts, paths * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTX_OK;
#else
    (void)h; (void)width; (void)height; (void)row; (void)max_steps; (void)steps; (void)counts;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_paths: a lab-library hook (librtx_hip_lab.so)");
#endif
}

int32_t rtx_debug_math(int32_t op, const double *a, const double *b, double *out, uint64_t n)
{
#ifndef RTX_LAB
    (void)op; (void)a; (void)b; (void)out; (void)n;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_math: a lab-library hook (librtx_hip_lab.so: the same sources, the same arithmetic)");
#else
    if (n == 0) return RTX_OK;
    if (!a || !out) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_math: null argument");
    if (op >= 17 && op <= 21)                       // the host forms of the index arithmetic: no device is touched
        return debug_math_host(op, a, b ? b : a, out, n) ? RTX_OK : fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_math: op 18 takes three values in b");
    if (usable_device_count() == 0) return fail(RTX_ERR_NO_DEVICE, "no gfx950 device");
    struct Bufs {                                   // freed on every return path
        double *p[3] = { nullptr, nullptr, nullptr };
        ~Bufs() { for (double *q : p) if (q) (void)hipFree(q); }
    } d;
    RTX_HIP_CHECK(hipSetDevice(0));
    for (double *&q : d.p) RTX_HIP_CHECK(hipMalloc((void **)&q, n * sizeof(double)));
    RTX_HIP_CHECK(hipMemcpy(d.p[0], a, n * sizeof(double), hipMemcpyHostToDevice));
    RTX_HIP_CHECK(hipMemcpy(d.p[1], b ? b : a, n * sizeof(double), hipMemcpyHostToDevice));
    RTX_HIP_CHECK(launch_debug_math(op, d.p[0], d.p[1], d.p[2], n, b ? b : a, nullptr));
    RTX_HIP_CHECK(hipMemcpy(out, d.p[2], n * sizeof(double), hipMemcpyDeviceToHost));
    return RTX_OK;
#endif
}

#ifdef RTX_LAB
namespace {
// device copies of the host arrays of rtx_debug_store_samples / _resolve / _gather: freed on every return path
struct DebugBufs {
    std::vector<void *> p;
    ~DebugBufs() { for (void *q : p) if (q) (void)hipFree(q); }
    // a device buffer of `bytes` bytes holding `host`'s, and `tail` bytes of 0xFF behind them (null host or 0 bytes: a null pointer,
    // nothing is allocated)
    hipError_t up(const void *host, size_t bytes, void **out, size_t tail = 0)
    {
        *out = nullptr;
        if (!host || bytes == 0) return hipSuccess;
        hipError_t e = hipMalloc(out, bytes + tail);
        if (e != hipSuccess) return e;
        p.push_back(*out);
        if (tail && (e = hipMemset(static_cast<char *>(*out) + bytes, 0xFF, tail)) != hipSuccess) return e;
        return hipMemcpy(*out, host, bytes, hipMemcpyHostToDevice);
    }
};
}  // namespace
#endif

int32_t rtx_debug_store_samples(const double *rgb, const uint64_t *slots, uint64_t n, uint64_t nonzero_base, double *records,
                                uint64_t n_records, uint32_t *mask, uint64_t n_words)
{
#ifndef RTX_LAB
    (void)rgb; (void)slots; (void)n; (void)nonzero_base; (void)records; (void)n_records; (void)mask; (void)n_words;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_store_samples: a lab-library hook (librtx_hip_lab.so)");
#else
    if (n == 0) return RTX_OK;
    if (!rgb || !slots || !records || !mask) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_store_samples: null argument");
    if (n > (1ull << 24) || n_records > (1ull << 26) || n_words > (1ull << 26) || nonzero_base > (1ull << 40))
        return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_store_samples: too large");
    {   // every record and every bit inside the caller's buffers, no slot twice
        std::vector<uint64_t> seen(slots, slots + n);
        std::sort(seen.begin(), seen.end());
        for (uint64_t i = 0; i < n; ++i) {
            if (seen[i] >= n_records || ((nonzero_base + seen[i]) >> 5) >= n_words)
                return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_store_samples: a slot's record or bit lies outside the buffers");
            if (i && seen[i] == seen[i - 1]) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_store_samples: a slot appears twice");
        }
    }
    if (usable_device_count() == 0) return fail(RTX_ERR_NO_DEVICE, "no gfx950 device");
    RTX_HIP_CHECK(hipSetDevice(0));
    DebugBufs d;
    void *d_rgb, *d_slots, *d_rec, *d_mask;
    RTX_HIP_CHECK(d.up(rgb, n * 3 * sizeof(double), &d_rgb));
    RTX_HIP_CHECK(d.up(slots, n * sizeof(uint64_t), &d_slots));
    RTX_HIP_CHECK(d.up(records, n_records * 4 * sizeof(double), &d_rec));
    RTX_HIP_CHECK(d.up(mask, n_words * sizeof(uint32_t), &d_mask));
    RowsView rv{};
    rv.nonzero = static_cast<uint32_t *>(d_mask);
    rv.nonzero_base = nonzero_base;
    RTX_HIP_CHECK(launch_debug_store_samples(static_cast<const double *>(d_rgb), static_cast<const uint64_t *>(d_slots), n,
                                             static_cast<double *>(d_rec), rv, nullptr));
    RTX_HIP_CHECK(hipMemcpy(records, d_rec, n_records * 4 * sizeof(double), hipMemcpyDeviceToHost));   // (the null stream: after the kernel)
    RTX_HIP_CHECK(hipMemcpy(mask, d_mask, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RTX_OK;
#endif
}

int32_t rtx_debug_resolve(const double *records, const uint32_t *mask, uint32_t width, uint32_t n_rows, uint32_t tiles_x,
                          uint32_t n_samples, uint64_t rays_per_pixel, int32_t first, int32_t last, double *acc, uint64_t acc_doubles,
                          double *out, uint64_t out_doubles)
{
#ifndef RTX_LAB
    (void)records; (void)mask; (void)width; (void)n_rows; (void)tiles_x; (void)n_samples; (void)rays_per_pixel; (void)first; (void)last;
    (void)acc; (void)acc_doubles; (void)out; (void)out_doubles;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_resolve: a lab-library hook (librtx_hip_lab.so)");
#else
    const uint64_t npix = (uint64_t)width * n_rows;
    if (npix == 0) return RTX_OK;
    if (tiles_x != 0 && tiles_x != (width + 7u) / 8u) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve: tiles_x is 0 or ceil(width / 8)");
    const uint64_t per_sample64 = tiles_x ? (uint64_t)tiles_x * ((n_rows + 7u) / 8u) * 64u : npix;     // as render_band sizes a sample
    if (per_sample64 * ((uint64_t)n_samples + 1) > (1ull << 26)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve: too large");
    if (n_samples != 0 && (!records || !mask)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve: null records or mask");
    if ((!first || !last) && (!acc || acc_doubles < 3 * npix)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve: acc holds 3 doubles per pixel");
    if (last && (!out || out_doubles < 3 * npix)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve: out holds 3 doubles per pixel");
    if (usable_device_count() == 0) return fail(RTX_ERR_NO_DEVICE, "no gfx950 device");
    RTX_HIP_CHECK(hipSetDevice(0));
    const uint64_t n_rays = per_sample64 * n_samples;
    DebugBufs d;
    void *d_rec, *d_mask, *d_acc, *d_out;
    // behind the caller's records and bits lie one more sample's worth of NaN records under set bits: a fold that reads a sample
    // too many stays inside the buffers and shows in the frame
    const size_t rec_bytes = n_rays * 4 * sizeof(double), mask_bytes = (size_t)((n_rays + 31) / 32) * sizeof(uint32_t);
    RTX_HIP_CHECK(d.up(records, rec_bytes, &d_rec, per_sample64 * 4 * sizeof(double)));
    RTX_HIP_CHECK(d.up(mask, mask_bytes, &d_mask, nonzero_mask_bytes(per_sample64) + sizeof(uint32_t)));
    RTX_HIP_CHECK(d.up(acc, acc_doubles * sizeof(double), &d_acc));
    RTX_HIP_CHECK(d.up(out, out_doubles * sizeof(double), &d_out));
    RowsView rv{};                                     // the fields launch_resolve reads, as render_band fills them
    rv.width = width; rv.n_rows = n_rows; rv.npix = (uint32_t)npix; rv.tiles_x = tiles_x;
    rv.n_samples = n_samples; rv.n_rays = n_rays;
    rv.nonzero = static_cast<uint32_t *>(d_mask); rv.nonzero_base = 0;
    RTX_HIP_CHECK(launch_resolve(static_cast<const double *>(d_rec), static_cast<double *>(d_acc), static_cast<double *>(d_out), rv,
                                 (uint32_t)per_sample64, rays_per_pixel, first != 0, last != 0, nullptr));
    if (d_acc) RTX_HIP_CHECK(hipMemcpy(acc, d_acc, acc_doubles * sizeof(double), hipMemcpyDeviceToHost));
    if (d_out) RTX_HIP_CHECK(hipMemcpy(out, d_out, out_doubles * sizeof(double), hipMemcpyDeviceToHost));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    return RTX_OK;
#endif
}

int32_t rtx_debug_resolve_moments(const double *records, const uint32_t *mask, uint32_t width, uint32_t n_rows, uint32_t tiles_x,
                                  uint32_t n_samples, double *sum, uint64_t sum_doubles, double *sum_sq, uint64_t sum_sq_doubles)
{
#ifndef RTX_LAB
    (void)records; (void)mask; (void)width; (void)n_rows; (void)tiles_x; (void)n_samples; (void)sum; (void)sum_doubles; (void)sum_sq;
    (void)sum_sq_doubles;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_resolve_moments: a lab-library hook (librtx_hip_lab.so)");
#else
    const uint64_t npix = (uint64_t)width * n_rows;
    if (npix == 0) return RTX_OK;
    if (tiles_x != 0 && tiles_x != (width + 7u) / 8u) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve_moments: tiles_x is 0 or ceil(width / 8)");
    const uint64_t per_sample64 = tiles_x ? (uint64_t)tiles_x * ((n_rows + 7u) / 8u) * 64u : npix;     // as render_band sizes a sample
    if (per_sample64 * ((uint64_t)n_samples + 1) > (1ull << 26)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve_moments: too large");
    if (n_samples != 0 && (!records || !mask)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve_moments: null records or mask");
    if (!sum || sum_doubles < 3 * npix) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve_moments: sum holds 3 doubles per pixel");
    if (sum_sq && sum_sq_doubles < 3 * npix) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_resolve_moments: sum_sq holds 3 doubles per pixel");
    if (usable_device_count() == 0) return fail(RTX_ERR_NO_DEVICE, "no gfx950 device");
    RTX_HIP_CHECK(hipSetDevice(0));
    const uint64_t n_rays = per_sample64 * n_samples;
    DebugBufs d;
    void *d_rec, *d_mask, *d_sum, *d_sq;
    // (as rtx_debug_resolve: one more sample's worth of NaN records under set bits behind the caller's records and bits)
    const size_t rec_bytes = n_rays * 4 * sizeof(double), mask_bytes = (size_t)((n_rays + 31) / 32) * sizeof(uint32_t);
    RTX_HIP_CHECK(d.up(records, rec_bytes, &d_rec, per_sample64 * 4 * sizeof(double)));
    RTX_HIP_CHECK(d.up(mask, mask_bytes, &d_mask, nonzero_mask_bytes(per_sample64) + sizeof(uint32_t)));
    RTX_HIP_CHECK(d.up(sum, sum_doubles * sizeof(double), &d_sum));
    RTX_HIP_CHECK(d.up(sum_sq, sum_sq_doubles * sizeof(double), &d_sq));
    RowsView rv{};                                     // the fields launch_resolve reads, as render_band fills them
    rv.width = width; rv.n_rows = n_rows; rv.npix = (uint32_t)npix; rv.tiles_x = tiles_x;
    rv.n_samples = n_samples; rv.n_rays = n_rays;
    rv.nonzero = static_cast<uint32_t *>(d_mask); rv.nonzero_base = 0;
    RTX_HIP_CHECK(launch_resolve(static_cast<const double *>(d_rec), static_cast<double *>(d_sum), nullptr, rv, (uint32_t)per_sample64,
                                 n_samples, false, false, nullptr, static_cast<double *>(d_sq)));
    RTX_HIP_CHECK(hipMemcpy(sum, d_sum, sum_doubles * sizeof(double), hipMemcpyDeviceToHost));
    if (d_sq) RTX_HIP_CHECK(hipMemcpy(sum_sq, d_sq, sum_sq_doubles * sizeof(double), hipMemcpyDeviceToHost));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    return RTX_OK;
#endif
}

int32_t rtx_debug_gather(int32_t form, const void *parts, uint32_t width, uint32_t height, uint32_t n, uint32_t cap_rows,
                         uint32_t block, int32_t flip, void *full)
{
#ifndef RTX_LAB
    (void)form; (void)parts; (void)width; (void)height; (void)n; (void)cap_rows; (void)block; (void)flip; (void)full;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_gather: a lab-library hook (librtx_hip_lab.so)");
#else
    if (form < 0 || form > 2) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: form is 0, 1 or 2");
    const uint64_t vals = (uint64_t)width * height * 3;
    if (vals == 0) return RTX_OK;
    if (!parts || !full) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: null argument");
    if (vals > (1ull << 26)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: too large");
    uint64_t in_vals = vals;                            // form 2: the band itself
    if (form != 2) {
        if (n == 0 || block == 0 || cap_rows == 0 || (uint64_t)n * cap_rows * width * 3 > (1ull << 26))
            return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: bad partition");
        if (form == 0 && flip) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: the f64 form has no flip");
        for (uint32_t y = 0; y < height; ++y) {        // every row the kernel reads lies inside its part's cap_rows
            const uint32_t b = y / block;
            if ((uint64_t)(b / n) * block + (y - b * block) >= cap_rows)
                return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_gather: cap_rows is below a part's row count");
        }
        in_vals = (uint64_t)n * cap_rows * width * 3;
    }
    if (usable_device_count() == 0) return fail(RTX_ERR_NO_DEVICE, "no gfx950 device");
    RTX_HIP_CHECK(hipSetDevice(0));
    const size_t in_bytes = form == 1 ? 1 : sizeof(double), out_bytes = form == 0 ? sizeof(double) : 1;
    DebugBufs d;
    void *d_parts, *d_full;
    RTX_HIP_CHECK(d.up(parts, in_vals * in_bytes, &d_parts));
    RTX_HIP_CHECK(d.up(full, vals * out_bytes, &d_full));
    if (form == 0)
        RTX_HIP_CHECK(launch_deinterleave(static_cast<const double *>(d_parts), static_cast<double *>(d_full), width, height, n, cap_rows,
                                          block, nullptr));
    else if (form == 1)
        RTX_HIP_CHECK(launch_deinterleave_u8(static_cast<const uint8_t *>(d_parts), static_cast<uint8_t *>(d_full), width, height, n,
                                             cap_rows, block, flip != 0, nullptr));
    else
        RTX_HIP_CHECK(launch_quantize_values(static_cast<const double *>(d_parts), static_cast<uint8_t *>(d_full), width, height, nullptr));
    RTX_HIP_CHECK(hipMemcpy(full, d_full, vals * out_bytes, hipMemcpyDeviceToHost));
    return RTX_OK;
#endif
}

int32_t rtx_debug_path_bounds(RtxSceneHandle h, const RtxRay *rays, const uint32_t *objects, const float *best_up, uint64_t n, uint32_t form,
                              uint32_t *out, double *scene_info, uint32_t *records, uint32_t *path_data, uint32_t path_steps)
{
#ifndef RTX_LAB
    (void)h; (void)rays; (void)objects; (void)best_up; (void)n; (void)form; (void)out; (void)scene_info; (void)records; (void)path_data;
    (void)path_steps;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_path_bounds: a lab-library hook (librtx_hip_lab.so)");
#else
    if (!h) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: null scene");
    if (scene_info) {
        const SceneView &v = h->sv;
        const double info[16] = { v.sphere_center[0], v.sphere_center[1], v.sphere_center[2], v.sphere_cmax, (double)v.bvh_origin_limit,
                                  (double)v.bvh_inv_max, v.tri_extent, (double)v.bvh_flags, (double)v.bvh_depth, (double)v.n_bvh_nodes,
                                  (double)v.n_tri_tree, (double)v.n_spheres, 0.0, 0.0, 0.0, 0.0 };
        std::memcpy(scene_info, info, sizeof info);
    }
    if (n == 0) return RTX_OK;
    if (!rays || !objects || !best_up || !out) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: null argument");
    if (n > (1ull << 22) || (path_data && n * (uint64_t)path_steps > (1ull << 24)))
        return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: too large");
    if ((form & ~0xB03u) != 0u) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: unknown form");
    const bool filter_records = (form & 0x800u) != 0u;          // a host-side option of `records`: the device sees the other bits
    form &= ~0x800u;
    const SceneView &sv = h->sv;
    if ((form & 2u) && !((sv.bvh_flags & 16u) && sv.bvh_q3nodes) && !((sv.bvh_flags & 8u) && sv.bvh_qnodes))
        return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: this scene's tree has no 64-byte nodes");
    if (sv.n_bvh_nodes > (1u << 22)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: the tree is too large");
    RTX_HIP_CHECK(hipSetDevice(h->device));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    // the resident tree and the maps from leaf entries to Scene.objects, as the device holds them
    const bool s_tree = (sv.bvh_flags & 1u) != 0u, t_tree = (sv.bvh_flags & 2u) != 0u;
    std::vector<Bvh4Node> nodes(sv.n_bvh_nodes);
    std::vector<uint32_t> prims(s_tree ? sv.n_spheres : 0u), sphere_id(sv.n_spheres), tri_fidx(t_tree ? sv.n_tri_tree : 0u);
    std::vector<TriX> tris(t_tree ? sv.n_tris : 0u);
    auto down = [](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
    RTX_HIP_CHECK(down(nodes.data(), sv.bvh_nodes, nodes.size() * sizeof(Bvh4Node)));
    RTX_HIP_CHECK(down(prims.data(), sv.bvh_prims, prims.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(sphere_id.data(), sv.sphere_id, sphere_id.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(tri_fidx.data(), sv.tri_fidx, tri_fidx.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(tris.data(), sv.tris, tris.size() * sizeof(TriX)));
    // Scene.objects index -> leaf entry (kQueueTri: a triangle filter record of the tree)
    constexpr uint32_t kTriEntry = 0x80000000u, kNoEntry = 0xFFFFFFFFu;
    std::vector<uint32_t> entry_of(sv.n_objects, kNoEntry);
    {
        std::vector<uint32_t> prim_entry(sv.n_spheres, kNoEntry);
        for (size_t k = 0; k < prims.size(); ++k) if (prims[k] < prim_entry.size()) prim_entry[prims[k]] = (uint32_t)k;
        for (size_t s = 0; s < sphere_id.size(); ++s)
            if (prim_entry[s] != kNoEntry && sphere_id[s] < sv.n_objects) entry_of[sphere_id[s]] = prim_entry[s];
        for (size_t r = 0; r < tri_fidx.size(); ++r)
            if (tri_fidx[r] < tris.size() && tris[tri_fidx[r]].id < sv.n_objects) entry_of[tris[tri_fidx[r]].id] = (uint32_t)r | kTriEntry;
    }
    // every leaf entry's path: one row of {link, child slot} per entry, found by one walk of the whole tree
    const uint32_t stride = std::max(sv.bvh_depth, 1u);
    const size_t n_rows = prims.size() + tri_fidx.size();
    std::vector<uint32_t> steps(2 * n_rows * stride, 0u), lens(n_rows + 1, 0u);
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    if (!nodes.empty()) {
        struct Frame { uint32_t link; std::vector<uint32_t> path; };
        std::vector<Frame> todo;
        todo.push_back({sv.bvh_root, {}});
        size_t visited = 0;
        while (!todo.empty()) {
            Frame f = std::move(todo.back());
            todo.pop_back();
            const uint32_t idx = f.link & ~kBvhFlatNode;
            if (idx >= nodes.size() || ++visited > nodes.size() || f.path.size() / 2 >= stride)
                return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: the resident tree is not a tree of the recorded depth");
            const Bvh4Node &w = nodes[idx];
            for (uint32_t c = 0; c < 4; ++c) {
                uint32_t lnk, cnt;
                if (f.link & kBvhFlatNode) {
                    const float l4[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, c4[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
                    lnk = bits(l4[c]); cnt = bits(c4[c]);
                } else { lnk = bits(w.a[c].w); cnt = bits(w.b[c].w); }
                if (cnt == 0xFFFFFFFFu) continue;
                std::vector<uint32_t> path = f.path;
                path.push_back(f.link); path.push_back(c);
                if (cnt == 0u) { todo.push_back({lnk, std::move(path)}); continue; }
                const bool tri = (cnt & kBvhTriLeaf) != 0u;
                for (uint32_t k = 0; k < (cnt & 0xFFFFu); ++k) {
                    const size_t e = (size_t)lnk + k;
                    if (e >= (tri ? tri_fidx.size() : prims.size())) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: a leaf entry outside its array");
                    const size_t row = tri ? prims.size() + e : e;
                    lens[row] = (uint32_t)(path.size() / 2);
                    std::copy(path.begin(), path.end(), steps.begin() + (ptrdiff_t)(2 * row * stride));
                }
            }
        }
    }
    std::vector<uint32_t> entries(n), rows(n);
    std::vector<Bvh4Node> leaf_nodes(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (objects[i] >= sv.n_objects) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_path_bounds: an object index outside Scene.objects");
        uint32_t e = entry_of[objects[i]];
        size_t row = n_rows;                                    // (the spare row: length 0)
        if (e != kNoEntry) {
            row = (e & kTriEntry) ? prims.size() + (e & ~kTriEntry) : e;
            if (lens[row] == 0u) e = kNoEntry;                  // (in no leaf: cannot happen for a tree rtx_debug_host_scene accepts)
        }
        if (e == kNoEntry) row = n_rows;
        entries[i] = e; rows[i] = (uint32_t)row;
        Bvh4Node &w = leaf_nodes[i];
        for (int c = 0; c < 4; ++c) {
            w.a[c] = make_float4(INFINITY, INFINITY, INFINITY, u32_as_f32(0u));
            w.b[c] = make_float4(-INFINITY, -INFINITY, -INFINITY, u32_as_f32(0xFFFFFFFFu));
        }
        if (e != kNoEntry) {
            w.a[0] = make_float4(-INFINITY, -INFINITY, -INFINITY, u32_as_f32(e & ~kTriEntry));
            w.b[0] = make_float4(INFINITY, INFINITY, INFINITY, u32_as_f32((e & kTriEntry) ? (kBvhTriLeaf | 1u) : 1u));
        }
    }
    if (records) {                                              // the object's resident f32 records, as the leaf tests read them
        std::vector<float4> cr(prims.size()), l32(prims.size()), t32(2 * tri_fidx.size()), geo(2 * tri_fidx.size());
        std::vector<float> s32(prims.empty() ? 0u : (((size_t)sv.n_spheres + 3) & ~(size_t)3) * 4);
        RTX_HIP_CHECK(down(cr.data(), sv.bvh_leaf_cr, cr.size() * sizeof(float4)));
        if (filter_records) {
            RTX_HIP_CHECK(down(l32.data(), sv.bvh_leaf_f32, l32.size() * sizeof(float4)));
            RTX_HIP_CHECK(down(s32.data(), sv.sphere_f32, s32.size() * sizeof(float)));
        }
        RTX_HIP_CHECK(down(t32.data(), sv.tri_f32, t32.size() * sizeof(float4)));
        RTX_HIP_CHECK(down(geo.data(), sv.tri_geo, geo.size() * sizeof(float4)));
        std::memset(records, 0, n * 16 * sizeof(uint32_t));
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t e = entries[i];
            if (e == kNoEntry) continue;
            if (e & kTriEntry) {
                const size_t r = e & ~kTriEntry;
                const float4 four[4] = { t32[2 * r], t32[2 * r + 1], geo[2 * r], geo[2 * r + 1] };
                std::memcpy(records + 16 * i, four, sizeof four);
            } else {
                std::memcpy(records + 16 * i, &cr[e], sizeof(float4));
                if (!filter_records) continue;
                std::memcpy(records + 16 * i + 4, &l32[e], sizeof(float4));
                const uint32_t k = prims[e];                    // the pair-interleaved filter record of the same sphere, as scalars
                if ((size_t)(k | 1u) * 4 + 3 < s32.size()) {
                    const float *f = s32.data() + (size_t)(k & ~1u) * 4 + (k & 1u);
                    const float four[4] = { f[0], f[2], f[4], f[6] };
                    std::memcpy(records + 16 * i + 8, four, sizeof four);
                }
            }
        }
    }
    if (path_data && path_steps) {                              // the object's child at every step, in the form the slab test reads
        std::vector<BvhQ3Node> q3((form & 2u) && (sv.bvh_flags & 16u) && sv.bvh_q3nodes ? nodes.size() : 0u);
        std::vector<BvhQNode> qn((form & 2u) && q3.empty() ? nodes.size() : 0u);
        RTX_HIP_CHECK(down(q3.data(), sv.bvh_q3nodes, q3.size() * sizeof(BvhQ3Node)));
        RTX_HIP_CHECK(down(qn.data(), sv.bvh_qnodes, qn.size() * sizeof(BvhQNode)));
        std::memset(path_data, 0, n * (size_t)path_steps * 16 * sizeof(uint32_t));
        for (uint64_t i = 0; i < n; ++i) {
            const size_t row = rows[i];
            for (uint32_t k = 0; k < lens[row] && k < path_steps; ++k) {
                const uint32_t link = steps[2 * (row * stride + k)], c = steps[2 * (row * stride + k) + 1], idx = link & ~kBvhFlatNode;
                uint32_t *w = path_data + 16 * ((size_t)i * path_steps + k);
                auto putf = [&](int at, float f) { std::memcpy(w + at, &f, 4); };
                if (!q3.empty()) {
                    const BvhQ3Node &q = q3[idx];
                    w[0] = 2u;
                    putf(1, q.ox); putf(2, q.oy); putf(3, q.oz); putf(4, q.sx); putf(5, q.sy); putf(6, q.sz);
                    w[7] = (q.lox >> (8 * c)) & 255u; w[8] = (q.loy >> (8 * c)) & 255u; w[9] = (q.loz >> (8 * c)) & 255u;
                    w[10] = (q.hix >> (8 * c)) & 255u; w[11] = (q.hiy >> (8 * c)) & 255u; w[12] = (q.hiz >> (8 * c)) & 255u;
                } else if (!qn.empty()) {
                    const BvhQNode &q = qn[idx];
                    w[0] = 3u;
                    putf(1, q.ox); putf(2, q.oy); putf(3, q.sx); putf(4, q.sy); w[5] = q.qx[c]; w[6] = q.qy[c];
                } else if (link & kBvhFlatNode) {
                    w[0] = 1u;
                    putf(1, nodes[idx].a[c].x); putf(2, nodes[idx].a[c].y); putf(3, nodes[idx].a[c].z); putf(4, nodes[idx].a[c].w);
                } else {
                    w[0] = 0u;
                    putf(1, nodes[idx].a[c].x); putf(2, nodes[idx].a[c].y); putf(3, nodes[idx].a[c].z);
                    putf(4, nodes[idx].b[c].x); putf(5, nodes[idx].b[c].y); putf(6, nodes[idx].b[c].z);
                }
                w[15] = link;
            }
        }
    }
    DebugBufs d;
    void *d_sv, *d_rays, *d_entries, *d_rows, *d_lens, *d_steps, *d_best, *d_leaf, *d_out;
    RTX_HIP_CHECK(d.up(&sv, sizeof(SceneView), &d_sv));
    RTX_HIP_CHECK(d.up(rays, n * sizeof(RtxRay), &d_rays));
    RTX_HIP_CHECK(d.up(entries.data(), n * sizeof(uint32_t), &d_entries));
    RTX_HIP_CHECK(d.up(rows.data(), n * sizeof(uint32_t), &d_rows));
    RTX_HIP_CHECK(d.up(lens.data(), lens.size() * sizeof(uint32_t), &d_lens));
    steps.resize(steps.size() + 2, 0u);                         // (never empty)
    RTX_HIP_CHECK(d.up(steps.data(), steps.size() * sizeof(uint32_t), &d_steps));
    RTX_HIP_CHECK(d.up(best_up, n * sizeof(float), &d_best));
    RTX_HIP_CHECK(d.up(leaf_nodes.data(), n * sizeof(Bvh4Node), &d_leaf));
    RTX_HIP_CHECK(d.up(out, n * 8 * sizeof(uint32_t), &d_out));
    static_assert(sizeof(RtxRay) == sizeof(QueryRay), "RtxRay layout");
    PathBoundsArgs a;
    a.rays = static_cast<const QueryRay *>(d_rays); a.entries = static_cast<const uint32_t *>(d_entries);
    a.rows = static_cast<const uint32_t *>(d_rows); a.lens = static_cast<const uint32_t *>(d_lens);
    a.steps = static_cast<const uint32_t *>(d_steps); a.best_up = static_cast<const float *>(d_best);
    a.leaf_nodes = static_cast<const float4 *>(d_leaf); a.out = static_cast<uint32_t *>(d_out);
    a.n = n; a.stride = stride; a.form = form;
    RTX_HIP_CHECK(launch_debug_path_bounds(static_cast<const SceneView *>(d_sv), a, nullptr));
    RTX_HIP_CHECK(hipMemcpy(out, d_out, n * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost));   // (the null stream: after the kernel)
    return RTX_OK;
#endif
}

int32_t rtx_debug_tile_lists(RtxSceneHandle h, uint32_t *info, uint32_t *counts, uint32_t *entries, uint64_t max_tiles)
{
#ifndef RTX_LAB
    (void)h; (void)info; (void)counts; (void)entries; (void)max_tiles;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_tile_lists: a lab-library hook (librtx_hip_lab.so)");
#else
    if (!h || !info) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_tile_lists: null argument");
    const SceneView &sv = h->sv;
    const uint32_t form = h->tl_form, n_tiles = form ? h->tl_tiles : 0u;
    // the launches' own sizes: one tile's share of the bytes they ask for is its cap x the entry's size
    const size_t head = ((size_t)n_tiles * sizeof(uint32_t) + 255) & ~(size_t)255;
    const size_t entry_bytes = form == 1u ? sizeof(TileEntry) : sizeof(uint2);
    const size_t bytes = form == 1u ? bvh_spheres_tile_list_bytes((uint64_t)n_tiles << 6) : wavefront_tile_list_bytes((uint64_t)n_tiles << 6);
    const uint32_t cap = form == 0u ? 0u : (uint32_t)((form == 1u ? bvh_spheres_tile_list_bytes(64) - 256 : wavefront_tile_list_bytes(64) - 256) / entry_bytes);
    const uint32_t words = (uint32_t)(entry_bytes / sizeof(uint32_t));
    const uint32_t head_info[8] = { form, h->tl_tiles_x, n_tiles, cap, words, h->tl_builds, 0u, 0u };
    std::memcpy(info, head_info, sizeof head_info);
    if (form == 0u || n_tiles == 0u || (!counts && !entries)) return RTX_OK;
    if (!counts || !entries || max_tiles < n_tiles) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_tile_lists: counts and entries hold info[2] tiles");
    if ((uint64_t)n_tiles * cap > (1ull << 22)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_tile_lists: too large");
    if (!h->tile_lists || h->tile_lists_bytes < bytes || bytes != head + (size_t)n_tiles * cap * entry_bytes)
        return fail(RTX_ERR_HIP, "internal: the handle's tile lists are smaller than the last launch's");
    RTX_HIP_CHECK(hipSetDevice(h->device));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> raw(bytes / sizeof(uint32_t));
    RTX_HIP_CHECK(hipMemcpy(raw.data(), h->tile_lists, bytes, hipMemcpyDeviceToHost));
    // leaf entry -> Scene.objects, through the tables the kernels themselves go through
    const bool s_tree = (sv.bvh_flags & 1u) != 0u, t_tree = (sv.bvh_flags & 2u) != 0u;
    std::vector<uint32_t> prims(s_tree ? sv.n_spheres : 0u), sphere_id(sv.n_spheres), tri_fidx(t_tree ? sv.n_tri_tree : 0u);
    std::vector<TriX> tris(t_tree ? sv.n_tris : 0u);
    auto down = [](void *dst, const void *src, size_t b) { return b ? hipMemcpy(dst, src, b, hipMemcpyDeviceToHost) : hipSuccess; };
    RTX_HIP_CHECK(down(prims.data(), sv.bvh_prims, prims.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(sphere_id.data(), sv.sphere_id, sphere_id.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(tri_fidx.data(), sv.tri_fidx, tri_fidx.size() * sizeof(uint32_t)));
    RTX_HIP_CHECK(down(tris.data(), sv.tris, tris.size() * sizeof(TriX)));
    constexpr uint32_t kNoObject = 0xFFFFFFFFu, kSphereEntry = 0x80000000u;
    auto sphere_object = [&](uint32_t prim) { return prim < sphere_id.size() && sphere_id[prim] < sv.n_objects ? sphere_id[prim] : kNoObject; };
    std::memcpy(counts, raw.data(), (size_t)n_tiles * sizeof(uint32_t));
    std::memset(entries, 0, (size_t)n_tiles * cap * 12 * sizeof(uint32_t));
    const uint32_t *lists = raw.data() + head / sizeof(uint32_t);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        if (counts[t] > cap) continue;                          // (kTileListWalk: the tile has no list; anything else above the cap: the caller's finding)
        for (uint32_t k = 0; k < counts[t]; ++k) {
            const uint32_t *src = lists + ((size_t)t * cap + k) * words;
            uint32_t *dst = entries + ((size_t)t * cap + k) * 12;
            std::memcpy(dst, src, entry_bytes);
            uint32_t object = kNoObject, kind = 0u;
            if (form == 1u) {                                   // TileEntry {rec, prim, t_lb, pad, pad}
                dst[8] = src[5];
                object = sphere_object(src[4]);
            } else {                                            // {entry, t_lb}: a sphere leaf entry (the flag) or a filter record
                dst[8] = src[1];
                const uint32_t e = src[0] & ~kSphereEntry;
                if (src[0] & kSphereEntry) object = e < prims.size() ? sphere_object(prims[e]) : kNoObject;
                else {
                    kind = 1u;
                    if (e < tri_fidx.size() && tri_fidx[e] < tris.size() && tris[tri_fidx[e]].id < sv.n_objects) object = tris[tri_fidx[e]].id;
                }
            }
            dst[9] = object; dst[10] = kind;
        }
    }
    return RTX_OK;
#endif
}

int32_t rtx_debug_sweep_filter(RtxSceneHandle h, const RtxRay *rays, const uint32_t *objects, uint64_t n, uint32_t *out, double *scene_info)
{
#ifndef RTX_LAB
    (void)h; (void)rays; (void)objects; (void)n; (void)out; (void)scene_info;
    return fail(RTX_ERR_UNSUPPORTED, "rtx_debug_sweep_filter: a lab-library hook (librtx_hip_lab.so)");
#else
    if (!h) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_sweep_filter: null scene");
    const SceneView &sv = h->sv;
    if (scene_info) {
        uint32_t q = 0, overflow = 0;
        mixed_queue_sizes(&q, &overflow);
        const double info[16] = { sv.sphere_center[0], sv.sphere_center[1], sv.sphere_center[2], sv.sphere_cmax, sv.tri_extent,
                                  (double)sv.n_spheres, (double)sv.n_tri_filter, (double)q, (double)overflow, (double)sv.n_planes,
                                  (double)sv.n_tris, (double)sv.n_objects, (double)sv.n_tri_tree, 0.0, 0.0, 0.0 };
        std::memcpy(scene_info, info, sizeof info);
    }
    if (n == 0) return RTX_OK;
    if (!rays || !out) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_sweep_filter: null argument");
    if (n > (1ull << 22)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_sweep_filter: too large");
    RTX_HIP_CHECK(hipSetDevice(h->device));
    RTX_HIP_CHECK(hipDeviceSynchronize());
    constexpr uint32_t kTriEntry = 0x80000000u, kNoEntry = 0xFFFFFFFFu;
    std::vector<uint32_t> entries;
    if (objects) {                                              // Scene.objects index -> the filter record, through the sweep's own tables
        std::vector<uint32_t> sphere_id(sv.n_spheres), tri_fidx(sv.n_tri_filter);
        std::vector<TriX> tris(sv.n_tri_filter ? sv.n_tris : 0u);
        auto down = [](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
        RTX_HIP_CHECK(down(sphere_id.data(), sv.sphere_id, sphere_id.size() * sizeof(uint32_t)));
        RTX_HIP_CHECK(down(tri_fidx.data(), sv.tri_fidx, tri_fidx.size() * sizeof(uint32_t)));
        RTX_HIP_CHECK(down(tris.data(), sv.tris, tris.size() * sizeof(TriX)));
        std::vector<uint32_t> entry_of(sv.n_objects, kNoEntry);
        for (size_t k = 0; k < sphere_id.size(); ++k) if (sphere_id[k] < sv.n_objects) entry_of[sphere_id[k]] = (uint32_t)k;
        for (size_t r = 0; r < tri_fidx.size(); ++r)
            if (tri_fidx[r] < tris.size() && tris[tri_fidx[r]].id < sv.n_objects) entry_of[tris[tri_fidx[r]].id] = (uint32_t)r | kTriEntry;
        entries.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            if (objects[i] >= sv.n_objects) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_debug_sweep_filter: an object index outside Scene.objects");
            entries[i] = entry_of[objects[i]];
        }
    }
    const size_t out_bytes = n * (objects ? 24 : 4) * sizeof(uint32_t);
    DebugBufs d;
    void *d_sv, *d_rays, *d_entries, *d_out;
    RTX_HIP_CHECK(d.up(&sv, sizeof(SceneView), &d_sv));
    RTX_HIP_CHECK(d.up(rays, n * sizeof(RtxRay), &d_rays));
    RTX_HIP_CHECK(d.up(entries.data(), entries.size() * sizeof(uint32_t), &d_entries));
    RTX_HIP_CHECK(d.up(out, out_bytes, &d_out));
    static_assert(sizeof(RtxRay) == sizeof(QueryRay), "RtxRay layout");
    SweepFilterArgs a;
    a.rays = static_cast<const QueryRay *>(d_rays); a.entries = static_cast<const uint32_t *>(d_entries);
    a.out = static_cast<uint32_t *>(d_out); a.n = n;
    RTX_HIP_CHECK(launch_debug_sweep_filter(static_cast<const SceneView *>(d_sv), a, nullptr));
    RTX_HIP_CHECK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));                  // (the null stream: after the kernel)
    return RTX_OK;
#endif
}

}  // extern "C"
