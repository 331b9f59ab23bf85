// rtx_rewind.hip -- rtx_rewind_hits_device, rtx_rewind_hits and rtx_object_motions (include/rtx_hip.h "Rewinding a pick buffer",
// DESIGN.md 3.16): the argument checks (made before any device is looked for), the one launch, the one-shot host form, and the host-only
// folding of update entries into the sorted list.  The device text is rtx_rewind.h, compiled into epilogue_kernel (rtx_kernels.hip) as
// one launch-uniform form.
#include "rtx_host.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

static_assert(sizeof(RewindMotion) == sizeof(RtxObjectMotion) && offsetof(RewindMotion, now) == offsetof(RtxObjectMotion, now) &&
              offsetof(RewindMotion, before) == offsetof(RtxObjectMotion, before), "RewindMotion is RtxObjectMotion");

bool shape_kind(uint32_t k) { return k == RTX_SPHERE || k == RTX_PLANE || k == RTX_TRIANGLE; }

// everything the two calls refuse alike, without a device.  aligned: the device form's 16-byte rule
int32_t check_call(const char *who, const RtxHit *hits, uint64_t n, const int64_t *objects, const RtxObjectMotion *motions, uint64_t m,
                   uint32_t flags, const RtxHit *out, bool aligned)
{
    const std::string w = std::string(who) + ": ";
    if (!hits || !out) return fail(RTX_ERR_INVALID_ARGUMENT, w + "null hits or output");
    if (aligned && ((((uintptr_t)hits) | ((uintptr_t)out)) & 15u)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "hits or output not 16-byte aligned");
    if (n == 0 || n >= 0xFFFFFFF0ull) return fail(RTX_ERR_INVALID_ARGUMENT, w + "n_hits is 0, or 2^32 - 16 or more");
    if (m >= (1ull << 31)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "2^31 moved objects or more");
    if (m > 0 && (!objects || !motions)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "moved objects without their list or records");
    if (flags != 0u) return fail(RTX_ERR_INVALID_ARGUMENT, w + "flags must be 0");
    const size_t h = (size_t)(n * sizeof(RtxHit));
    const Range r[4] = { { hits, h }, { m ? objects : nullptr, (size_t)(m * 8) }, { m ? motions : nullptr, (size_t)(m * sizeof(RtxObjectMotion)) },
                         { out, h } };
    if (ranges_overlap(r, 4)) return fail(RTX_ERR_INVALID_ARGUMENT, w + "input and output buffers overlap");
    return RTX_OK;
}

}  // namespace

extern "C" {

int32_t rtx_rewind_hits_device(const RtxHit *d_hits, uint64_t n_hits, const int64_t *d_objects, const RtxObjectMotion *d_motions, uint64_t m,
                               uint32_t flags, RtxHit *d_out, int32_t device, void *stream_)
{
    if (int32_t rc = check_call("rtx_rewind_hits_device", d_hits, n_hits, d_objects, d_motions, m, flags, d_out, true)) return rc;
    if (int32_t rc = check_device(device, "rtx_rewind_hits_device")) return rc;
    RTX_HIP_CHECK(hipSetDevice(device));
    RewindArgs r{};
    r.hits = reinterpret_cast<const QueryHit *>(d_hits); r.out = reinterpret_cast<QueryHit *>(d_out);
    r.n = (uint32_t)n_hits; r.m = (uint32_t)m;
    if (m) { r.objects = reinterpret_cast<const long long *>(d_objects); r.motions = reinterpret_cast<const RewindMotion *>(d_motions); }
    RTX_HIP_CHECK(launch_rewind(r, static_cast<hipStream_t>(stream_)));
    return RTX_OK;
}

int32_t rtx_rewind_hits(const RtxHit *hits, uint64_t n_hits, const int64_t *objects, const RtxObjectMotion *motions, uint64_t m, RtxHit *out)
{
    if (int32_t rc = check_call("rtx_rewind_hits", hits, n_hits, objects, motions, m, 0u, out, false)) return rc;
    for (uint64_t k = 0; k < m; ++k) {
        RtxObjectMotion mk;                                 // (a copy: the caller's records may be unaligned)
        std::memcpy(&mk, (const char *)motions + k * sizeof mk, sizeof mk);
        int64_t a, b = 0;
        std::memcpy(&a, (const char *)objects + k * 8, 8);
        if (k) std::memcpy(&b, (const char *)objects + (k - 1) * 8, 8);
        if (k && !(b < a)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_rewind_hits: the object list is not strictly ascending");
        if (!shape_kind(mk.kind) && mk.kind != RTX_MOTION_LOST) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_rewind_hits: unknown kind");
        if (mk.reserved != 0u) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_rewind_hits: reserved must be 0");
    }
    if (int32_t rc = check_device(0, "rtx_rewind_hits")) return rc;
    RTX_HIP_CHECK(hipSetDevice(0));
    // one allocation: the hits, the list, the records, then the output
    const uint64_t sizes[4] = { n_hits * sizeof(RtxHit), m * 8, m * sizeof(RtxObjectMotion), n_hits * sizeof(RtxHit) };
    const void *src[3] = { hits, objects, motions };
    uint64_t off[5] = { 0 };
    for (int i = 0; i < 4; ++i) off[i + 1] = off[i] + ((sizes[i] + 127u) & ~(uint64_t)127u);
    char *base = nullptr;
    RTX_HIP_CHECK(hipMalloc((void **)&base, off[4]));
    struct Free { char *p; ~Free() { (void)hipFree(p); } } guard{ base };
    auto at = [&](int i) -> void * { return sizes[i] ? base + off[i] : nullptr; };
    for (int i = 0; i < 3; ++i)
        if (sizes[i]) RTX_HIP_CHECK(hipMemcpy(at(i), src[i], sizes[i], hipMemcpyHostToDevice));
    if (int32_t rc = rtx_rewind_hits_device((const RtxHit *)at(0), n_hits, (const int64_t *)at(1), (const RtxObjectMotion *)at(2), m, 0u,
                                            (RtxHit *)at(3), 0, nullptr)) return rc;
    RTX_HIP_CHECK(hipDeviceSynchronize());
    RTX_HIP_CHECK(hipMemcpy(out, at(3), sizes[3], hipMemcpyDeviceToHost));
    return RTX_OK;
}

int32_t rtx_object_motions(const uint64_t *indices, const RtxObject *before, const RtxObject *now, uint64_t n, int64_t *objects_out,
                           RtxObjectMotion *motions_out, uint64_t *m_out)
{
    const char *who = "rtx_object_motions: ";
    if (!m_out) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "null m_out");
    if (n >= (1ull << 31)) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "2^31 entries or more");
    if (n > 0 && (!indices || !before || !now || !objects_out || !motions_out))
        return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "null indices, records or outputs");
    for (uint64_t i = 0; i < n; ++i) {
        if (indices[i] >> 63) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "an index of 2^63 or more");
        if (!shape_kind(now[i].kind)) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "a new record of an unknown kind");
        if (!shape_kind(before[i].kind) && before[i].kind != RTX_MOTION_LOST)
            return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + "a previous record of an unknown kind");
    }
    // entries in index order, call order kept among equal indices: the first of a run gives `before`, the last `now`
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return indices[a] < indices[b]; });
    static const int kWords[3] = { 4, 6, 9 };
    uint64_t m = 0;
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a;
        while (b + 1 < n && indices[order[b + 1]] == indices[order[a]]) ++b;
        const RtxObject &was = before[order[a]], &is = now[order[b]];
        RtxObjectMotion rec;
        std::memset(&rec, 0, sizeof rec);
        bool keep = true;
        if (was.kind != is.kind) {                          // (RTX_MOTION_LOST in `before` is never a shape kind: it ends up here)
            rec.kind = RTX_MOTION_LOST;
        } else if (std::memcmp(was.geom, is.geom, (size_t)kWords[is.kind] * sizeof(double)) == 0) {
            keep = false;                                   // a material update
        } else {
            rec.kind = is.kind;
            std::memcpy(rec.now, is.geom, sizeof rec.now);
            std::memcpy(rec.before, was.geom, sizeof rec.before);
        }
        if (keep) { objects_out[m] = (int64_t)indices[order[a]]; motions_out[m] = rec; ++m; }
        a = b + 1;
    }
    *m_out = m;
    return RTX_OK;
}

}  // extern "C"
