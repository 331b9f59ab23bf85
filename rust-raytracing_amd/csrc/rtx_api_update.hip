// rtx_api_update.hip -- rtx_scene_update_objects, rtx_scene_set_visible and rtx_scene_append_objects (include/rtx_hip.h, DESIGN.md
// "Moving objects", "Hidden objects"): the device side of an update that rtx_pack.hip planned -- the tables of the resident pack, the
// launches of scene_update_kernel in run_update's order (rtx_pack.h: the order the host reference refit_packed runs too), and the
// rebuild every entry point falls back to, which keeps the hidden set.
#include "rtx_host.h"

#include <cstring>

namespace {

// A device copy of a host table (nothing is allocated for an empty one).
template <class T>
hipError_t put_table(T **dst, const std::vector<T> &v)
{
    if (v.empty()) return hipSuccess;
    const hipError_t e = hipMalloc((void **)dst, v.size() * sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

// The device side of the refit tables of the resident pack, made at the first REFIT or RECORDS call after it (a hidden object has
// hide_record's rows in them: the nothing box, reach 0).
int32_t ensure_update_tables(RtxSceneHandle_ *h)
{
    auto &b = h->upd;
    if (!b.d_status) RTX_HIP_CHECK(hipMalloc((void **)&b.d_status, 3 * sizeof(unsigned long long)));
    if (!b.h_status) RTX_HIP_CHECK(hipHostMalloc((void **)&b.h_status, 3 * sizeof(unsigned long long), hipHostMallocDefault));
    if (b.valid) return RTX_OK;
    drop_update_tables(h);
    const RefitTables &t = h->refit;
    std::vector<float> box32;
    std::vector<double> reach;
    derive_all_spheres(h->objects.data(), h->objects.size(), t, h->sv.n_spheres, box32, reach, h->hidden.empty() ? nullptr : h->hidden.data());
    RTX_HIP_CHECK(put_table(&b.box32, box32));
    RTX_HIP_CHECK(put_table(&b.reach, reach));
    RTX_HIP_CHECK(put_table(&b.levels, t.level_nodes));
    b.valid = true;
    return RTX_OK;
}

// The triangle half of the device tables (derive_all_spheres' analogue), made at the first call that rewrites a triangle in place.
int32_t ensure_mesh_tables(RtxSceneHandle_ *h)
{
    auto &b = h->upd;
    if (b.mesh_valid) return RTX_OK;
    const RefitTables &t = h->refit;
    std::vector<float> tribox32;
    std::vector<double> tri_reach;
    derive_all_triangles(h->objects.data(), h->objects.size(), t, tribox32, tri_reach, h->hidden.empty() ? nullptr : h->hidden.data());
    RTX_HIP_CHECK(put_table(&b.tribox32, tribox32));
    RTX_HIP_CHECK(put_table(&b.tri_reach, tri_reach));
    if (!b.all_levels) RTX_HIP_CHECK(put_table(&b.all_levels, t.all_level_nodes));
    b.mesh_valid = true;
    return RTX_OK;
}

// The device side of one planned update (plan.how is REFIT or RECORDS): the tables it needs, the entries through the pinned staging
// buffer, run_update's launches on `stream` behind whatever earlier calls enqueued, one pinned read-back.  On return the work has
// completed; plan.how is REBUILT when a 64-byte node had no encoding (the caller replaces every array), else h->sv holds the new
// sphere_cmax / tri_extent.  A visibility plan on a pack without kept words allocates them and lets mode E fill them first.
int32_t apply_plan(RtxSceneHandle_ *h, UpdatePlan &plan, hipStream_t stream)
{
    auto &b = h->upd;
    touch_scene(h);                                       // (the resident arrays are rewritten in place: a refit, new records, a hide or show)
    if (int32_t rc = ensure_update_tables(h)) return rc;
    if (plan.tri_geom) if (int32_t rc = ensure_mesh_tables(h)) return rc;
    const RefitTables &t = h->refit;
    plan.capture = plan.visibility && !b.keep_valid;
    if (plan.capture) {
        if (!t.all_level_nodes.empty() && !b.all_levels) RTX_HIP_CHECK(put_table(&b.all_levels, t.all_level_nodes));
        if (h->sv.n_bvh_nodes) RTX_HIP_CHECK(hipMalloc((void **)&b.keep, (size_t)h->sv.n_bvh_nodes * kKeepWords * sizeof(uint32_t)));
        b.keep_valid = true;
    }
    const size_t ne = plan.entries.size(), bytes = ne * sizeof(UpdateEntry);
    if (b.h_cap < ne) {
        if (b.h_entries) { RTX_HIP_CHECK(hipHostFree(b.h_entries)); b.h_entries = nullptr; b.h_cap = 0; }
        RTX_HIP_CHECK(hipHostMalloc((void **)&b.h_entries, bytes, hipHostMallocDefault));
        b.h_cap = ne;
    }
    if (b.d_cap < ne) {
        if (b.d_entries) { RTX_HIP_CHECK(hipFree(b.d_entries)); b.d_entries = nullptr; b.d_cap = 0; }
        RTX_HIP_CHECK(hipMalloc((void **)&b.d_entries, bytes));
        b.d_cap = ne;
    }
    std::memcpy(b.h_entries, plan.entries.data(), bytes);
    {
        if (int32_t rc = adopt_stream(h, stream)) return rc;      // the writes below wait for what earlier calls enqueued
        DoneGuard done{h, stream};
        const SceneView &sv = h->sv;
        RTX_HIP_CHECK(hipMemcpyAsync(b.d_entries, b.h_entries, bytes, hipMemcpyHostToDevice, stream));
        const size_t status_bytes = (plan.any_tri ? 3 : 2) * sizeof(unsigned long long);      // (the third word: mode D's)
        RTX_HIP_CHECK(hipMemsetAsync(b.d_status, 0, status_bytes, stream));
        UpdateArgs u = update_args(sv, t, b.d_entries, b.box32, b.reach, b.tribox32, b.tri_reach, plan.tri_geom, b.keep);
        u.status = b.d_status;
        hipError_t scene_update_launch = hipSuccess;
        run_update(u, t, plan, b.levels, b.all_levels, sv.n_spheres, sv.n_tris,
                   [&](const UpdateArgs &a) { return (scene_update_launch = launch_scene_update(a, stream)) == hipSuccess; });
        RTX_HIP_CHECK(scene_update_launch);
        RTX_HIP_CHECK(hipMemcpyAsync(b.h_status, b.d_status, status_bytes, hipMemcpyDeviceToHost, stream));
        RTX_HIP_CHECK(hipStreamSynchronize(stream));
    }
    if (b.h_status[0] & (kUpdateStatusNoQ3 | kUpdateStatusNoQ)) { plan.how = RTX_UPDATED_REBUILT; return RTX_OK; }
    if (plan.any_sphere) { std::memcpy(&h->sv.sphere_cmax, &b.h_status[1], sizeof(double)); h->sv_dirty = true; }
    if (plan.any_tri) { std::memcpy(&h->sv.tri_extent, &b.h_status[2], sizeof(double)); h->sv_dirty = true; }
    return RTX_OK;
}

// Replaces the object list by `all` and packs it again (an append, an update or a show that rebuilds) -- the list with its REAL
// geometries, so a hidden object keeps its slot and can be shown in place -- then hides `hidden`'s objects on the fresh arrays (the
// hide pass: hide entries for all of them, from a pack in which nothing is hidden).  The new arrays are uploaded first and swapped in
// on success (upload_packed), so a failed pack leaves the resident scene and the handle's list as they were.  The caller has
// synchronised with the device: a render may still read the arrays about to be replaced.
int32_t repack_objects(RtxSceneHandle_ *h, std::vector<RtxObject> &all, std::vector<uint8_t> &hidden, hipStream_t stream)
{
    RtxScene sc{};
    sc.config = h->cfg;
    sc.camera = h->cam;
    sc.n_objects = all.size();
    sc.objects = all.data();
    PackedScene p;
    if (int32_t rc = pack_scene(&sc, p)) return rc;
    if (int32_t rc = upload_packed(h, p)) return rc;
    h->objects.swap(all);
    h->hidden.clear();                                        // (the tables of the fresh pack are those of the all-visible list)
    std::vector<uint64_t> idx;
    for (size_t k = 0; k < hidden.size(); ++k) if (hidden[k]) idx.push_back(k);
    if (idx.empty()) return RTX_OK;
    const std::vector<uint8_t> none(h->objects.size(), 0);
    UpdatePlan plan;
    if (int32_t rc = plan_visibility(h->objects, none, h->refit, 0.0, idx.data(), idx.size(), 0u, plan)) return rc;
    if (!(h->sv.sphere_cmax < 1.0e14)) plan.any_sphere = false;   // (mode C only runs over finite reaches; such a pack stays "every ray sweeps")
    if (int32_t rc = apply_plan(h, plan, stream)) return rc;
    h->hidden.swap(hidden);
    h->hidden.resize(h->objects.size(), 0);
    if (plan.how == RTX_UPDATED_REBUILT) return fail(RTX_ERR_UNSUPPORTED, "hidden objects: a 64-byte node of the fresh pack has no encoding without them");
    return RTX_OK;
}

// The handle's visibility bytes at the length of `n` objects.
std::vector<uint8_t> hidden_bytes(const RtxSceneHandle_ *h, size_t n)
{
    std::vector<uint8_t> v = h->hidden;
    v.resize(n, 0);
    return v;
}

}  // namespace

extern "C" {

int32_t rtx_scene_append_objects(RtxSceneHandle scene, const RtxObject *objects, uint64_t n_objects)
{
    if (!scene || (n_objects && !objects)) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_append_objects: null argument");
    if (n_objects == 0) return RTX_OK;
    touch_scene(scene);
    if (scene->objects.size() + n_objects > 0xFFFFFFF0ull) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_append_objects: too many objects");
    RTX_HIP_CHECK(hipSetDevice(scene->device));
    RTX_HIP_CHECK(hipDeviceSynchronize());                  // a render may still read the arrays about to be replaced
    if (int32_t rc = check_watchdog(scene, true)) return rc;
    std::vector<RtxObject> all = scene->objects;
    all.insert(all.end(), objects, objects + n_objects);
    std::vector<uint8_t> hidden = hidden_bytes(scene, all.size());      // the new objects are visible
    return repack_objects(scene, all, hidden, nullptr);     // (on failure the resident scene is as it was)
}

int32_t rtx_scene_update_objects(RtxSceneHandle h, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                                 void *stream_, uint32_t *how)
{
    if (how) *how = RTX_UPDATED_NOTHING;
    if (!h) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_update_objects: null scene");
    touch_scene(h);
    UpdatePlan plan;
    if (int32_t rc = plan_update(h->objects, h->refit, h->sv.sphere_cmax, indices, objects, n, mode, plan, h->hidden.empty() ? nullptr : h->hidden.data()))
        return rc;
    if (plan.entries.empty()) return RTX_OK;
    RTX_HIP_CHECK(hipSetDevice(h->device));
    if (int32_t rc = check_watchdog(h, true)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (plan.how != RTX_UPDATED_REBUILT) {
        if (int32_t rc = apply_plan(h, plan, stream)) return rc;
        if (plan.how != RTX_UPDATED_REBUILT)                    // (else every array is replaced below)
            for (const UpdateEntry &e : plan.entries) std::memcpy(&h->objects[e.object], &e.kind, sizeof(RtxObject));
    }
    if (plan.how == RTX_UPDATED_REBUILT) {                      // the update as a rebuild: rtx_scene_append_objects' path on the modified list
        RTX_HIP_CHECK(hipDeviceSynchronize());                  // a render may still read the arrays about to be replaced
        std::vector<RtxObject> all = h->objects;
        for (const UpdateEntry &e : plan.entries) std::memcpy(&all[e.object], &e.kind, sizeof(RtxObject));
        std::vector<uint8_t> hidden = hidden_bytes(h, all.size());
        if (int32_t rc = repack_objects(h, all, hidden, stream)) return rc;
    }
    if (how) *how = plan.how;
    return RTX_OK;
}

int32_t rtx_scene_set_visible(RtxSceneHandle h, const uint64_t *indices, uint64_t n, uint32_t visible, void *stream_, uint32_t *how)
{
    if (how) *how = RTX_UPDATED_NOTHING;
    if (!h) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_visible: null scene");
    touch_scene(h);
    std::vector<uint8_t> hidden = hidden_bytes(h, h->objects.size());
    UpdatePlan plan;
    if (int32_t rc = plan_visibility(h->objects, hidden, h->refit, h->sv.sphere_cmax, indices, n, visible, plan)) return rc;
    if (plan.entries.empty()) return RTX_OK;
    RTX_HIP_CHECK(hipSetDevice(h->device));
    if (int32_t rc = check_watchdog(h, true)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (h->hidden.empty()) h->hidden.assign(h->objects.size(), 0);      // (before the tables are made: they read it)
    if (plan.how != RTX_UPDATED_REBUILT) if (int32_t rc = apply_plan(h, plan, stream)) return rc;
    for (const UpdateEntry &e : plan.entries) hidden[e.object] = (e.tri & kEntryHide) ? 1 : 0;
    if (plan.how == RTX_UPDATED_REBUILT) {                      // a shown shape that cannot be taken in place: the pack of the list, then the hide pass
        RTX_HIP_CHECK(hipDeviceSynchronize());                  // a render may still read the arrays about to be replaced
        std::vector<RtxObject> all = h->objects;
        if (int32_t rc = repack_objects(h, all, hidden, stream)) return rc;
    } else h->hidden.swap(hidden);
    if (how) *how = plan.how;
    return RTX_OK;
}

int32_t rtx_scene_get_visible(RtxSceneHandle h, uint8_t *mask)
{
    if (!h || (!mask && !h->objects.empty())) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_get_visible: null argument");
    for (size_t k = 0; k < h->objects.size(); ++k) mask[k] = (k < h->hidden.size() && h->hidden[k]) ? 0 : 1;
    return RTX_OK;
}

}  // extern "C"
