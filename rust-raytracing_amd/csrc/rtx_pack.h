// rtx_pack.h -- what the host decides about a scene without a device (rtx_pack.hip): Scene.objects packed into the arrays the kernels
// read, the tables and the plan of an in-place update (rtx_scene_update_objects), the host reference of the device's update path,
// digests and the invariant walk.  Nothing declared here calls the HIP runtime: rtx_pack.hip links and runs without it
// (tools/host_pack_check.cpp runs it under the sanitizers).
#pragma once

#include "../../include/rtx_hip.h"
#include "rtx_device.h"
#include "rtx_refit.h"

#include <string>
#include <vector>

// What the host translation units call across files lives in rtx::host, hidden: none of it is an export of the library.
#define RTX_HOST_BEGIN namespace rtx { namespace host __attribute__((visibility("hidden"))) {
#define RTX_HOST_END } }

// What rtx_scene_update_objects needs to know about the resident tree, kept on the host from every pack (upload, append, rebuild).
struct RefitTables {
    double scale = -1.0;                                  // the build's largest finite box coordinate ((origin_limit - 1) / 4); < 0: no tree was built
    double abs_pad = 0.0;
    double centre[3] = { 0.0, 0.0, 0.0 };
    bool sphere_tree = false;                             // the spheres are in the tree (bvh_flags bit 0)
    std::vector<uint32_t> local;                          // object index -> index in spheres[] / planes[] / tris[] (the kind: h->objects)
    std::vector<uint32_t> slot;                           // sphere -> its leaf entry (the inverse of bvh.prims); empty without a sphere tree
    std::vector<uint32_t> level_nodes, level_begin;       // the non-flat wide nodes grouped by depth: level d = level_nodes[level_begin[d] .. level_begin[d + 1])
    // the triangle half (RTX_UPDATE_DEFORM): per triangle its class and free axis as pack_scene decided them (classify_triangle) and its
    // record in tri_f32 (tri_fidx inverted; kNoSlot: class "none"; < n_tri_tree: a tree record, the index in tri_geo too)
    std::vector<uint8_t> tri_class, tri_axis;
    std::vector<uint32_t> tri_rec;
    uint32_t n_tri_tree = 0;
    std::vector<uint32_t> all_level_nodes, all_level_begin;   // EVERY wide node by depth, a footprint node with kBvhFlatNode set
};

RTX_HOST_BEGIN

// The calling thread's last error (rtx_last_error), set by fail: one string for every host translation unit.
int32_t fail(RtxStatus st, const std::string &msg);
const std::string &last_error();
bool debug_prints();

// Everything rtx_scene_upload prepares on the host: per-type shape arrays with scene-order ids, the ray-independent
// precompute, the f32 filter records and the BVH.  (pack_scene; rtx_debug_host_scene runs it without a GPU.)
struct PackedScene {
    SceneView sv{};
    std::vector<SphereX> spheres; std::vector<uint32_t> sphere_id;
    std::vector<PlaneX> planes; std::vector<TriX> tris;
    std::vector<MaterialX> mats;
    std::vector<float4> sph32, tri32, leaf32, leaf_cr, tri_geo;
    std::vector<uint32_t> tri_fidx;
    std::vector<uint8_t> tri_rec_free_axis;          // per tree record (leaf order): the axis its footprint is unbounded along
    std::vector<uint8_t> tri_class, tri_axis;        // per triangle: classify_triangle's answer
    BvhBuild bvh;
    Bvh4Build bvh4;
    std::vector<BvhQNode> qnodes;                    // the 64-byte form of bvh4's nodes, when the tree allows it
    std::vector<BvhQ3Node> q3nodes;                  // the 64-byte form of a sphere tree's nodes
};

// The class of a triangle before any demotion, decided in ONE place for pack_scene (which record it gets, whether it may enter the
// tree) and plan_update (whether new vertices can be written in place):
//   kTriNone       no filter record: it can never be hit
//   kTriAlways     a record, tested for every segment: the projection the elimination reads is not usable for a footprint
//   kTriQualified  may enter the tree with its footprint in the plane that leaves out `free_axis`
enum : uint8_t { kTriNone = 0, kTriAlways = 1, kTriQualified = 2 };
struct TriClass { uint8_t cls; uint8_t free_axis; };

TriClass classify_triangle(const TriX &t, const double geom[9], const double centre[3]);
int32_t pack_scene(const RtxScene *scene, PackedScene &p);

RefitTables make_refit_tables(const PackedScene &p);

// An update after validation: the de-duplicated entries (the last entry of an index wins) and the path they take.
struct UpdatePlan {
    std::vector<UpdateEntry> entries;
    uint32_t how = RTX_UPDATED_NOTHING;
    bool any_sphere = false;                              // a sphere's geometry changes: sphere_cmax is taken again
    bool tri_geom = false;                                // a triangle's geometry changes in place (RTX_UPDATE_DEFORM): the triangle tables are needed
    bool tri_refit = false;                               // ... and it has a tree record: every level is refitted, footprint nodes included
    bool any_tri = false;                                 // ... and it is qualified: tri_extent is taken again
    bool visibility = false;                              // rtx_scene_set_visible's plan: mode B needs the kept words
    bool capture = false;                                 // ... and the pack has none yet (the caller sets it): mode E runs first
};

int32_t plan_update(const std::vector<RtxObject> &cur, const RefitTables &t, double cmax, const uint64_t *indices, const RtxObject *objects,
                    uint64_t n, uint32_t mode, UpdatePlan &plan, const uint8_t *hidden = nullptr);
int32_t plan_visibility(const std::vector<RtxObject> &cur, const std::vector<uint8_t> &hidden, const RefitTables &t, double cmax,
                        const uint64_t *indices, uint64_t n, uint32_t visible, UpdatePlan &plan);
void derive_all_spheres(const RtxObject *objects, size_t n_objects, const RefitTables &t, size_t n_spheres, std::vector<float> &box32,
                        std::vector<double> &reach, const uint8_t *hidden = nullptr);
void derive_all_triangles(const RtxObject *objects, size_t n_objects, const RefitTables &t, std::vector<float> &tribox32, std::vector<double> &tri_reach,
                          const uint8_t *hidden = nullptr);
UpdateArgs update_args(const SceneView &where, const RefitTables &t, const UpdateEntry *entries, float *box32, double *reach, float *tribox32,
                       double *tri_reach, bool tri_geom, uint32_t *keep = nullptr);

// The steps of one update in the order they run, written once for the device and for its host reference.  `run` performs one step --
// a launch of scene_update_kernel (rtx_scene_update_objects), or rtx_refit.h's functions in a loop (refit_packed) -- and returns false
// to stop.  Mode A over the entries; under REFIT the levels as mode B, deepest first: a node reads what its children's step wrote (a
// moved triangle of the tree: every level, footprint nodes included -- all_levels; spheres alone: the non-flat levels, as ever);
// mode C when a sphere moved; mode D when a qualified triangle did.  A visibility plan on a pack without kept words (plan.capture)
// starts with mode E over every wide node: the words are read before anything of this update is written.
template <class Run>
bool run_update(UpdateArgs u, const RefitTables &t, const UpdatePlan &plan, const uint32_t *levels, const uint32_t *all_levels,
                uint32_t n_spheres, uint32_t n_tris, Run run)
{
    if (plan.capture) {
        const bool all = !t.all_level_nodes.empty();
        u.mode = 4u; u.n = (uint32_t)(all ? t.all_level_nodes.size() : t.level_nodes.size());
        u.level = all ? all_levels : levels;
        if (!run(u)) return false;
    }
    u.mode = 0u; u.n = (uint32_t)plan.entries.size();
    if (!run(u)) return false;
    if (plan.how == RTX_UPDATED_REFIT) {
        const std::vector<uint32_t> &begin = plan.tri_refit ? t.all_level_begin : t.level_begin;
        const uint32_t *nodes = plan.tri_refit ? all_levels : levels;
        for (size_t d = begin.empty() ? 0 : begin.size() - 1; d-- > 0;) {
            u.mode = 1u; u.n = begin[d + 1] - begin[d];
            u.level = nodes + begin[d];
            if (!run(u)) return false;
        }
    }
    if (plan.any_sphere) { u.mode = 2u; u.n = n_spheres; if (!run(u)) return false; }
    if (plan.any_tri) { u.mode = 3u; u.n = n_tris; if (!run(u)) return false; }
    return true;
}

unsigned long long refit_packed(PackedScene &p, const RefitTables &t, const UpdatePlan &plan, std::vector<float> &box32, std::vector<double> &reach,
                                std::vector<float> &tribox32, std::vector<double> &tri_reach, std::vector<uint32_t> *keep = nullptr);
void digest_packed(const PackedScene &p, uint64_t *digests);
void digest_packed_mesh(const PackedScene &p, uint64_t *digests);
int32_t check_packed(const PackedScene &p, const RtxObject *objects, uint64_t *stats, const uint8_t *hidden = nullptr);
#ifdef RTX_LAB
int32_t host_refit(const char *who, const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                   uint64_t *stats, uint32_t *how, uint64_t *digests, double *info);
// rtx_debug_host_set_visible (include/rtx_hip.h): the kinds of its steps, and the words per child of its dump.
enum : uint32_t { kHostStepHide = 0, kHostStepShow = 1, kHostStepUpdate = 2 /* + RTX_UPDATE_* */, kHostStepAppend = 5 };
constexpr uint32_t kHostDumpWords = 17;
int32_t host_visibility(const char *who, const RtxScene *scene, const uint32_t *step_kind, const uint64_t *step_begin, uint64_t n_steps,
                        const uint64_t *indices, const RtxObject *objects, uint32_t *how, uint64_t *stats, uint64_t *digests, double *info,
                        uint8_t *mask, uint32_t *dump, uint64_t dump_words);
#endif

RTX_HOST_END
