// rtx_query.hip -- query_closest_kernel: closest_object (scene.rs:243-251) for rays the caller brings (rtx_scene_closest_hits)
// or for the zero-offset primary ray of every pixel of a frame (rtx_scene_primary_hits, the pick buffer).
//
// Persistent waves; a wave takes rays from the launch's atomic head in chunks (wf_take) and each lane owns one ray: the
// segment body of a tree kernel -- the origin-range gate, the walk, the exhaustive fallback, planes and
// shapes outside the tree swept for every ray, the (t, scene index) minimum -- on the product's faster steps:
//   TRIS = false  a sphere tree: the 64-byte nodes, node and leaf visits apart (sphere_walk_phased), candidates queued with
//                 their f32 lower bound, the exact tests after the walk;
//   TRIS = true   a tree that holds triangles (a pure footprint tree with its 64-byte nodes, or a joint tree): mesh_step with
//                 tri_bounds, the queue flushed into the exact tests whenever it fills.
// The walk does not know which surface the ray starts on: no self-hit pre-test (the render's mesh kernel has one; here the
// triangle a ray sits on is found like any other, its t_lo bound is ~0 and it always reaches the exact test).
//
// Exactness ("Ray queries").  The f32 code only selects candidates; every reported hit is the f64 test in the
// reference's operation order.  The f32 bounds were derived for unit directions, so a ray takes the walk only when
// |d.d - 1| <= kQueryDirTol and d is finite; anything else (a non-unit or non-finite direction, an origin beyond
// bvh_origin_limit * kBvhRange64, a NaN origin, RTX_KERNEL_EXACT, a scene without a usable tree, a stack or candidate
// overflow) tests every shape exactly -- every triangle, not just the ones with a filter record, since upload drops the
// triangles the cull test rejects for every UNIT direction.
//
// The any-hit mode (QueryArgs.mode, rtx_scene_any_hits; DESIGN.md "Occlusion queries"): occluded[i] = some object's distance is
// normal, positive and < t_max[i] -- closest_object's distance < t_max[i], without the search for the nearest.  A launch-uniform
// switch of the same two instances, taken once per launch (the mode has its own ray loop: the closest-hit loop carries none of its
// arguments -- with the branch inside the shared loop the closest-hit rates fell by 0.5-2 %): the limit seeds best_up, so the walk
// prunes what starts behind it; planes and the shapes outside the tree are tested BEFORE the walk; and a lane retires -- drops its stack and
// its queued candidates -- as soon as a hit before the limit is certain: best_up, which only certain hits lower (the sphere
// leaves' t_lo > K bound, tri_bounds' upper bound), has fallen below t_max, or an exact test said so.
//
// The path mode (QueryArgs.mode, rtx_scene_trace_paths; DESIGN.md "Path queries"): render_ray for the caller's rays -- the third
// launch-uniform loop of the same two instances.  A lane owns a path and is refilled at the segment boundary; a segment is the
// closest-hit loop's body (query_closest_ray) followed by advance_and_shade, with the render's draws 6 + 2b, 7 + 2b for bounce b.
// Its sample form (QueryArgs.rays == null, rtx_scene_trace_samples; DESIGN.md "Progressive and adaptive sampling"): the lane builds
// render_pixel's own ray for its (pixel, sample) pair with gen_primary on the full frame's RowsView where the path mode reads the
// caller's ray -- a launch-uniform choice at the take, everything after it unchanged.
//
// The refine mode (QueryArgs.mode, rtx_render_blocks_refine; DESIGN.md "Refinement to a threshold"): adaptive sampling decided on the
// device -- the fifth launch-uniform loop of the same two instances.  A lane owns a PIXEL of the band while the noise rule selects it:
// the rule is evaluated on the pixel's running sums at the take, each path is the sample form's, and its colour is folded into the
// sums in memory at the path's end (query_refine_loop).
//
// The feature mode (QueryArgs.mode, rtx_scene_pixel_features; DESIGN.md "Pixel features"): the denoiser's guide buffers -- the fourth
// launch-uniform loop of the same two instances.  A lane owns a PIXEL of the band: for every sample it builds render_pixel's own
// lens-jittered ray (gen_primary), asks query_closest_ray, and adds the winner's colours, normal and distance to the sums, which live in
// the pixel's output record, not in registers.
//
// The multi-hit mode (QueryArgs.mode, rtx_scene_multi_hits / rtx_scene_primary_multi_hits; DESIGN.md "Multi-hit queries"): the k nearest
// objects along each ray, sorted -- the sixth launch-uniform loop of the same two instances.  The lane's sorted list lives in the
// ray's own k output records; the walks prune against the list's k-th distance and their leaf code never lowers that bound itself.
#include "rtx_launch.h"
#include "rtx_mesh_step.h"
#include "rtx_wavefront.h"

namespace rtx {

constexpr int kQueryWaves = 4;                                   // workgroups per CU (4 waves each)
constexpr int kQuerySphStack = 30;                               // LDS stack rows: (30 + 1 sink + 2 * kSphQueue) KB per workgroup
constexpr int kQueryMeshStack = 38 - 2 * kMeshQueue;             // (26 + 1 sink + 2 * kMeshQueue) KB per workgroup
constexpr uint32_t kQueryLeafLanes = 8;                          // sphere_walk_phased: a leaf visit runs for this many lanes
// |d.d - 1| at most this: 2^-40.  A normalised f64 vector is within a few 2^-53 of unit length; the f32 bounds budget their
// errors in units of u = 2^-24 with at least a factor 2 to spare, and converting d to f32 alone moves it by u.
constexpr double kQueryDirTol = 9.094947017729282e-13;

__device__ __forceinline__ bool query_dir_ok(V3 d)
{
    const double n2 = d.x * d.x + d.y * d.y + d.z * d.z;
    return fabs(n2 - 1.0) <= kQueryDirTol;                        // (NaN / inf components: false)
}

// the sphere leaves' ray for a tree that may hold none: idle (no sphere record passes) unless the tree has sphere leaves
__device__ __forceinline__ void query_sphere_ray(const SceneView &sv, V3 pos, V3 dir, SphereRay &sr)
{
    sr.px = sr.py = sr.pz = sr.dx = sr.dy = sr.dz = sr.Kg = sr.K = 0.f; sr.c0 = __builtin_inff();
    if (sv.bvh_flags & 1u) sphere_ray_from(sv, pos, dir, sr);
}

// every shape exactly (spheres, planes, then every triangle -- Scene.objects order decides ties through hit_consider)
__device__ __forceinline__ void query_sweep(const SceneView &sv, const LeafArrays &la, const RayX &rx, bool spheres, bool tris, Hit &h,
                                            unsigned long long &exact)
{
    if (spheres) {
        for (uint32_t k = 0; k < sv.n_spheres; ++k) {
            double t;
            if (sphere_distance(la.spheres[k], rx, &t)) hit_consider(h, t, la.sphere_ids[k], 0, k);
        }
        exact += sv.n_spheres;
    }
    for (uint32_t k = 0; k < sv.n_planes; ++k) {
        double t;
        if (plane_distance(sv.planes[k], rx, &t)) hit_consider(h, t, sv.planes[k].id, 1, k);
    }
    exact += sv.n_planes;
    if (tris) {
        for (uint32_t k = 0; k < sv.n_tris; ++k) {
            double t;
            if (triangle_distance(la.tris[k], rx, &t)) hit_consider(h, t, la.tris[k].id, 2, k);
        }
        exact += sv.n_tris;
    }
}

// the exact tests of the queued candidates that can still win
__device__ __forceinline__ void query_flush(const LeafArrays &la, const RayX &rx, const uint32_t *lq, uint32_t tid, uint32_t queue,
                                            uint32_t qcnt, float best_up, Hit &h, unsigned long long &exact)
{
#pragma unroll 1
    for (uint32_t e = 0; e < qcnt; ++e) {
        if (__uint_as_float(lq[(size_t)(queue + e) * kBvhThreads + tid]) <= best_up) {
            const uint32_t idx = lq[(size_t)e * kBvhThreads + tid];
            double t;
            if (idx & kQueueTri) {
                const uint32_t tk = la.tri_fidx[idx & ~kQueueTri];
                if (triangle_distance(la.tris[tk], rx, &t)) hit_consider(h, t, la.tris[tk].id, 2, tk);
            } else {
                if (sphere_distance(la.spheres[idx], rx, &t)) hit_consider(h, t, la.sphere_ids[idx], 0, idx);
            }
            exact += 1;
        }
    }
}

// one walk of a tree that holds triangles (PLAIN 2: 64-byte footprint nodes; 0: joint nodes), flushing whenever the queue is full
template <int PLAIN, class RAY>
__device__ __forceinline__ void query_mesh_walk(const float4 *__restrict__ nodes, const LeafArrays &la, const MeshArrays &ma, const RAY &q,
                                                const SphereRay &sr, const TriFilterParams &tpar, const RayX &rx, uint32_t root, bool &overflow,
                                                Hit &h, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long &exact,
                                                uint32_t &nbox, uint32_t &nleaf)
{
    float best_up = __builtin_inff();
    uint32_t node = root, sp = 0, qcnt = 0, resume = 0, resume_node = 0;
    float4 nd[MeshNode<PLAIN>::n];
    if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, node, nd);
    while (node != kNone || resume != 0u) {
        if (mesh_step<true, PLAIN, kQueryMeshStack>(nodes, ma, q, sr, tpar, nd, node, sp, qcnt, overflow, best_up, resume, resume_node, ls, lq,
                                                     tid, spill, spill_entries, spill_stride, glane, nbox, nleaf))
            continue;
        query_flush(la, rx, lq, tid, kMeshQueue, qcnt, best_up, h, exact);
        qcnt = 0;
        if (h.id != kNone) best_up = fminf(best_up, round_up32(h.t));
        if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, resume_node, nd);
    }
    query_flush(la, rx, lq, tid, kMeshQueue, qcnt, best_up, h, exact);
}

// ---- the any-hit mode ---------------------------------------------------------------------------------------------------------
// closest_object's filter (scene.rs:249) and the caller's limit, strict
__device__ __forceinline__ bool query_before(double t, double t_max) { return is_normal_positive(t) && t < t_max; }

// query_sweep, stopping at the first hit before the limit (planes first: one of them often settles the ray)
__device__ __forceinline__ bool query_sweep_any(const SceneView &sv, const LeafArrays &la, const RayX &rx, bool spheres, bool tris, double t_max,
                                                unsigned long long &exact)
{
    double t;
    for (uint32_t k = 0; k < sv.n_planes; ++k) {
        exact += 1;
        if (plane_distance(sv.planes[k], rx, &t) && query_before(t, t_max)) return true;
    }
    if (spheres) {
        for (uint32_t k = 0; k < sv.n_spheres; ++k) {
            exact += 1;
            if (sphere_distance(la.spheres[k], rx, &t) && query_before(t, t_max)) return true;
        }
    }
    if (tris) {
        for (uint32_t k = 0; k < sv.n_tris; ++k) {
            exact += 1;
            if (triangle_distance(la.tris[k], rx, &t) && query_before(t, t_max)) return true;
        }
    }
    return false;
}

// query_flush, stopping at the first hit before the limit
__device__ __forceinline__ bool query_flush_any(const LeafArrays &la, const RayX &rx, const uint32_t *lq, uint32_t tid, uint32_t queue,
                                                uint32_t qcnt, float best_up, double t_max, unsigned long long &exact)
{
#pragma unroll 1
    for (uint32_t e = 0; e < qcnt; ++e) {
        if (__uint_as_float(lq[(size_t)(queue + e) * kBvhThreads + tid]) <= best_up) {
            const uint32_t idx = lq[(size_t)e * kBvhThreads + tid];
            double t;
            bool hit;
            if (idx & kQueueTri) hit = triangle_distance(la.tris[la.tri_fidx[idx & ~kQueueTri]], rx, &t);
            else hit = sphere_distance(la.spheres[idx], rx, &t);
            exact += 1;
            if (hit && query_before(t, t_max)) return true;
        }
    }
    return false;
}

// query_mesh_walk's loop with best_up seeded by the limit; the lane leaves it -- its stack, the leaf children still to be read and
// its queue dropped -- once a hit before the limit is certain.  Returns whether one is.
template <int PLAIN, class RAY>
__device__ __forceinline__ bool query_mesh_walk_any(const float4 *__restrict__ nodes, const LeafArrays &la, const MeshArrays &ma, const RAY &q,
                                                    const SphereRay &sr, const TriFilterParams &tpar, const RayX &rx, uint32_t root, float best_up,
                                                    double t_max, bool &overflow, uint32_t *ls, uint32_t *lq, uint32_t tid,
                                                    uint32_t *__restrict__ spill, uint32_t spill_entries, size_t spill_stride, size_t glane,
                                                    unsigned long long &exact, uint32_t &nbox, uint32_t &nleaf)
{
    uint32_t node = root, sp = 0, qcnt = 0, resume = 0, resume_node = 0;
    float4 nd[MeshNode<PLAIN>::n];
    if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, node, nd);
    while (node != kNone || resume != 0u) {
        const bool go = mesh_step<true, PLAIN, kQueryMeshStack>(nodes, ma, q, sr, tpar, nd, node, sp, qcnt, overflow, best_up, resume, resume_node,
                                                                ls, lq, tid, spill, spill_entries, spill_stride, glane, nbox, nleaf);
        if ((double)best_up < t_max) return true;                     // a certain hit's upper bound lies before the limit
        if (go) continue;
        if (query_flush_any(la, rx, lq, tid, kMeshQueue, qcnt, best_up, t_max, exact)) return true;
        qcnt = 0;
        if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, resume_node, nd);
    }
    return query_flush_any(la, rx, lq, tid, kMeshQueue, qcnt, best_up, t_max, exact);
}

// One ray of the any-hit mode, t_max > 0 (the caller's gate): 1 when some object's distance is normal, positive and < t_max.
template <bool TRIS>
__device__ __forceinline__ uint32_t query_any_ray(const SceneView &sv, const float4 *__restrict__ nodes, const LeafArrays &la, const MeshArrays &ma,
                                                  V3 pos, V3 dir, const RayX &rx, bool walk, bool in32, double t_max, uint32_t *ls, uint32_t *lq,
                                                  uint32_t tid, uint32_t *__restrict__ spill, uint32_t spill_entries, size_t spill_stride,
                                                  size_t glane, unsigned long long &exact, unsigned long long &box_tests,
                                                  unsigned long long &leaf_filters)
{
    if (!walk) return query_sweep_any(sv, la, rx, true, true, t_max, exact) ? 1u : 0u;
    // the shapes the tree does not answer for, before the walk: every plane, the spheres and the triangle records outside it
    if (query_sweep_any(sv, la, rx, (sv.bvh_flags & 1u) == 0u, false, t_max, exact)) return 1u;
    for (uint32_t k = (sv.bvh_flags & 2u) ? sv.n_tri_tree : 0u; k < sv.n_tri_filter; ++k) {
        double t;
        exact += 1;
        if (triangle_distance(la.tris[la.tri_fidx[k]], rx, &t) && query_before(t, t_max)) return 1u;
    }
    // the walk prunes with the limit from its first box on: t_lo <= best_up keeps every hit with t < t_max <= best_up
    const float best0 = fmaxf(round_up32(t_max), 1.17549435e-38f);      // (+inf when t_max is; never a denormal a compare may flush)
    bool overflow = false, occ = false;
    uint32_t nbox = 0, nleaf = 0;
    if constexpr (TRIS) {
        SphereRay sr;
        query_sphere_ray(sv, pos, dir, sr);
        TriFilterParams tpar;
        tri_filter_from_ray(sv, pos, dir, tpar);
        const bool plain = (sv.bvh_flags & 4u) != 0u;
        if (in32) {
            Ray32 q;
            make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q);
            if (plain) occ = query_mesh_walk_any<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, best0, t_max, overflow, ls, lq, tid, spill,
                                                    spill_entries, spill_stride, glane, exact, nbox, nleaf);
            else occ = query_mesh_walk_any<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, best0, t_max, overflow, ls, lq, tid, spill,
                                              spill_entries, spill_stride, glane, exact, nbox, nleaf);
        } else {
            Ray64 q;
            make_ray64(pos, rx.dirn, (double)sv.bvh_inv_max, q);
            if (plain) occ = query_mesh_walk_any<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, best0, t_max, overflow, ls, lq, tid, spill,
                                                    spill_entries, spill_stride, glane, exact, nbox, nleaf);
            else occ = query_mesh_walk_any<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, best0, t_max, overflow, ls, lq, tid, spill,
                                              spill_entries, spill_stride, glane, exact, nbox, nleaf);
        }
    } else {
        SphereRay sr;
        sphere_ray_from(sv, pos, dir, sr);
        Ray32 q0;
        make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q0);
        Ray32S q;
        q.ix = q0.ix; q.iy = q0.iy; q.iz = q0.iz; q.nx = q0.nx; q.ny = q0.ny; q.nz = q0.nz;
        q.e = ray32_slack(q0, in32);
        float best_up = best0;
        uint32_t node = sv.bvh_root, sp = 0, qcnt = 0;
        // sphere_walk_phased's iteration -- node visits and leaf visits apart, chosen for the wave -- with the retirement check after
        // a leaf visit, the only place best_up falls
        while (node != kNone) {
            const bool at_leaf = (node >> 29) != 0u;
            const unsigned long long lm = __ballot(at_leaf), am = __ballot(true);
            if ((uint32_t)__popcll(lm) >= kQueryLeafLanes || lm == am) {
                if (at_leaf) {
                    sphere_leaf_step<kQuerySphStack, true>(la.sphere_f32, la.sphere_prims, sr, node, sp, ls, lq, tid, spill, spill_stride, glane,
                                                           best_up, qcnt, overflow, nleaf);
                    if ((double)best_up < t_max) { occ = true; node = kNone; sp = 0; qcnt = 0; }
                }
            } else if (!at_leaf) {
                sphere_node_step_q3<kQuerySphStack, true>(nodes, q, node, sp, ls, tid, spill, spill_entries, spill_stride, glane, best_up,
                                                          overflow, nbox);
            }
        }
        if (!occ && !overflow) occ = query_flush_any(la, rx, lq, tid, kSphQueue, qcnt, best_up, t_max, exact);
    }
    box_tests += nbox;
    leaf_filters += nleaf;
    // a walk cut short by a full stack or queue, no certain hit seen: every shape exactly (a certain hit stays one whatever overflowed)
    if (!occ && overflow) occ = query_sweep_any(sv, la, rx, true, true, t_max, exact);
    return occ ? 1u : 0u;
}

// whether the ray may take the walk (its f32 bounds hold for it) and which slab test it gets: the gate of query_closest_ray (the
// closest-hit and the path loop) and of the any-hit loop
__device__ __forceinline__ bool query_walkable(const SceneView &sv, uint32_t tree, V3 pos, V3 dir, bool &in32)
{
    const float omax = fmaxf(fmaxf(__builtin_fabsf((float)pos.x), __builtin_fabsf((float)pos.y)), __builtin_fabsf((float)pos.z));
    // (fmaxf drops a NaN operand: a NaN coordinate is asked for by name.  Such a ray has no reportable hit either way -- every distance is
    // NaN -- but it does not belong in the walk: tests/test_walk_bounds.py.  The frame kernels' gates (rtx_bvh_spheres.hip, rtx_bvh_mesh.hip,
    // rtx_wavefront.hip and the lab kernels) restate the fmaxf form and are left as they are: same results, and no hook looks at them)
    const bool numbers = (pos.x == pos.x) & (pos.y == pos.y) & (pos.z == pos.z);
    in32 = numbers && omax <= sv.bvh_origin_limit;                                      // NaN origin -> exhaustive branch
    return tree && numbers && query_dir_ok(dir) && (in32 || omax <= sv.bvh_origin_limit * kBvhRange64);
}

// One closest_object call (scene.rs:243-251) for the ray (pos, dir): the origin-range gate, the walk, the flush, planes and the
// shapes outside the tree, or the sweep of every shape -- the segment body of the closest-hit loop and of the path loop.
template <bool TRIS>
__device__ __forceinline__ void query_closest_ray(const SceneView &sv, uint32_t tree, const float4 *__restrict__ nodes, const LeafArrays &la,
                                                  const MeshArrays &ma, V3 pos, V3 dir, const RayX &rx, Hit &h, uint32_t *ls, uint32_t *lq,
                                                  uint32_t tid, uint32_t *__restrict__ spill, uint32_t spill_entries, size_t spill_stride,
                                                  size_t glane, unsigned long long &exact, unsigned long long &box_tests,
                                                  unsigned long long &leaf_filters)
{
    hit_init(h);
    bool in32;
    const bool walk = query_walkable(sv, tree, pos, dir, in32);
    bool covered = false;
    if (walk) {
        bool overflow = false;
        uint32_t nbox = 0, nleaf = 0;
        if constexpr (TRIS) {
            SphereRay sr;
            query_sphere_ray(sv, pos, dir, sr);
            TriFilterParams tpar;
            tri_filter_from_ray(sv, pos, dir, tpar);
            const bool plain = (sv.bvh_flags & 4u) != 0u;
            if (in32) {
                Ray32 q;
                make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q);
                if (plain) query_mesh_walk<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, overflow, h, ls, lq, tid, spill, spill_entries,
                                              spill_stride, glane, exact, nbox, nleaf);
                else query_mesh_walk<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, overflow, h, ls, lq, tid, spill, spill_entries,
                                        spill_stride, glane, exact, nbox, nleaf);
            } else {                                  // origin far outside the scene: the same walk with an f64 slab test
                Ray64 q;
                make_ray64(pos, rx.dirn, (double)sv.bvh_inv_max, q);
                if (plain) query_mesh_walk<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, overflow, h, ls, lq, tid, spill, spill_entries,
                                              spill_stride, glane, exact, nbox, nleaf);
                else query_mesh_walk<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, overflow, h, ls, lq, tid, spill, spill_entries,
                                        spill_stride, glane, exact, nbox, nleaf);
            }
        } else {
            SphereRay sr;
            sphere_ray_from(sv, pos, dir, sr);
            Ray32 q0;
            make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q0);
            Ray32S q;                                 // (a far origin: Ray32's planes widened by the slack of noi's rounding)
            q.ix = q0.ix; q.iy = q0.iy; q.iz = q0.iz; q.nx = q0.nx; q.ny = q0.ny; q.nz = q0.nz;
            q.e = ray32_slack(q0, in32);
            float best_up = __builtin_inff();
            uint32_t node = sv.bvh_root, sp = 0, qcnt = 0;
#if defined(RTX_LAB) && defined(RTX_SPH_PROFILE)      // the lab profile builds count in stage 2 of the renders only: the walk's count goes nowhere here
            unsigned long long rtx_prof = 0;
#define RTX_QUERY_PROF_PASS , rtx_prof
#else
#define RTX_QUERY_PROF_PASS
#endif
            sphere_walk_phased<kQuerySphStack, true>(nodes, la.sphere_f32, la.sphere_prims, q, sr, node, sp, ls, lq, tid, spill,
                                                     spill_entries, spill_stride, glane, best_up, qcnt, overflow, nbox, nleaf,
                                                     0u, 0u, 0u, kQueryLeafLanes RTX_QUERY_PROF_PASS);
#undef RTX_QUERY_PROF_PASS
            if (!overflow) query_flush(la, rx, lq, tid, kSphQueue, qcnt, best_up, h, exact);
        }
        box_tests += nbox;
        leaf_filters += nleaf;
        covered = !overflow;
    }
    if (covered) {
        // the tree answered for its shapes: the spheres outside it, every plane, the triangle records outside it
        query_sweep(sv, la, rx, (sv.bvh_flags & 1u) == 0u, false, h, exact);
        const uint32_t from = (sv.bvh_flags & 2u) ? sv.n_tri_tree : 0u;
        for (uint32_t k = from; k < sv.n_tri_filter; ++k) {
            const uint32_t tk = la.tri_fidx[k];
            double t;
            if (triangle_distance(la.tris[tk], rx, &t)) hit_consider(h, t, la.tris[tk].id, 2, tk);
        }
        exact += sv.n_tri_filter - from;
    } else {
        hit_init(h);                                  // (a walk cut short: start over, every shape exactly)
        query_sweep(sv, la, rx, true, true, h, exact);
    }
}

// The kernel's ray loop in the any-hit mode: the same persistent waves and chunks, one byte per ray.  A loop of its own, entered
// once per launch, so that the closest-hit loop carries none of this mode's arguments or state.
template <bool TRIS>
__device__ __forceinline__ void query_any_loop(const SceneView &sv, const QueryArgs &qa, const float4 *__restrict__ nodes, const LeafArrays &la,
                                               const MeshArrays &ma, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                               uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long *__restrict__ head,
                                               unsigned long long &segs, unsigned long long &exact, unsigned long long &box_tests,
                                               unsigned long long &leaf_filters)
{
    const unsigned long long grab = wf_grab_size(qa.n);
    WfChunk ch{0ull, 0ull, false};
    for (;;) {
        unsigned long long i = 0;
        const bool mine = wf_take(ch, head, grab, qa.n, true, i);
        if (ch.drained && __ballot(mine) == 0ull) break;
        if (!mine) continue;
        ++segs;
        const double t_max = qa.t_max ? qa.t_max[i] : __builtin_inf();
        uint32_t occ = 0;
        if (t_max > 0.0) {                                               // (NaN, zero, negative: never occluded, nothing is tested)
            const QueryRay &qr = qa.rays[i];
            const V3 pos = mk(qr.position[0], qr.position[1], qr.position[2]);
            const V3 dir = mk(qr.direction[0], qr.direction[1], qr.direction[2]);
            const RayX rx = make_rayx(pos, dir);
            bool in32;
            const bool walk = query_walkable(sv, qa.walk, pos, dir, in32);
            occ = query_any_ray<TRIS>(sv, nodes, la, ma, pos, dir, rx, walk, in32, t_max, ls, lq, tid, spill, spill_entries, spill_stride,
                                      glane, exact, box_tests, leaf_filters);
        }
        qa.occluded[i] = (uint8_t)occ;
    }
}

// ---- the path mode -------------------------------------------------------------------------------------------------------------
// render_ray (scene.rs:223-242) for the caller's rays: a lane owns one PATH, a variable number of segments, and is refilled at the
// segment boundary -- at the top of every iteration each lane without a path takes the next ray of the wave's chunk (wf_take compacts
// the takers by ballot), so no lane waits for the wave's longest path.  One iteration is one closest_object call (query_closest_ray)
// and advance_and_shade, or the end of the path: a miss, max_bounces + 1 segments, or light_color == 0 (scene.rs:227-231).  A loop of
// its own, entered once per launch: the closest-hit and any-hit loops carry none of its arguments or state.
template <bool TRIS>
__device__ __forceinline__ void query_path_loop(const SceneView &sv, const QueryArgs &qa, const float4 *__restrict__ nodes, const LeafArrays &la,
                                                const MeshArrays &ma, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long *__restrict__ head,
                                                unsigned long long &segs, unsigned long long &exact, unsigned long long &box_tests,
                                                unsigned long long &leaf_filters)
{
    const unsigned long long grab = wf_grab_size(qa.n);
    const uint32_t bounce_limit = sv.max_bounces >= 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)sv.max_bounces + 1u;     // scene.rs:227
    WfChunk ch{0ull, 0ull, false};
    RayState r;
    uint32_t idx = 0;                                                    // the path's entry (n < 2^32)
    bool have = false;
    r.pos = r.dir = r.result = r.light = mk(0.0, 0.0, 0.0);
    r.key = 0; r.draw = 6; r.bounce = 0;
    for (;;) {
        unsigned long long i = 0;
        bool got = wf_take(ch, head, grab, qa.n, !have, i);
        if (!ch.drained && __ballot(!have && !got) != 0ull) {            // the chunk ran out under the takers: the next one, now
            unsigned long long i2 = 0;
            if (wf_take(ch, head, grab, qa.n, !have && !got, i2)) { got = true; i = i2; }
        }
        if (got && qa.rays == nullptr) {                                 // launch-uniform: the sample form -- render_pixel's own ray
            const unsigned long long pix = qa.ids[2 * i], smp = qa.ids[2 * i + 1];
            if (pix < (unsigned long long)qa.rv->npix && smp <= 0xFFFFFFFFull) {          // (before any table is indexed)
                gen_primary(sv, *qa.rv, (uint32_t)pix, (uint32_t)smp, r);                // key (seed, pix, smp), draws 0..5; r.draw = 6
                idx = (uint32_t)i;
                have = true;
            } else {                                                     // no such pixel or sample: NaN, nothing is traced
                const double nan = __builtin_nan("");
                double *out = qa.rgb + 3ull * i;
                out[0] = nan; out[1] = nan; out[2] = nan;
                if (qa.segments) qa.segments[i] = 0u;
            }
        } else if (got) {
            const QueryRay &qr = qa.rays[i];
            r.pos = mk(qr.position[0], qr.position[1], qr.position[2]);                      // Ray::new (ray.rs:14-21): no norm()
            r.dir = mk(qr.direction[0], qr.direction[1], qr.direction[2]);
            r.result = mk(0.0, 0.0, 0.0);
            r.light = mk(1.0, 1.0, 1.0);
            r.key = qa.ids ? rng_key(sv.seed, qa.ids[2 * i], qa.ids[2 * i + 1]) : rng_key(sv.seed, i, 0ull);
            r.draw = 6;                                                  // (draws 0..5 are the lens jitter's: a render's sample continues here)
            r.bounce = 0;
            idx = (uint32_t)i;
            have = true;
        }
        if (ch.drained && __ballot(have) == 0ull) break;                 // wave-uniform
        if (!have) continue;
        const RayX rx = make_rayx(r.pos, r.dir);
        Hit h;
        ++segs;
        query_closest_ray<TRIS>(sv, qa.walk, nodes, la, ma, r.pos, r.dir, rx, h, ls, lq, tid, spill, spill_entries, spill_stride, glane, exact,
                                box_tests, leaf_filters);
        uint32_t nseg = r.bounce + 1u;                                   // closest_object calls so far
        bool done = true;                                                // scene.rs:232: None ends the path
        if (h.id != kNone) {
            advance_and_shade(sv, h, r);
            done = (r.bounce >= bounce_limit) || light_is_zero(r);       // scene.rs:227-228
        }
        if (done) {
            double *out = qa.rgb + 3ull * idx;
            out[0] = r.result.x; out[1] = r.result.y; out[2] = r.result.z;
            if (qa.segments) qa.segments[idx] = nseg;
            have = false;
        }
    }
}

// ---- the feature mode ----------------------------------------------------------------------------------------------------------
// Per pixel of the band, over the S = rays_per_pixel rays render_pixel builds for it (scene.rs:196-207: gen_primary with the sample
// index s, so the RNG key and the draws 0..5 are the render's): the sums of the first hits' base_color, emission_color, normal_at and
// distance, left folds from +0.0 in sample order (a miss adds nothing), then sum / S -- the render's fold (iter_ops.rs:4-8) -- the
// distance over the samples that hit, hits / S, and sample 0's winner.  A lane owns a pixel, entry i of the launch = local pixel i of
// the band, row-major like the pick form (a wave's 64 lanes are a 64 x 1 strip of one sample at a time, as the rows of a caller's
// primary rays are in the path mode; the 8x8 tiles of ray_index_to_pixel_tiled were not measured against it).  Every lane runs the
// same S samples, so no lane is refilled inside a pixel.  The ten f64 sums are parked in the pixel's own output record -- the lane
// owns it -- and read, added to and written back after each sample that hit: held across the walk they would be 20 VGPRs more than
// the 128 this kernel may have.  Only the hit count stays in a register.  A loop of its own, entered once per launch: the other
// loops carry none of its arguments or state.
template <bool TRIS>
__device__ __forceinline__ void query_feature_loop(const SceneView &sv, const QueryArgs &qa, const float4 *__restrict__ nodes, const LeafArrays &la,
                                                   const MeshArrays &ma, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                   uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long *__restrict__ head,
                                                   unsigned long long &segs, unsigned long long &exact, unsigned long long &box_tests,
                                                   unsigned long long &leaf_filters)
{
    const unsigned long long grab = wf_grab_size(qa.n);
    const uint32_t n_samples = (uint32_t)sv.rays_per_pixel;             // (the host refuses 2^32 and more)
    const RowsView &rv = *qa.rv;
    WfChunk ch{0ull, 0ull, false};
    for (;;) {
        unsigned long long i = 0;
        const bool mine = wf_take(ch, head, grab, qa.n, true, i);
        if (ch.drained && __ballot(mine) == 0ull) break;
        if (!mine) continue;
        QueryFeatures *const out = qa.features + i;
        for (int c = 0; c < 3; ++c) out->albedo[c] = out->emission[c] = out->normal[c] = 0.0;
        out->depth = 0.0;
        out->object = -1;
        uint32_t hits = 0;
        for (uint32_t s = 0; s < n_samples; ++s) {
            RayState r;
            gen_primary(sv, rv, (uint32_t)i, s, r);
            const RayX rx = make_rayx(r.pos, r.dir);
            Hit h;
            ++segs;
            query_closest_ray<TRIS>(sv, qa.walk, nodes, la, ma, r.pos, r.dir, rx, h, ls, lq, tid, spill, spill_entries, spill_stride, glane, exact,
                                    box_tests, leaf_filters);
            if (h.id != kNone) {
                const MaterialX m = sv.materials[h.id];
                const V3 nrm = normal_at(sv, h, vadd(r.pos, vmuls(r.dir, h.t)));             // scene.rs:234, object.rs:37-39
                out->albedo[0] += m.base_color.x; out->albedo[1] += m.base_color.y; out->albedo[2] += m.base_color.z;
                out->emission[0] += m.emission_color.x; out->emission[1] += m.emission_color.y; out->emission[2] += m.emission_color.z;
                out->normal[0] += nrm.x; out->normal[1] += nrm.y; out->normal[2] += nrm.z;
                out->depth += h.t;
                if (s == 0u) out->object = (long long)h.id;
                ++hits;
            }
            __asm__ volatile("" ::: "memory");                           // the sums stay in the record: no promotion to registers across the walk
        }
        const double ds = (double)n_samples;                             // sum / len (iter_ops.rs:4-8): a division; 0 / 0 = NaN when S == 0
        for (int c = 0; c < 3; ++c) {
            out->albedo[c] = out->albedo[c] / ds;
            out->emission[c] = out->emission[c] / ds;
            out->normal[c] = out->normal[c] / ds;
        }
        out->depth = hits != 0u ? out->depth / (double)hits : __builtin_inf();
        out->coverage = (double)hits / ds;
    }
}

// ---- the refine mode -----------------------------------------------------------------------------------------------------------
// The rule of rtx_render_blocks_refine for a pixel with n samples, sums s and sums of squares q: every operation one rounded f64
// operation in the header's order (-ffp-contract=off), every comparison with a NaN false.
__device__ __forceinline__ bool refine_selected(const QueryRefineRule &rule, uint32_t n, double s0, double s1, double s2, double q0, double q1,
                                                double q2)
{
    if (n >= rule.max_samples) return false;
    if (n < 2u) return true;
    const double dn = (double)n;
    const double v0 = q0 - s0 * s0 / dn, v1 = q1 - s1 * s1 / dn, v2 = q2 - s2 * s2 / dn;
    const double e = ((v0 + v1) + v2) / (dn - 1.0) / dn;                 // the summed per-channel variance of the mean
    const double m = ((s0 + s1) + s2) / dn;
    const double b = rule.threshold * (m + rule.floor);
    return e > b * b;
}

// Entry i is local pixel i of the band (qa.rv is the band's RowsView, as the feature mode's).  The lane that takes it reads the pixel's
// count and sums, evaluates the rule and either starts the pixel's next sample or stays free -- and the wave keeps taking until no lane
// is free or the queue is dry, BEFORE the walk: an iteration costs the other lanes a whole segment walk, and most entries are not
// selected.  From there the loop is the path loop's: one closest_object call and advance_and_shade per iteration.  A lane owns its
// pixel until the rule, the cap or the rounds stop it: at a path's end the colour is added to the pixel's sums in memory (plain adds;
// the square is rounded before its add), and the lane either goes on with the next sample of the round or evaluates the rule at the
// round's end.  What a lane carries across the walk is k, the samples it has traced for its pixel in this call: the sample index is
// sample_begin + extra[pixel] + k (extra[pixel] is written when the lane lets go of the pixel), the round is k / n_more; the draw index
// is derived from the bounce count.  The three counts of the call are wave-uniform: the lanes' events of an iteration are flags,
// counted by ballot at the top of the next one, and added to the words behind the queue's head once per wave.  The rule is read from
// device memory behind those words, so the kernel's arguments -- which every loop of the kernel holds in registers -- are the other
// modes'.  A loop of its own, entered once per launch: with the take and the fold inside query_path_loop, the path legs of the joint
// scene ran 23 % slower.
template <bool TRIS>
__device__ __forceinline__ void query_refine_loop(const SceneView &sv, const QueryArgs &qa, const float4 *__restrict__ nodes, const LeafArrays &la,
                                                  const MeshArrays &ma, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                  uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long *__restrict__ head,
                                                  unsigned long long &segs, unsigned long long &exact, unsigned long long &box_tests,
                                                  unsigned long long &leaf_filters)
{
    const unsigned long long grab = wf_grab_size(qa.n);
    const uint32_t bounce_limit = sv.max_bounces >= 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)sv.max_bounces + 1u;     // scene.rs:227
    const QueryRefineRule rule = *reinterpret_cast<const QueryRefineRule *>(head + kQueryRefineRule);
    const RowsView &rv = *qa.rv;
    WfChunk ch{0ull, 0ull, false};
    RayState r;
    uint32_t idx = 0;                                                    // the lane's pixel (n < 2^32)
    uint32_t k = 0;                                                      // the samples traced for it in this call
    bool have = false, fresh = false, ev_sample = false, ev_still = false;   // a sample to start; this iteration's events
    uint32_t n_pixels = 0, n_samples = 0, n_still = 0;                   // the wave's counts (wave-uniform; pixels <= n < 2^32)
    r.pos = r.dir = r.result = r.light = mk(0.0, 0.0, 0.0);
    r.key = 0; r.draw = 6; r.bounce = 0;
    for (;;) {
        n_samples += (uint32_t)__popcll(__ballot(ev_sample));
        n_still += (uint32_t)__popcll(__ballot(ev_still));
        ev_sample = ev_still = false;
        if (n_samples >= 0x80000000u) {                                  // (wave-uniform: the 32-bit count never wraps)
            if ((tid & 63u) == 0u) atomicAdd(head + kQueryRefineCounts + 1, (unsigned long long)n_samples);
            n_samples = 0;
        }
        while (!ch.drained && __ballot(!have) != 0ull) {                 // wave-uniform: every free lane takes, until none is free
            unsigned long long i = 0;
            const bool mine = wf_take(ch, head, grab, qa.n, !have, i);
            bool start = false;
            if (mine) {
                const uint32_t n = rule.sample_begin + qa.extra[i];
                if (n < rule.max_samples) {
                    start = n < 2u;
                    if (!start) {
                        const double *S = qa.sum + 3ull * i, *Q = qa.sum_sq + 3ull * i;
                        start = refine_selected(rule, n, S[0], S[1], S[2], Q[0], Q[1], Q[2]);
                    }
                }
            }
            if (start) { idx = (uint32_t)i; k = 0; have = true; fresh = true; }
            n_pixels += (uint32_t)__popcll(__ballot(start));
        }
        if (have && fresh) gen_primary(sv, rv, idx, rule.sample_begin + qa.extra[idx] + k, r);   // key (seed, y * width + x, sample), draws 0..5
        fresh = false;
        if (ch.drained && __ballot(have) == 0ull) break;                 // wave-uniform
        if (!have) continue;
        const RayX rx = make_rayx(r.pos, r.dir);
        Hit h;
        ++segs;
        query_closest_ray<TRIS>(sv, qa.walk, nodes, la, ma, r.pos, r.dir, rx, h, ls, lq, tid, spill, spill_entries, spill_stride, glane, exact,
                                box_tests, leaf_filters);
        bool done = true;                                                // scene.rs:232: None ends the path
        if (h.id != kNone) {
            r.draw = 6u + 2u * r.bounce;                                 // (the draws of bounce b: not carried across the walk)
            advance_and_shade(sv, h, r);
            done = (r.bounce >= bounce_limit) || light_is_zero(r);       // scene.rs:227-228
        }
        if (done) {
            double *S = qa.sum + 3ull * idx, *Q = qa.sum_sq + 3ull * idx;
            const double s0 = S[0] + r.result.x, s1 = S[1] + r.result.y, s2 = S[2] + r.result.z;
            const double q0 = Q[0] + r.result.x * r.result.x, q1 = Q[1] + r.result.y * r.result.y, q2 = Q[2] + r.result.z * r.result.z;
            S[0] = s0; S[1] = s1; S[2] = s2;
            Q[0] = q0; Q[1] = q1; Q[2] = q2;
            ++k;
            ev_sample = true;
            const uint32_t n = rule.sample_begin + qa.extra[idx] + k;
            if (n < rule.max_samples) {
                const uint32_t rounds_done = k / rule.n_more;
                if (k - rounds_done * rule.n_more != 0u) fresh = true;   // inside a round
                else {                                                   // a round's end: the rule again
                    const bool sel = refine_selected(rule, n, s0, s1, s2, q0, q1, q2);
                    fresh = sel && rounds_done < rule.rounds;
                    ev_still = sel && !fresh;
                }
            }
            if (!fresh) { qa.extra[idx] += k; have = false; }
            __asm__ volatile("" ::: "memory");                           // the sums stay in memory: nothing of them is held across the walk
        }
    }
    if ((tid & 63u) == 0u) {
        if (n_pixels) atomicAdd(head + kQueryRefineCounts, (unsigned long long)n_pixels);
        if (n_samples) atomicAdd(head + kQueryRefineCounts + 1, (unsigned long long)n_samples);
        if (n_still) atomicAdd(head + kQueryRefineCounts + 2, (unsigned long long)n_still);
    }
}

// ---- the multi-hit mode --------------------------------------------------------------------------------------------------------
// The k nearest objects of ray i in (distance, scene index) order (rtx_scene_multi_hits; DESIGN.md "Multi-hit queries"): what
// closest_object returns when it is asked k times with the earlier winners retained out of Scene.objects -- every object whose
// distance passes closest_object's filter and lies before t_max[i], sorted.  The lane's list lives in the ray's own k output records
// (the lane owns them; 16 doubles per entry are more than the kernel's registers hold): while the ray is walked an entry is
// {word 0: kind << 32 | local, word 6: distance, word 7: scene index} of the record's eight 64-bit words, kept sorted by insertion;
// position and normal are written over them at the ray's end.  Every access goes through the same unsigned long long view.
//
// The bound.  The walks prune against best_up; here it is max(round_up32(t_max), FLT_MIN) -- the any-hit mode's seed -- while the
// list holds fewer than k entries and min(that, round_up32(list[k-1].distance)) once it is full.  An object that belongs to the final
// list has (t, id) <= the k-th entry of every intermediate list (entries only ever move down), so t <= list[k-1].distance <= the
// bound, its boxes and its own t_lo are lower bounds of t, and `t_lo <= bound` keeps it -- also at a tie with the k-th distance.
// Only exact hits already in the list lower the bound: the leaf code runs in its TIGHTEN = false form.
__device__ __forceinline__ double multi_distance(const unsigned long long *rec, uint32_t j) { return __longlong_as_double((long long)rec[8u * j + 6u]); }

__device__ __forceinline__ float multi_bound(const unsigned long long *rec, uint32_t k, uint32_t cnt, float bound0)
{
    return cnt == k ? fminf(bound0, round_up32(multi_distance(rec, k - 1u))) : bound0;
}

// closest_object's filter and the limit, then the sorted insert; a full list drops its last entry.  Returns whether the list changed.
__device__ __forceinline__ bool multi_insert(unsigned long long *rec, uint32_t k, uint32_t &cnt, double t_max, double t, uint32_t id, uint32_t kind,
                                             uint32_t local)
{
    if (!query_before(t, t_max)) return false;
    uint32_t j = cnt;
    if (cnt == k) {
        j = k - 1u;
        const double tl = multi_distance(rec, j);
        if (!(t < tl || (t == tl && id < (uint32_t)rec[8u * j + 7u]))) return false;
    } else cnt += 1u;
#pragma unroll 1
    while (j != 0u) {
        const unsigned long long dp = rec[8u * (j - 1u) + 6u], ip = rec[8u * (j - 1u) + 7u];
        const double tp = __longlong_as_double((long long)dp);
        if (!(t < tp || (t == tp && id < (uint32_t)ip))) break;
        rec[8u * j] = rec[8u * (j - 1u)];
        rec[8u * j + 6u] = dp;
        rec[8u * j + 7u] = ip;
        j -= 1u;
    }
    rec[8u * j] = ((unsigned long long)kind << 32) | local;
    rec[8u * j + 6u] = (unsigned long long)__double_as_longlong(t);
    rec[8u * j + 7u] = id;
    return true;
}

// query_sweep into the list
__device__ __forceinline__ void multi_sweep(const SceneView &sv, const LeafArrays &la, const RayX &rx, bool spheres, bool tris,
                                            unsigned long long *rec, uint32_t k, uint32_t &cnt, double t_max, unsigned long long &exact)
{
    double t;
    if (spheres) {
        for (uint32_t s = 0; s < sv.n_spheres; ++s)
            if (sphere_distance(la.spheres[s], rx, &t)) (void)multi_insert(rec, k, cnt, t_max, t, la.sphere_ids[s], 0, s);
        exact += sv.n_spheres;
    }
    for (uint32_t s = 0; s < sv.n_planes; ++s)
        if (plane_distance(sv.planes[s], rx, &t)) (void)multi_insert(rec, k, cnt, t_max, t, sv.planes[s].id, 1, s);
    exact += sv.n_planes;
    if (tris) {
        for (uint32_t s = 0; s < sv.n_tris; ++s)
            if (triangle_distance(la.tris[s], rx, &t)) (void)multi_insert(rec, k, cnt, t_max, t, la.tris[s].id, 2, s);
        exact += sv.n_tris;
    }
}

// query_flush into the list; the bound follows the list from one candidate to the next
__device__ __forceinline__ void multi_flush(const LeafArrays &la, const RayX &rx, const uint32_t *lq, uint32_t tid, uint32_t queue, uint32_t qcnt,
                                            float bound0, float &bound, unsigned long long *rec, uint32_t k, uint32_t &cnt, double t_max,
                                            unsigned long long &exact)
{
#pragma unroll 1
    for (uint32_t e = 0; e < qcnt; ++e) {
        if (__uint_as_float(lq[(size_t)(queue + e) * kBvhThreads + tid]) <= bound) {
            const uint32_t idx = lq[(size_t)e * kBvhThreads + tid];
            double t;
            bool in = false;
            if (idx & kQueueTri) {
                const uint32_t tk = la.tri_fidx[idx & ~kQueueTri];
                if (triangle_distance(la.tris[tk], rx, &t)) in = multi_insert(rec, k, cnt, t_max, t, la.tris[tk].id, 2, tk);
            } else {
                if (sphere_distance(la.spheres[idx], rx, &t)) in = multi_insert(rec, k, cnt, t_max, t, la.sphere_ids[idx], 0, idx);
            }
            if (in) bound = multi_bound(rec, k, cnt, bound0);
            exact += 1;
        }
    }
}

// query_mesh_walk's loop with the list's bound: the step never lowers it (TIGHTEN = false), a flush does
template <int PLAIN, class RAY>
__device__ __forceinline__ void query_mesh_walk_multi(const float4 *__restrict__ nodes, const LeafArrays &la, const MeshArrays &ma, const RAY &q,
                                                      const SphereRay &sr, const TriFilterParams &tpar, const RayX &rx, uint32_t root, float bound0,
                                                      unsigned long long *rec, uint32_t k, uint32_t &cnt, double t_max, bool &overflow, uint32_t *ls,
                                                      uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill, uint32_t spill_entries,
                                                      size_t spill_stride, size_t glane, unsigned long long &exact, uint32_t &nbox, uint32_t &nleaf)
{
    float bound = multi_bound(rec, k, cnt, bound0);
    uint32_t node = root, sp = 0, qcnt = 0, resume = 0, resume_node = 0;
    float4 nd[MeshNode<PLAIN>::n];
    if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, node, nd);
    while (node != kNone || resume != 0u) {
        if (mesh_step<true, PLAIN, kQueryMeshStack, false>(nodes, ma, q, sr, tpar, nd, node, sp, qcnt, overflow, bound, resume, resume_node, ls,
                                                            lq, tid, spill, spill_entries, spill_stride, glane, nbox, nleaf))
            continue;
        multi_flush(la, rx, lq, tid, kMeshQueue, qcnt, bound0, bound, rec, k, cnt, t_max, exact);
        qcnt = 0;
        if constexpr (kMeshPipe) mesh_load_node<PLAIN>(nodes, resume_node, nd);
    }
    multi_flush(la, rx, lq, tid, kMeshQueue, qcnt, bound0, bound, rec, k, cnt, t_max, exact);
}

// One ray of the multi-hit mode, t_max > 0 (the caller's gate): the list of its objects before t_max, the first k of them.
template <bool TRIS>
__device__ __forceinline__ void query_multi_ray(const SceneView &sv, const float4 *__restrict__ nodes, const LeafArrays &la, const MeshArrays &ma,
                                                V3 pos, V3 dir, const RayX &rx, bool walk, bool in32, double t_max, unsigned long long *rec,
                                                uint32_t k, uint32_t &cnt, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long &exact,
                                                unsigned long long &box_tests, unsigned long long &leaf_filters)
{
    cnt = 0;
    if (!walk) { multi_sweep(sv, la, rx, true, true, rec, k, cnt, t_max, exact); return; }
    // the shapes the tree does not answer for, BEFORE the walk (as the any-hit mode): every plane, the spheres and the triangle records
    // outside it -- whatever they put into the list bounds the walk from its first box on
    multi_sweep(sv, la, rx, (sv.bvh_flags & 1u) == 0u, false, rec, k, cnt, t_max, exact);
    const uint32_t from = (sv.bvh_flags & 2u) ? sv.n_tri_tree : 0u;
    for (uint32_t s = from; s < sv.n_tri_filter; ++s) {
        const uint32_t tk = la.tri_fidx[s];
        double t;
        if (triangle_distance(la.tris[tk], rx, &t)) (void)multi_insert(rec, k, cnt, t_max, t, la.tris[tk].id, 2, tk);
    }
    exact += sv.n_tri_filter - from;
    const float bound0 = fmaxf(round_up32(t_max), 1.17549435e-38f);     // (+inf when t_max is; never a denormal a compare may flush)
    bool overflow = false;
    uint32_t nbox = 0, nleaf = 0;
    if constexpr (TRIS) {
        SphereRay sr;
        query_sphere_ray(sv, pos, dir, sr);
        TriFilterParams tpar;
        tri_filter_from_ray(sv, pos, dir, tpar);
        const bool plain = (sv.bvh_flags & 4u) != 0u;
        if (in32) {
            Ray32 q;
            make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q);
            if (plain) query_mesh_walk_multi<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, bound0, rec, k, cnt, t_max, overflow, ls, lq, tid, spill,
                                                spill_entries, spill_stride, glane, exact, nbox, nleaf);
            else query_mesh_walk_multi<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, bound0, rec, k, cnt, t_max, overflow, ls, lq, tid, spill,
                                          spill_entries, spill_stride, glane, exact, nbox, nleaf);
        } else {
            Ray64 q;
            make_ray64(pos, rx.dirn, (double)sv.bvh_inv_max, q);
            if (plain) query_mesh_walk_multi<2>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, bound0, rec, k, cnt, t_max, overflow, ls, lq, tid, spill,
                                                spill_entries, spill_stride, glane, exact, nbox, nleaf);
            else query_mesh_walk_multi<0>(nodes, la, ma, q, sr, tpar, rx, sv.bvh_root, bound0, rec, k, cnt, t_max, overflow, ls, lq, tid, spill,
                                          spill_entries, spill_stride, glane, exact, nbox, nleaf);
        }
    } else {
        SphereRay sr;
        sphere_ray_from(sv, pos, dir, sr);
        Ray32 q0;
        make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q0);
        Ray32S q;
        q.ix = q0.ix; q.iy = q0.iy; q.iz = q0.iz; q.nx = q0.nx; q.ny = q0.ny; q.nz = q0.nz;
        q.e = ray32_slack(q0, in32);
        float bound = multi_bound(rec, k, cnt, bound0);
        uint32_t node = sv.bvh_root, sp = 0, qcnt = 0;
        // sphere_walk_phased's iteration, as the any-hit mode runs it; a lane whose queue may not take the leaf's records has its
        // candidates tested first (with k > 1 nothing overtakes them: four live candidates are the rule, not the exception)
        while (node != kNone) {
            const bool at_leaf = (node >> 29) != 0u;
            const unsigned long long lm = __ballot(at_leaf), am = __ballot(true);
            if ((uint32_t)__popcll(lm) >= kQueryLeafLanes || lm == am) {
                if (at_leaf) {
                    if (qcnt + (node >> 29) > (uint32_t)kSphQueue) {
                        multi_flush(la, rx, lq, tid, kSphQueue, qcnt, bound0, bound, rec, k, cnt, t_max, exact);
                        qcnt = 0;
                    }
                    sphere_leaf_step<kQuerySphStack, true, false>(la.sphere_f32, la.sphere_prims, sr, node, sp, ls, lq, tid, spill, spill_stride,
                                                                  glane, bound, qcnt, overflow, nleaf);
                }
            } else if (!at_leaf) {
                sphere_node_step_q3<kQuerySphStack, true>(nodes, q, node, sp, ls, tid, spill, spill_entries, spill_stride, glane, bound, overflow,
                                                          nbox);
            }
        }
        if (!overflow) multi_flush(la, rx, lq, tid, kSphQueue, qcnt, bound0, bound, rec, k, cnt, t_max, exact);
    }
    box_tests += nbox;
    leaf_filters += nleaf;
    if (overflow) {                                   // a walk cut short by a full stack or queue: start over, every shape exactly
        cnt = 0;
        multi_sweep(sv, la, rx, true, true, rec, k, cnt, t_max, exact);
    }
}

// The kernel's ray loop in the multi-hit mode.  A loop of its own, entered once per launch: the other loops carry none of its
// arguments or state.
template <bool TRIS>
__device__ __forceinline__ void query_multi_loop(const SceneView &sv, const QueryArgs &qa, const float4 *__restrict__ nodes, const LeafArrays &la,
                                                 const MeshArrays &ma, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t *__restrict__ spill,
                                                 uint32_t spill_entries, size_t spill_stride, size_t glane, unsigned long long *__restrict__ head,
                                                 unsigned long long &segs, unsigned long long &exact, unsigned long long &box_tests,
                                                 unsigned long long &leaf_filters)
{
    const unsigned long long grab = wf_grab_size(qa.n);
    const uint32_t k = qa.mode >> kQueryMultiShift;
    WfChunk ch{0ull, 0ull, false};
    for (;;) {
        unsigned long long i = 0;
        const bool mine = wf_take(ch, head, grab, qa.n, true, i);
        if (ch.drained && __ballot(mine) == 0ull) break;
        if (!mine) continue;
        ++segs;
        unsigned long long *const rec = reinterpret_cast<unsigned long long *>(qa.hits) + 8ull * k * i;
        const double t_max = qa.t_max ? qa.t_max[i] : __builtin_inf();
        uint32_t cnt = 0;
        V3 pos, dir;
        if (qa.rv) {                                                     // the pick buffer's ray, as the closest-hit loop builds it
            pos = sv.cam_pos;
            dir = vnorm(vsub(primary_focal_point(sv, *qa.rv, (uint32_t)i), pos));
        } else {
            const QueryRay &qr = qa.rays[i];
            pos = mk(qr.position[0], qr.position[1], qr.position[2]);
            dir = mk(qr.direction[0], qr.direction[1], qr.direction[2]);
        }
        if (t_max > 0.0) {                                               // (NaN, zero, negative: an empty list, nothing is tested)
            const RayX rx = make_rayx(pos, dir);
            bool in32;
            const bool walk = query_walkable(sv, qa.walk, pos, dir, in32);
            query_multi_ray<TRIS>(sv, nodes, la, ma, pos, dir, rx, walk, in32, t_max, rec, k, cnt, ls, lq, tid, spill, spill_entries, spill_stride,
                                  glane, exact, box_tests, leaf_filters);
        }
        // the answers over the list: scene.rs:234's hit point and object.rs:37-39's normal there, as the closest-hit loop writes them;
        // behind them the closest-hit loop's miss
#pragma unroll 1
        for (uint32_t j = 0; j < k; ++j) {
            unsigned long long *const w = rec + 8u * j;
            if (j < cnt) {
                Hit h;
                h.t = __longlong_as_double((long long)w[6]);
                h.id = (uint32_t)w[7];
                h.kind = (uint32_t)(w[0] >> 32);
                h.local = (uint32_t)w[0];
                const V3 p = vadd(pos, vmuls(dir, h.t));
                const V3 nrm = normal_at(sv, h, p);
                w[0] = (unsigned long long)__double_as_longlong(p.x); w[1] = (unsigned long long)__double_as_longlong(p.y);
                w[2] = (unsigned long long)__double_as_longlong(p.z);
                w[3] = (unsigned long long)__double_as_longlong(nrm.x); w[4] = (unsigned long long)__double_as_longlong(nrm.y);
                w[5] = (unsigned long long)__double_as_longlong(nrm.z);
                w[7] = (unsigned long long)(long long)h.id;
            } else {
                const unsigned long long nan = (unsigned long long)__double_as_longlong(__builtin_nan(""));
                w[0] = w[1] = w[2] = w[3] = w[4] = w[5] = nan;
                w[6] = (unsigned long long)__double_as_longlong(__builtin_inf());
                w[7] = ~0ull;
            }
        }
        if (qa.counts) qa.counts[i] = cnt;
    }
}

template <bool TRIS>
__global__ __launch_bounds__(kBvhThreads, kQueryWaves) void query_closest_kernel(const SceneView *__restrict__ svp, const QueryArgs qa,
                                                                                 const float4 *__restrict__ nodes, const LeafArrays la,
                                                                                 const MeshArrays ma, uint32_t *__restrict__ spill,
                                                                                 uint32_t spill_entries, Counters *__restrict__ ctr,
                                                                                 unsigned long long *__restrict__ head)
{
    constexpr int STACK = TRIS ? kQueryMeshStack : kQuerySphStack;
    constexpr int QUEUE = TRIS ? kMeshQueue : kSphQueue;
    const SceneView &sv = *svp;
    __shared__ uint32_t lds_stack[STACK + 1][kBvhThreads];             // + the sink row of the branch-free pushes
    __shared__ uint32_t lds_q[2 * QUEUE][kBvhThreads];                 // candidate entries, then their t_lo
    uint32_t *const ls = &lds_stack[0][0];
    uint32_t *const lq = &lds_q[0][0];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const size_t spill_stride = (size_t)gridDim.x * kBvhThreads, glane = (size_t)blockIdx.x * kBvhThreads + tid;
    const unsigned long long grab = wf_grab_size(qa.n);
    unsigned long long segs = 0, box_tests = 0, leaf_filters = 0, exact = 0;
    WfChunk ch{0ull, 0ull, false};

    if (qa.mode == kQueryAnyHit)                                         // launch-uniform: the any-hit mode has its own ray loop
        query_any_loop<TRIS>(sv, qa, nodes, la, ma, ls, lq, tid, spill, spill_entries, spill_stride, glane, head, segs, exact, box_tests,
                             leaf_filters);
    else if (qa.mode == kQueryPaths)                                     // launch-uniform: so has the path mode
        query_path_loop<TRIS>(sv, qa, nodes, la, ma, ls, lq, tid, spill, spill_entries, spill_stride, glane, head, segs, exact, box_tests,
                              leaf_filters);
    else if (qa.mode == kQueryFeatures)                                  // launch-uniform: and the feature mode
        query_feature_loop<TRIS>(sv, qa, nodes, la, ma, ls, lq, tid, spill, spill_entries, spill_stride, glane, head, segs, exact, box_tests,
                                 leaf_filters);
    else if (qa.mode == kQueryRefine)                                    // launch-uniform: and the refine mode
        query_refine_loop<TRIS>(sv, qa, nodes, la, ma, ls, lq, tid, spill, spill_entries, spill_stride, glane, head, segs, exact, box_tests,
                                leaf_filters);
    else if ((qa.mode & kQueryModeMask) == kQueryMulti)                  // launch-uniform: and the multi-hit mode (k above the mode)
        query_multi_loop<TRIS>(sv, qa, nodes, la, ma, ls, lq, tid, spill, spill_entries, spill_stride, glane, head, segs, exact, box_tests,
                               leaf_filters);
    else for (;;) {
        unsigned long long i = 0;
        const bool mine = wf_take(ch, head, grab, qa.n, true, i);         // (every lane of the wave is here: lane 0 takes the chunk)
        if (ch.drained && __ballot(mine) == 0ull) break;                 // wave-uniform
        if (!mine) continue;
        V3 pos, dir;
        if (qa.rv) {                                                     // the pick buffer: render_pixel's ray without the offsets
            pos = sv.cam_pos;
            dir = vnorm(vsub(primary_focal_point(sv, *qa.rv, (uint32_t)i), pos));      // scene.rs:203-207, i = y * width + x
        } else {
            const QueryRay &qr = qa.rays[i];
            pos = mk(qr.position[0], qr.position[1], qr.position[2]);
            dir = mk(qr.direction[0], qr.direction[1], qr.direction[2]);
        }
        const RayX rx = make_rayx(pos, dir);
        Hit h;
        ++segs;
        query_closest_ray<TRIS>(sv, qa.walk, nodes, la, ma, pos, dir, rx, h, ls, lq, tid, spill, spill_entries, spill_stride, glane, exact,
                                box_tests, leaf_filters);
        // the answer: scene.rs:234's hit point and object.rs:37-39's normal there (what advance_and_shade hands the bounce)
        QueryHit out;
        if (h.id != kNone) {
            const V3 p = vadd(pos, vmuls(dir, h.t));
            const V3 n = normal_at(sv, h, p);
            out.position[0] = p.x; out.position[1] = p.y; out.position[2] = p.z;
            out.normal[0] = n.x; out.normal[1] = n.y; out.normal[2] = n.z;
            out.distance = h.t;
            out.object = (long long)h.id;
        } else {
            const double nan = __builtin_nan("");
            out.position[0] = out.position[1] = out.position[2] = nan;
            out.normal[0] = out.normal[1] = out.normal[2] = nan;
            out.distance = __builtin_inf();
            out.object = -1;
        }
        qa.hits[i] = out;
    }
    unsigned long long filt = box_tests + leaf_filters;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        segs += __shfl_xor(segs, off, 64);
        exact += __shfl_xor(exact, off, 64);
        filt += __shfl_xor(filt, off, 64);
        box_tests += __shfl_xor(box_tests, off, 64);
    }
    if (lane == 0) {
        const uint32_t shard = (blockIdx.x * (kBvhThreads >> 6) + (tid >> 6)) & (kCounterShards - 1);
        if (segs) atomicAdd(&ctr[shard].segments, segs);
        if (exact) atomicAdd(&ctr[shard].exact_tests, exact);
        if (filt) atomicAdd(&ctr[shard].filter_tests, filt);
        if (box_tests) atomicAdd(&ctr[2 + (shard % (kCounterShards - 2))].pad_, box_tests);   // shards 0,1 carry debug flags
    }
}

// which walk a scene's tree allows: 1 a sphere tree with its 64-byte nodes, 2 a tree that holds triangles (a pure footprint tree
// only with its 64-byte nodes), 0 none (every ray is swept)
uint32_t query_tree_kind(const SceneView &sv)
{
    if (sv.n_bvh_nodes == 0) return 0u;
    if ((sv.bvh_flags & 19u) == 17u && sv.bvh_q3nodes != nullptr) return 1u;
    if ((sv.bvh_flags & 2u) != 0u && ((sv.bvh_flags & 4u) == 0u || ((sv.bvh_flags & 8u) != 0u && sv.bvh_qnodes != nullptr))) return 2u;
    return 0u;
}

uint32_t query_spill_entries(const SceneView &sv)
{
    const uint32_t kind = query_tree_kind(sv);
    if (kind == 0u) return 0u;
    const uint32_t need = 3u * sv.bvh_depth + 2u;                   // a 4-wide node pushes at most 3 entries per level
    const uint32_t rows = (uint32_t)(kind == 1u ? kQuerySphStack : kQueryMeshStack);
    return need > rows ? need - rows : 0u;
}

uint32_t query_blocks(uint64_t n, int n_cus)
{
    const uint64_t want = (n + kBvhThreads - 1) / kBvhThreads;
    const uint64_t cap = (uint64_t)n_cus * kQueryWaves;
    return (uint32_t)(want < cap ? want : cap);
}

size_t query_spill_bytes(uint32_t entries, int n_cus)
{
    return (size_t)entries * (size_t)n_cus * kQueryWaves * kBvhThreads * sizeof(uint32_t);
}

hipError_t launch_query_closest(const SceneView *d_sv, const SceneView &sv, const QueryArgs &qa, bool walk, uint32_t *spill,
                                uint32_t spill_entries, int n_cus, Counters *counters, unsigned long long *head, hipStream_t stream)
{
    const uint32_t blocks = query_blocks(qa.n, n_cus);
    if (blocks == 0) return hipSuccess;
    const uint32_t kind = walk ? query_tree_kind(sv) : 0u;
    QueryArgs a = qa;
    a.walk = kind != 0u ? 1u : 0u;
    LeafArrays la;
    la.sphere_f32 = sv.bvh_leaf_cr; la.sphere_prims = sv.bvh_prims; la.spheres = sv.spheres; la.sphere_ids = sv.sphere_id;
    la.tri_f32 = sv.tri_f32; la.tri_fidx = sv.tri_fidx; la.tris = sv.tris;
    MeshArrays ma;
    ma.sphere_cr = sv.bvh_leaf_cr; ma.sphere_prims = sv.bvh_prims; ma.tri_f32 = sv.tri_f32; ma.tri_geo = sv.tri_geo;
    const float4 *nodes = kind == 1u ? reinterpret_cast<const float4 *>(sv.bvh_q3nodes)
                        : (kind == 2u && (sv.bvh_flags & 4u) != 0u) ? reinterpret_cast<const float4 *>(sv.bvh_qnodes)
                        : reinterpret_cast<const float4 *>(sv.bvh_nodes);
    if (!spill) spill_entries = 0u;
    if (kind == 2u)
        hipLaunchKernelGGL(query_closest_kernel<true>, dim3(blocks), dim3(kBvhThreads), 0, stream, d_sv, a, nodes, la, ma, spill, spill_entries,
                           counters, head);
    else
        hipLaunchKernelGGL(query_closest_kernel<false>, dim3(blocks), dim3(kBvhThreads), 0, stream, d_sv, a, nodes, la, ma, spill, spill_entries,
                           counters, head);
    return hipGetLastError();
}


#ifdef RTX_LAB
// ---- rtx_debug_path_bounds (librtx_hip_lab.so only) ----------------------------------------------------------------------------
// What the walks' f32 bounds decide for ONE (ray, object) pair: a thread runs the walks' own device functions -- the slab tests of the
// 128-byte, footprint and 64-byte nodes, the sphere and triangle leaf bounds -- along the root -> leaf path of its object, which the
// host found in the flat tree, with the caller's best_up.  Nothing of their arithmetic is restated here: the kernel prepares the
// ray as query_closest_ray does, calls, and reads the results back from the functions' own outputs (return value, node, stack, queue).
constexpr int kPathStack = 8;                                    // LDS stack rows of the one-visit calls (they start on an empty stack)
constexpr uint32_t kPbNoWalk = 3u;                             // word 0, bits 0-1: 0 Ray32, 1 Ray32S (slack != 0), 2 Ray64, 3 no walk
constexpr uint32_t kPbInTree = 4u, kPbCandidate = 8u, kPbCertain = 16u, kPbTriangle = 32u, kPbNoForm = 64u;

// the entered children of one visit that started on an empty stack: the next node and what lies below it
__device__ __forceinline__ bool pb_entered(uint32_t target, uint32_t node, uint32_t sp, const uint32_t *ls, uint32_t tid)
{
    bool in = node == target;
    for (uint32_t r = 0; r < sp; ++r) in = in || ls[(size_t)r * kBvhThreads + tid] == target;
    return in;
}

// j's child at every step of the path; *entered counts the steps that enter it, *bound is the largest entry distance returned
template <class RAY>
__device__ __forceinline__ void pb_path(const SceneView &sv, const PathBoundsArgs &a, const RAY &q, uint32_t row, uint32_t len, float best_up,
                                        uint32_t *ls, uint32_t tid, uint32_t &entered, float &bound, uint32_t &first_miss, bool &no_form)
{
    const bool small = (a.form & 2u) != 0u;                      // the 64-byte forms
    const float4 *nodes128 = reinterpret_cast<const float4 *>(sv.bvh_nodes);
    for (uint32_t s = 0; s < len; ++s) {
        const uint32_t link = a.steps[2 * ((size_t)row * a.stride + s)], c = a.steps[2 * ((size_t)row * a.stride + s) + 1];
        const uint32_t idx = link & ~kBvhFlatNode;
        bool in = false;
        if (!small) {
            const float4 *np = nodes128 + 8 * (size_t)idx;
            const float tc = (link & kBvhFlatNode) ? rect_entry32(np[c], q, best_up) : box_entry32(np[c], np[4 + c], q, best_up);
            in = tc < __builtin_inff();
            if (in) bound = fmaxf(bound, tc);
        } else if ((sv.bvh_flags & 16u) != 0u && sv.bvh_q3nodes != nullptr) {
            if constexpr (sizeof(q.ix) == sizeof(float)) {       // (sphere_node_step_q3 has no f64 form)
                const float4 *qn = reinterpret_cast<const float4 *>(sv.bvh_q3nodes);
                const uint32_t *words = reinterpret_cast<const uint32_t *>(sv.bvh_q3nodes + idx);
                const uint32_t target = words[2 * c];            // {link0, ox, link1, oy} {link2, oz, link3, sx}
                uint32_t node = idx, sp = 0, nbox = 0;
                bool overflow = false;
                sphere_node_step_q3<kPathStack, false>(qn, q, node, sp, ls, tid, nullptr, 0u, 0, 0, best_up, overflow, nbox);
                in = pb_entered(target, node, sp, ls, tid);
            } else no_form = true;
        } else if ((sv.bvh_flags & 8u) != 0u && sv.bvh_qnodes != nullptr) {
            const float4 *np = reinterpret_cast<const float4 *>(sv.bvh_qnodes) + 4 * (size_t)idx;
            const float4 n0 = np[0], n1 = np[1], n2 = np[2];     // as mesh_step<2> opens the node (rtx_mesh_step.h, `if constexpr (PLAIN == 2)`
                                                                 // under `resume == 0u`: Ax / Ay, qx / qy, qnode_offset) -- a copy: keep in step
            const auto Ax = n0.z * q.ix, Ay = n0.w * q.iy;
            const auto Bx = qnode_offset(n0.x, q.ix, q.nx), By = qnode_offset(n0.y, q.iy, q.ny);
            const uint32_t qx = __float_as_uint(c == 0 ? n1.x : (c == 1 ? n1.y : (c == 2 ? n1.z : n1.w)));
            const uint32_t qy = __float_as_uint(c == 0 ? n2.x : (c == 1 ? n2.y : (c == 2 ? n2.z : n2.w)));
            const float tc = qrect_entry(qx, qy, Ax, Bx, Ay, By, best_up, ray_slack(q));
            in = tc < __builtin_inff();
            if (in) bound = fmaxf(bound, tc);
        } else no_form = true;
        if (in) entered += 1;
        else if (first_miss == kNone) first_miss = s;
    }
}

// the leaf test of j's record with the bound `bu`; returns whether j became a candidate, *tlo its lower bound; bu is updated
template <class RAY>
__device__ __forceinline__ bool pb_leaf(const SceneView &sv, const PathBoundsArgs &a, const RAY &q, const SphereRay &sr, const TriFilterParams &tpar,
                                        bool tri, uint32_t rec, size_t i, float &bu, float &tlo, uint32_t *ls, uint32_t *lq, uint32_t tid,
                                        bool &no_form)
{
    const uint32_t leaf = (a.form >> 8) & 3u;
    uint32_t node = 0, sp = 0, qcnt = 0, nbox = 0, nleaf = 0;
    bool overflow = false;
    tlo = __builtin_inff();
    if (leaf == 0u && !tri) {
        node = (1u << 29) | rec;
        sphere_leaf_step_at<kPathStack, false, kBvhThreads>(sv.bvh_leaf_cr, sv.bvh_prims, sr, node, sp, ls, lq, tid, tid, nullptr, 0, 0, bu, qcnt,
                                                            overflow, nleaf);
        if (qcnt == 1u) tlo = __uint_as_float(lq[(size_t)kSphQueue * kBvhThreads + tid]);
        return qcnt == 1u;
    }
    if (leaf == 0u) {
        const float4 A = sv.tri_f32[2 * (size_t)rec], B = sv.tri_f32[2 * (size_t)rec + 1];
        if ((int)tri_filter_sign(A, B, tpar) < 0) return false;
        float thi;
        tlo = tri_bounds(A, sv.tri_geo[2 * (size_t)rec], sv.tri_geo[2 * (size_t)rec + 1], tpar, thi);
        if (!(tlo <= bu && tlo < __builtin_inff())) return false;             // (a copy of mesh_step's candidate rule and bound update, its
        bu = fminf(bu, thi);                                                  // triangle-leaf loop; leaf form 2 runs mesh_step's own)
        return true;
    }
    if (leaf == 3u && !tri) {                                   // the packet kernel's test of one record of a leaf
        sph_packet_leaf_test(sv.bvh_leaf_cr[rec], sv.bvh_prims[rec], sr, lq, tid, bu, qcnt, overflow);
        if (qcnt == 1u) tlo = __uint_as_float(lq[(size_t)kSphQueue * kBvhThreads + tid]);
        return qcnt == 1u;
    }
    if (leaf == 3u) { no_form = true; return false; }
    // the leaf code inlined in a node visit: the host's one-child 128-byte node of j's record, its box unbounded
    const float4 *one = a.leaf_nodes + 8 * i;
    if (leaf == 1u && !tri) {
        sphere_step<kPathStack, false>(one, sv.bvh_leaf_cr, sv.bvh_prims, q, sr, node, sp, ls, lq, tid, nullptr, 0u, 0, 0, bu, qcnt, overflow, nbox,
                                       nleaf);
        if (qcnt == 1u) tlo = __uint_as_float(lq[(size_t)kSphQueue * kBvhThreads + tid]);
        return qcnt == 1u;
    }
    if (leaf == 2u) {
        MeshArrays ma;
        ma.sphere_cr = sv.bvh_leaf_cr; ma.sphere_prims = sv.bvh_prims; ma.tri_f32 = sv.tri_f32; ma.tri_geo = sv.tri_geo;
        float4 nd[MeshNode<0>::n];
        uint32_t resume = 0, resume_node = 0;
        (void)mesh_step<false, 0, kPathStack>(one, ma, q, sr, tpar, nd, node, sp, qcnt, overflow, bu, resume, resume_node, ls, lq, tid, nullptr, 0u,
                                              0, 0, nbox, nleaf);
        if (qcnt == 1u) tlo = __uint_as_float(lq[(size_t)kMeshQueue * kBvhThreads + tid]);
        return qcnt == 1u;
    }
    no_form = true;
    return false;
}

template <class RAY>
__device__ __forceinline__ void pb_element(const SceneView &sv, const PathBoundsArgs &a, const RAY &q, const SphereRay &sr, const TriFilterParams &tpar,
                                           size_t i, uint32_t *ls, uint32_t *lq, uint32_t tid, uint32_t &flags, uint32_t *out)
{
    const uint32_t row = a.rows[i], entry = a.entries[i], len = a.lens[row];
    const bool tri = (entry & kQueueTri) != 0u;
    const float best_up = a.best_up[i];
    uint32_t entered = 0, first_miss = kNone;
    float bound = -__builtin_inff();
    bool no_form = false;
    pb_path(sv, a, q, row, len, best_up, ls, tid, entered, bound, first_miss, no_form);
    float bu = best_up, tlo, tlo_inf, thi = __builtin_inff();
    const bool cand = pb_leaf(sv, a, q, sr, tpar, tri, entry & ~kQueueTri, i, bu, tlo, ls, lq, tid, no_form);
    (void)pb_leaf(sv, a, q, sr, tpar, tri, entry & ~kQueueTri, i, thi, tlo_inf, ls, lq, tid, no_form);   // best_up = +inf: falls iff certain
    flags |= (cand ? kPbCandidate : 0u) | (thi < __builtin_inff() ? kPbCertain : 0u) | (tri ? kPbTriangle : 0u) | (no_form ? kPbNoForm : 0u);
    out[1] = len; out[2] = entered; out[3] = __float_as_uint(bound); out[4] = __float_as_uint(cand ? tlo : tlo_inf);
    out[5] = __float_as_uint(thi); out[6] = __float_as_uint(bu); out[7] = first_miss;
}

__global__ __launch_bounds__(kBvhThreads) void debug_path_bounds_kernel(const SceneView *__restrict__ svp, const PathBoundsArgs a)
{
    constexpr int QROWS = 2 * (kMeshQueue > kSphQueue ? kMeshQueue : kSphQueue);
    __shared__ uint32_t lds_stack[kPathStack + 1][kBvhThreads];
    __shared__ uint32_t lds_q[QROWS][kBvhThreads];
    const SceneView &sv = *svp;
    const uint32_t tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kBvhThreads + tid;
    if (i >= a.n) return;
    uint32_t *const ls = &lds_stack[0][0], *const lq = &lds_q[0][0];
    uint32_t *out = a.out + 8 * i;
    for (int k = 0; k < 8; ++k) out[k] = 0u;
    out[7] = kNone;
    const QueryRay &qr = a.rays[i];
    const V3 pos = mk(qr.position[0], qr.position[1], qr.position[2]);
    const V3 dir = mk(qr.direction[0], qr.direction[1], qr.direction[2]);
    const RayX rx = make_rayx(pos, dir);
    bool in32;
    const bool walk = query_walkable(sv, 1u, pos, dir, in32);
    uint32_t flags = a.entries[i] != kNone ? kPbInTree : 0u;
    if (!walk) { out[0] = flags | kPbNoWalk; return; }
    if (!(flags & kPbInTree)) { out[0] = flags; return; }
    // the ray as the walks prepare it
    SphereRay sr;
    query_sphere_ray(sv, pos, dir, sr);
    TriFilterParams tpar;
    if (sv.bvh_flags & 2u) tri_filter_from_ray(sv, pos, dir, tpar); else tri_filter_idle(tpar);
    if (in32 || (a.form & 1u) == 0u) {
        Ray32 q0;
        make_ray32(pos, rx.dirn, (double)sv.bvh_inv_max, q0);
        Ray32S q;
        q.ix = q0.ix; q.iy = q0.iy; q.iz = q0.iz; q.nx = q0.nx; q.ny = q0.ny; q.nz = q0.nz;
        q.e = ray32_slack(q0, in32);             // 0 inside origin_limit: the bits of Ray32
        flags |= in32 ? 0u : 1u;
        pb_element(sv, a, q, sr, tpar, i, ls, lq, tid, flags, out);
    } else {
        Ray64 q;
        make_ray64(pos, rx.dirn, (double)sv.bvh_inv_max, q);
        flags |= 2u;
        pb_element(sv, a, q, sr, tpar, i, ls, lq, tid, flags, out);
    }
    out[0] = flags;
}

hipError_t launch_debug_path_bounds(const SceneView *d_sv, const PathBoundsArgs &a, hipStream_t stream)
{
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(debug_path_bounds_kernel, dim3((unsigned)((a.n + kBvhThreads - 1) / kBvhThreads)), dim3(kBvhThreads), 0, stream, d_sv, a);
    return hipGetLastError();
}
#endif  // RTX_LAB

}  // namespace rtx
