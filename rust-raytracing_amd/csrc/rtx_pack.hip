// rtx_pack.hip -- the host-only half of the API (rtx_pack.h): scene packing (Scene.objects -> per-type arrays with scene-order ids,
// the ray-independent precompute, the f32 filter records, the BVH), update planning and the host reference of the device's update
// path, digests, the invariant walk.  No HIP runtime call in this file: its object has no undefined hip* symbol.  It is a .hip file
// only so that float4 and the __host__ __device__ text of rtx_refit.h and rtx_bvh.h compile unchanged.
#include "rtx_pack.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

RTX_HOST_BEGIN

namespace {

thread_local std::string g_last_error;

// Triangles per BVH leaf (RTX_TUNE_TRI_LEAF_SHIFT bits of RtxConfig.tuning: 1..6 -- a leaf must fit the walk's 6-entry
// candidate queue, or every visit of it ends in the exhaustive sweep).  A tree of (x, y) footprints alone (`plain`: C3, C5)
// gets 5: a packet tests a leaf's records for 64 rays at once and the regrouping kernel's leaf half reads one leaf per lane
// per iteration (rtx_mesh_step.h), so fewer, fuller leaves pay.  Measured, C3 1080p x 8 / C5 band x 4 in ms, the wavefront
// form | the regrouping kernel alone:  3: 41.7 / 59.5 | 79.8 / 75.2,  4: 39.5 / 56.4 | 76.5 / 72.3,  5: 38.0 / 55.2 | 77.4 / 72.1,
// 6: 38.6 / 56.6 | 78.9 / 74.0  (2, before the step was split: 53.2 / 72.6 | 99.2 / 94.7).  A joint tree keeps 2 (240k axis-aligned
// faces: 222 ms at 2, 242 at 4).
uint32_t tri_leaf_size(bool plain, uint32_t tuning)
{
    const uint32_t t = (tuning >> RTX_TUNE_TRI_LEAF_SHIFT) & 15u;
    const uint32_t v = t ? t : (plain ? 5u : 2u);
    return v > kQNodeLeafMax ? kQNodeLeafMax : v;
}

}  // namespace

int32_t fail(RtxStatus st, const std::string &msg)
{
    g_last_error = msg;
    return (int32_t)st;
}

const std::string &last_error() { return g_last_error; }

bool debug_prints()
{
    static const bool on = std::getenv("RTX_HIP_DEBUG") != nullptr;      // diagnostics on stderr only; changes no result
    return on;
}

TriClass classify_triangle(const TriX &t, const double geom[9], const double centre[3])
{
    TriClass c{kTriNone, 2};
    if (t.degenerate) return c;                                       // Triangle::contains is always false (triangle.rs:64,83)
    const double kabs = dot(t.n, t.v0);
    if (!std::isfinite(kabs) || !std::isfinite(t.n.x) || !std::isfinite(t.n.y) || !std::isfinite(t.n.z))
        return c;                                                     // NaN normal: every comparison of the exact test fails
    if (kabs < -(1.0 + 1e-9)) return c;                               // n.(v0 - dir) < 0 for every unit dir (triangle.rs:115)
    c.cls = kTriAlways;
    double v[3][3];
    bool finite = true;
    for (int k = 0; k < 9; ++k) { v[k / 3][k % 3] = geom[k] - centre[k % 3]; finite = finite && std::isfinite(geom[k]); }
    const int free_axis = 3 - (int)t.i - (int)t.j;                    // t.i != t.j: the two rows the elimination reads
    const int a0 = free_axis == 0 ? 1 : 0, a1 = free_axis == 2 ? 1 : 2;
    const double r0 = v[1][a0] - v[0][a0], r1 = v[1][a1] - v[0][a1], s0 = v[2][a0] - v[0][a0], s1 = v[2][a1] - v[0][a1];
    const double det = r0 * s1 - r1 * s0;
    if (finite && t.i != t.j && std::fabs(det) > 1e-6 * std::hypot(r0, r1) * std::hypot(s0, s1)) { c.cls = kTriQualified; c.free_axis = (uint8_t)free_axis; }
    return c;
}

int32_t pack_scene(const RtxScene *scene, PackedScene &p)
{
    const uint64_t n = scene->n_objects;
    std::vector<SphereX> &spheres = p.spheres; std::vector<uint32_t> &sphere_id = p.sphere_id;
    std::vector<PlaneX> &planes = p.planes; std::vector<TriX> &tris = p.tris;
    std::vector<MaterialX> &mats = p.mats;
    mats.assign(n, MaterialX());
    double lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (uint64_t k = 0; k < n; ++k) {
        const RtxObject &o = scene->objects[k];
        mats[k].base_color = mk(o.base_color[0], o.base_color[1], o.base_color[2]);
        mats[k].emission_color = mk(o.emission_color[0], o.emission_color[1], o.emission_color[2]);
        mats[k].roughness = o.roughness;
        switch (o.kind) {
            case RTX_SPHERE:
                spheres.push_back(make_sphere(o.geom));
                sphere_id.push_back((uint32_t)k);
                for (int c = 0; c < 3; ++c) {
                    if (std::isfinite(o.geom[c])) { lo[c] = std::fmin(lo[c], o.geom[c]); hi[c] = std::fmax(hi[c], o.geom[c]); }
                }
                break;
            case RTX_PLANE: planes.push_back(make_plane(o.geom, (uint32_t)k)); break;
            case RTX_TRIANGLE:
                tris.push_back(make_triangle(o.geom, (uint32_t)k));
                for (int c = 0; c < 9; ++c)
                    if (std::isfinite(o.geom[c])) { lo[c % 3] = std::fmin(lo[c % 3], o.geom[c]); hi[c % 3] = std::fmax(hi[c % 3], o.geom[c]); }
                break;
            default:
                return fail(RTX_ERR_UNSUPPORTED, "object " + std::to_string(k) + ": kind " + std::to_string(o.kind) +
                                                     " has no device primitive (user CustomShape impls cannot run on the GPU)");
        }
    }
    // f32 filter records, relative to the centre of the spheres' bounding box, pair-interleaved for
    // v_pk_fma_f32: record 2k = {x[2k], x[2k+1], y[2k], y[2k+1]}, record 2k+1 = {z.., w..}, w = |c|^2 - r^2;
    // padded to a multiple of 4 spheres with a sentinel that never passes (w = 1e30)
    const size_t ns4 = (spheres.size() + 3) & ~(size_t)3;
    std::vector<float4> &sph32 = p.sph32;
    sph32.assign(ns4, make_float4(0.f, 0.f, 0.f, 0.f));
    std::vector<float> fx(ns4, 0.f), fy(ns4, 0.f), fz(ns4, 0.f), fw(ns4, 1.0e30f);
    double centre[3] = { 0, 0, 0 };
    for (int c = 0; c < 3; ++c) if (lo[c] <= hi[c]) centre[c] = 0.5 * (lo[c] + hi[c]);
    double cmax = 0.0;
    for (size_t k = 0; k < spheres.size(); ++k) {
        const RtxObject &o = scene->objects[sphere_id[k]];
        double cx = o.geom[0] - centre[0], cy = o.geom[1] - centre[1], cz = o.geom[2] - centre[2];
        double cc = cx * cx + cy * cy + cz * cz;
        double reach = std::sqrt(cc) + std::fabs(o.geom[3]);
        if (!(reach <= cmax)) cmax = reach;                   // NaN/inf propagate: every ray then takes the exact sweep
        fx[k] = (float)cx; fy[k] = (float)cy; fz[k] = (float)cz; fw[k] = (float)(cc - spheres[k].rr);
    }
    if (!(cmax < 1.0e14)) {
        // non-finite or enormous sphere data: the f32 records cannot represent it.  Every record becomes
        // "always a candidate" (w = -1e30), so every ray overflows its queue and takes the exact f64 sweep.
        for (size_t k = 0; k < ns4; ++k) { fx[k] = fy[k] = fz[k] = 0.f; fw[k] = -1.0e30f; }
    }
    for (size_t k = 0; k < ns4; k += 2) {
        sph32[k] = make_float4(fx[k], fx[k + 1], fy[k], fy[k + 1]);
        sph32[k + 1] = make_float4(fz[k], fz[k + 1], fw[k], fw[k + 1]);
    }
    // triangle filter records (rtx_device.h "triangle filter"): only triangles that can be hit at all.  Triangle::contains
    // decides a hit from two coordinates of the hit point -- rows (i, j) of its elimination: (x, y) unless a zero pivot
    // swaps another row in (triangle.rs:60-71,81-87; e.g. every face in a plane x = const is solved in (y, z)) -- so the
    // triangle enters the tree with its footprint in THAT coordinate plane, unbounded along the third axis (rtx_bvh.h).
    // Triangles solved in (x, y) also get a real filter record; the others a pass-all record (their leaf box already
    // says "the ray passes over the footprint").  An ill-conditioned projection (the rounding of a, b could report a
    // hit outside the footprint) keeps a triangle outside the tree: tested for every segment.
    struct TriRec { float4 A, B, g0, g1; uint32_t tri; };
    std::vector<TriRec> tree_recs[3], always_recs;                     // tree_recs[f]: the elimination does not read axis f
    std::vector<BvhBox> tri_boxes[3];
    double tri_extent = 0.0;
    p.tri_class.assign(tris.size(), (uint8_t)kTriNone);
    p.tri_axis.assign(tris.size(), (uint8_t)2);
    for (size_t k = 0; k < tris.size(); ++k) {
        const TriX &t = tris[k];
        const RtxObject &o = scene->objects[t.id];
        const TriClass tc = classify_triangle(t, o.geom, centre);
        p.tri_class[k] = tc.cls; p.tri_axis[k] = tc.free_axis;
        if (tc.cls == kTriNone) continue;
        const double kabs = dot(t.n, t.v0);
        double v[3][3];
        for (int c = 0; c < 9; ++c) v[c / 3][c % 3] = o.geom[c] - centre[c % 3];
        const int free_axis = 3 - (int)t.i - (int)t.j;                // t.i != t.j: the two rows the elimination reads
        const int a0 = free_axis == 0 ? 1 : 0, a1 = free_axis == 2 ? 1 : 2;
        const double r0 = v[1][a0] - v[0][a0], r1 = v[1][a1] - v[0][a1], s0 = v[2][a0] - v[0][a0], s1 = v[2][a1] - v[0][a1];
        const double det = r0 * s1 - r1 * s0;
        BvhBox fp;
        const bool in_tree = tc.cls == kTriQualified && triangle_footprint(o.geom, fp, free_axis);
        TriRec rec;
        rec.A = make_float4(0.f, 0.f, 0.f, 0.f);                       // "always a candidate"
        rec.B = make_float4(0.f, 0.f, 0.f, 0.f);
        rec.g0 = make_float4(0.f, 0.f, 0.f, 0.f);
        rec.g1 = make_float4(0.f, 0.f, NAN, 0.f);                      // n.v0 = NaN: no f32 bounds for this record (outside the tree)
        rec.tri = (uint32_t)k;
        if (in_tree) {
            // (a, b) = M (q - v0)_uv with M the inverse of [r s] in the two rows Triangle::contains' elimination reads
            // (triangle.rs:55-100; (u, v) = (x, y), (x, z) or (y, z)); n.v0 in absolute coordinates for the cull test
            // (triangle.rs:115); the plane's code for tri_bounds (rtx_mesh_step.h)
            const double m00 = s1 / det, m01 = -s0 / det, m10 = -r1 / det, m11 = r0 / det;
            const double kc = t.n.x * v[0][0] + t.n.y * v[0][1] + t.n.z * v[0][2];
            rec.g0 = make_float4((float)v[0][a0], (float)v[0][a1], (float)m00, (float)m01);
            rec.g1 = make_float4((float)m10, (float)m11, (float)kabs, (float)(2 - free_axis));
            rec.A = make_float4((float)t.n.x, (float)t.n.y, (float)t.n.z, (float)kc);
            rec.B = make_float4(0.f, 0.f, 1.0e30f, 1.0e30f);           // no (x, y) rectangle to test: every ray passes the footprint filter
            for (int c = 0; c < 9; ++c) tri_extent = std::fmax(tri_extent, std::fabs(v[c / 3][c % 3]));
        }
        if (in_tree && free_axis == 2) {
            const double xlo = std::fmin(v[0][0], std::fmin(v[1][0], v[2][0])), xhi = std::fmax(v[0][0], std::fmax(v[1][0], v[2][0]));
            const double ylo = std::fmin(v[0][1], std::fmin(v[1][1], v[2][1])), yhi = std::fmax(v[0][1], std::fmax(v[1][1], v[2][1]));
            const double grow = 1.0 + 1.0 / 1048576.0;
            rec.B = make_float4((float)(0.5 * (xlo + xhi)), (float)(0.5 * (ylo + yhi)),
                                round_up_f32(0.5 * (xhi - xlo) * grow + 1e-30), round_up_f32(0.5 * (yhi - ylo) * grow + 1e-30));
        }
        if (in_tree) { tree_recs[free_axis].push_back(rec); tri_boxes[free_axis].push_back(fp); }
        else always_recs.push_back(rec);
    }
    // a plane with fewer than 5 triangles gets no sub-tree: those are tested for every segment ((x, y) ones keep their
    // filter record, which is valid outside the tree too)
    std::vector<TriRec> demoted;
    for (int f = 0; f < 3; ++f)
        if (tree_recs[f].size() <= 4) {
            for (const TriRec &r : tree_recs[f]) (f == 2 ? demoted : always_recs).push_back(r);
            tree_recs[f].clear(); tri_boxes[f].clear();
        }

    // flat BVH over the sphere boxes and the triangle footprints (rtx_bvh.h); fewer than 5 spheres, or non-finite
    // spheres, get no sub-tree (the BVH kernel then tests those shapes for every segment)
    std::vector<BvhBox> sphere_boxes(spheres.size());
    bool spheres_finite = true;
    for (size_t k = 0; k < spheres.size() && spheres_finite; ++k)
        spheres_finite = sphere_box(scene->objects[sphere_id[k]].geom, sphere_boxes[k]);
    if (!spheres_finite || sphere_boxes.size() <= 4) sphere_boxes.clear();
    const bool use_sah = (scene->config.tuning & RTX_TUNE_BVH_MEDIAN) == 0u;
    BvhBuild &bvh = p.bvh;
    const bool plain_tree = sphere_boxes.empty() && tri_boxes[0].empty() && tri_boxes[1].empty();   // (x, y) footprints alone (free axis 2)
    bvh = build_bvh(sphere_boxes, tri_boxes, tri_leaf_size(plain_tree, scene->config.tuning), use_sah);
    Bvh4Build &bvh4 = p.bvh4;
    bvh4 = collapse_to_bvh4(bvh);

    // records in leaf order first (a triangle leaf's link indexes them; tri_order indexes [plane xy][xz][yz]), then the
    // ones outside the tree
    std::vector<float4> &tri32 = p.tri32;
    std::vector<uint32_t> &tri_fidx = p.tri_fidx;
    std::vector<TriRec> all_tree;
    std::vector<uint8_t> all_free;
    for (int f = 2; f >= 0; --f)
        for (const TriRec &r : tree_recs[f]) { all_tree.push_back(r); all_free.push_back((uint8_t)f); }
    tri32.reserve(2 * (all_tree.size() + demoted.size() + always_recs.size()) + 2);
    p.tri_rec_free_axis.clear();
    size_t n_in_tree = 0;
    if (bvh.has_tris) {
        for (uint32_t idx : bvh.tri_order) {
            const TriRec &r = all_tree[idx];
            tri32.push_back(r.A); tri32.push_back(r.B); tri_fidx.push_back(r.tri); p.tri_rec_free_axis.push_back(all_free[idx]);
            p.tri_geo.push_back(r.g0); p.tri_geo.push_back(r.g1);
        }
        n_in_tree = bvh.tri_order.size();
    } else {                                    // (the build was refused: coordinates too large for the f32 slab test)
        for (size_t k = 0; k < all_tree.size(); ++k) (all_free[k] == 2 ? demoted : always_recs).push_back(all_tree[k]);
    }
    p.sv.n_tri_tree = (uint32_t)n_in_tree;
    for (const TriRec &r : demoted) { tri32.push_back(r.A); tri32.push_back(r.B); tri_fidx.push_back(r.tri); }
    for (const TriRec &r : always_recs) { tri32.push_back(r.A); tri32.push_back(r.B); tri_fidx.push_back(r.tri); }
    if (!tri32.empty()) {                       // one pad record (a walk may read records in pairs)
        tri32.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
        tri32.push_back(make_float4(0.f, 0.f, 0.f, 0.f));
    }
    p.sv.n_tri_filter = (uint32_t)tri_fidx.size();
    p.sv.tri_extent = tri_extent;
    p.sv.n_objects = (uint32_t)n;
    p.sv.n_spheres = (uint32_t)spheres.size();
    p.sv.n_planes = (uint32_t)planes.size();
    p.sv.n_tris = (uint32_t)tris.size();
    for (int c = 0; c < 3; ++c) p.sv.sphere_center[c] = centre[c];
    p.sv.sphere_cmax = cmax;

    p.sv.n_bvh_nodes = (uint32_t)bvh4.nodes.size();
    p.sv.bvh_depth = (uint32_t)bvh4.depth;
    p.sv.bvh_root = bvh4.root;
    p.sv.bvh_origin_limit = (float)bvh.origin_limit;
    p.sv.bvh_inv_max = (float)std::fmin(1.0e30, 1.0e37 / std::fmax(bvh.origin_limit, 1.0));     // |o * inv|, |b * inv| stay finite in f32
    p.sv.bvh_flags = (bvh.has_spheres ? 1u : 0u) | (bvh.has_tris ? 2u : 0u) |
                     (bvh.has_tris && !bvh.has_spheres && tree_recs[1].empty() && tree_recs[0].empty() ? 4u : 0u);
    if ((p.sv.bvh_flags & 4u) && build_qnodes(bvh4, p.qnodes)) p.sv.bvh_flags |= 8u;
    else p.qnodes.clear();
#ifndef RTX_LAB
    // the product library holds the pure-footprint kernels in their 64-byte-node instances only: a tree whose nodes have no such
    // form (coordinates beyond the quantisation's range) walks as a joint tree, which takes any node
    if ((p.sv.bvh_flags & 12u) == 4u) p.sv.bvh_flags &= ~4u;
#endif
    if ((p.sv.bvh_flags & 3u) == 1u && build_q3nodes(bvh4, bvh.abs_pad, p.q3nodes)) p.sv.bvh_flags |= 16u;     // spheres only
    else p.q3nodes.clear();
    if (debug_prints())
        std::fprintf(stderr, "[rtx_hip] upload: %zu spheres, %zu triangles (%zu in the tree: %zu xy / %zu xz / %zu yz footprints, %zu tested per segment), bvh: %zu binary nodes, %zu wide nodes, depth %d\n",
                     spheres.size(), tris.size(), n_in_tree, tree_recs[2].size(), tree_recs[1].size(), tree_recs[0].size(),
                     demoted.size() + always_recs.size(), bvh.nodes.size(), bvh4.nodes.size(), bvh4.depth);
    std::vector<float4> &leaf32 = p.leaf32;
    leaf32.assign(bvh.prims.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t k = 0; k < bvh.prims.size(); ++k) {
        const uint32_t p = bvh.prims[k];
        leaf32[k] = make_float4(fx[p], fy[p], fz[p], fw[p]);
    }
    // the spheres kernel's leaf record {c - centre, |r|} (sphere.rs:24 squares the radius: its sign does not matter);
    // |r| rounded up, which only adds candidates
    p.leaf_cr.assign(bvh.prims.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t k = 0; k < bvh.prims.size(); ++k) {
        const uint32_t q = bvh.prims[k];
        p.leaf_cr[k] = make_float4(fx[q], fy[q], fz[q], round_up_f32(std::fabs(scene->objects[sphere_id[q]].geom[3])));
    }

    return RTX_OK;
}

RefitTables make_refit_tables(const PackedScene &p)
{
    RefitTables t;
    t.abs_pad = p.bvh.abs_pad;
    t.scale = p.bvh.origin_limit > 0.0 ? (p.bvh.origin_limit - 1.0) / 4.0 : -1.0;
    for (int c = 0; c < 3; ++c) t.centre[c] = p.sv.sphere_center[c];
    t.sphere_tree = (p.sv.bvh_flags & 1u) != 0u;
    t.local.assign(p.mats.size(), 0u);
    for (size_t k = 0; k < p.sphere_id.size(); ++k) t.local[p.sphere_id[k]] = (uint32_t)k;
    for (size_t k = 0; k < p.planes.size(); ++k) t.local[p.planes[k].id] = (uint32_t)k;
    for (size_t k = 0; k < p.tris.size(); ++k) t.local[p.tris[k].id] = (uint32_t)k;
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    t.tri_class = p.tri_class; t.tri_axis = p.tri_axis;
    t.tri_rec.assign(p.tris.size(), kNoSlot);
    for (size_t r = 0; r < p.tri_fidx.size(); ++r) t.tri_rec[p.tri_fidx[r]] = (uint32_t)r;
    t.n_tri_tree = p.sv.n_tri_tree;
    if (t.n_tri_tree) {                                       // every wide node by depth (the sphere-only list below stops at footprint links)
        std::vector<uint32_t> cur, next;
        cur.push_back(p.bvh4.root);
        t.all_level_begin.push_back(0u);
        while (!cur.empty()) {
            next.clear();
            for (uint32_t entry : cur) {
                t.all_level_nodes.push_back(entry);
                const Bvh4Node &w = p.bvh4.nodes[entry & ~kBvhFlatNode];
                const float lk[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, ct[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
                for (int c = 0; c < 4; ++c) {
                    const bool flat = (entry & kBvhFlatNode) != 0u;
                    const uint32_t link = bits(flat ? lk[c] : w.a[c].w), count = bits(flat ? ct[c] : w.b[c].w);
                    if (count == 0u) next.push_back(flat ? (link | kBvhFlatNode) : link);
                }
            }
            t.all_level_begin.push_back((uint32_t)t.all_level_nodes.size());
            cur.swap(next);
        }
    }
    if (!t.sphere_tree) return t;
    t.slot.assign(p.spheres.size(), kNoSlot);
    for (size_t k = 0; k < p.bvh.prims.size(); ++k) t.slot[p.bvh.prims[k]] = (uint32_t)k;
    std::vector<uint32_t> cur, next;
    if (!(p.bvh4.root & kBvhFlatNode)) cur.push_back(0u);
    t.level_begin.push_back(0u);
    while (!cur.empty()) {
        next.clear();
        for (uint32_t idx : cur) {
            t.level_nodes.push_back(idx);
            const Bvh4Node &w = p.bvh4.nodes[idx];
            for (int c = 0; c < 4; ++c)
                if (bits(w.b[c].w) == 0u && !(bits(w.a[c].w) & kBvhFlatNode)) next.push_back(bits(w.a[c].w));
        }
        t.level_begin.push_back((uint32_t)t.level_nodes.size());
        cur.swap(next);
    }
    return t;
}

// ---- rtx_scene_update_objects: what the host decides (no HIP call: rtx_debug_host_refit runs it without a GPU) -------------------

// Validates (nothing is written before every entry passed), removes duplicates and chooses the path (include/rtx_hip.h, "Which path
// runs").  `cur` is the resident object list, `cmax` the resident sphere_cmax.  Every scene-wide constant of pack_scene either stays a
// valid bound under REFIT / RECORDS or sends the update to REBUILT:
//   sphere_center   kept: the f32 records are offsets from ANY fixed point; what depends on it is sphere_cmax, which mode C recomputes
//                   against the kept centre, and the < 1e14 limit of pack_scene, which every new reach is held to here
//   origin_limit, abs_pad, bvh_inv_max   functions of `scale`: a new box beyond it rebuilds
//   tri_extent, the triangle records     under AUTO triangle geometry never changes here (it rebuilds).  Under RTX_UPDATE_DEFORM a triangle
//                   that keeps its class and free axis (classify_triangle: the decision pack_scene takes) is rewritten against the kept
//                   centre and mode D takes tri_extent again; the class rule keeps tri_fidx, the leaf order and which records are real
//   bvh_depth, bvh_flags, the topology   the tree keeps its shape; a sphere that turns non-finite (it would leave the tree) rebuilds
// What one shape's NEW geometry `o.geom` means for an entry of the resident kind (the per-shape half of "Which path runs", shared by
// plan_update and plan_visibility, which shows an object with the geometry it has now): fills e.slot / e.tri and the plan's flags,
// raises `rebuild` when the geometry cannot be written in place, `refit` when boxes above it change.
static void plan_shape(const RefitTables &t, uint32_t mode, const RtxObject &o, UpdateEntry &e, UpdatePlan &plan, bool &rebuild, bool &refit)
{
    if (o.kind == RTX_TRIANGLE) {
        bool finite = true;
        for (int c = 0; c < 9; ++c) finite = finite && std::isfinite(o.geom[c]);
        const uint32_t k = e.local;
        TriClass tc{kTriNone, 2};
        if (mode == RTX_UPDATE_DEFORM && finite) tc = classify_triangle(make_triangle(o.geom, e.object), o.geom, t.centre);
        if (mode != RTX_UPDATE_DEFORM || !finite || tc.cls != t.tri_class[k] || (tc.cls == kTriQualified && tc.free_axis != t.tri_axis[k]))
            rebuild = true;                                   // AUTO: always, as ever; DEFORM: the class or the free axis changes
        else {
            plan.tri_geom = true;
            e.tri = kTriEntryGeom; e.slot = t.tri_rec[k];
            if (tc.cls == kTriQualified) {
                e.tri |= kTriEntryQualified | ((uint32_t)tc.free_axis << kTriEntryAxisShift);
                plan.any_tri = true;
                BvhBox fp;
                if (!triangle_footprint(o.geom, fp, tc.free_axis)) rebuild = true;
                else if (t.scale >= 0.0)
                    for (int a = 0; a < 3; ++a)
                        if (a != tc.free_axis && (std::fabs(fp.lo[a]) > t.scale || std::fabs(fp.hi[a]) > t.scale)) rebuild = true;
                if (e.slot < t.n_tri_tree) { e.tri |= kTriEntryTree; plan.tri_refit = true; refit = true; }
            }
        }
    } else if (o.kind == RTX_SPHERE) {
        plan.any_sphere = true;
        BvhBox b;
        if (!sphere_box(o.geom, b)) rebuild = true;
        else {
            if (t.scale >= 0.0)
                for (int a = 0; a < 3; ++a) if (std::fabs(b.lo[a]) > t.scale || std::fabs(b.hi[a]) > t.scale) rebuild = true;
            const double cx = o.geom[0] - t.centre[0], cy = o.geom[1] - t.centre[1], cz = o.geom[2] - t.centre[2];
            if (!(std::sqrt(cx * cx + cy * cy + cz * cz) + std::fabs(o.geom[3]) < 1.0e14)) rebuild = true;
        }
        if (t.sphere_tree) { e.slot = t.slot[e.local]; refit = true; }
    }
}

// `hidden` (null: nothing is): the handle's visibility bytes.  An entry for a hidden object updates the host's object and the material
// record alone (kEntryNoGeom); its geometry is judged when the object is shown (plan_visibility).  A kind change rebuilds as ever.
int32_t plan_update(const std::vector<RtxObject> &cur, const RefitTables &t, double cmax, const uint64_t *indices, const RtxObject *objects,
                    uint64_t n, uint32_t mode, UpdatePlan &plan, const uint8_t *hidden)
{
    plan = UpdatePlan();
    if (mode != RTX_UPDATE_AUTO && mode != RTX_UPDATE_REBUILD && mode != RTX_UPDATE_DEFORM) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_update_objects: unknown mode");
    if (n == 0) return RTX_OK;
    if (!indices || !objects) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_update_objects: null argument");
    for (uint64_t i = 0; i < n; ++i) {
        if (indices[i] >= cur.size())
            return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_update_objects: index " + std::to_string(indices[i]) + " is not below n_objects");
        if (objects[i].kind > RTX_TRIANGLE)
            return fail(RTX_ERR_UNSUPPORTED, "rtx_scene_update_objects: entry " + std::to_string(i) + ": kind " + std::to_string(objects[i].kind) +
                                                 " has no device primitive");
        if (objects[i].reserved != 0u) return fail(RTX_ERR_UNSUPPORTED, "rtx_scene_update_objects: entry " + std::to_string(i) + ": reserved is not zero");
    }
    std::vector<uint8_t> seen(cur.size(), 0);
    plan.entries.reserve((size_t)std::min<uint64_t>(n, cur.size()));
    bool rebuild = mode == RTX_UPDATE_REBUILD || !(cmax < 1.0e14);
    bool refit = false;
    for (uint64_t i = n; i-- > 0;) {
        const uint64_t idx = indices[i];
        if (seen[idx]) continue;
        seen[idx] = 1;
        const RtxObject &o = objects[i];
        UpdateEntry e;
        std::memset(&e, 0, sizeof e);
        e.object = (uint32_t)idx; e.local = t.local[idx]; e.slot = kNoSlot;
        static_assert(sizeof(RtxObject) == 136 && offsetof(UpdateEntry, kind) == 16, "UpdateEntry carries an RtxObject");
        std::memcpy(&e.kind, &o, sizeof o);
        if (o.kind != cur[idx].kind) rebuild = true;
        else if (hidden && hidden[idx]) e.tri = kEntryNoGeom;
        else if (o.kind == RTX_TRIANGLE) {
            if (std::memcmp(o.geom, cur[idx].geom, sizeof o.geom) != 0) plan_shape(t, mode, o, e, plan, rebuild, refit);      // (same geometry: a material update)
        } else if (o.kind == RTX_SPHERE && std::memcmp(o.geom, cur[idx].geom, 4 * sizeof(double)) != 0)                       // (likewise)
            plan_shape(t, mode, o, e, plan, rebuild, refit);
        plan.entries.push_back(e);
    }
    plan.how = rebuild ? RTX_UPDATED_REBUILT : (refit ? RTX_UPDATED_REFIT : RTX_UPDATED_RECORDS);
    return RTX_OK;
}

// rtx_scene_set_visible: what the host decides (no HIP call).  `hidden` holds the handle's bytes (1: hidden) and is NOT changed: the
// caller flips the bytes of plan.entries after the plan ran.  Entries already in the requested state are dropped; a hide entry names
// the records hide_record rewrites; a show entry is plan_shape's entry for the object's current geometry under RTX_UPDATE_DEFORM's
// rules (a plane: its record alone).  REFIT when a changed shape has a slot in the tree, REBUILT when a shown shape's geometry cannot be
// taken in place (the resident class, axis and range are those of the pack, which packed the object's real geometry of that time).
int32_t plan_visibility(const std::vector<RtxObject> &cur, const std::vector<uint8_t> &hidden, const RefitTables &t, double cmax,
                        const uint64_t *indices, uint64_t n, uint32_t visible, UpdatePlan &plan)
{
    plan = UpdatePlan();
    if (visible > 1u) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_visible: visible is neither 0 nor 1");
    if (n == 0) return RTX_OK;
    if (!indices) return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_visible: null indices");
    for (uint64_t i = 0; i < n; ++i)
        if (indices[i] >= cur.size())
            return fail(RTX_ERR_INVALID_ARGUMENT, "rtx_scene_set_visible: index " + std::to_string(indices[i]) + " is not below n_objects");
    std::vector<uint8_t> seen(cur.size(), 0);
    bool rebuild = false, refit = false;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t idx = indices[i];
        if (seen[idx] || (hidden[idx] != 0) == (visible == 0u)) continue;
        seen[idx] = 1;
        const RtxObject &o = cur[idx];
        UpdateEntry e;
        std::memset(&e, 0, sizeof e);
        e.object = (uint32_t)idx; e.local = t.local[idx]; e.slot = kNoSlot;
        std::memcpy(&e.kind, &o, sizeof o);
        if (visible) plan_shape(t, RTX_UPDATE_DEFORM, o, e, plan, rebuild, refit);
        else {
            e.tri = kEntryHide;
            if (o.kind == RTX_SPHERE) {
                plan.any_sphere = true;
                if (t.sphere_tree) { e.slot = t.slot[e.local]; refit = true; }
            } else if (o.kind == RTX_TRIANGLE) {
                plan.tri_geom = true;
                e.slot = t.tri_rec[e.local];
                if (t.tri_class[e.local] == kTriQualified) plan.any_tri = true;
                if (e.slot < t.n_tri_tree) { e.tri |= kTriEntryTree; plan.tri_refit = true; refit = true; }
            }
        }
        plan.entries.push_back(e);
    }
    if (plan.entries.empty()) return RTX_OK;
    plan.visibility = true;
    if (!(cmax < 1.0e14)) rebuild = true;                     // (plan_update's rule: the resident f32 sphere records are not real ones)
    plan.how = rebuild ? RTX_UPDATED_REBUILT : (refit ? RTX_UPDATED_REFIT : RTX_UPDATED_RECORDS);
    return RTX_OK;
}

// box32 / reach of every sphere of `objects` (what mode B and mode C read for the spheres an update does not name).
void derive_all_spheres(const RtxObject *objects, size_t n_objects, const RefitTables &t, size_t n_spheres, std::vector<float> &box32,
                        std::vector<double> &reach, const uint8_t *hidden)
{
    box32.assign(n_spheres * 6, 0.f);
    reach.assign(n_spheres, 0.0);
    for (size_t k = 0; k < n_objects; ++k) {
        if (objects[k].kind != RTX_SPHERE) continue;
        const size_t q = t.local[k];
        if (hidden && hidden[k]) {                            // hide_record's rows: the nothing box, reach 0
            for (int a = 0; a < 3; ++a) { box32[6 * q + a] = INFINITY; box32[6 * q + 3 + a] = -INFINITY; }
            continue;
        }
        const SphereDerived d = derive_sphere(objects[k].geom, t.centre, t.abs_pad);
        for (int a = 0; a < 3; ++a) { box32[6 * q + a] = d.lo[a]; box32[6 * q + 3 + a] = d.hi[a]; }
        reach[q] = d.reach;
    }
}

// tribox32 (per tree record) / tri_reach (per triangle) of every triangle of `objects`: what modes B and D read for the triangles an
// update does not name.
void derive_all_triangles(const RtxObject *objects, size_t n_objects, const RefitTables &t, std::vector<float> &tribox32, std::vector<double> &tri_reach,
                          const uint8_t *hidden)
{
    tribox32.assign((size_t)t.n_tri_tree * 6, 0.f);
    tri_reach.assign(t.tri_class.size(), 0.0);
    for (size_t k = 0; k < n_objects; ++k) {
        if (objects[k].kind != RTX_TRIANGLE) continue;
        const uint32_t q = t.local[k];
        if (t.tri_class[q] != kTriQualified) continue;
        if (hidden && hidden[k]) {                            // hide_record's rows
            if (t.tri_rec[q] < t.n_tri_tree) for (int a = 0; a < 3; ++a) { tribox32[(size_t)t.tri_rec[q] * 6 + a] = INFINITY; tribox32[(size_t)t.tri_rec[q] * 6 + 3 + a] = -INFINITY; }
            continue;
        }
        const TriDerived d = derive_triangle(objects[k].geom, (uint32_t)k, true, (int)t.tri_axis[q], t.centre, t.abs_pad);
        tri_reach[q] = d.reach;
        if (t.tri_rec[q] < t.n_tri_tree) for (int a = 0; a < 6; ++a) tribox32[(size_t)t.tri_rec[q] * 6 + a] = d.box[a];
    }
}

// The UpdateArgs of an update of the arrays `where` points at -- a PackedScene's vectors on the host (host_view), the resident arrays
// on the device -- with the tables of their pack; mode, n, level and status are the caller's.  The triangle half is set only when
// the plan moves a triangle; `keep` is the kept-words table, null while the pack has none.
UpdateArgs update_args(const SceneView &sv, const RefitTables &t, const UpdateEntry *entries, float *box32, double *reach, float *tribox32,
                       double *tri_reach, bool tri_geom, uint32_t *keep)
{
    UpdateArgs u{};
    u.entries = entries;
    u.spheres = const_cast<SphereX *>(sv.spheres); u.planes = const_cast<PlaneX *>(sv.planes);
    u.materials = const_cast<MaterialX *>(sv.materials);
    u.sphere_f32 = reinterpret_cast<float *>(const_cast<float4 *>(sv.sphere_f32));
    u.leaf_f32 = const_cast<float4 *>(sv.bvh_leaf_f32); u.leaf_cr = const_cast<float4 *>(sv.bvh_leaf_cr);
    u.box32 = box32; u.reach = reach;
    u.nodes = const_cast<Bvh4Node *>(sv.bvh_nodes);
    u.q3nodes = (sv.bvh_flags & 16u) ? const_cast<BvhQ3Node *>(sv.bvh_q3nodes) : nullptr;
    u.prims = sv.bvh_prims;
    for (int c = 0; c < 3; ++c) u.centre[c] = t.centre[c];
    u.abs_pad = t.abs_pad;
    u.keep = keep;
    if (keep) u.qnodes = (sv.bvh_flags & 8u) ? const_cast<BvhQNode *>(sv.bvh_qnodes) : nullptr;      // (mode E reads the links of both 64-byte forms)
    if (tri_geom) {
        u.tris = const_cast<TriX *>(sv.tris); u.tri_f32 = const_cast<float4 *>(sv.tri_f32); u.tri_geo = const_cast<float4 *>(sv.tri_geo);
        u.tribox32 = tribox32; u.tri_reach = tri_reach;
        u.qnodes = (sv.bvh_flags & 8u) ? const_cast<BvhQNode *>(sv.bvh_qnodes) : nullptr;
    }
    return u;
}

// The arrays an update writes, where a packed scene holds them: p.sv with the pointers a SceneView has on the device.
static SceneView host_view(PackedScene &p)
{
    SceneView v = p.sv;
    v.spheres = p.spheres.data(); v.planes = p.planes.data(); v.tris = p.tris.data(); v.materials = p.mats.data();
    v.sphere_f32 = p.sph32.data(); v.tri_f32 = p.tri32.data(); v.tri_geo = p.tri_geo.data();
    v.bvh_nodes = p.bvh4.nodes.data(); v.bvh_qnodes = p.qnodes.data(); v.bvh_q3nodes = p.q3nodes.data();
    v.bvh_prims = p.bvh.prims.data(); v.bvh_leaf_f32 = p.leaf32.data(); v.bvh_leaf_cr = p.leaf_cr.data();
    return v;
}

// The host reference of the device path on a packed scene: run_update's steps with rtx_refit.h's functions in place of the launches.
// Returns the status word (kUpdateStatusNoQ3 / kUpdateStatusNoQ: a 64-byte node has no encoding -- the caller rebuilds).  tribox32 /
// tri_reach are read only when the plan moves a triangle.
unsigned long long refit_packed(PackedScene &p, const RefitTables &t, const UpdatePlan &plan, std::vector<float> &box32, std::vector<double> &reach,
                                std::vector<float> &tribox32, std::vector<double> &tri_reach, std::vector<uint32_t> *keep)
{
    unsigned long long status = 0ull;
    if (keep && plan.capture) keep->assign(p.bvh4.nodes.size() * (size_t)kKeepWords, 0u);
    const UpdateArgs u = update_args(host_view(p), t, plan.entries.data(), box32.data(), reach.data(), tribox32.data(), tri_reach.data(), plan.tri_geom,
                                     keep && !keep->empty() ? keep->data() : nullptr);
    run_update(u, t, plan, t.level_nodes.data(), t.all_level_nodes.data(), p.sv.n_spheres, p.sv.n_tris, [&](const UpdateArgs &a) {
        if (a.mode == 0u) for (uint32_t i = 0; i < a.n; ++i) update_record(a, i);
        else if (a.mode == 1u) for (uint32_t k = 0; k < a.n; ++k) status |= refit_level_entry(a, a.level[k]);
        else if (a.mode == 4u) for (uint32_t k = 0; k < a.n; ++k) capture_keep(a, a.level[k]);
        else {                                                // modes C and D: the max of non-negative doubles, from 0.0
            const double *src = a.mode == 2u ? a.reach : a.tri_reach;
            double m = 0.0;
            for (uint32_t k = 0; k < a.n; ++k) m = src[k] > m ? src[k] : m;
            (a.mode == 2u ? p.sv.sphere_cmax : p.sv.tri_extent) = m;
        }
        return true;
    });
    return status;
}

// FNV-1a-64 digests of a scene's arrays, in the order of rtx_debug_host_refit: nodes, 64-byte sphere nodes, leaf records (bvh_leaf_f32
// then bvh_leaf_cr), sphere_f32, spheres, planes, materials, the bits of sphere_cmax.
static uint64_t fnv1a(uint64_t h, const void *data, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(data);
    for (size_t k = 0; k < bytes; ++k) { h ^= b[k]; h *= 0x100000001B3ull; }
    return h;
}
static constexpr uint64_t kFnvBasis = 0xCBF29CE484222325ull;

void digest_packed(const PackedScene &p, uint64_t *digests)
{
    digests[0] = fnv1a(kFnvBasis, p.bvh4.nodes.data(), p.bvh4.nodes.size() * sizeof(Bvh4Node));
    digests[1] = fnv1a(kFnvBasis, p.q3nodes.data(), p.q3nodes.size() * sizeof(BvhQ3Node));
    digests[2] = fnv1a(fnv1a(kFnvBasis, p.leaf32.data(), p.leaf32.size() * sizeof(float4)), p.leaf_cr.data(), p.leaf_cr.size() * sizeof(float4));
    digests[3] = fnv1a(kFnvBasis, p.sph32.data(), p.sph32.size() * sizeof(float4));
    digests[4] = fnv1a(kFnvBasis, p.spheres.data(), p.spheres.size() * sizeof(SphereX));
    digests[5] = fnv1a(kFnvBasis, p.planes.data(), p.planes.size() * sizeof(PlaneX));
    digests[6] = fnv1a(kFnvBasis, p.mats.data(), p.mats.size() * sizeof(MaterialX));
    digests[7] = fnv1a(kFnvBasis, &p.sv.sphere_cmax, sizeof(double));
}

// digest_packed, then (rtx_debug_host_refit_mesh) the triangle records, tri_f32, tri_geo, the 64-byte footprint nodes, the bits of tri_extent.
void digest_packed_mesh(const PackedScene &p, uint64_t *digests)
{
    digest_packed(p, digests);
    digests[8] = fnv1a(kFnvBasis, p.tris.data(), p.tris.size() * sizeof(TriX));
    digests[9] = fnv1a(kFnvBasis, p.tri32.data(), p.tri32.size() * sizeof(float4));
    digests[10] = fnv1a(kFnvBasis, p.tri_geo.data(), p.tri_geo.size() * sizeof(float4));
    digests[11] = fnv1a(kFnvBasis, p.qnodes.data(), p.qnodes.size() * sizeof(BvhQNode));
    digests[12] = fnv1a(kFnvBasis, &p.sv.tri_extent, sizeof(double));
    digests[13] = digests[14] = digests[15] = 0;
}

// The invariant walk of rtx_debug_host_scene / rtx_debug_host_refit over a packed scene and the object list it stands for: every
// shape's box inside its leaf child's box, every child inside its parent's, every 64-byte node's decoded child box around the
// 128-byte child's.  `stats`: include/rtx_hip.h, rtx_debug_host_scene.
// `hidden` (null: nothing is; rtx_scene_set_visible): a hidden shape needs no containing box and may lie under an empty slot; every
// VISIBLE shape of the tree is still found in exactly one leaf, inside its box.  Nodes below an empty slot are not reached, so the
// depth and "every node is reached" are then not held.
int32_t check_packed(const PackedScene &p, const RtxObject *objects, uint64_t *stats, const uint8_t *hidden)
{
    for (int k = 0; k < 16; ++k) stats[k] = 0;
    stats[0] = p.spheres.size(); stats[1] = p.tris.size(); stats[2] = p.sv.n_tri_filter; stats[3] = p.sv.n_tri_tree;
    stats[4] = p.bvh4.nodes.size(); stats[5] = (uint64_t)p.bvh4.depth; stats[6] = p.bvh.nodes.size(); stats[7] = p.sv.bvh_flags;
    stats[12] = 3ull * (uint64_t)p.bvh4.depth + 2ull;
    if (p.bvh4.nodes.empty()) return RTX_OK;

    struct Box { float lo[3], hi[3]; };
    auto inside = [](const Box &c, const Box &o) {
        for (int a = 0; a < 3; ++a) if (!(c.lo[a] >= o.lo[a] && c.hi[a] <= o.hi[a])) return false;
        return true;
    };
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
    const size_t n_nodes = p.bvh4.nodes.size();
    std::vector<uint8_t> node_seen(n_nodes, 0), sphere_seen(p.spheres.size(), 0), tri_seen(p.sv.n_tri_tree, 0);
    struct Item { uint32_t link; Box box; int depth; };
    std::vector<Item> todo;
    Box all;
    for (int a = 0; a < 3; ++a) { all.lo[a] = -INFINITY; all.hi[a] = INFINITY; }
    todo.push_back({p.bvh4.root, all, 1});
    int depth = 0;
    while (!todo.empty()) {
        const Item it = todo.back();
        todo.pop_back();
        const uint32_t idx = it.link & ~kBvhFlatNode;
        const bool flat = (it.link & kBvhFlatNode) != 0u;
        if (idx >= n_nodes) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: link out of range");
        if (node_seen[idx]++) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: node reached twice");
        depth = std::max(depth, it.depth);
        if (flat) stats[11] += 1;
        const Bvh4Node &w = p.bvh4.nodes[idx];
        for (int c = 0; c < 4; ++c) {
            Box b;
            uint32_t link, count;
            if (flat) {
                const float lk[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, ct[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
                b.lo[0] = w.a[c].x; b.lo[1] = w.a[c].y; b.hi[0] = w.a[c].z; b.hi[1] = w.a[c].w; b.lo[2] = -INFINITY; b.hi[2] = INFINITY;
                link = bits(lk[c]); count = bits(ct[c]);
            } else {
                b.lo[0] = w.a[c].x; b.lo[1] = w.a[c].y; b.lo[2] = w.a[c].z; b.hi[0] = w.b[c].x; b.hi[1] = w.b[c].y; b.hi[2] = w.b[c].z;
                link = bits(w.a[c].w); count = bits(w.b[c].w);
            }
            if (count == 0xFFFFFFFFu) continue;                                   // empty slot
            if (!inside(b, it.box)) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: child box outside its parent's");
            if (count == 0u) { todo.push_back({link, b, it.depth + 1}); continue; }
            const uint32_t n = count & 0xFFFFu;
            stats[10] = std::max<uint64_t>(stats[10], n);
            if (count & kBvhTriLeaf) {
                for (uint32_t k = 0; k < n; ++k) {
                    const uint32_t rec = link + k;
                    if (rec >= p.sv.n_tri_tree) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: triangle record out of range");
                    if (tri_seen[rec]++) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: triangle in two leaves");
                    const TriX &tx = p.tris[p.tri_fidx[rec]];
                    const RtxObject &o = objects[tx.id];
                    if (hidden && hidden[tx.id]) continue;
                    const int free_axis = p.tri_rec_free_axis[rec];
                    if (free_axis != 3 - (int)tx.i - (int)tx.j) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: footprint plane differs from the elimination's rows");
                    if (flat && free_axis != 2) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: a flat node holds a triangle that is not solved in (x, y)");
                    if (!(std::isinf(b.lo[free_axis]) && std::isinf(b.hi[free_axis]))) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: triangle leaf bounded along the axis its test does not read");
                    BvhBox fp;
                    if (!triangle_footprint(o.geom, fp, free_axis)) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: non-finite triangle in the tree");
                    for (int a = 0; a < 3; ++a)
                        if (a != free_axis && !((double)b.lo[a] <= fp.lo[a] && (double)b.hi[a] >= fp.hi[a]))
                            return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: footprint outside its leaf");
                    stats[9] += 1;
                    stats[13 + (free_axis == 2 ? 0 : 1)] += 1;          // 13: (x, y) footprints, 14: (x, z) and (y, z)
                }
            } else {
                for (uint32_t k = 0; k < n; ++k) {
                    if (link + k >= p.bvh.prims.size()) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: sphere entry out of range");
                    const uint32_t sidx = p.bvh.prims[link + k];
                    if (sidx >= p.spheres.size() || sphere_seen[sidx]++) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: sphere in two leaves");
                    if (hidden && hidden[p.sphere_id[sidx]]) continue;
                    BvhBox sb;
                    if (!sphere_box(objects[p.sphere_id[sidx]].geom, sb)) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: non-finite sphere in the tree");
                    for (int a = 0; a < 3; ++a)
                        if (!((double)b.lo[a] <= sb.lo[a] && (double)b.hi[a] >= sb.hi[a]))
                            return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: sphere outside its leaf");
                    stats[8] += 1;
                }
            }
        }
    }
    if (p.sv.bvh_flags & 8u) {                     // the 64-byte form: every decoded child rectangle contains the 128-byte node's
        if (p.qnodes.size() != n_nodes) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: quantised node count differs");
        for (size_t k = 0; k < n_nodes; ++k) {
            const Bvh4Node &w = p.bvh4.nodes[k];
            const BvhQNode &q = p.qnodes[k];
            const float lk[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, ct[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
            for (int c = 0; c < 4; ++c) {
                const uint32_t count = bits(ct[c]), type = q.link[c] >> kQNodeShift;
                if ((count == 0xFFFFFFFFu) != (type == kQNodeEmpty)) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: quantised node: empty slot differs");
                if (type == kQNodeEmpty) continue;
                if ((q.link[c] & kQNodeIndexMask) != (bits(lk[c]) & ~kBvhFlatNode) || (type == 0u) != (count == 0u) ||
                    (type != 0u && type != (count & 0xFFFFu)))
                    return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: quantised node: link / count differs");
                const double lx = (double)q.ox + (double)(q.qx[c] & 0xFFFFu) * q.sx, hx = (double)q.ox + (double)(q.qx[c] >> 16) * q.sx;
                const double ly = (double)q.oy + (double)(q.qy[c] & 0xFFFFu) * q.sy, hy = (double)q.oy + (double)(q.qy[c] >> 16) * q.sy;
                if (!(lx <= (double)w.a[c].x && ly <= (double)w.a[c].y && hx >= (double)w.a[c].z && hy >= (double)w.a[c].w))
                    return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: quantised rectangle does not contain the child's");
            }
        }
        stats[15] = p.qnodes.size();
    }
    if (p.sv.bvh_flags & 16u) {                    // a sphere tree's 64-byte form: every decoded child box contains the 128-byte node's
        if (p.q3nodes.size() != n_nodes) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: 64-byte sphere node count differs");
        for (size_t k = 0; k < n_nodes; ++k) {
            const Bvh4Node &w = p.bvh4.nodes[k];
            const BvhQ3Node &q = p.q3nodes[k];
            const uint32_t *lows[3] = { &q.lox, &q.loy, &q.loz }, *highs[3] = { &q.hix, &q.hiy, &q.hiz };
            const float org[3] = { q.ox, q.oy, q.oz }, stp[3] = { q.sx, q.sy, q.sz };
            for (int c = 0; c < 4; ++c) {
                const uint32_t count = bits(w.b[c].w), type = q.link(c) >> kQNodeShift;
                if ((count == 0xFFFFFFFFu) != (type == kQNodeEmpty)) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: 64-byte sphere node: empty slot differs");
                if (type == kQNodeEmpty) continue;
                if ((q.link(c) & kQNodeIndexMask) != bits(w.a[c].w) || (type == 0u) != (count == 0u) || (type != 0u && type != count))
                    return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: 64-byte sphere node: link / count differs");
                const float l[3] = { w.a[c].x, w.a[c].y, w.a[c].z }, hh[3] = { w.b[c].x, w.b[c].y, w.b[c].z };
                for (int a = 0; a < 3; ++a) {
                    // decoded exactly as the device does: one f32 FMA of an exact product
                    const float dl = std::fmaf((float)((*lows[a] >> (8 * c)) & 255u), stp[a], org[a]);
                    const float dh = std::fmaf((float)((*highs[a] >> (8 * c)) & 255u), stp[a], org[a]);
                    if (!((double)dl <= (double)l[a] - p.bvh.abs_pad * 0.999 && (double)dh >= (double)hh[a] + p.bvh.abs_pad * 0.999))
                        return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: decoded 64-byte box does not contain the child's (+ pad)");
                }
            }
        }
        stats[15] = p.q3nodes.size();
    }
    uint64_t live_spheres = p.spheres.size(), live_tris = p.sv.n_tri_tree;
    if (hidden) {
        for (size_t k = 0; k < p.spheres.size(); ++k) if (hidden[p.sphere_id[k]]) live_spheres -= 1;
        for (uint32_t r = 0; r < p.sv.n_tri_tree; ++r) if (hidden[p.tris[p.tri_fidx[r]].id]) live_tris -= 1;
        if (depth > p.bvh4.depth) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: deeper than recorded");
    } else {
        if (depth != p.bvh4.depth) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: recorded depth differs");
        for (size_t k = 0; k < n_nodes; ++k) if (!node_seen[k]) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: unreachable node");
    }
    if ((p.sv.bvh_flags & 1u) && stats[8] != live_spheres) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: a sphere is in no leaf");
    if ((p.sv.bvh_flags & 2u) && stats[9] != live_tris) return fail(RTX_ERR_INVALID_ARGUMENT, "bvh check: a triangle is in no leaf");
    return RTX_OK;
}

#ifdef RTX_LAB
// rtx_debug_host_refit / rtx_debug_host_refit_mesh: `who` names the hook in messages; digests: 8 values, or 16 when `info` is given.
int32_t host_refit(const char *who, const RtxScene *scene, const uint64_t *indices, const RtxObject *objects, uint64_t n, uint32_t mode,
                   uint64_t *stats, uint32_t *how, uint64_t *digests, double *info)
{
    if (!scene || !stats || !how || !digests) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (scene->n_objects && !scene->objects) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": objects is null");
    *how = RTX_UPDATED_NOTHING;
    const uint64_t split = mode >> 16;                       // (lab) entries [0, split) are one update, [split, n) the next
    mode &= 0xFFFFu;
    if (split > n) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": the split point is beyond n");
    std::vector<RtxObject> cur(scene->objects, scene->objects + scene->n_objects);
    RtxScene sc = *scene;
    PackedScene p;
    if (int32_t rc = pack_scene(&sc, p)) return rc;
    RefitTables t = make_refit_tables(p);
    const uint64_t cut[3] = { 0, split, n };
    for (int part = split ? 0 : 1; part < 2; ++part) {
        const uint64_t first = cut[part], count = cut[part + 1] - cut[part];
        UpdatePlan plan;
        if (int32_t rc = plan_update(cur, t, p.sv.sphere_cmax, indices ? indices + first : nullptr, objects ? objects + first : nullptr, count, mode, plan))
            return rc;
        if (plan.how == RTX_UPDATED_REFIT || plan.how == RTX_UPDATED_RECORDS) {
            std::vector<float> box32, tribox32;
            std::vector<double> reach, tri_reach;
            derive_all_spheres(cur.data(), cur.size(), t, p.spheres.size(), box32, reach);
            if (plan.tri_geom) derive_all_triangles(cur.data(), cur.size(), t, tribox32, tri_reach);
            if (refit_packed(p, t, plan, box32, reach, tribox32, tri_reach) & (kUpdateStatusNoQ3 | kUpdateStatusNoQ)) plan.how = RTX_UPDATED_REBUILT;
        }
        for (const UpdateEntry &e : plan.entries) std::memcpy(&cur[e.object], &e.kind, sizeof(RtxObject));
        if (plan.how == RTX_UPDATED_REBUILT) {
            sc.objects = cur.data();
            p = PackedScene();
            if (int32_t rc = pack_scene(&sc, p)) return rc;
            t = make_refit_tables(p);
        }
        if (plan.how > *how) *how = plan.how;
    }
    if (info) {
        digest_packed_mesh(p, digests);
        for (int c = 0; c < 3; ++c) info[c] = t.centre[c];
        info[3] = p.sv.tri_extent; info[4] = p.sv.sphere_cmax; info[5] = t.abs_pad; info[6] = t.scale; info[7] = 0.0;
    } else digest_packed(p, digests);
    return check_packed(p, cur.data(), stats);
}
// ---- the host model of a resident handle (rtx_debug_host_set_visible, tools/host_pack_check.cpp): every step rtx_scene_set_visible,
// rtx_scene_update_objects and rtx_scene_append_objects take on a handle, on a PackedScene, with refit_packed in place of the launches.
namespace {

struct HostResident {
    RtxScene sc{};
    std::vector<RtxObject> cur;
    std::vector<uint8_t> hidden;
    PackedScene p;
    RefitTables t;
    std::vector<float> box32, tribox32;
    std::vector<double> reach, tri_reach;
    std::vector<uint32_t> keep;
    bool tables = false, mesh_tables = false, keep_valid = false;
};

// One planned update on the arrays (the device: apply_plan, rtx_api_update.hip).  True: a 64-byte node had no encoding.
bool host_apply(HostResident &r, UpdatePlan &plan)
{
    if (!r.tables) { derive_all_spheres(r.cur.data(), r.cur.size(), r.t, r.p.spheres.size(), r.box32, r.reach, r.hidden.data()); r.tables = true; }
    if (plan.tri_geom && !r.mesh_tables) { derive_all_triangles(r.cur.data(), r.cur.size(), r.t, r.tribox32, r.tri_reach, r.hidden.data()); r.mesh_tables = true; }
    plan.capture = plan.visibility && !r.keep_valid;
    if (plan.capture) r.keep_valid = true;
    return (refit_packed(r.p, r.t, plan, r.box32, r.reach, r.tribox32, r.tri_reach, &r.keep) & (kUpdateStatusNoQ3 | kUpdateStatusNoQ)) != 0ull;
}

// The pack of the list with its REAL geometries, then the hide pass on the fresh arrays (the device: repack_objects).
int32_t host_repack(HostResident &r)
{
    r.sc.n_objects = r.cur.size();
    r.sc.objects = r.cur.data();
    r.p = PackedScene();
    if (int32_t rc = pack_scene(&r.sc, r.p)) return rc;
    r.t = make_refit_tables(r.p);
    r.tables = r.mesh_tables = r.keep_valid = false;
    r.keep.clear();
    std::vector<uint64_t> idx;
    for (size_t k = 0; k < r.hidden.size(); ++k) if (r.hidden[k]) idx.push_back(k);
    if (idx.empty()) return RTX_OK;
    const std::vector<uint8_t> none(r.cur.size(), 0);
    UpdatePlan plan;
    if (int32_t rc = plan_visibility(r.cur, none, r.t, 0.0, idx.data(), idx.size(), 0u, plan)) return rc;
    if (!(r.p.sv.sphere_cmax < 1.0e14)) plan.any_sphere = false;      // (mode C only runs over finite reaches; such a pack stays "every ray sweeps")
    std::vector<uint8_t> keep_hidden;
    keep_hidden.swap(r.hidden);                               // (the tables of the fresh pack are those of the all-visible list)
    r.hidden = none;
    const bool bad = host_apply(r, plan);
    r.hidden.swap(keep_hidden);
    if (bad) return fail(RTX_ERR_UNSUPPORTED, "hidden objects: a 64-byte node of the fresh pack has no encoding without them");
    return RTX_OK;
}

}  // namespace

int32_t host_visibility(const char *who, const RtxScene *scene, const uint32_t *step_kind, const uint64_t *step_begin, uint64_t n_steps,
                        const uint64_t *indices, const RtxObject *objects, uint32_t *how, uint64_t *stats, uint64_t *digests, double *info,
                        uint8_t *mask, uint32_t *dump, uint64_t dump_words)
{
    if (!scene || !stats || !digests || (n_steps && (!step_kind || !step_begin || !how)))
        return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (scene->n_objects && !scene->objects) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": objects is null");
    HostResident r;
    r.sc = *scene;
    r.cur.assign(scene->objects, scene->objects + scene->n_objects);
    r.hidden.assign(r.cur.size(), 0);
    if (int32_t rc = host_repack(r)) return rc;
    for (uint64_t s = 0; s < n_steps; ++s) {
        how[s] = RTX_UPDATED_NOTHING;
        if (step_begin[s + 1] < step_begin[s]) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": step ranges do not ascend");
        const uint64_t first = step_begin[s], count = step_begin[s + 1] - first;
        const uint64_t *idx = indices ? indices + first : nullptr;
        const RtxObject *obj = objects ? objects + first : nullptr;
        UpdatePlan plan;
        if (step_kind[s] == kHostStepAppend) {
            if (count && !obj) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": an append step without objects");
            if (count == 0) continue;
            r.cur.insert(r.cur.end(), obj, obj + count);
            r.hidden.resize(r.cur.size(), 0);
            if (int32_t rc = host_repack(r)) return rc;
            how[s] = RTX_UPDATED_REBUILT;
            continue;
        }
        if (step_kind[s] <= kHostStepShow) {
            if (int32_t rc = plan_visibility(r.cur, r.hidden, r.t, r.p.sv.sphere_cmax, idx, count, step_kind[s] == kHostStepShow ? 1u : 0u, plan)) return rc;
        } else if (step_kind[s] <= kHostStepUpdate + RTX_UPDATE_DEFORM) {
            if (int32_t rc = plan_update(r.cur, r.t, r.p.sv.sphere_cmax, idx, obj, count, step_kind[s] - kHostStepUpdate, plan, r.hidden.data())) return rc;
        } else return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown step kind");
        if (plan.entries.empty()) continue;
        if (plan.how != RTX_UPDATED_REBUILT && host_apply(r, plan)) plan.how = RTX_UPDATED_REBUILT;
        for (const UpdateEntry &e : plan.entries) {
            if (plan.visibility) r.hidden[e.object] = (e.tri & kEntryHide) ? 1 : 0;
            else std::memcpy(&r.cur[e.object], &e.kind, sizeof(RtxObject));
        }
        if (plan.how == RTX_UPDATED_REBUILT) if (int32_t rc = host_repack(r)) return rc;
        how[s] = plan.how;
    }
    digest_packed_mesh(r.p, digests);
    if (info) {
        for (int c = 0; c < 3; ++c) info[c] = r.t.centre[c];
        info[3] = r.p.sv.tri_extent; info[4] = r.p.sv.sphere_cmax; info[5] = r.t.abs_pad; info[6] = r.t.scale; info[7] = (double)r.p.bvh4.nodes.size();
    }
    if (mask) for (size_t k = 0; k < r.hidden.size(); ++k) mask[k] = r.hidden[k] ? 0 : 1;
    if (dump) {
        // per wide node and child, kHostDumpWords words: the link and count words as they are now; the six words of its box (a footprint
        // child: z unbounded, or the nothing box when empty); the pack's link and count; the number of leaf entries (the pack's) and
        // their objects (at most 6)
        const size_t n_nodes = r.p.bvh4.nodes.size();
        if (dump_words < n_nodes * 4 * (size_t)kHostDumpWords) return fail(RTX_ERR_INVALID_ARGUMENT, std::string(who) + ": the dump buffer is too small");
        std::vector<uint8_t> flat(n_nodes, 0);
        for (uint32_t e : r.t.all_level_nodes) if (e & kBvhFlatNode) flat[e & ~kBvhFlatNode] = 1;
        auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; };
        for (size_t k = 0; k < n_nodes; ++k) {
            const Bvh4Node &w = r.p.bvh4.nodes[k];
            const float lk[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, ct[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
            for (int c = 0; c < 4; ++c) {
                uint32_t *d = dump + (k * 4 + c) * (size_t)kHostDumpWords;
                for (uint32_t j = 0; j < kHostDumpWords; ++j) d[j] = 0u;
                float box[6];
                if (flat[k]) {
                    d[0] = bits(lk[c]); d[1] = bits(ct[c]);
                    box[0] = w.a[c].x; box[1] = w.a[c].y; box[3] = w.a[c].z; box[4] = w.a[c].w;
                    const bool nothing = !(box[0] <= box[3]);
                    box[2] = nothing ? INFINITY : -INFINITY; box[5] = nothing ? -INFINITY : INFINITY;
                } else {
                    d[0] = bits(w.a[c].w); d[1] = bits(w.b[c].w);
                    box[0] = w.a[c].x; box[1] = w.a[c].y; box[2] = w.a[c].z; box[3] = w.b[c].x; box[4] = w.b[c].y; box[5] = w.b[c].z;
                }
                for (int a = 0; a < 6; ++a) d[2 + a] = bits(box[a]);
                d[8] = r.keep_valid ? r.keep[k * kKeepWords + c] : d[0];
                d[9] = r.keep_valid ? r.keep[k * kKeepWords + 4 + c] : d[1];
                if (d[9] == 0u || d[9] == 0xFFFFFFFFu) continue;
                const uint32_t n = d[9] & 0xFFFFu;
                d[10] = n;
                for (uint32_t j = 0; j < n && j < 6u; ++j)
                    d[11 + j] = (d[9] & kBvhTriLeaf) ? r.p.tris[r.p.tri_fidx[d[8] + j]].id : r.p.sphere_id[r.p.bvh.prims[d[8] + j]];
            }
        }
    }
    return check_packed(r.p, r.cur.data(), stats, r.hidden.data());
}
#endif

RTX_HOST_END
