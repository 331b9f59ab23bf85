// rtx_refit.h -- the arithmetic of rtx_scene_update_objects, written once: scene_update_kernel (rtx_update.hip) and the host
// reference refit_packed (rtx_pack.hip) compile from this text, so the device's arrays can be held to the host's bit for bit.
//
// Every expression that has a twin in pack_scene, sphere_box, bvh_append_tree or build_q3nodes is that twin's expression (same
// operations in the same order; -ffp-contract=off), with two exceptions that have no device form there:
//   * round_down_f32 / round_up_f32 step to the neighbouring float with bit operations, not nextafterf (same values);
//   * the 64-byte node's step is chosen by integer arithmetic on the exponent, not log2 / exp2, so that host and device agree to
//     the bit.  It keeps build_q3nodes' invariants (listed at q3_encode) but need not pick build_q3nodes' step.
#pragma once

#include "rtx_bvh.h"
#include "rtx_scene.h"

namespace rtx {

// One de-duplicated entry of an update as the device reads it.
struct UpdateEntry {
    uint32_t object;                       // index in Scene.objects
    uint32_t local;                        // index in spheres[] / planes[] / tris[]
    uint32_t slot;                         // sphere in the tree: its leaf entry (the inverse of bvh_prims), else kNoSlot;
                                           // triangle with new geometry: its record in tri_f32 (the inverse of tri_fidx), else kNoSlot
    uint32_t tri;                          // triangle: kTriEntry* bits (0: its geometry is the resident one)
    uint32_t kind, reserved;               // RtxObject, field by field (the C struct is not visible to every includer)
    double geom[9];
    double base_color[3], emission_color[3], roughness;
};
static_assert(sizeof(UpdateEntry) == 16 + 136, "UpdateEntry = 4 words + RtxObject");
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
// UpdateEntry.tri: the geometry changed (RTX_UPDATE_DEFORM); the class is "qualified"; the record is a tree record (it has tri_geo and
// tribox32 rows); the free axis of a qualified triangle in bits 4..5.  The host decides all of it (plan_update).
constexpr uint32_t kTriEntryGeom = 1u, kTriEntryQualified = 2u, kTriEntryTree = 4u, kTriEntryAxisShift = 4u;

// What one launch of scene_update_kernel works on.  `mode` is launch-uniform:
//   0 (A) records: one thread per entry;  1 (B) one level of wide nodes: one thread per node of `level`;  2 (C) sphere_cmax;
//   3 (D) tri_extent.  The triangle arrays are null in a launch of an update that moves no triangle: mode B then leaves triangle
//   leaves and footprint nodes as they are.
struct UpdateArgs {
    uint32_t mode, n;
    const UpdateEntry *entries;
    SphereX *spheres; PlaneX *planes; MaterialX *materials;
    float *sphere_f32;                     // the pair-interleaved records as scalars
    float4 *leaf_f32, *leaf_cr;
    float *box32;                          // per sphere: lo.xyz, hi.xyz of its padded f32 box
    double *reach;                         // per sphere: |c - centre| + |r|
    Bvh4Node *nodes; BvhQ3Node *q3nodes;   // q3nodes: null when the tree has no 64-byte form
    const uint32_t *prims;
    const uint32_t *level;                 // mode B: the node indices of this level (kBvhFlatNode set: a footprint node)
    unsigned long long *status;            // [0]: kUpdateStatus* bits;  [1]: the bits of the new sphere_cmax;  [2]: of the new tri_extent
    TriX *tris;                            // the triangle half (null: no triangle moves)
    float4 *tri_f32, *tri_geo;
    float *tribox32;                       // per tree record: lo.xyz, hi.xyz of its padded f32 footprint (-inf / +inf along its free axis)
    double *tri_reach;                     // per triangle: max |v - centre| over its nine coordinates (0: not qualified)
    BvhQNode *qnodes;                      // null when the tree has no 64-byte footprint form
    double centre[3];
    double abs_pad;
};
constexpr unsigned long long kUpdateStatusNoQ3 = 1ull, kUpdateStatusNoQ = 2ull;     // a BvhQ3Node / a BvhQNode has no encoding

RTX_HD uint32_t refit_f32_bits(float f) { union { float f; uint32_t u; } v; v.f = f; return v.u; }
RTX_HD float refit_bits_f32(uint32_t u) { union { float f; uint32_t u; } v; v.u = u; return v.f; }
RTX_HD uint64_t refit_f64_bits(double d) { union { double d; uint64_t u; } v; v.d = d; return v.u; }
RTX_HD double refit_bits_f64(uint64_t u) { union { double d; uint64_t u; } v; v.u = u; return v.d; }

// round_down_f32 / round_up_f32 of rtx_bvh.h: the neighbour of a float is its bit pattern +/- 1 (zero: the smallest denormal of the
// other sign; +inf steps down to FLT_MAX as nextafterf does; a NaN compares false and stays).
RTX_HD float refit_round_down_f32(double x)
{
    float f = (float)x;
    if ((double)f > x) {
        const uint32_t u = refit_f32_bits(f);
        if ((u << 1) == 0u) f = refit_bits_f32(0x80000001u);
        else f = refit_bits_f32((u >> 31) ? u + 1u : u - 1u);
    }
    return f;
}

RTX_HD float refit_round_up_f32(double x)
{
    float f = (float)x;
    if ((double)f < x) {
        const uint32_t u = refit_f32_bits(f);
        if ((u << 1) == 0u) f = refit_bits_f32(0x00000001u);
        else f = refit_bits_f32((u >> 31) ? u - 1u : u + 1u);
    }
    return f;
}

// Everything of one sphere that is derived from its geometry, the scene's `centre` and the tree's abs_pad.
struct SphereDerived {
    SphereX exact;
    float fx, fy, fz, fw;                  // pack_scene's f32 filter record: c - centre, |c - centre|^2 - r^2
    float r_up;                            // |r| rounded up (bvh_leaf_cr.w)
    double reach;
    float lo[3], hi[3];                    // sphere_box() widened by abs_pad, rounded outward (bvh_append_tree's leaf box)
};

RTX_HD SphereDerived derive_sphere(const double g[4], const double centre[3], double abs_pad)
{
    SphereDerived d;
    d.exact = make_sphere(g);
    const double cx = g[0] - centre[0], cy = g[1] - centre[1], cz = g[2] - centre[2];
    const double cc = cx * cx + cy * cy + cz * cz;
    const double r = fabs(g[3]);
    d.reach = sqrt(cc) + r;
    d.fx = (float)cx; d.fy = (float)cy; d.fz = (float)cz; d.fw = (float)(cc - d.exact.rr);
    d.r_up = refit_round_up_f32(r);
    for (int a = 0; a < 3; ++a) {          // sphere_box (rtx_bvh.h), then bvh_append_tree's padding and rounding
        const double pad = (fabs(g[a]) + r) * (1.0 / 1048576.0) + 1e-300;
        const double lo = g[a] - r - pad, hi = g[a] + r + pad;
        d.lo[a] = refit_round_down_f32(lo - abs_pad);
        d.hi[a] = refit_round_up_f32(hi + abs_pad);
    }
    return d;
}

// Everything of one triangle that is derived from its vertices, the scene's `centre` and the tree's abs_pad: pack_scene's expressions
// in pack_scene's order (min / max as comparisons: the values of fmin / fmax for finite operands, and one answer for -0 against +0
// on host and device).  `qualified` and `f` (the free axis) are the host's classification (classify_triangle, rtx_pack.hip); a
// triangle that is not qualified has the "always a candidate" record and no footprint.
struct TriDerived {
    TriX exact;
    float4 A, B, g0, g1;                   // tri_f32[2 rec], [2 rec + 1]; tri_geo[2 rec], [2 rec + 1]
    double reach;
    float box[6];                          // triangle_footprint() widened by abs_pad, rounded outward (bvh_append_tree's leaf box)
};

RTX_HD double refit_min3(double x0, double x1, double x2) { const double m = x2 < x1 ? x2 : x1; return m < x0 ? m : x0; }
RTX_HD double refit_max3(double x0, double x1, double x2) { const double m = x2 > x1 ? x2 : x1; return m > x0 ? m : x0; }

RTX_HD TriDerived derive_triangle(const double g[9], uint32_t object, bool qualified, int f, const double centre[3], double abs_pad)
{
    TriDerived d;
    d.exact = make_triangle(g, object);
    d.A = make_float4(0.f, 0.f, 0.f, 0.f); d.B = make_float4(0.f, 0.f, 0.f, 0.f);
    d.g0 = make_float4(0.f, 0.f, 0.f, 0.f); d.g1 = make_float4(0.f, 0.f, 0.f, 0.f);
    d.reach = 0.0;
    for (int a = 0; a < 3; ++a) { d.box[a] = -INFINITY; d.box[3 + a] = INFINITY; }
    if (!qualified) return d;
    const TriX &t = d.exact;
    const double kabs = dot(t.n, t.v0);
    double v[3][3];
    for (int c = 0; c < 9; ++c) v[c / 3][c % 3] = g[c] - centre[c % 3];
    const int a0 = f == 0 ? 1 : 0, a1 = f == 2 ? 1 : 2;
    const double r0 = v[1][a0] - v[0][a0], r1 = v[1][a1] - v[0][a1], s0 = v[2][a0] - v[0][a0], s1 = v[2][a1] - v[0][a1];
    const double det = r0 * s1 - r1 * s0;
    const double m00 = s1 / det, m01 = -s0 / det, m10 = -r1 / det, m11 = r0 / det;
    const double kc = t.n.x * v[0][0] + t.n.y * v[0][1] + t.n.z * v[0][2];
    d.g0 = make_float4((float)v[0][a0], (float)v[0][a1], (float)m00, (float)m01);
    d.g1 = make_float4((float)m10, (float)m11, (float)kabs, (float)(2 - f));
    d.A = make_float4((float)t.n.x, (float)t.n.y, (float)t.n.z, (float)kc);
    d.B = make_float4(0.f, 0.f, 1.0e30f, 1.0e30f);
    for (int c = 0; c < 9; ++c) { const double m = fabs(v[c / 3][c % 3]); d.reach = m > d.reach ? m : d.reach; }
    if (f == 2) {
        const double xlo = refit_min3(v[0][0], v[1][0], v[2][0]), xhi = refit_max3(v[0][0], v[1][0], v[2][0]);
        const double ylo = refit_min3(v[0][1], v[1][1], v[2][1]), yhi = refit_max3(v[0][1], v[1][1], v[2][1]);
        const double grow = 1.0 + 1.0 / 1048576.0;
        d.B = make_float4((float)(0.5 * (xlo + xhi)), (float)(0.5 * (ylo + yhi)),
                          refit_round_up_f32(0.5 * (xhi - xlo) * grow + 1e-30), refit_round_up_f32(0.5 * (yhi - ylo) * grow + 1e-30));
    }
    for (int a = 0; a < 3; ++a) {          // triangle_footprint (rtx_bvh.h), then bvh_append_tree's padding and rounding
        if (a == f) continue;
        const double lo = refit_min3(g[a], g[3 + a], g[6 + a]), hi = refit_max3(g[a], g[3 + a], g[6 + a]);
        const double al = fabs(lo), ah = fabs(hi);
        const double pad = (al > ah ? al : ah) * (1.0 / 1048576.0) + 1e-300;
        const double blo = lo - pad, bhi = hi + pad;
        d.box[a] = refit_round_down_f32(blo - abs_pad);
        d.box[3 + a] = refit_round_up_f32(bhi + abs_pad);
    }
    return d;
}

// ---- mode A ---------------------------------------------------------------------------------------------------------------------
RTX_HD void update_record(const UpdateArgs &u, uint32_t i)
{
    const UpdateEntry &e = u.entries[i];
    MaterialX m;
    m.base_color = mk(e.base_color[0], e.base_color[1], e.base_color[2]);
    m.emission_color = mk(e.emission_color[0], e.emission_color[1], e.emission_color[2]);
    m.roughness = e.roughness;
    u.materials[e.object] = m;
    if (e.kind == 1u) { u.planes[e.local] = make_plane(e.geom, e.object); return; }
    if (e.kind == 2u && (e.tri & kTriEntryGeom)) {                   // a triangle that keeps its class and gets new vertices (DEFORM)
        const uint32_t k = e.local;
        const TriDerived d = derive_triangle(e.geom, e.object, (e.tri & kTriEntryQualified) != 0u, (int)((e.tri >> kTriEntryAxisShift) & 3u),
                                             u.centre, u.abs_pad);
        u.tris[k] = d.exact;
        u.tri_reach[k] = d.reach;
        if (e.slot == kNoSlot) return;                               // class "none": no filter record
        u.tri_f32[2 * (size_t)e.slot] = d.A; u.tri_f32[2 * (size_t)e.slot + 1] = d.B;
        if (!(e.tri & kTriEntryTree)) return;
        u.tri_geo[2 * (size_t)e.slot] = d.g0; u.tri_geo[2 * (size_t)e.slot + 1] = d.g1;
        float *b = u.tribox32 + (size_t)e.slot * 6;
        for (int a = 0; a < 6; ++a) b[a] = d.box[a];
        return;
    }
    if (e.kind != 0u) return;                                        // a triangle: its geometry did not change (the host checked)
    const uint32_t k = e.local;
    const SphereDerived d = derive_sphere(e.geom, u.centre, u.abs_pad);
    u.spheres[k] = d.exact;
    float *f = u.sphere_f32 + (size_t)(k & ~1u) * 4 + (k & 1u);      // records 2p, 2p + 1 = {x0, x1, y0, y1} {z0, z1, w0, w1}
    f[0] = d.fx; f[2] = d.fy; f[4] = d.fz; f[6] = d.fw;
    u.reach[k] = d.reach;
    if (e.slot == kNoSlot) return;
    u.leaf_f32[e.slot] = make_float4(d.fx, d.fy, d.fz, d.fw);
    u.leaf_cr[e.slot] = make_float4(d.fx, d.fy, d.fz, d.r_up);
    float *b = u.box32 + (size_t)k * 6;
    for (int a = 0; a < 3; ++a) { b[a] = d.lo[a]; b[3 + a] = d.hi[a]; }
}

// ---- mode B ---------------------------------------------------------------------------------------------------------------------
// 2^k as a double, k within the normal range.
RTX_HD double refit_pow2(int k) { return refit_bits_f64((uint64_t)(k + 1023) << 52); }

// The 64-byte form of one node from its (refitted) 128-byte form.  build_q3nodes' invariants: the steps are powers of two and normal
// f32 values; o is a multiple of the step and exact in f32; |o / s| + 256 < 2^24; lo is floored and hi ceiled after a further abs_pad;
// 0 <= ql <= qh <= 255; an empty slot reads 255 / 0; links and types as they were.  False: no such encoding.
RTX_HD bool q3_encode(const Bvh4Node &w, double abs_pad, BvhQ3Node &q)
{
    double lo[3] = { (double)INFINITY, (double)INFINITY, (double)INFINITY }, hi[3] = { -(double)INFINITY, -(double)INFINITY, -(double)INFINITY };
    uint32_t cnt[4];
    bool any = false;
    for (int c = 0; c < 4; ++c) {
        cnt[c] = refit_f32_bits(w.b[c].w);
        if (cnt[c] == 0xFFFFFFFFu) continue;
        any = true;
        const float l[3] = { w.a[c].x, w.a[c].y, w.a[c].z }, h[3] = { w.b[c].x, w.b[c].y, w.b[c].z };
        for (int a = 0; a < 3; ++a) {
            const double dl = (double)l[a] - abs_pad, dh = (double)h[a] + abs_pad;
            if (!(fabs(dl) < 1.0e300) || !(fabs(dh) < 1.0e300)) return false;           // not finite
            lo[a] = dl < lo[a] ? dl : lo[a];
            hi[a] = dh > hi[a] ? dh : hi[a];
        }
    }
    double o[3], sc[3];
    for (int a = 0; a < 3; ++a) {
        o[a] = 0.0; sc[a] = 1.0;
        if (!any) continue;
        const double ext = hi[a] - lo[a];
        if (ext > 0.0) {
            // ext = m * 2^e, 1 <= m < 2: ext / 2^(e - 7) = 128 m in [128, 256); one more doubling when that is above 254
            const uint64_t eb = refit_f64_bits(ext);
            const int e = (int)((eb >> 52) & 0x7FFu) - 1023;
            if (e < -900) return false;                                                   // (a denormal extent: no normal f32 step)
            int k = e - 7;
            if (ext / refit_pow2(k) > 254.0) k += 1;
            if (k < -126 || k > 99) return false;                                         // the step must stay a normal f32 (and <= 1e30)
            sc[a] = refit_pow2(k);
        }
        o[a] = floor(lo[a] / sc[a]) * sc[a];                                              // a multiple of the step
        int guard = 0;
        while ((hi[a] - o[a]) / sc[a] > 255.0) {
            if (++guard > 4) return false;
            sc[a] *= 2.0;
            if (sc[a] > 1.0e30) return false;
            o[a] = floor(lo[a] / sc[a]) * sc[a];
        }
        if (!(fabs(o[a] / sc[a]) + 256.0 < 16777216.0)) return false;                    // o + q * s must be exact in f32
        if ((double)(float)o[a] != o[a]) return false;
    }
    const uint32_t keep[4] = { q.link0, q.link1, q.link2, q.link3 };
    BvhQ3Node r;
    r.link0 = keep[0]; r.link1 = keep[1]; r.link2 = keep[2]; r.link3 = keep[3];
    r.ox = (float)o[0]; r.oy = (float)o[1]; r.oz = (float)o[2]; r.sx = (float)sc[0]; r.sy = (float)sc[1]; r.sz = (float)sc[2];
    uint32_t lows[3] = { 0u, 0u, 0u }, highs[3] = { 0u, 0u, 0u };
    for (int c = 0; c < 4; ++c) {
        if (cnt[c] == 0xFFFFFFFFu) {                                  // empty: an inverted box (lo 255, hi 0) is never entered
            for (int a = 0; a < 3; ++a) lows[a] |= 255u << (8 * c);
            continue;
        }
        const float l[3] = { w.a[c].x, w.a[c].y, w.a[c].z }, h[3] = { w.b[c].x, w.b[c].y, w.b[c].z };
        for (int a = 0; a < 3; ++a) {
            const double ql = floor(((double)l[a] - abs_pad - o[a]) / sc[a]), qh = ceil(((double)h[a] + abs_pad - o[a]) / sc[a]);
            if (!(ql >= 0.0 && qh <= 255.0 && ql <= qh)) return false;
            lows[a] |= (uint32_t)ql << (8 * c);
            highs[a] |= (uint32_t)qh << (8 * c);
        }
    }
    r.lox = lows[0]; r.loy = lows[1]; r.loz = lows[2]; r.hix = highs[0]; r.hiy = highs[1]; r.hiz = highs[2];
    q = r;
    return true;
}

// The 64-byte form of one footprint node from its (refitted) 128-byte form, under build_qnodes' invariants: o = the smallest lo of
// the non-empty children (an f32 value: exact), s = the smallest power of two with ext / s <= 65535 -- which is build_qnodes' step,
// found on the exponent field -- a normal f32 and <= 1e30; lo floored (>= 0), hi ceiled (<= 65535); an empty child reads
// 0x0000FFFF; the link words as they were.  False: no such encoding.
RTX_HD bool qnode_encode(const Bvh4Node &w, BvhQNode &q)
{
    const uint32_t ct[4] = { refit_f32_bits(w.b[1].x), refit_f32_bits(w.b[1].y), refit_f32_bits(w.b[1].z), refit_f32_bits(w.b[1].w) };
    double lo[2] = { (double)INFINITY, (double)INFINITY }, hi[2] = { -(double)INFINITY, -(double)INFINITY };
    bool any = false;
    for (int c = 0; c < 4; ++c) {
        if (ct[c] == 0xFFFFFFFFu) continue;
        const float r[4] = { w.a[c].x, w.a[c].y, w.a[c].z, w.a[c].w };
        for (int k = 0; k < 4; ++k) if ((refit_f32_bits(r[k]) & 0x7F800000u) == 0x7F800000u) return false;       // not finite
        any = true;
        for (int a = 0; a < 2; ++a) {
            const double l = (double)r[a], h = (double)r[2 + a];
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    double o[2], sc[2];
    for (int a = 0; a < 2; ++a) {
        o[a] = any ? lo[a] : 0.0;
        sc[a] = 1.0;
        const double ext = any ? hi[a] - lo[a] : 0.0;
        if (ext > 0.0) {
            // ext = m * 2^e, 1 <= m < 2: ext / 2^(e - 15) = 32768 m in [32768, 65536); one more doubling when that is above 65535
            const int e = (int)((refit_f64_bits(ext) >> 52) & 0x7FFu) - 1023;
            if (e < -900) return false;
            int k = e - 15;
            if (ext / refit_pow2(k) > 65535.0) k += 1;
            if (k < -126 || k > 99) return false;                                         // the step must stay a normal f32 (and <= 1e30)
            sc[a] = refit_pow2(k);
        }
    }
    BvhQNode r = q;                                                                       // (the links)
    r.ox = (float)o[0]; r.oy = (float)o[1]; r.sx = (float)sc[0]; r.sy = (float)sc[1];
    for (int c = 0; c < 4; ++c) {
        if (ct[c] == 0xFFFFFFFFu) { r.qx[c] = 0x0000FFFFu; r.qy[c] = 0x0000FFFFu; continue; }
        const double l0 = floor(((double)w.a[c].x - o[0]) / sc[0]), h0 = ceil(((double)w.a[c].z - o[0]) / sc[0]);
        const double l1 = floor(((double)w.a[c].y - o[1]) / sc[1]), h1 = ceil(((double)w.a[c].w - o[1]) / sc[1]);
        if (!(l0 >= 0.0 && l1 >= 0.0 && h0 <= 65535.0 && h1 <= 65535.0)) return false;
        r.qx[c] = (uint32_t)l0 | ((uint32_t)h0 << 16);
        r.qy[c] = (uint32_t)l1 | ((uint32_t)h1 << 16);
    }
    q = r;
    return true;
}

// One footprint node (the flat layout: a[c] = {lo.x, lo.y, hi.x, hi.y}, the links in b[0], the counts in b[1]): the rectangle of a
// triangle leaf is the min / max of tribox32 over its records, that of an interior child -- a footprint node too, refitted by the
// previous launch -- the min / max of its four rectangles (an empty slot's {inf, inf, -inf, -inf} never wins).  This is the builder's
// rectangle for the same topology: the builder rounds the union of the padded f64 footprints, x -> round_down_f32(x - abs_pad) is
// monotone (round_up likewise), so the rounded union is the union of the rounded rectangles, at every level.  Empty slots, links and
// counts are not touched.  False when the node's 64-byte form (u.qnodes != null) cannot be encoded.
RTX_HD bool refit_flat_node(const UpdateArgs &u, uint32_t idx)
{
    Bvh4Node &w = u.nodes[idx];
    const uint32_t lk[4] = { refit_f32_bits(w.b[0].x), refit_f32_bits(w.b[0].y), refit_f32_bits(w.b[0].z), refit_f32_bits(w.b[0].w) };
    const uint32_t ct[4] = { refit_f32_bits(w.b[1].x), refit_f32_bits(w.b[1].y), refit_f32_bits(w.b[1].z), refit_f32_bits(w.b[1].w) };
    for (int c = 0; c < 4; ++c) {
        if (ct[c] == 0xFFFFFFFFu) continue;
        float lo[2] = { INFINITY, INFINITY }, hi[2] = { -INFINITY, -INFINITY };
        if (ct[c] == 0u) {
            const Bvh4Node &ch = u.nodes[lk[c] & ~kBvhFlatNode];
            for (int k = 0; k < 4; ++k) {
                const float l[2] = { ch.a[k].x, ch.a[k].y }, h[2] = { ch.a[k].z, ch.a[k].w };
                for (int a = 0; a < 2; ++a) { lo[a] = l[a] < lo[a] ? l[a] : lo[a]; hi[a] = h[a] > hi[a] ? h[a] : hi[a]; }
            }
        } else {
            const uint32_t n = ct[c] & 0xFFFFu;
            for (uint32_t k = 0; k < n; ++k) {
                const float *b = u.tribox32 + (size_t)(lk[c] + k) * 6;
                for (int a = 0; a < 2; ++a) { lo[a] = b[a] < lo[a] ? b[a] : lo[a]; hi[a] = b[3 + a] > hi[a] ? b[3 + a] : hi[a]; }
            }
        }
        w.a[c] = make_float4(lo[0], lo[1], hi[0], hi[1]);
    }
    if (!u.qnodes) return true;
    BvhQNode q = u.qnodes[idx];
    if (!qnode_encode(w, q)) return false;
    u.qnodes[idx] = q;
    return true;
}

// One non-flat wide node: the boxes of its sphere leaves from box32, of its non-flat interior children from those children's four
// boxes (refitted by the previous launch: the levels run deepest first).  When triangles move (u.tribox32 != null) a triangle leaf
// gets the min / max of tribox32 over its records -- unbounded along their free axis -- and a footprint child the (x, y) union of that
// node's four rectangles, unbounded in z; otherwise triangle leaves and footprint children stay.  Empty slots stay.
// Link and count words are not touched.  (min / max as comparisons: one answer for -0 against +0 on host and device.)  Returns false when the node's 64-byte form (u.q3nodes != null) cannot be encoded.
RTX_HD bool refit_node(const UpdateArgs &u, uint32_t idx)
{
    Bvh4Node &w = u.nodes[idx];
    for (int c = 0; c < 4; ++c) {
        const uint32_t link = refit_f32_bits(w.a[c].w), count = refit_f32_bits(w.b[c].w);
        if (count == 0xFFFFFFFFu) continue;
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        if (count & kBvhTriLeaf) {
            if (!u.tribox32) continue;
            const uint32_t n = count & 0xFFFFu;
            for (uint32_t k = 0; k < n; ++k) {
                const float *b = u.tribox32 + (size_t)(link + k) * 6;
                for (int a = 0; a < 3; ++a) { lo[a] = b[a] < lo[a] ? b[a] : lo[a]; hi[a] = b[3 + a] > hi[a] ? b[3 + a] : hi[a]; }
            }
        } else if (count == 0u && (link & kBvhFlatNode)) {
            if (!u.tribox32) continue;
            const Bvh4Node &ch = u.nodes[link & ~kBvhFlatNode];
            for (int k = 0; k < 4; ++k) {
                const float l[2] = { ch.a[k].x, ch.a[k].y }, h[2] = { ch.a[k].z, ch.a[k].w };
                for (int a = 0; a < 2; ++a) { lo[a] = l[a] < lo[a] ? l[a] : lo[a]; hi[a] = h[a] > hi[a] ? h[a] : hi[a]; }
            }
            lo[2] = -INFINITY; hi[2] = INFINITY;
        } else if (count == 0u) {
            const Bvh4Node &ch = u.nodes[link];
            for (int k = 0; k < 4; ++k) {
                const float l[3] = { ch.a[k].x, ch.a[k].y, ch.a[k].z }, h[3] = { ch.b[k].x, ch.b[k].y, ch.b[k].z };
                for (int a = 0; a < 3; ++a) { lo[a] = l[a] < lo[a] ? l[a] : lo[a]; hi[a] = h[a] > hi[a] ? h[a] : hi[a]; }
            }
        } else {
            const uint32_t n = count & 0xFFFFu;
            for (uint32_t k = 0; k < n; ++k) {
                const float *b = u.box32 + (size_t)u.prims[link + k] * 6;
                for (int a = 0; a < 3; ++a) { lo[a] = b[a] < lo[a] ? b[a] : lo[a]; hi[a] = b[3 + a] > hi[a] ? b[3 + a] : hi[a]; }
            }
        }
        w.a[c].x = lo[0]; w.a[c].y = lo[1]; w.a[c].z = lo[2];
        w.b[c].x = hi[0]; w.b[c].y = hi[1]; w.b[c].z = hi[2];
    }
    if (!u.q3nodes) return true;
    BvhQ3Node q = u.q3nodes[idx];
    if (!q3_encode(w, u.abs_pad, q)) return false;
    u.q3nodes[idx] = q;
    return true;
}

// One entry of a level list: the status bits its node raises.
RTX_HD unsigned long long refit_level_entry(const UpdateArgs &u, uint32_t entry)
{
    if (entry & kBvhFlatNode) return refit_flat_node(u, entry & ~kBvhFlatNode) ? 0ull : kUpdateStatusNoQ;
    return refit_node(u, entry) ? 0ull : kUpdateStatusNoQ3;
}

}  // namespace rtx
