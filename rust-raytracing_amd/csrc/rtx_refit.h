// rtx_refit.h -- the arithmetic of rtx_scene_update_objects and rtx_scene_set_visible, written once: scene_update_kernel (rtx_update.hip) and the host
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
// UpdateEntry.tri, any kind (rtx_scene_set_visible): kEntryHide -- the object is hidden: its records become the ones of hide_record
// below and its material stays; kEntryNoGeom -- an update of a HIDDEN object: the material record alone (its new geometry is judged
// when it is shown).  An entry that SHOWS an object is an ordinary entry with the object's current geometry.
constexpr uint32_t kEntryHide = 0x100u, kEntryNoGeom = 0x200u;
// The kept words of one wide node (UpdateArgs.keep): the pack's four link and four count words of its 128-byte form, then the four
// link words of its 64-byte form (0 when the tree has none).
constexpr uint32_t kKeepWords = 12u;

// What one launch of scene_update_kernel works on.  `mode` is launch-uniform:
//   0 (A) records: one thread per entry;  1 (B) one level of wide nodes: one thread per node of `level`;  2 (C) sphere_cmax;
//   3 (D) tri_extent;  4 (E) the kept words: one thread per wide node (capture_keep).  The triangle arrays are null in a launch of an update that moves no triangle: mode B then leaves triangle
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
    uint32_t *keep;                        // kKeepWords per wide node, made by mode E at the first visibility call after a pack; null before
                                           // it: mode B then touches no link or count word
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
// A hidden object's records (rtx_scene_set_visible): the exact record of all-NaN geometry with the id kept -- no f64 test accepts
// it -- and f32 records that are never CERTAIN in any stage that lowers a pruning bound ("Hidden objects", reader by
// reader):
//   sphere_f32, leaf_f32   pack_scene's pad sentinel {0, 0, 0, 1e30}: filter_disc1 / filter_disc2 only select candidates
//   leaf_cr                NaN coordinates: Dp = NaN, and every reader enters its bounds with `Dp >= 0`, false
//   tri_f32, tri_geo       pack_scene's record of a triangle outside the tree {A = 0, B = 0, g0 = 0, g1 = (0, 0, NaN, 0)} with A.w = 1e30:
//                          n = 0, so n.d = 0 and tri_bounds never reaches the block that sets t_hi; |n.(v0 - p)| = 1e30, so
//                          tri_filter_sign drops it for every ray with a d.x or d.y (A.w = 0 would make it a candidate for all)
//   box32, tribox32        the nothing box (+inf lo, -inf hi on every axis): it never wins a min / max;  reach, tri_reach   0
// The NaNs that make_plane / make_triangle derive (a norm, the elimination's pivots) are written as THE quiet NaN: which NaN an
// operation on NaNs returns is the one thing host and device need not agree on, and no test reads a NaN's sign or payload.
RTX_HD double refit_canon(double x) { return x == x ? x : refit_bits_f64(0x7FF8000000000000ull); }
RTX_HD V3 refit_canon3(V3 v) { return mk(refit_canon(v.x), refit_canon(v.y), refit_canon(v.z)); }

RTX_HD void hide_record(const UpdateArgs &u, const UpdateEntry &e)
{
    const double nan = refit_bits_f64(0x7FF8000000000000ull);
    const double g[9] = { nan, nan, nan, nan, nan, nan, nan, nan, nan };
    const uint32_t k = e.local;
    if (e.kind == 1u) {
        PlaneX p = make_plane(g, e.object);
        p.position = refit_canon3(p.position); p.normal = refit_canon3(p.normal); p.nhat = refit_canon3(p.nhat);
        u.planes[k] = p;
        return;
    }
    if (e.kind == 2u) {
        TriX t = make_triangle(g, e.object);
        t.v0 = refit_canon3(t.v0); t.n = refit_canon3(t.n); t.nn = refit_canon3(t.nn);
        t.piv1 = refit_canon(t.piv1); t.f = refit_canon(t.f); t.piv2 = refit_canon(t.piv2); t.g = refit_canon(t.g);
        u.tris[k] = t;
        u.tri_reach[k] = 0.0;
        if (e.slot == kNoSlot) return;
        u.tri_f32[2 * (size_t)e.slot] = make_float4(0.f, 0.f, 0.f, 1.0e30f); u.tri_f32[2 * (size_t)e.slot + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!(e.tri & kTriEntryTree)) return;
        u.tri_geo[2 * (size_t)e.slot] = make_float4(0.f, 0.f, 0.f, 0.f);
        u.tri_geo[2 * (size_t)e.slot + 1] = make_float4(0.f, 0.f, refit_bits_f32(0x7FC00000u), 0.f);
        float *b = u.tribox32 + (size_t)e.slot * 6;
        for (int a = 0; a < 3; ++a) { b[a] = INFINITY; b[3 + a] = -INFINITY; }
        return;
    }
    SphereX sp = make_sphere(g);
    sp.rr = refit_canon(sp.rr);
    u.spheres[k] = sp;
    float *f = u.sphere_f32 + (size_t)(k & ~1u) * 4 + (k & 1u);
    f[0] = 0.f; f[2] = 0.f; f[4] = 0.f; f[6] = 1.0e30f;
    u.reach[k] = 0.0;
    if (e.slot == kNoSlot) return;
    const float qnan = refit_bits_f32(0x7FC00000u);
    u.leaf_f32[e.slot] = make_float4(0.f, 0.f, 0.f, 1.0e30f);
    u.leaf_cr[e.slot] = make_float4(qnan, qnan, qnan, 0.f);
    float *b = u.box32 + (size_t)k * 6;
    for (int a = 0; a < 3; ++a) { b[a] = INFINITY; b[3 + a] = -INFINITY; }
}

RTX_HD void update_record(const UpdateArgs &u, uint32_t i)
{
    const UpdateEntry &e = u.entries[i];
    if (e.tri & kEntryHide) { hide_record(u, e); return; }
    MaterialX m;
    m.base_color = mk(e.base_color[0], e.base_color[1], e.base_color[2]);
    m.emission_color = mk(e.emission_color[0], e.emission_color[1], e.emission_color[2]);
    m.roughness = e.roughness;
    u.materials[e.object] = m;
    if (e.tri & kEntryNoGeom) return;
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
// monotone (round_up likewise), so the rounded union is the union of the rounded rectangles, at every level.  The pack's empty slots
// stay; links and counts are not touched unless the kept words exist (refit_node).  False when the node's 64-byte form (u.qnodes !=
// null) cannot be encoded.
RTX_HD bool refit_flat_node(const UpdateArgs &u, uint32_t idx)
{
    Bvh4Node &w = u.nodes[idx];
    uint32_t lk[4] = { refit_f32_bits(w.b[0].x), refit_f32_bits(w.b[0].y), refit_f32_bits(w.b[0].z), refit_f32_bits(w.b[0].w) };
    uint32_t ct[4] = { refit_f32_bits(w.b[1].x), refit_f32_bits(w.b[1].y), refit_f32_bits(w.b[1].z), refit_f32_bits(w.b[1].w) };
    const uint32_t *kw = u.keep ? u.keep + (size_t)idx * kKeepWords : nullptr;
    BvhQNode q;
    if (u.qnodes) q = u.qnodes[idx];
    for (int c = 0; c < 4; ++c) {
        const uint32_t link = kw ? kw[c] : lk[c], count = kw ? kw[4 + c] : ct[c];        // the pack's words: what the slot holds when something below is alive
        if (count == 0xFFFFFFFFu) continue;
        float lo[2] = { INFINITY, INFINITY }, hi[2] = { -INFINITY, -INFINITY };
        if (count == 0u) {
            const Bvh4Node &ch = u.nodes[link & ~kBvhFlatNode];
            for (int k = 0; k < 4; ++k) {
                const float l[2] = { ch.a[k].x, ch.a[k].y }, h[2] = { ch.a[k].z, ch.a[k].w };
                for (int a = 0; a < 2; ++a) { lo[a] = l[a] < lo[a] ? l[a] : lo[a]; hi[a] = h[a] > hi[a] ? h[a] : hi[a]; }
            }
        } else {
            const uint32_t n = count & 0xFFFFu;
            for (uint32_t k = 0; k < n; ++k) {
                const float *b = u.tribox32 + (size_t)(link + k) * 6;
                for (int a = 0; a < 2; ++a) { lo[a] = b[a] < lo[a] ? b[a] : lo[a]; hi[a] = b[3 + a] > hi[a] ? b[3 + a] : hi[a]; }
            }
        }
        w.a[c] = make_float4(lo[0], lo[1], hi[0], hi[1]);
        if (!kw) continue;
        const bool alive = lo[0] <= hi[0];                               // (nothing alive below: the union is the nothing rectangle, the slot's empty form)
        lk[c] = alive ? link : 0u; ct[c] = alive ? count : 0xFFFFFFFFu;
        if (u.qnodes) q.link[c] = alive ? kw[8 + c] : (kQNodeEmpty << kQNodeShift);
    }
    if (kw) {
        w.b[0] = make_float4(refit_bits_f32(lk[0]), refit_bits_f32(lk[1]), refit_bits_f32(lk[2]), refit_bits_f32(lk[3]));
        w.b[1] = make_float4(refit_bits_f32(ct[0]), refit_bits_f32(ct[1]), refit_bits_f32(ct[2]), refit_bits_f32(ct[3]));
    }
    if (!u.qnodes) return true;
    if (!qnode_encode(w, q)) return false;
    u.qnodes[idx] = q;
    return true;
}

// One non-flat wide node: the boxes of its sphere leaves from box32, of its non-flat interior children from those children's four
// boxes (refitted by the previous launch: the levels run deepest first).  When triangles move (u.tribox32 != null) a triangle leaf
// gets the min / max of tribox32 over its records -- unbounded along their free axis -- and a footprint child the (x, y) union of that
// node's four rectangles, unbounded in z; otherwise triangle leaves and footprint children stay.  The pack's empty slots stay.
// Without kept words (u.keep == null) link and count words are not touched.  With them (a visibility call has run on this pack) the
// union is taken over what the PACK's words name, and a slot with nothing alive below -- the nothing box -- is written as the empty
// slot, any other slot gets the pack's words back: hiding and showing are this one path (refit_flat_node likewise).
// (min / max as comparisons: one answer for -0 against +0 on host and device.)  Returns false when the node's 64-byte form (u.q3nodes != null) cannot be encoded.
RTX_HD bool refit_node(const UpdateArgs &u, uint32_t idx)
{
    Bvh4Node &w = u.nodes[idx];
    const uint32_t *kw = u.keep ? u.keep + (size_t)idx * kKeepWords : nullptr;
    BvhQ3Node q;
    if (u.q3nodes) q = u.q3nodes[idx];
    uint32_t ql[4] = { 0u, 0u, 0u, 0u };
    if (u.q3nodes) { ql[0] = q.link0; ql[1] = q.link1; ql[2] = q.link2; ql[3] = q.link3; }
    for (int c = 0; c < 4; ++c) {
        // (with the kept words: the pack's link and count, which the slot holds when something below it is alive)
        const uint32_t link = kw ? kw[c] : refit_f32_bits(w.a[c].w), count = kw ? kw[4 + c] : refit_f32_bits(w.b[c].w);
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
            if (lo[0] <= hi[0]) { lo[2] = -INFINITY; hi[2] = INFINITY; }             // (four empty rectangles: the nothing box)
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
        if (!kw) continue;
        // nothing alive below (every entry hidden, every slot of the child empty): the union is the nothing box on every axis -- the
        // pack's empty slot, link 0 and count ~0; else the pack's words again
        const bool alive = lo[0] <= hi[0] && lo[1] <= hi[1];
        w.a[c].w = refit_bits_f32(alive ? link : 0u);
        w.b[c].w = refit_bits_f32(alive ? count : 0xFFFFFFFFu);
        ql[c] = alive ? kw[8 + c] : (kQNodeEmpty << kQNodeShift);
    }
    if (!u.q3nodes) return true;
    q.link0 = ql[0]; q.link1 = ql[1]; q.link2 = ql[2]; q.link3 = ql[3];
    if (!q3_encode(w, u.abs_pad, q)) return false;
    u.q3nodes[idx] = q;
    return true;
}

// Mode E: the kept words of wide node `idx` (flat: kBvhFlatNode was set in its level entry), read from the arrays as the pack left
// them -- the first visibility call after a pack runs it before anything else.
RTX_HD void capture_keep(const UpdateArgs &u, uint32_t entry)
{
    const uint32_t idx = entry & ~kBvhFlatNode;
    const Bvh4Node &w = u.nodes[idx];
    uint32_t *kw = u.keep + (size_t)idx * kKeepWords;
    if (entry & kBvhFlatNode) {
        const float lk[4] = { w.b[0].x, w.b[0].y, w.b[0].z, w.b[0].w }, ct[4] = { w.b[1].x, w.b[1].y, w.b[1].z, w.b[1].w };
        for (int c = 0; c < 4; ++c) { kw[c] = refit_f32_bits(lk[c]); kw[4 + c] = refit_f32_bits(ct[c]); kw[8 + c] = u.qnodes ? u.qnodes[idx].link[c] : 0u; }
        return;
    }
    for (int c = 0; c < 4; ++c) { kw[c] = refit_f32_bits(w.a[c].w); kw[4 + c] = refit_f32_bits(w.b[c].w); }
    kw[8] = kw[9] = kw[10] = kw[11] = 0u;
    if (u.q3nodes) { const BvhQ3Node &q = u.q3nodes[idx]; kw[8] = q.link0; kw[9] = q.link1; kw[10] = q.link2; kw[11] = q.link3; }
}

// One entry of a level list: the status bits its node raises.
RTX_HD unsigned long long refit_level_entry(const UpdateArgs &u, uint32_t entry)
{
    if (entry & kBvhFlatNode) return refit_flat_node(u, entry & ~kBvhFlatNode) ? 0ull : kUpdateStatusNoQ;
    return refit_node(u, entry) ? 0ull : kUpdateStatusNoQ3;
}

}  // namespace rtx
