// rtx_refit.h -- the arithmetic of rtx_scene_update_objects, written once: scene_update_kernel (rtx_update.hip) and the host
// reference refit_packed (rtx_api.hip) compile from this text, so the device's arrays can be held to the host's bit for bit.
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
    uint32_t slot;                         // sphere in the tree: its leaf entry (the inverse of bvh_prims), else kNoSlot
    uint32_t pad_;
    uint32_t kind, reserved;               // RtxObject, field by field (the C struct is not visible to every includer)
    double geom[9];
    double base_color[3], emission_color[3], roughness;
};
static_assert(sizeof(UpdateEntry) == 16 + 136, "UpdateEntry = 4 words + RtxObject");
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// What one launch of scene_update_kernel works on.  `mode` is launch-uniform:
//   0 (A) records: one thread per entry;  1 (B) one level of wide nodes: one thread per node of `level`;  2 (C) sphere_cmax.
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
    const uint32_t *level;                 // mode B: the node indices of this level
    unsigned long long *status;            // [0]: bit 0 = a 64-byte node could not be encoded;  [1]: the bits of the new sphere_cmax
    double centre[3];
    double abs_pad;
};
constexpr unsigned long long kUpdateStatusNoQ3 = 1ull;

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

// One non-flat wide node: the boxes of its sphere leaves from box32, of its non-flat interior children from those children's four
// boxes (refitted by the previous launch: the levels run deepest first); triangle leaves, footprint children and empty slots stay.
// Link and count words are not touched.  (min / max as comparisons: one answer for -0 against +0 on host and device.)  Returns false when the node's 64-byte form (u.q3nodes != null) cannot be encoded.
RTX_HD bool refit_node(const UpdateArgs &u, uint32_t idx)
{
    Bvh4Node &w = u.nodes[idx];
    for (int c = 0; c < 4; ++c) {
        const uint32_t link = refit_f32_bits(w.a[c].w), count = refit_f32_bits(w.b[c].w);
        if (count == 0xFFFFFFFFu || (count & kBvhTriLeaf)) continue;
        float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
        if (count == 0u) {
            if (link & kBvhFlatNode) continue;
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

}  // namespace rtx
