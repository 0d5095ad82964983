// tri_search.h -- Mesh::hit: brute force in file order, the phantom-aware triangle trees (binary
// and 4-wide nodes, bvh.h) and the primary strip lists.
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include "device_math.h"
#include "serial_jobs.h"

namespace rtamd {
namespace {

// ------------------------------------------------------------ triangle stage
// Triangle::intersect (common.rs:129-166), after the t-range check passed:
// the three edge tests against the hit point o + t*d.
__device__ __forceinline__ bool tri_edges(F3 n, F3 v0, F3 v1, F3 v2, F3 pt) {
    if (dot(n, cross(v1 - v0, pt - v0)) < 0.0f) return false;
    if (dot(n, cross(v2 - v1, pt - v1)) < 0.0f) return false;
    if (dot(n, cross(v0 - v2, pt - v2)) < 0.0f) return false;
    return true;
}

// The reference's plane step and t-range check (common.rs:131-150), with its
// sign: t = (n.o + d) / cos; false when |cos| < 1e-8 or t is out of range.
__device__ __forceinline__ bool tri_plane(float4 N, F3 org, F3 dir, float best_t, float &t) {
    const float cosl = (N.x * dir.x + N.y * dir.y) + N.z * dir.z;
    if (-1e-8f < cosl && cosl < 1e-8f) return false;
    t = (((N.x * org.x + N.y * org.y) + N.z * org.z) + N.w) / cosl;
    return !(t < 0.001f || t > best_t);
}

// Mesh::hit (common.rs:178-223) in file order: t_max = best_t, first wins ties.
__device__ __forceinline__ void triangles_brute(const TraceParams &p, F3 org, F3 dir, float best_t,
                                                float &tri_t, int &tri_i, uint32_t &tri_in) {
    const float tmin = 0.001f;
    for (uint32_t j = 0; j < p.ntri; ++j) {
        const float4 N = p.tri_hot[j];
        const float cosl = (N.x * dir.x + N.y * dir.y) + N.z * dir.z;
        if (-1e-8f < cosl && cosl < 1e-8f) continue;
        const float t = (((N.x * org.x + N.y * org.y) + N.z * org.z) + N.w) / cosl;
        if (t < tmin || t > best_t) continue;
        ++tri_in;
        const float4 *g = p.tri_geo + 4u * j;
        const float4 A = g[0], B = g[1], Cc = g[2];
        if (!tri_edges(f3(N.x, N.y, N.z), f3(A.x, A.y, A.z), f3(B.x, B.y, B.z), f3(Cc.x, Cc.y, Cc.z),
                       org + scale(dir, t)))
            continue;
        if (t < tri_t) { tri_t = t; tri_i = (int)j; }
    }
}

// One triangle in any order, with the reference's winner: the smallest
// accepted t, lowest index on ties (a NaN/inf t is never recorded).
__device__ __forceinline__ bool tri_merge(float t, int idx, float &tri_t, int &tri_i) {
    const bool take = t < tri_t || (t == tri_t && tri_t < __builtin_inff() && idx < tri_i);
    if (take) { tri_t = t; tri_i = idx; }
    return take;
}

// One tree-ordered triangle record (bvh.h TriangleBVH::tris).
__device__ __forceinline__ bool tri_record(const float4 *r, F3 org, F3 dir, float best_t,
                                           float &tri_t, int &tri_i, uint32_t &tri_in) {
    const float4 N = r[0];
    float t;
    if (!tri_plane(N, org, dir, best_t, t)) return false;
    ++tri_in;
    const float4 A = r[1], B = r[2], Cc = r[3];
    if (!tri_edges(f3(N.x, N.y, N.z), f3(A.x, A.y, A.z), f3(B.x, B.y, B.z), f3(Cc.x, Cc.y, Cc.z),
                   org + scale(dir, t)))
        return false;
    return tri_merge(t, (int)__float_as_uint(A.w), tri_t, tri_i);
}

// Triangles through the phantom-aware BVH (bvh.h).  An accepted hit lies on
// its triangle translated by 2(n^.o)n^ (the reference's sign of n.o), up to
// rounding.  Per node the kernel bounds s = n^.o over the node's normal box,
// widens the box by the interval of 2 s m_k on each axis k (m over the normal
// box) plus rho, a rounding margin that dominates every error term
// (<= ~40u (dist + |o| + M)), and skips only nodes the ray
// certainly misses or enters beyond min(best_t, tri_t).
//
// cam (bounce 0, org == camera origin): the lane walks the camera-origin tree
// instead, whose boxes already are the phantoms of that origin padded by rho
// (bvh.h CameraTriangleBVH) -- same step, no widening, so lanes at bounce 0
// and lanes further down their paths do not serialise.
//
// tri_begin: brute-forced triangles, then the walk's margin.  Returns false
// when the walk is not needed (far / non-finite origin: every record is tested
// here instead -- the margins would overflow; same result by the
// order-independent merge).
__device__ __forceinline__ bool tri_begin(const TraceParams &p, F3 org, F3 dir, float best_t,
                                          bool cam, float &rho, float &tri_t, int &tri_i,
                                          uint32_t &tri_in, uint32_t &tri_done) {
    tri_done += p.tloose;
    for (uint32_t k = 0; k < p.tloose; ++k) {  // slivers / non-finite data
        const uint32_t j = p.tbvh_loose[k];
        const float4 N = p.tri_hot[j];
        float t;
        if (!tri_plane(N, org, dir, best_t, t)) continue;
        ++tri_in;
        const float4 *g = p.tri_geo + 4u * j;
        const float4 A = g[0], B = g[1], Cc = g[2];
        if (tri_edges(f3(N.x, N.y, N.z), f3(A.x, A.y, A.z), f3(B.x, B.y, B.z), f3(Cc.x, Cc.y, Cc.z),
                      org + scale(dir, t)))
            tri_merge(t, (int)j, tri_t, tri_i);
    }
    const float onorm = (fabsf(org.x) + fabsf(org.y)) + fabsf(org.z);
    if (!cam && !(onorm < 1e18f)) {
        tri_done += p.ttris;
        for (uint32_t j = 0; j < p.ttris; ++j)
            tri_record(p.tbvh_tris + 4u * j, org, dir, best_t, tri_t, tri_i, tri_in);
        return false;
    }
    // distance from o to any phantom point: |o - c| + radius + 2|o|
    const float dist = ((fabsf(org.x - p.tbvh_c[0]) + fabsf(org.y - p.tbvh_c[1])) +
                        fabsf(org.z - p.tbvh_c[2])) + p.tbvh_r + 2.0f * onorm;
    rho = cam ? 0.0f : 1e-5f * ((dist + onorm) + p.tbvh_mag);
    return true;
}

// One node of the triangle tree (static or camera-origin); an entered leaf is
// handed back in `leaf` as (first << 3) | count, like sphere_node.
__device__ __forceinline__ bool tri_node(const TraceParams &p, F3 nlo, F3 nhi, F3 inv, F3 dlt2, bool cam,
                                         float cap, uint32_t &node, uint32_t &leaf,
                                         uint32_t &node_tests) {
    ++node_tests;
    // Quantised nodes (bvh.h QuantGrid): u16 coordinates decoded with one fma
    // on the tree's grid; the host rounds every face outward *after* this
    // exact decode, so a decoded box contains the float box.
    // one 32-B sector per node: (static) box | normals | a | link,
    // (camera) box | a | link; fixed child-a-first order (bvh.cpp)
    const uint4 *qn = (cam ? p.cam_nodes : p.tbvh_nodes) + 2u * node;
    const uint4 q0 = qn[0], q1 = qn[1];
    const uint32_t a = cam ? q0.w : q1.z;
    const uint32_t miss = cam ? q1.x : q1.w;
    const float gbx = cam ? p.cq_base[0] : p.tq_base[0], gsx = cam ? p.cq_step[0] : p.tq_step[0];
    const float gby = cam ? p.cq_base[1] : p.tq_base[1], gsy = cam ? p.cq_step[1] : p.tq_step[1];
    const float gbz = cam ? p.cq_base[2] : p.tq_base[2], gsz = cam ? p.cq_step[2] : p.tq_step[2];
    auto lo16 = [](uint32_t w) { return (float)(w & 0xFFFFu); };
    auto hi16 = [](uint32_t w) { return (float)(w >> 16); };
    const float4 B0 = make_float4(__builtin_fmaf(lo16(q0.x), gsx, gbx), __builtin_fmaf(hi16(q0.x), gsy, gby),
                                  __builtin_fmaf(lo16(q0.y), gsz, gbz), 0.0f);
    const float4 B1 = make_float4(__builtin_fmaf(hi16(q0.y), gsx, gbx), __builtin_fmaf(lo16(q0.z), gsy, gby),
                                  __builtin_fmaf(hi16(q0.z), gsz, gbz), 0.0f);
    // normal box; the camera tree has none (no widening): its lanes decode
    // with a zero grid, so every word of the node is used on every path and
    // the node stays two 16-B loads (with the decode under `if (!cam)` the
    // compiler split the second half into a dword and a dwordx3 load: three
    // memory instructions per node, C5 +24 %)
    const float nb = cam ? 0.0f : p.tq_nbase, ns = cam ? 0.0f : p.tq_nstep;
    const float4 N0 = make_float4(__builtin_fmaf(lo16(q0.w), ns, nb), __builtin_fmaf(hi16(q0.w), ns, nb),
                                  __builtin_fmaf(lo16(q1.x), ns, nb), 0.0f);
    const float4 N1 = make_float4(__builtin_fmaf(hi16(q1.x), ns, nb), __builtin_fmaf(lo16(q1.y), ns, nb),
                                  __builtin_fmaf(hi16(q1.y), ns, nb), 0.0f);
    // 2s = n^.(2d) over the normal box, d = o - oc (the tree's box origin,
    // bvh.h); dlt2 = 2d is exact, so 2s m below has the bits of 2 (s m)
    const float ax = N0.x * dlt2.x, bx = N1.x * dlt2.x;
    const float ay = N0.y * dlt2.y, by = N1.y * dlt2.y;
    const float az = N0.z * dlt2.z, bz = N1.z * dlt2.z;
    const float sl = (fminf(ax, bx) + fminf(ay, by)) + fminf(az, bz);
    const float sh = (fmaxf(ax, bx) + fmaxf(ay, by)) + fmaxf(az, bz);
    // phantom offset 2 s m_k over 2s in [sl, sh], m_k in [N0.k, N1.k]
    auto widen = [&](float lo, float hi, float m0, float m1, float nl, float nh, float iv, float &t0,
                     float &t1) {
        const float a = sl * m0, b = sl * m1, c = sh * m0, d = sh * m1;
        const float omin = fminf(fminf(a, b), fminf(c, d));
        const float omax = fmaxf(fmaxf(a, b), fmaxf(c, d));
        // (l - (o + rho)) inv and (h - (o - rho)) inv, nl = -((o + rho) inv),
        // nh = -((o - rho) inv) per ray (sphere_slabs with e = rho): the faces
        // move out by rho, plus <= u|o + rho| + 3u|l - o| of rounding, far
        // inside rho
        t0 = __builtin_fmaf(lo + omin, iv, nl);
        t1 = __builtin_fmaf(hi + omax, iv, nh);
    };
    float t0x, t1x, t0y, t1y, t0z, t1z;
    widen(B0.x, B1.x, N0.x, N1.x, nlo.x, nhi.x, inv.x, t0x, t1x);
    widen(B0.y, B1.y, N0.y, N1.y, nlo.y, nhi.y, inv.y, t0y, t1y);
    widen(B0.z, B1.z, N0.z, N1.z, nlo.z, nhi.z, inv.z, t0z, t1z);
    const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    // tn > cap as an integer compare (cap > 0 or +inf; see sphere_node: a
    // NaN tn only comes from a NaN ray, which records no triangle)
    const bool skip = tn > tf || tf < 0.001f || __float_as_int(tn) > __float_as_int(cap);
    // a: child | axis << 29, or leaf bit | first << 3 | count
    const bool is_leaf = (a & kLeafBitDev) != 0;
    const uint32_t child = a & 0x1FFFFFFFu;
    node = (skip || is_leaf) ? miss : child;
    leaf = a & ~kLeafBitDev;  // read only when the flag is set
    return !skip && is_leaf;
}

// One child of a 4-wide static-tree node (bvh.h TriangleBVH::wnodes): the
// same decode, widening and skip rule as tri_node's static branch, from the
// child's six box / normal-box words.  Returns whether the child is entered
// (its entry distance in tn).
__device__ __forceinline__ bool tri_wide_child(const TraceParams &p, uint32_t w0, uint32_t w1, uint32_t w2,
                                               uint32_t w3, uint32_t w4, uint32_t w5, F3 nlo, F3 nhi,
                                               F3 inv, F3 dlt2, float cap, float &tn) {
    auto lo16 = [](uint32_t w) { return (float)(w & 0xFFFFu); };
    auto hi16 = [](uint32_t w) { return (float)(w >> 16); };
    const float gsx = p.tq_step[0], gsy = p.tq_step[1], gsz = p.tq_step[2];
    // normal box: halves (exact in f32), one conversion each
    auto h16lo = [](uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xFFFFu)); };
    auto h16hi = [](uint32_t w) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)); };
    // The grid decode is folded into the slab values: nlo / nhi arrive as
    // gb inv + nl and gb inv + nh (the wide walk's set-up), so a face value is
    // (q gs + o) inv + that -- two fmas per face instead of the decode fma, an
    // add and an fma (6 VALU fewer per child; A/B on C5: 149.5 -> 147.6 ms).
    // Rounding: the face moves by <= ~4u (|gb| + |q gs| + |o|) against the
    // exact decode, inside rho = 1e-5 (dist + |o|_1 + M) with the other
    // terms (<= ~40u (dist + |o| + M), tri_begin): the widened box still
    // holds every phantom.
    const float nx0 = h16lo(w3), ny0 = h16hi(w3), nz0 = h16lo(w4);
    const float nx1 = h16hi(w4), ny1 = h16lo(w5), nz1 = h16hi(w5);
    const float ax = nx0 * dlt2.x, bx = nx1 * dlt2.x;
    const float ay = ny0 * dlt2.y, by = ny1 * dlt2.y;
    const float az = nz0 * dlt2.z, bz = nz1 * dlt2.z;
    const float sl = (fminf(ax, bx) + fminf(ay, by)) + fminf(az, bz);
    const float sh = (fmaxf(ax, bx) + fmaxf(ay, by)) + fmaxf(az, bz);
    auto widen = [&](float qlo, float qhi, float m0, float m1, float c0, float c1, float gs, float iv, float &t0,
                     float &t1) {
        const float a = sl * m0, b = sl * m1, c = sh * m0, d = sh * m1;
        const float omin = fminf(fminf(a, b), fminf(c, d));
        const float omax = fmaxf(fmaxf(a, b), fmaxf(c, d));
        t0 = __builtin_fmaf(__builtin_fmaf(qlo, gs, omin), iv, c0);
        t1 = __builtin_fmaf(__builtin_fmaf(qhi, gs, omax), iv, c1);
    };
    float t0x, t1x, t0y, t1y, t0z, t1z;
    widen(lo16(w0), hi16(w1), nx0, nx1, nlo.x, nhi.x, gsx, inv.x, t0x, t1x);
    widen(hi16(w0), lo16(w2), ny0, ny1, nlo.y, nhi.y, gsy, inv.y, t0y, t1y);
    widen(lo16(w1), hi16(w2), nz0, nz1, nlo.z, nhi.z, gsz, inv.z, t0z, t1z);
    tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    return !(tn > tf || tf < 0.001f || __float_as_int(tn) > __float_as_int(cap));
}

__device__ __forceinline__ void tri_leaf(const TraceParams &p, F3 org, F3 dir, bool cam,
                                         uint32_t leaf, float best_t, float &tri_t, int &tri_i,
                                         uint32_t &tri_in, uint32_t &tri_done, const float4 *wrecs = nullptr) {
    // (wrecs: the wide walk's records, TraceParams::tw_tris)
    const float4 *recs = wrecs ? wrecs : cam ? p.cam_tris : p.tbvh_tris;
    const uint32_t first = leaf >> 3, end = first + (leaf & 7u);
    tri_done += leaf & 7u;
    for (uint32_t j = first; j < end; ++j)
        tri_record(recs + 4u * j, org, dir, best_t, tri_t, tri_i, tri_in);
}

// Primary ray against its pixel strip's candidate records (bvh.h
// PrimaryTriLists) plus the `always` records, in any order (tri_merge).
template <bool kSerial>
__device__ __forceinline__ void tri_primary_list(const TraceParams &p, uint32_t job, F3 org, F3 dir,
                                                 float best_t, float &tri_t, int &tri_i,
                                                 uint32_t &tri_in, uint32_t &tri_done) {
    uint32_t s, col, row;
    job_pixel<kSerial>(p, job, s, col, row);
    const uint32_t strip = row * p.ptl_spr + col / kPrimaryTriStripW;
    const uint32_t b = p.ptl_off[strip], e = p.ptl_off[strip + 1];
    tri_done += (e - b) + (p.ptl_end - p.ptl_always);
    for (uint32_t j = b; j < e; ++j)
        tri_record(p.cam_tris + 4u * p.ptl_items[j], org, dir, best_t, tri_t, tri_i, tri_in);
    for (uint32_t j = p.ptl_always; j < p.ptl_end; ++j)
        tri_record(p.cam_tris + 4u * p.ptl_items[j], org, dir, best_t, tri_t, tri_i, tri_in);
}

// The same for an adaptive accumulation pass (trace_body.h AdaptTail): the job's
// launch-local pixel is frame pixel list[lp] (top row first).
__device__ __forceinline__ void tri_primary_list_adapt(const TraceParams &p, const uint32_t *list, uint32_t job,
                                                       F3 org, F3 dir, float best_t, float &tri_t, int &tri_i,
                                                       uint32_t &tri_in, uint32_t &tri_done) {
    const uint32_t idx = list[fdiv(job, p.div_spp)];
    const uint32_t q = fdiv(idx, p.div_width);
    const uint32_t col = idx - q * p.width, row = p.height - 1u - q;
    const uint32_t strip = row * p.ptl_spr + col / kPrimaryTriStripW;
    const uint32_t b = p.ptl_off[strip], e = p.ptl_off[strip + 1];
    tri_done += (e - b) + (p.ptl_end - p.ptl_always);
    for (uint32_t j = b; j < e; ++j)
        tri_record(p.cam_tris + 4u * p.ptl_items[j], org, dir, best_t, tri_t, tri_i, tri_in);
    for (uint32_t j = p.ptl_always; j < p.ptl_end; ++j)
        tri_record(p.cam_tris + 4u * p.ptl_items[j], org, dir, best_t, tri_t, tri_i, tri_in);
}

}  // namespace
}  // namespace rtamd
