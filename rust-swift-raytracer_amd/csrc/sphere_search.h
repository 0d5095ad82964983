// sphere_search.h -- World::hit over the spheres: brute force in file order, and the exact BVH
// (bvh.h) from global memory, from the workgroup's LDS copy (box records) and from
// the corner-record LDS image; stage_tree copies the tree into LDS.
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include "device_math.h"

namespace rtamd {
namespace {

// ------------------------------------------------------------ sphere stage
// Brute force, file order, shrinking t_max (common.rs:241-247).  Batches of
// kBatch spheres: all scalar loads issue up front, the discriminants
// (independent of t_max) are computed for the whole batch, and the in-order
// root/t_max updates run only when some lane's discriminant is non-negative
// (rare; wave-uniform skip).
// The last batch tests only the scene's spheres: a wave-uniform guard skips
// the padding's arithmetic (world.txt's 9 spheres took 16 tests per ray with
// padded batches).
template <bool kWaveGuard>
__device__ __forceinline__ void spheres_brute(const TraceParams &p, F3 org, F3 dir, float &best_t,
                                              int &best_i) {
    const float tmin = 0.001f;
    const uint32_t n = p.nsph;
    for (uint32_t i0 = 0; i0 < n; i0 += kBatch) {
        const uint32_t m = n - i0;  // spheres left (>= kBatch except in the last batch)
        float hb[kBatch], disc[kBatch];
        bool any = false;
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            hb[k] = 0.0f;
            disc[k] = -1.0f;
            if (k != 0u && k >= m) continue;  // (wave-uniform)
            const float4 S = uniform_load(p.sph_hot, i0 + k);
            const float ocx = org.x - S.x, ocy = org.y - S.y, ocz = org.z - S.z;
            hb[k] = (ocx * dir.x + ocy * dir.y) + ocz * dir.z;
            const float cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - S.w;
            disc[k] = hb[k] * hb[k] - cc;  // a == 1.0 exactly (maths.rs:127)
            any |= disc[k] >= 0.0f;
        }
        if (!any) continue;
#pragma unroll
        for (uint32_t k = 0; k < kBatch; ++k) {
            if (disc[k] >= 0.0f) {
                const float sq = xsqrt<kWaveGuard>(disc[k]);
                const float r1 = -hb[k] - sq;
                const float r2 = -hb[k] + sq;
                const bool ok1 = (tmin < r1) && (r1 < best_t);
                const bool ok2 = (tmin < r2) && (r2 < best_t);
                if (ok1 || ok2) {
                    best_t = ok1 ? r1 : r2;  // r1 <= r2: the smaller valid root
                    best_i = (int)(i0 + k);
                }
            }
        }
    }
}

// One sphere in any order: same arithmetic as Sphere::hit (common.rs:74-92);
// the candidate (root1 if > t_min, else root2 if > t_min) is independent of
// t_max, and the reference keeps the smallest candidate, lowest index first.
template <bool kWaveGuard>
__device__ __forceinline__ bool sphere_candidate(float4 S, F3 org, F3 dir, int idx, float &best_t,
                                                 int &best_i) {
    const float tmin = 0.001f;
    const float ocx = org.x - S.x, ocy = org.y - S.y, ocz = org.z - S.z;
    const float hb = (ocx * dir.x + ocy * dir.y) + ocz * dir.z;
    const float cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - S.w;
    const float disc = hb * hb - cc;
    if (!(disc >= 0.0f)) return false;
    const float sq = xsqrt<kWaveGuard>(disc);
    const float r1 = -hb - sq;
    const float r2 = -hb + sq;
    const bool v1 = tmin < r1;
    const float c = v1 ? r1 : r2;
    const bool valid = v1 || (tmin < r2);
    // c < best_t || (c == best_t && best_t < inf && idx < best_i) as one
    // unsigned compare of (t bits, index) keys: both t are positive (c > t_min,
    // best_t > t_min or +inf), so their bits order like the values; best_i is
    // -1 (all ones) only while best_t is +inf, and c = +inf, which that rule
    // never takes, is excluded
    const uint64_t kc = ((uint64_t)__float_as_uint(c) << 32) | (uint32_t)idx;
    const uint64_t kb = ((uint64_t)__float_as_uint(best_t) << 32) | (uint32_t)best_i;
    // (a block of its own around the compare and the two moves: folding it into
    // the select mask of two v_cndmask measured 0.016 ms slower on C2 and 0.19 ms
    // on C3)
    const bool take = valid && c != __builtin_inff() && kc < kb;
    if (take) { best_t = c; best_i = idx; }
    return take;
}

constexpr float kErrK = 3.0e-3f;  // >= 2.7x the derived sqrt(30u) = 1.12e-3

// Where the traversal reads the tree from: global memory (any size) or the
// workgroup's LDS copy (staged once per persistent workgroup).
struct BvhView {
    const float4 *nodes;     // global: 2 per node; LDS: 64-B records (box | 8 x u32 link pairs),
                             // or 128-B corner records (8 x (near corner | link pair); corner::trace_kernel)
    const uint32_t *miss32;  // global: 8 x u32 per node
    const uint16_t *miss16;  // (unused: the LDS links live in the node records)
    const float4 *prims;
    const uint32_t *ids;
    const float4 *shade;     // per-sphere shading records (2 x float4): LDS, or (global walk, corner records)
    const uint32_t *kinds;   // p.sph_shade / p.sph_kind in global memory
};

// Spheres through the exact-pruning BVH (bvh.h): big spheres first (brute
// force, wave-uniform), then a stackless octant-ordered traversal that the
// kernel can advance a bounded number of nodes per loop iteration.  Every
// node box is inflated per ray by e, which bounds how far a computed
// candidate's point can lie outside its sphere: with
// s = min(A, best_t + R)(1+3K) + R >= |o - c| + r for every sphere that can
// still win, the squared-distance excess is <= 30u s^2, so the point is
// within min(sqrt(30u) s, 15u s^2 / r) of the surface.  e takes the smaller
// of K s (K = 3e-3) and Kq s^2 / rmin (Kq = 40.5u), both 2.7x the bound,
// plus e_abs for the slab arithmetic.  A node is skipped only when the
// inflated box is certainly missed or certainly starts beyond best_t.
__device__ __forceinline__ float slab_rcp(float d) {
    return __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d), -1e20f, 1e20f);
}

struct SphBound { float A, e_abs; };  // per-ray inputs of the inflation
__device__ __forceinline__ SphBound sph_bound(const TraceParams &p, F3 org) {
    const float ax = org.x - p.bvh_c[0], ay = org.y - p.bvh_c[1], az = org.z - p.bvh_c[2];
    // (v_sqrt_f32, <= 1 ulp: the 1e-5 factor covers it; A is only a bound)
    return SphBound{__builtin_amdgcn_sqrtf((ax * ax + ay * ay) + az * az) * 1.00001f + p.bvh_r,
                    2e-6f * ((fabsf(org.x) + fabsf(org.y)) + fabsf(org.z) + p.bvh_mag)};
}
constexpr float kErrKq = 40.5f * 0x1p-24f;  // 2.7 x 15u
__device__ __forceinline__ float sph_inflation(const TraceParams &p, SphBound b, float bt) {
    const float s = fminf(b.A, bt + p.bvh_rmax) * (1.0f + 3.0f * kErrK) + p.bvh_rmax;  // fminf(A, inf) = A
    // fminf drops the NaN of 0 * inf (rmin == 0): the linear bound then applies
    return fminf(kErrK * s, (kErrKq * s) * (s * p.bvh_inv_rmin)) + b.e_abs;
}

// kPeel (the plain instance): the first big sphere's record and id are read
// at once and whatever nbig is -- both arrays hold an entry even when no sphere
// is big (device_state.cpp) -- so one wait covers them and the count; the loop
// takes the others.
template <bool kWaveGuard, bool kPeel = false>
__device__ __forceinline__ void spheres_big(const TraceParams &p, F3 org, F3 dir, float &best_t,
                                            int &best_i) {
    if constexpr (kPeel) {
        const uint32_t n = p.nbig;
        const float4 S0 = uniform_load(p.big_hot, 0);
        const int id0 = (int)uniform_load_u32(p.big_id, 0);
        if (n != 0u) sphere_candidate<kWaveGuard>(S0, org, dir, id0, best_t, best_i);
        for (uint32_t k = 1; k < n; ++k)
            sphere_candidate<kWaveGuard>(uniform_load(p.big_hot, k), org, dir, (int)uniform_load_u32(p.big_id, k),
                                         best_t, best_i);
        return;
    }
    for (uint32_t k = 0; k < p.nbig; ++k) {
        // (both scalar loads: a vector load here made the ray setup wait on
        // every outstanding vector memory op, vmcnt(0))
        const float4 S = uniform_load(p.big_hot, k);
        sphere_candidate<kWaveGuard>(S, org, dir, (int)uniform_load_u32(p.big_id, k), best_t, best_i);
    }
}

// One node of the sphere tree.  node becomes the end marker when the search
// is over: kNodeEndDev, or 0xFFFF for the LDS copy's u16 links.  A leaf the
// ray enters is handed back in `leaf` as (first << 3) | count for
// sphere_leaf.  (Deferring leaf tests until every lane of the wave has one
// pending -- "while-while" -- measured 6% slower on C2 and 60% on C5.)
// kLds: `ooff` = 4 * octant (the link word's offset in the record); global
// memory: `ooff` = the octant, `octm` unused.
template <bool kLds>
__device__ __forceinline__ bool sphere_node(const BvhView &v, F3 inv, uint32_t ooff, float best_t, F3 nlo,
                                            F3 nhi, uint32_t &node, uint32_t &leaf, uint32_t &node_tests) {
    ++node_tests;
    // LDS copy: `node` is the record's LDS byte address (64-B records: box |
    // per octant one u32 of two u16 links: the node to visit next when the box
    // is entered -- the near child, or for a leaf its miss link -- and when it
    // is skipped), so the next node is one select of a half of one LDS word
    float4 B0, B1;
    uint32_t miss, hit = 0;
    if (kLds) {
#if defined(__HIP_DEVICE_COMPILE__)
        // `node` is the record's LDS address (staged as such: no base add)
        typedef const __attribute__((address_space(3))) char *lds_cptr;
        const lds_cptr rec = (lds_cptr)(uintptr_t)node;
        B0 = *(const __attribute__((address_space(3))) float4 *)rec;
        B1 = *(const __attribute__((address_space(3))) float4 *)(rec + 16);
        const uint32_t lw = *(const __attribute__((address_space(3))) uint32_t *)(rec + 32 + ooff);
        hit = lw & 0xFFFFu;
        miss = lw >> 16;
#else
        B0 = B1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        miss = 0;
#endif
    } else {
        B0 = v.nodes[2 * node];
        B1 = v.nodes[2 * node + 1];
        miss = v.miss32[8 * node + ooff];
    }
    // Slab values b * inv - lo * inv as one fma each, nlo = -(lo * inv) per ray
    // (sphere_slabs): the result is the exact slab value of a face moved by
    // <= u|lo| + 3u|b - lo| (rounded lo * inv, rcp, the fma's rounding), which
    // e_abs = 2e-6 (|o|_1 + M) covers ~8x, so [tn, tf] is the exact interval
    // of a box that still contains every inflated sphere of the node: plain
    // comparisons are safe.  inv is finite (ray setup), so no 0 * inf NaN.
    // lo = o + e, hi = o - e:  (bmin - e) - o == bmin - (o + e)
    const float t0x = __builtin_fmaf(B0.x, inv.x, nlo.x), t1x = __builtin_fmaf(B1.x, inv.x, nhi.x);
    const float t0y = __builtin_fmaf(B0.y, inv.y, nlo.y), t1y = __builtin_fmaf(B1.y, inv.y, nhi.y);
    const float t0z = __builtin_fmaf(B0.z, inv.z, nlo.z), t1z = __builtin_fmaf(B1.z, inv.z, nhi.z);
    const float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
    const float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
    // tn > best_t as a signed-integer compare: best_t is positive (or +inf)
    // and tn is finite for any ray that can produce a candidate (inv and the
    // slab offsets are finite), so the orders agree; a NaN ray has no
    // candidate, so skipping for it changes nothing.  (As a float compare the
    // compiler folds it into tn > min(tf, best_t) and canonicalises best_t at
    // every node.)
    const bool skip = tn > tf || tf < 0.001f || __float_as_int(tn) > __float_as_int(best_t);
    if (kLds) {
        // staged leaf word: (first << 3) | count for a leaf (count >= 1), 0 else
        leaf = __float_as_uint(B0.w);
        node = skip ? miss : hit;
        return !skip && leaf != 0u;
    }
    const uint32_t a = __float_as_uint(B0.w);
    const bool is_leaf = (a & kLeafBitDev) != 0;
    // near child first
    const uint32_t child = a + ((ooff >> __float_as_uint(B1.w)) & 1u);
    node = (skip || is_leaf) ? miss : child;
    // (returned as a flag, so the caller branches on it directly; leaf is only
    // read when it is set)
    leaf = ((a & ~kLeafBitDev) << 3) | __float_as_uint(B1.w);
    return !skip && is_leaf;
}

// One node of the corner-record LDS tree (bvh.h SphereBVH::corner): the same
// test as sphere_node from two reads, the ray octant's near corner with its
// link word and the far corner (the near corner of octant 7 - o).  `node` is a
// node index; offn / offf = the LDS base plus the two slots' offsets in a
// record (16 o and 16 (7 - o)); nn / nf = the near and far faces' slab offsets
// (sphere_corner_slabs).  Picking the near face by the sign of inv instead of
// min / max gives the same tn and tf bit for bit: per axis the far value
// exceeds the near one (DESIGN.md 5.2 point 4), so min and max would pick the
// same two values.  v_max3 / v_min3 drop a NaN operand like fminf / fmaxf do
// and give NaN when all three are, which no compare below takes for a skip.
// tn_out, lw_out (the deferred walk records them for a leaf it enters): the
// box's t_near, which the third skip condition compared, and the link word.
__device__ __forceinline__ bool sphere_node_corner(uint32_t offn, uint32_t offf, F3 inv, float best_t, F3 nn,
                                                   F3 nf, uint32_t &node, uint32_t &leaf, uint32_t &node_tests,
                                                   float &tn_out, uint32_t &lw_out, bool &any_leaf) {
    ++node_tests;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef float f3v __attribute__((ext_vector_type(3)));
    // (node << 7) + offset as one v_lshl_add_u32 per read: the compiler shares
    // the shift between the two addresses instead, three instructions
    uint32_t an, af;
    asm("v_lshl_add_u32 %0, %1, 7, %2" : "=v"(an) : "v"(node), "v"(offn));
    asm("v_lshl_add_u32 %0, %1, 7, %2" : "=v"(af) : "v"(node), "v"(offf));
    const float4 N = *(const __attribute__((address_space(3))) float4 *)(uintptr_t)an;
    const f3v Fc = *(const __attribute__((address_space(3))) f3v *)(uintptr_t)af;
    const float tnx = __builtin_fmaf(N.x, inv.x, nn.x), tfx = __builtin_fmaf(Fc.x, inv.x, nf.x);
    const float tny = __builtin_fmaf(N.y, inv.y, nn.y), tfy = __builtin_fmaf(Fc.y, inv.y, nf.y);
    const float tnz = __builtin_fmaf(N.z, inv.z, nn.z), tfz = __builtin_fmaf(Fc.z, inv.z, nf.z);
    const float tn = fmaxf(fmaxf(tnx, tny), tnz);
    const float tf = fminf(fminf(tfx, tfy), tfz);
    // (the three skip conditions of sphere_node)
    const bool skip = tn > tf || tf < 0.001f || __float_as_int(tn) > __float_as_int(best_t);
    // link word: miss | next << 16, a leaf's upper half = kCornerLeaf | leaf word
    // (the sign bit), its next node the miss link
    const uint32_t lw = __float_as_uint(N.w);
    const bool is_leaf = (int32_t)lw < 0;
    node = (skip || is_leaf) ? (lw & 0xFFFFu) : (lw >> 16);
    leaf = (lw >> 16) & 0x7FFFu;
    tn_out = tn;
    lw_out = lw;
    // (whether some lane of the wave enters a leaf, from ballots of the
    // compares themselves: each is the compare's own result mask, no VALU.
    // max(tn, 0.001) > tf is `tn > tf || tf < 0.001f`, NaN operands included:
    // the form the compiler gives the first two skip conditions anyway)
    any_leaf = (__builtin_amdgcn_ballot_w64(is_leaf) &
                ~(__builtin_amdgcn_ballot_w64(fmaxf(tn, 0.001f) > tf) |
                  __builtin_amdgcn_ballot_w64(__float_as_int(tn) > __float_as_int(best_t)))) != 0;
    return !skip && is_leaf;
#else
    (void)offn; (void)offf; (void)inv; (void)best_t; (void)nn; (void)nf;
    node = 0xFFFFu;
    leaf = 0;
    tn_out = 0.0f;
    lw_out = 0;
    any_leaf = false;
    return false;
#endif
}
__device__ __forceinline__ bool sphere_node_corner(uint32_t offn, uint32_t offf, F3 inv, float best_t, F3 nn,
                                                   F3 nf, uint32_t &node, uint32_t &leaf, uint32_t &node_tests) {
    float tn;
    uint32_t lw;
    bool any_leaf;
    return sphere_node_corner(offn, offf, inv, best_t, nn, nf, node, leaf, node_tests, tn, lw, any_leaf);
}

// The corner walk's first node (an index): the root's near child for the
// ray's octant, as sphere_walk_entry.  lbase: the image's LDS address.
__device__ __forceinline__ uint32_t sphere_corner_entry(uint32_t lbase, uint32_t oct, uint32_t nnodes) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (nnodes > 1u)
        return *(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)(lbase + 16u * oct + 12u) >> 16;
#endif
    (void)lbase; (void)oct; (void)nnodes;
    return 0;
}

// The corner walk's slab offsets: sphere_slabs' values, sorted per axis by the
// ray's octant.  The near face is lo where the direction is positive (offset
// -((o + e) inv), sphere_slabs' nlo) and hi where it is negative (-((o - e)
// inv), its nhi); the far face takes the other one.
__device__ __forceinline__ void sphere_corner_slabs(F3 org, F3 inv, float e, uint32_t oct, F3 &nn, F3 &nf) {
    const float ex = (oct & 1u) ? -e : e, ey = (oct & 2u) ? -e : e, ez = (oct & 4u) ? -e : e;
    nn = f3(-((org.x + ex) * inv.x), -((org.y + ey) * inv.y), -((org.z + ez) * inv.z));
    nf = f3(-((org.x - ex) * inv.x), -((org.y - ey) * inv.y), -((org.z - ez) * inv.z));
}

// The walk's first node.  With the LDS tree the root's own box test is
// skipped: the walk starts at the root's near child for the ray's octant (the
// root's `next` link).  The root box holds every tree sphere, so skipping its
// test only forgoes a cull (exact); a ray that starts inside
// the scene's box -- nearly every ray -- enters it anyway (one node test per
// walk fewer).  A one-node tree (the root a leaf) starts at the root.
template <bool kLds>
__device__ __forceinline__ uint32_t sphere_walk_entry(uint32_t root, uint32_t oct, uint32_t nnodes) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (kLds && nnodes > 1u) {
        typedef const __attribute__((address_space(3))) char *lds_cptr;
        return *(const __attribute__((address_space(3))) uint32_t *)((lds_cptr)(uintptr_t)root + 32 + 4u * oct) &
               0xFFFFu;
    }
#endif
    (void)oct;
    (void)nnodes;
    return root;
}

// The walk's per-ray slab offsets for inflation e: nlo = -((o + e) inv),
// nhi = -((o - e) inv).
__device__ __forceinline__ void sphere_slabs(F3 org, F3 inv, float e, F3 &nlo, F3 &nhi) {
    nlo = f3(-((org.x + e) * inv.x), -((org.y + e) * inv.y), -((org.z + e) * inv.z));
    nhi = f3(-((org.x - e) * inv.x), -((org.y - e) * inv.y), -((org.z - e) * inv.z));
}

// Tests a pending leaf.  The node boxes keep the inflation derived from the
// best t at the walk's start: a larger best t only inflates them more (still
// exact), and re-deriving it after every new best (the round-1
// to round-4 code) cost ~20 VALU per improvement for boxes ~1 % tighter.
// kAhead (LDS copies only): the second sphere's record and index are read
// with the first one's, before the first test, so a two-sphere leaf waits for
// the LDS once; a one-sphere leaf's read of entry first + 1 stays inside the
// workgroup's LDS image (the id words follow the records) and is not used.
template <bool kWaveGuard, bool kAhead = false>
__device__ __forceinline__ void sphere_leaf(const BvhView &v, F3 org, F3 dir, uint32_t leaf, float &best_t,
                                            int &best_i, uint32_t &sph_tests) {
    const uint32_t first = leaf >> 3, n = leaf & 7u;
    // leaves hold 1 or 2 spheres (leaf size 2): straight-line tests, the loop
    // only for larger leaves (RT_AMD_LEAF)
    sph_tests += n;
    float4 S1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    int i1 = 0;
    if (kAhead) {
        S1 = v.prims[first + 1];
        i1 = (int)v.ids[first + 1];
    }
    sphere_candidate<kWaveGuard>(v.prims[first], org, dir, (int)v.ids[first], best_t, best_i);
    if (n > 1u) {
        if (!kAhead) {
            S1 = v.prims[first + 1];
            i1 = (int)v.ids[first + 1];
        }
        sphere_candidate<kWaveGuard>(S1, org, dir, i1, best_t, best_i);
        for (uint32_t j = first + 2; j < first + n; ++j)
            sphere_candidate<kWaveGuard>(v.prims[j], org, dir, (int)v.ids[j], best_t, best_i);
    }
}

// The sphere tree's view for a kernel; kLds: copied into the workgroup's LDS
// (one barrier).  Returns the walk's first node (its LDS address with kLds).
// LDS layout: node records (64 B: box float4 x 2 | 8 x u32 links) | prims
// (float4) | shade (2 x float4 / sphere) | ids (u32) | kinds (u32), at the
// start of the dynamic LDS (trace_lds_bytes).  A record is
//   (lo.xyz, leaf word) (hi.xyz, 0) and, per ray octant o, the u32
//   next(o) | miss(o) << 16: the node to visit when the box is entered (the
//   near child along the split axis for the octant's sign, the DFS order of
//   bvh.h; a leaf's own miss link) and when it is skipped,
// with the leaf word (first << 3) | count for leaves and 0 for inner nodes.
// Node references are record LDS addresses (base + index * 64; the kernels
// have no static LDS before it, so base is 0 and they stay below 0xFFFF: the
// copy holds <= kLdsTreeMaxNodes nodes); 0xFFFF stays the end marker.
// Corner layout (kCorner instances: sphere-only frame kernels): corner records
// (128 B, bvh.h SphereBVH::corner, `corner`, copied verbatim: their links are
// node indices) | prims (float4) | ids (u32).  The shading records and kinds
// are not staged: view.shade / view.kinds point at p.sph_shade / p.sph_kind.
// Returns the image's LDS address.
template <bool kLds, bool kCorner>
__device__ __forceinline__ uint32_t stage_tree(const TraceParams &p, const uint4 *corner, float4 *lds,
                                               BvhView &view) {
    if (!kLds) {
        view = BvhView{p.bvh_nodes, p.bvh_miss, nullptr, p.bvh_prims, p.bvh_prim_id,
                       p.sph_shade, p.sph_kind};
        return 0;
    }
    float4 *n4 = lds;
    const uint32_t lbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) float4 *)lds;
    if (kCorner) {
        float4 *c4 = n4 + 8u * p.nnodes;
        uint32_t *cid = reinterpret_cast<uint32_t *>(c4 + p.nprims);
        const float4 *g = reinterpret_cast<const float4 *>(corner);
        for (uint32_t i = threadIdx.x; i < 8u * p.nnodes; i += blockDim.x) n4[i] = g[i];
        for (uint32_t i = threadIdx.x; i < p.nprims; i += blockDim.x) {
            c4[i] = p.bvh_prims[i];
            cid[i] = p.bvh_prim_id[i];
        }
        __syncthreads();
        view = BvhView{n4, nullptr, nullptr, c4, cid, p.sph_shade, p.sph_kind};
        return lbase;
    }
    float4 *p4 = n4 + 4 * p.nnodes;
    float4 *s4 = p4 + p.nprims;
    uint32_t *id = reinterpret_cast<uint32_t *>(s4 + 2 * p.nsph_padded);
    uint32_t *kd = id + p.nprims;
    const uint16_t *g16 = p.bvh_miss16;
    auto addr = [&](uint32_t l) { return l == 0xFFFFu ? 0xFFFFu : lbase + l * 64u; };
    for (uint32_t i = threadIdx.x; i < p.nnodes; i += blockDim.x) {
        float4 b0 = p.bvh_nodes[2 * i];
        const uint32_t a = __float_as_uint(b0.w);
        float4 b1 = p.bvh_nodes[2 * i + 1];
        const bool is_leaf = (a & kLeafBitDev) != 0;
        const uint32_t axis = __float_as_uint(b1.w);  // (leaves: the count)
        b0.w = __uint_as_float(is_leaf ? ((a & ~kLeafBitDev) << 3) | axis : 0u);
        b1.w = 0.0f;
        n4[4 * i] = b0;
        n4[4 * i + 1] = b1;
        uint32_t w[8];
        for (uint32_t o = 0; o < 8; ++o) {
            const uint32_t miss = addr(g16[8 * i + o]);
            const uint32_t next = is_leaf ? miss : lbase + (a + ((o >> axis) & 1u)) * 64u;
            w[o] = next | (miss << 16);
        }
        n4[4 * i + 2] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]),
                                    __uint_as_float(w[3]));
        n4[4 * i + 3] = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]),
                                    __uint_as_float(w[7]));
    }
    for (uint32_t i = threadIdx.x; i < p.nprims; i += blockDim.x) {
        p4[i] = p.bvh_prims[i];
        id[i] = p.bvh_prim_id[i];
    }
    for (uint32_t i = threadIdx.x; i < p.nsph_padded; i += blockDim.x) {
        s4[2 * i] = p.sph_shade[2 * i];
        s4[2 * i + 1] = p.sph_shade[2 * i + 1];
        kd[i] = p.sph_kind[i];
    }
    __syncthreads();
    view = BvhView{n4, nullptr, nullptr, p4, id, s4, kd};
    return lbase;
}

}  // namespace
}  // namespace rtamd
