// serial_coalesce.h -- SERIAL mode's coalescing block search (kRngSerialCoalesce; the mode's other
// kernels: serial.hip).  Its kernels are not in the anonymous namespace.
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include "sphere_search.h"
#include "tri_search.h"

namespace rtamd {

// ---- SERIAL mode: coalescing block search (kRngSerialCoalesce; the mode's
// other kernels: serial.hip)
// The count pass traces every (sample, candidate) pair of an iteration (L K
// traces), yet the candidate paths of a block coalesce: two candidates whose
// offsets meet at some sample share every later step, and in a random walk
// with per-sample variance s^2 only about K / sqrt(pi s^2 n) of K neighbouring
// starts are still distinct after n samples.  Here one workgroup owns one
// block of R samples: it keeps the block's distinct live offsets (sorted, in
// LDS) and the live slot of each of the K candidates of the block's first
// sample, traces each live offset once per sample, and merges equal offsets.
// It writes what serial_walk_blocks_kernel derives from the count table --
// bend (the block end of every candidate, or kWalkLeft | the samples walked)
// and path (the offset of every candidate at every sample) -- so the
// superblock, finish and gather kernels run unchanged.

// One sample of the reference's ray_color (common.rs:263-285) from stream
// state rng, for frame sample j: the number of diffuse/metal scatters b (the
// sample draws 2 + 3b numbers, common.rs:335-336 and 32-38).  The same helper
// arithmetic as trace_kernel's lane state machine, without colours: whole
// walks, the static triangle tree at every bounce (the camera tree and the
// primary lists are exact shortcuts of it), no sphere lists.
template <bool kBvh, bool kLds, int kMesh>
__device__ __forceinline__ uint32_t serial_trace_b(const TraceParams &p, const BvhView &view, uint32_t sph_root,
                                                uint32_t rng, uint32_t j) {
    constexpr bool kWaveGuard = kMesh < 2;  // (as in trace_body)
    const uint32_t pix = fdiv(j, p.div_sspp);
    const uint32_t row = fdiv(pix, p.div_width);
    const uint32_t col = pix - row * p.width;
    const float un = draw_plus(rng, (float)col);  // camera.rs:84-89 via common.rs:335-337
    const float vn = draw_plus(rng, (float)row);
#ifndef RT_NO_XDIV
    const bool xd = p.xdiv_uv != 0;
#else
    const bool xd = false;
#endif
    const float u = xd ? xdiv(un, p.wden, p.wrcp) : un / p.wden;
    const float v = xd ? xdiv(vn, p.hden, p.hrcp) : vn / p.hden;
    const F3 h = f3(p.cam[6], p.cam[7], p.cam[8]);
    const F3 vv = f3(p.cam[9], p.cam[10], p.cam[11]);
    F3 org = f3(p.cam[0], p.cam[1], p.cam[2]);
    const F3 llc = f3(p.cam[3], p.cam[4], p.cam[5]);
    F3 dir = unit<kWaveGuard>(((llc + scale(h, u)) + scale(vv, v)) - org);
    uint32_t b = 0, cnt = 0;  // (cnt: the helpers' work counters, unused)
    for (int32_t bounce = 0; bounce < p.depth; ++bounce) {
        const F3 inv = f3(slab_rcp(dir.x), slab_rcp(dir.y), slab_rcp(dir.z));
        const uint32_t oct = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
        float best_t = __builtin_inff();
        int best_i = -1;
        if (kBvh) {  // World::hit (common.rs:241-247) through the exact tree
            spheres_big<kWaveGuard>(p, org, dir, best_t, best_i);
            constexpr uint32_t kEnd = kLds ? 0xFFFFu : kNodeEndDev;
            const SphBound bnd = sph_bound(p, org);
            F3 nlo, nhi;
            sphere_slabs(org, inv, sph_inflation(p, bnd, best_t), nlo, nhi);
            const uint32_t ooff = kLds ? 4u * oct : oct;
            uint32_t node = sphere_walk_entry<kLds>(sph_root, oct, p.nnodes);
            do {
                uint32_t leaf;
                if (sphere_node<kLds>(view, inv, ooff, best_t, nlo, nhi, node, leaf, cnt))
                    sphere_leaf<kWaveGuard>(view, org, dir, leaf, best_t, best_i, cnt);
            } while (node != kEnd);
        } else {
            spheres_brute<kWaveGuard>(p, org, dir, best_t, best_i);
        }
        float tri_t = __builtin_inff();  // Mesh::hit (common.rs:178-223)
        int tri_i = -1;
        if (kMesh == 2) {
            float e = 0.0f;
            if (tri_begin(p, org, dir, best_t, false, e, tri_t, tri_i, cnt, cnt)) {
                const F3 dlt2 = f3(2.0f * (org.x - p.tbvh_oc[0]), 2.0f * (org.y - p.tbvh_oc[1]),
                                   2.0f * (org.z - p.tbvh_oc[2]));
                F3 nlo, nhi;
                sphere_slabs(org, inv, e, nlo, nhi);
                float cap = fminf(best_t, tri_t);
                uint32_t node = 0;
                do {
                    uint32_t leaf;
                    if (tri_node(p, nlo, nhi, inv, dlt2, false, cap, node, leaf, cnt)) {
                        tri_leaf(p, org, dir, false, leaf, best_t, tri_t, tri_i, cnt, cnt);
                        cap = fminf(best_t, tri_t);
                    }
                } while (node != kNodeEndDev);
            }
        } else if (kMesh == 1) {
            triangles_brute(p, org, dir, best_t, tri_t, tri_i, cnt);
        }
        if (tri_i < 0 && best_i < 0) return b;  // background (common.rs:276-281): no draws
        F3 pos, nrm;
        uint32_t kind;
        float param;
        if (tri_i >= 0) {  // a triangle wins a tie against a sphere
            pos = org + scale(dir, tri_t);
            const float4 *g = p.tri_geo + 4u * (uint32_t)tri_i;
            const float4 A = g[0], Nn = g[3];
            nrm = f3(Nn.x, Nn.y, Nn.z);
            const float *m = p.mats + 8u * __float_as_uint(A.w);
            kind = __float_as_uint(m[0]);
            param = m[4];
        } else {
            const float4 S = view.shade[2 * best_i];
            param = view.shade[2 * best_i + 1].w;
            kind = view.kinds[best_i];
            pos = org + scale(dir, best_t);
            nrm = unit<kWaveGuard>(divide_by<kWaveGuard>(pos - f3(S.x, S.y, S.z), S.w));  // common.rs:95
        }
        F3 v = nrm;
        bool keep_normal = false;
        if (kind == kMatDiffuse || kind == kMatMetal) {
            const F3 ru = draw_unit<kWaveGuard>(rng);
            ++b;
            if (kind == kMatDiffuse) {  // materials.rs:42-52
                v = nrm + ru;
                const float eps = 1e-8f;
                keep_normal = fabsf(v.x) < eps && fabsf(v.y) < eps && fabsf(v.z) < eps;
            } else {  // materials.rs:54-63: absorbed when the scatter points inward
                const F3 refl = dir - scale(nrm, 2.0f * dot(dir, nrm));
                v = refl + scale(ru, param);
                if (!(dot(v, nrm) >= 0.0f)) return b;
            }
        } else if (kind == kMatDielectric) {  // materials.rs:65-97 (no draws)
            F3 n2 = nrm;
            float eta = param;
            if (dot(dir, nrm) >= 0.0f) { n2 = -nrm; eta = 1.0f / param; }
            const float cos_t = dot(-dir, n2);
            const F3 perp = scale(dir + scale(n2, cos_t), eta);
            const F3 par = scale(n2, -xsqrt<kWaveGuard>(fabsf(1.0f - dot(perp, perp))));
            v = perp + par;
        } else {
            return b;  // Emission (materials.rs:100-102)
        }
        org = pos;
        dir = keep_normal ? nrm : unit<kWaveGuard>(v);
    }
    return b;  // depth exhausted (common.rs:284)
}

// Exclusive prefix sum of one u32 per thread over the 256-thread workgroup
// (wave scans, then the 4 wave totals); *total gets the sum.  Contains barriers.
__device__ __forceinline__ uint32_t block_exscan256(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const uint32_t lane = threadIdx.x & (kWave - 1u), wv = threadIdx.x / kWave;
    uint32_t x = v;
#pragma unroll
    for (uint32_t off = 1; off < kWave; off <<= 1) {
        const uint32_t y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == kWave - 1u) wsum[wv] = x;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wv; ++w) before += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + x - v;
}

constexpr uint32_t kCoalesceThreads = 256;
constexpr uint32_t kSlotDead = 0xFFFFFFFFu;

// LDS bytes of the coalescing workgroup after the tree: cand (u16 x K), three
// u32 lists of Kp = K + depth + 1 live offsets, two bitmaps and a prefix of W
// words (all 16-B aligned)
__host__ __device__ inline size_t coalesce_lds_bytes(uint32_t K, uint32_t depth) {
    const size_t Kp = (size_t)K + depth + 1, W = (Kp + 31) / 32;
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    return al(2 * (size_t)K) + 3 * al(4 * Kp) + 3 * al(4 * W) + 16;
}

// Waves per SIMD the brute-force coalescing kernels are compiled for (their
// live set fits 64 VGPRs without spills at 8; 1 = unconstrained, 76 VGPRs, 6
// waves); the tree variants stay unconstrained (they would spill at 8)
#ifndef RT_COALESCE_WAVES_BRUTE
#define RT_COALESCE_WAVES_BRUTE 8
#endif
template <bool kBvh, bool kLds, int kMesh>
__global__ __launch_bounds__(kCoalesceThreads)
__attribute__((amdgpu_waves_per_eu(kBvh ? 1 : RT_COALESCE_WAVES_BRUTE, 8)))
void serial_coalesce_kernel(TraceParams p, uint32_t *__restrict__ path,
                                                                           uint32_t *__restrict__ bend, uint32_t L,
                                                                           uint32_t Kmax, uint32_t R,
                                                                           uint32_t tree_bytes,
                                                                           unsigned long long *__restrict__ dbg) {
    if (p.ctrl[0] != 0u) return;
    const uint32_t K = serial_k(p.ctrl, Kmax);
    const uint32_t a = p.ctrl[4];
    const uint32_t n = min(L, p.nserial - a);
    const uint32_t nb = (n + R - 1) / R;
    const uint32_t blk = blockIdx.x;
    if (blk >= nb) return;  // (whole workgroup, before any barrier)
    extern __shared__ float4 lds[];
    BvhView view;
    const uint32_t sph_root = stage_tree<kLds, false>(p, nullptr, lds, view);
    const uint32_t depth = p.depth > 0 ? (uint32_t)p.depth : 0u;
    const uint32_t Kp = K + depth + 1, W = (Kp + 31) / 32;
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    char *c = reinterpret_cast<char *>(lds) + tree_bytes;
    uint16_t *cand = reinterpret_cast<uint16_t *>(c);  // live slot of each candidate (0xFFFF: left)
    c += al(2 * K);
    uint32_t *LB = reinterpret_cast<uint32_t *>(c);    // live offsets, ascending
    c += al(4 * Kp);
    uint32_t *LBn = reinterpret_cast<uint32_t *>(c);   // the next sample's
    c += al(4 * Kp);
    uint32_t *NB = reinterpret_cast<uint32_t *>(c);    // each live offset's end (kSlotDead: left)
    c += al(4 * Kp);
    uint32_t *bits0 = reinterpret_cast<uint32_t *>(c);  // the ends present, relative to the window
    c += al(4 * W);
    uint32_t *bits1 = reinterpret_cast<uint32_t *>(c);
    c += al(4 * W);
    uint32_t *wpre = reinterpret_cast<uint32_t *>(c);   // exclusive popcount prefix of the bitmap
    c += al(4 * W);
    uint32_t *wsum = reinterpret_cast<uint32_t *>(c);   // block_exscan256's wave totals
    // (all dynamic: the tree's LDS node addresses assume no static LDS below it)
    const uint32_t t = threadIdx.x;
    const uint32_t j0 = blk * R, j1 = min(j0 + R, n);
    const size_t stride = (size_t)nb * K;
    const uint32_t base = p.slo[j0];
    for (uint32_t k = t; k < K; k += kCoalesceThreads) {
        cand[k] = (uint16_t)k;
        LB[k] = base + k;
    }
    for (uint32_t w = t; w < W; w += kCoalesceThreads) bits0[w] = bits1[w] = 0u;
    uint32_t nlive = K;
    uint32_t d_traces = 0, d_passes = 0;  // (dbg: RT_AMD_SERIAL_DEBUG)
    __syncthreads();
    for (uint32_t s = 0; j0 + s < j1; ++s) {
        d_traces += nlive;
        d_passes += (nlive + kCoalesceThreads - 1) / kCoalesceThreads;
        const uint32_t jl = j0 + s;
        const uint32_t l = p.slo[jl];  // the window of sample jl: [l, l + K)
        uint32_t *bits = (s & 1u) ? bits1 : bits0;
        uint32_t *bnext = (s & 1u) ? bits0 : bits1;
        // every distinct live offset once: its sample's end offset
        for (uint32_t i = t; i < nlive; i += kCoalesceThreads) {
            const uint32_t B = LB[i];
            uint32_t e = kSlotDead;
            if (B >= l && B - l < K) {
                e = B + serial_trace_b<kBvh, kLds, kMesh>(p, view, sph_root, p.win[2u * jl + 3u * B], a + jl);
                const uint32_t r = e - l;  // < K + depth
                atomicOr(&bits[r >> 5], 1u << (r & 31u));
            }
            NB[i] = e;
        }
        __syncthreads();
        // ranks of the distinct ends: popcount prefix over the bitmap words
        const uint32_t per = (W + kCoalesceThreads - 1) / kCoalesceThreads;
        const uint32_t w0 = min(t * per, W), w1 = min(w0 + per, W);
        uint32_t cntw = 0;
        for (uint32_t w = w0; w < w1; ++w) cntw += __popc(bits[w]);
        uint32_t total = 0;
        uint32_t run = block_exscan256(cntw, wsum, &total);
        for (uint32_t w = w0; w < w1; ++w) {
            wpre[w] = run;
            run += __popc(bits[w]);
        }
        __syncthreads();
        auto rank = [&](uint32_t e) {
            const uint32_t r = e - l;
            return wpre[r >> 5] + __popc(bits[r >> 5] & ((1u << (r & 31u)) - 1u));
        };
        for (uint32_t i = t; i < nlive; i += kCoalesceThreads) {
            const uint32_t e = NB[i];
            if (e != kSlotDead) LBn[rank(e)] = e;  // (merged slots write the same value)
        }
        for (uint32_t k = t; k < K; k += kCoalesceThreads) {
            const uint32_t sl = cand[k];
            if (sl == 0xFFFFu) continue;
            path[(size_t)s * stride + (size_t)blk * K + k] = LB[sl];
            const uint32_t e = NB[sl];
            if (e == kSlotDead) {
                cand[k] = 0xFFFFu;
                bend[(size_t)blk * K + k] = kWalkLeft | s;
            } else {
                cand[k] = (uint16_t)rank(e);
            }
        }
        for (uint32_t w = t; w < W; w += kCoalesceThreads) bnext[w] = 0u;
        nlive = total;
        uint32_t *sw = LB;
        LB = LBn;
        LBn = sw;
        __syncthreads();
    }
    for (uint32_t k = t; k < K; k += kCoalesceThreads) {
        const uint32_t sl = cand[k];
        if (sl != 0xFFFFu) bend[(size_t)blk * K + k] = LB[sl];
    }
    if (dbg != nullptr && t == 0) {
        atomicAdd(dbg, (unsigned long long)d_traces);
        atomicAdd(dbg + 1, (unsigned long long)d_passes);
        atomicAdd(dbg + 2, 1ull);
        atomicAdd(dbg + 3, (unsigned long long)K * (j1 - j0));
    }
}

}  // namespace rtamd
