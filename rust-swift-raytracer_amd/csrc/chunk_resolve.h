// chunk_resolve.h -- the in-kernel resolve of one finished chunk of a wave's sample ring (frames,
// accumulation passes, adaptive passes).
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include "device_math.h"

namespace rtamd {
namespace {

// One resolved pixel: gamma + `as u8` (common.rs:344-356), RGBA8 at the
// tile row of launch-local pixel lp.
__device__ __forceinline__ uint32_t resolve_channel(const TraceParams &p, float sum) {
    return sat_u8(__builtin_sqrtf(sum * p.inv_spp) * 255.999f);
}
template <bool kPlain = false>
__device__ __forceinline__ void resolve_store_u8(const TraceParams &p, uint32_t lp, uint32_t R, uint32_t G,
                                                 uint32_t B) {
    const uint32_t q = fdiv<kPlain>(lp, p.div_width);
    const uint32_t col = lp - q * p.width;
    p.out[(size_t)(p.slab_row0 + q) * p.width + col] = R | (G << 8) | (B << 16) | (p.alpha_u8 << 24);
}
__device__ __forceinline__ void resolve_store(const TraceParams &p, uint32_t lp, float r, float g,
                                              float b) {
    resolve_store_u8(p, lp, resolve_channel(p, r), resolve_channel(p, g), resolve_channel(p, b));
}

// Fused resolve of one finished chunk (wave-uniform call, all lanes active):
// jobs [base, base + len) are whole pixels (chunks and partitions are
// pixel-aligned), their samples sit at ring offset `off` of the wave's ring
// (planes `plane` floats apart).  Each pixel's samples are summed in order
// (common.rs:333-341, the same fold as resolve_kernel).  The samples were
// stored by this wave: a workgroup-scope fence orders them (one CU, one L1).
//
// One lane per (pixel, plane) when 3 * pixels <= 64 and spp % 4 == 0: lane
// c * np + g folds plane c of pixel g in sample order from float4 loads (4
// in flight per round) and converts its own sum (gamma + `as u8`, one pass
// for the three planes), then the pixel's lane collects the G and B bytes with
// two shuffles: spp adds and spp / 4 loads per lane (A/B on C2 -1.7 %
// against folding float4 groups through ds_bpermute, 3 * spp bpermutes and
// adds per pixel).  Other chunks, and the triangle kernels (kPlaneLanes
// false: at their 64-VGPR cap the float4 rounds spill, C5 +7 %), sum one
// pixel per lane.
// which kernel families fold with plane lanes: the sphere kernels and the
// wide triangle walk (A/B on C5, 1-pixel chunks: 149.8 -> 148.1 ms, 2 VGPRs
// spilled); the binary triangle walk keeps one lane per pixel
#define RT_PLANE_LANES(mesh) ((mesh) < 2 || (mesh) == 3)
// kAccum (accumulation passes, trace_body.h AccumTail): a pixel's fold starts from
// its stored sum (sums: three planes of width * height floats, indexed like
// p.out) instead of 0.0f and the new sum is stored back before gamma -- the
// f32 fold of common.rs:333-341 stopped after a sample and continued from the
// stored sum is the fold that never stopped.  A pixel belongs to one chunk of
// one wave per pass, so nothing else touches its three sums.
__device__ __forceinline__ size_t resolve_index(const TraceParams &p, uint32_t lp) {
    const uint32_t q = fdiv(lp, p.div_width);
    const uint32_t col = lp - q * p.width;
    return (size_t)(p.slab_row0 + q) * p.width + col;
}
// kPlain (the plain instance, render.h trace_plain_ok): every chunk of the
// launch has the plane-lane shape and both dividers are in their general form,
// so neither is tested and the pixel-lane loop is not compiled.
template <bool kPlaneLanes, bool kAccum = false, bool kPlain = false>
__device__ __forceinline__ void resolve_chunk(const TraceParams &p, const float *ring, uint32_t plane,
                                              uint32_t off, uint32_t base, uint32_t len,
                                              uint32_t lane, float *sums = nullptr) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t spp = p.spp;
    static_assert(!kPlain || (kPlaneLanes && !kAccum), "the plain instance: plane lanes, frames");
    const uint32_t np = fdiv<kPlain>(len, p.div_spp), pix0 = fdiv<kPlain>(base, p.div_spp);
    if (kPlaneLanes && (kPlain || (3u * np <= kWave && (spp & 3u) == 0))) {
        const uint32_t c = lane >= np ? (lane >= 2u * np ? 2u : 1u) : 0u;
        const uint32_t g = lane - c * np;
        const bool on = lane < 3u * np;
        const float *src = ring + off + c * plane + (on ? g : 0u) * spp;
        float acc = 0.0f;
        float *held = nullptr;  // (kAccum) the lane's plane sum
        if (kAccum) {
            held = sums + (size_t)c * ((size_t)p.width * p.height) + resolve_index(p, pix0 + (on ? g : 0u));
            if (on) acc = *held;
        }
        for (uint32_t k = 0; k < spp; k += 16u) {
            float4 v[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                v[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (on && k + 4u * q < spp) v[q] = *reinterpret_cast<const float4 *>(src + k + 4u * q);
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                if (k + 4u * q < spp) {  // (wave-uniform)
                    acc = acc + v[q].x;
                    acc = acc + v[q].y;
                    acc = acc + v[q].z;
                    acc = acc + v[q].w;
                }
            }
        }
        // gamma + `as u8` of the lane's own plane sum (resolve_store's
        // operations on the same value: the same byte), one pass for the
        // three planes; the pixel's lane then collects the G and B bytes
        if (kAccum && on) *held = acc;
        const uint32_t ch = resolve_channel(p, acc);
        const uint32_t G = (uint32_t)__shfl((int)ch, (int)(lane < np ? np + lane : lane));
        const uint32_t B = (uint32_t)__shfl((int)ch, (int)(lane < np ? 2u * np + lane : lane));
        if (lane < np) resolve_store_u8<kPlain>(p, pix0 + lane, ch, G, B);
        return;
    }
    for (uint32_t i = lane; i < np; i += kWave) {
        const float *src = ring + off + i * spp;
        float r = 0.0f, g = 0.0f, b = 0.0f;
        float *held = nullptr;  // (kAccum) the pixel's R sum; G and B a plane further each
        const size_t hplane = kAccum ? (size_t)p.width * p.height : 0u;
        if (kAccum) {
            held = sums + resolve_index(p, pix0 + i);
            r = held[0];
            g = held[hplane];
            b = held[2 * hplane];
        }
        for (uint32_t k = 0; k < spp; ++k) {
            r = r + src[k];
            g = g + src[plane + k];
            b = b + src[2 * plane + k];
        }
        if (kAccum) {
            held[0] = r;
            held[hplane] = g;
            held[2 * hplane] = b;
        }
        resolve_store(p, pix0 + i, r, g, b);
    }
}

// The chunk resolve of an adaptive accumulation pass (trace_body.h AdaptTail):
// resolve_chunk<., kAccum> with every pixel index mapped through the pass's
// list (launch-local pixel lp is frame pixel list[lp]) and a fourth fold per
// pixel, q <- q + y y with y = (r + g) + b of each ring sample in sample order,
// starting from the stored sumsq and stored back (each operation rounded on
// its own: this file compiles without contraction).  Plane lanes: a fourth
// lane group folds q, so the shape needs 4 * pixels <= 64; pixel lanes: a
// fourth running value.  RGBA8 goes to p.out[list[lp]].
template <bool kPlaneLanes>
__device__ __forceinline__ void resolve_chunk_adapt(const TraceParams &p, const float *ring, uint32_t plane,
                                                    uint32_t off, uint32_t base, uint32_t len, uint32_t lane,
                                                    float *sums, float *sumsq, const uint32_t *list) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t spp = p.spp;
    const uint32_t np = fdiv(len, p.div_spp), pix0 = fdiv(base, p.div_spp);
    const size_t hplane = (size_t)p.width * p.height;
    if (kPlaneLanes && 4u * np <= kWave && (spp & 3u) == 0) {
        const uint32_t c = lane >= np ? (lane >= 2u * np ? (lane >= 3u * np ? 3u : 2u) : 1u) : 0u;
        const uint32_t g = lane - c * np;
        const bool on = lane < 4u * np;
        const size_t idx = list[pix0 + (on ? g : 0u)];
        const float *src = ring + off + (on ? g : 0u) * spp;  // the pixel's R samples
        float *held = (c < 3u ? sums + (size_t)c * hplane : sumsq) + idx;
        float acc = on ? *held : 0.0f;
        if (on) {
            if (c < 3u) {
                for (uint32_t k = 0; k < spp; k += 4u) {
                    const float4 v = *reinterpret_cast<const float4 *>(src + c * plane + k);
                    acc = acc + v.x;
                    acc = acc + v.y;
                    acc = acc + v.z;
                    acc = acc + v.w;
                }
            } else {
                for (uint32_t k = 0; k < spp; k += 4u) {
                    const float4 r = *reinterpret_cast<const float4 *>(src + k);
                    const float4 gg = *reinterpret_cast<const float4 *>(src + plane + k);
                    const float4 b = *reinterpret_cast<const float4 *>(src + 2u * plane + k);
                    const float y0 = (r.x + gg.x) + b.x, y1 = (r.y + gg.y) + b.y;
                    const float y2 = (r.z + gg.z) + b.z, y3 = (r.w + gg.w) + b.w;
                    acc = acc + y0 * y0;
                    acc = acc + y1 * y1;
                    acc = acc + y2 * y2;
                    acc = acc + y3 * y3;
                }
            }
            *held = acc;
        }
        const uint32_t ch = resolve_channel(p, acc);
        const uint32_t G = (uint32_t)__shfl((int)ch, (int)(lane < np ? np + lane : lane));
        const uint32_t B = (uint32_t)__shfl((int)ch, (int)(lane < np ? 2u * np + lane : lane));
        if (lane < np) p.out[idx] = ch | (G << 8) | (B << 16) | (p.alpha_u8 << 24);
        return;
    }
    for (uint32_t i = lane; i < np; i += kWave) {
        const float *src = ring + off + i * spp;
        const size_t idx = list[pix0 + i];
        float *held = sums + idx;
        float r = held[0], g = held[hplane], b = held[2 * hplane], q = sumsq[idx];
        for (uint32_t k = 0; k < spp; ++k) {
            const float sr = src[k], sg = src[plane + k], sb = src[2 * plane + k];
            r = r + sr;
            g = g + sg;
            b = b + sb;
            const float y = (sr + sg) + sb;
            q = q + y * y;
        }
        held[0] = r;
        held[hplane] = g;
        held[2 * hplane] = b;
        sumsq[idx] = q;
        p.out[idx] = resolve_channel(p, r) | (resolve_channel(p, g) << 8) | (resolve_channel(p, b) << 16) |
                     (p.alpha_u8 << 24);
    }
}

}  // namespace
}  // namespace rtamd
