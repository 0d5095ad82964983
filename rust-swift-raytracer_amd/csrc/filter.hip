// filter.hip -- the edge-avoiding a-trous filter over per-pixel mean colours,
// stopped at geometric edges by the first-hit records (DESIGN.md 5.9;
// include/raytracer_amd.h rt_filter_*).
//
// pack turns the input into what a level gathers: per pixel one 16-byte colour
// {r, g, b, L} and two 16-byte guides {normal, prim bits}, {position, zs}.  A
// level is one lane per pixel, a wave per 8 x 8 tile as first_hit_kernel: a
// tap's loads are eight 128-byte row runs per array, and neighbouring waves
// share the lines.  Taps are gathered straight through L2.
//
// Every step of the contract is one rounded f32 operation: this unit compiles
// without contraction, `/` and sqrt are the correctly rounded ones, and no
// reciprocal or rsqrt shortcut appears.  A tap that is skipped adds nothing;
// the 25 accumulations keep their order (j outer, i inner) in every lane.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exactdiv.h"
#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

#include "device_math.h"

namespace rtamd {
namespace {

constexpr uint32_t kFilterThreads = 256;
constexpr uint32_t kTile = 8;  // a wave's pixels: kTile x kTile

__global__ __launch_bounds__(kFilterThreads) void filter_pack_kernel(FilterPack a) {
    const uint32_t i = blockIdx.x * kFilterThreads + threadIdx.x;
    if (i >= a.npix) return;
    float r, g, b;
    if (a.rgb) {
        const float *c = a.rgb + 3u * (size_t)i;
        r = c[0];
        g = c[1];
        b = c[2];
    } else {
        // what the frame's resolve takes the square root of (chunk_resolve.h)
        const uint32_t n = a.count ? a.count[i] : a.held;
        const float inv = 1.0f / (float)n;
        r = a.sums[i] * inv;
        g = a.sums[a.plane + i] * inv;
        b = a.sums[2 * a.plane + i] * inv;
    }
    a.col[i] = make_float4(r, g, b, (r + g) + b);
    // RtFirstHit: prim, t, normal[3], position[3]
    const float4 r0 = a.records[2u * (size_t)i], r1 = a.records[2u * (size_t)i + 1u];
    a.g0[i] = make_float4(r0.z, r0.w, r1.x, r0.x);
    a.g1[i] = make_float4(r1.y, r1.z, r1.w, a.sigma_z * r0.y);
}

__device__ __forceinline__ uint32_t gamma_u8(float c) { return sat_u8(__builtin_sqrtf(c) * 255.999f); }

__device__ __forceinline__ void filter_store(const FilterLevel &a, uint32_t idx, float r, float g, float b) {
    if (a.out_rgb) {
        float *o = a.out_rgb + 3u * (size_t)idx;
        o[0] = r;
        o[1] = g;
        o[2] = b;
    }
    if (a.out_rgba) a.out_rgba[idx] = gamma_u8(r) | (gamma_u8(g) << 8) | (gamma_u8(b) << 16) | (255u << 24);
}

// levels = 0: the outputs from the packed input
__global__ __launch_bounds__(kFilterThreads) void filter_store_kernel(FilterLevel a) {
    const uint32_t i = blockIdx.x * kFilterThreads + threadIdx.x;
    if (i >= a.width * a.height) return;
    const float4 c = a.cin[i];
    filter_store(a, i, c.x, c.y, c.z);
}

// kLast: the outputs instead of the next level's colours
template <bool kLast>
__global__ __launch_bounds__(kFilterThreads) void filter_level_kernel(FilterLevel a) {
    // the lane's pixel: wave -> tile, lane -> pixel of the tile
    const uint32_t wave = blockIdx.x * (kFilterThreads / kWave) + threadIdx.x / kWave;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t tiles_x = (a.width + kTile - 1u) / kTile;
    const uint32_t ty = wave / tiles_x, tx = wave - ty * tiles_x;
    const uint32_t x = tx * kTile + (lane & (kTile - 1u)), y = ty * kTile + lane / kTile;
    if (x >= a.width || y >= a.height) return;
    const uint32_t idx = y * a.width + x;

    const float4 cp = a.cin[idx], P0 = a.g0[idx], P1 = a.g1[idx];
    const uint32_t prim_p = __float_as_uint(P0.w);
    const bool hp = prim_p != 0u;
    const float Lp = cp.w, zs = P1.w;
    const int step = (int)a.step;

    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    for (int j = 0; j < 5; ++j) {
        const float hj = j == 2 ? 0.375f : (j == 1 || j == 3) ? 0.25f : 0.0625f;
        // (unsigned: a tap left of or above the frame wraps far past its size)
        const uint32_t qy = y + (uint32_t)((j - 2) * step);
        const bool row_in = qy < a.height;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const float hi = i == 2 ? 0.375f : (i == 1 || i == 3) ? 0.25f : 0.0625f;
            const uint32_t qx = x + (uint32_t)((i - 2) * step);
            const bool in = row_in && qx < a.width;
            // (a tap outside the frame reads the centre and is dropped below)
            const uint32_t qi = in ? qy * a.width + qx : idx;
            const float4 cq = a.cin[qi], Q0 = a.g0[qi], Q1 = a.g1[qi];
            const uint32_t prim_q = __float_as_uint(Q0.w);
            const bool hq = prim_q != 0u;
            const bool keep = in && hp == hq && (a.same_prim == 0u || prim_p == prim_q);
            float w = hj * hi;
            if (hp) {
                float d = ((P0.x * Q0.x) + (P0.y * Q0.y)) + (P0.z * Q0.z);
                d = d > 0.0f ? d : 0.0f;
                for (uint32_t s = 0; s < a.squarings; ++s) d = d * d;
                const float vx = Q1.x - P1.x, vy = Q1.y - P1.y, vz = Q1.z - P1.z;
                const float e = __builtin_fabsf(((vx * P0.x) + (vy * P0.y)) + (vz * P0.z)) / zs;
                const float wz = 1.0f / (1.0f + e * e);
                w = (w * d) * wz;
            }
            const float el = __builtin_fabsf(cq.w - Lp) / a.sl;
            const float wl = 1.0f / (1.0f + el * el);
            w = w * wl;
            if (keep && w > 0.0f) {  // (false for NaN)
                nr = nr + w * cq.x;
                ng = ng + w * cq.y;
                nb = nb + w * cq.z;
                den = den + w;
            }
        }
    }
    const bool any = den > 0.0f;
    const float r = any ? nr / den : cp.x, g = any ? ng / den : cp.y, b = any ? nb / den : cp.z;
    if (kLast) filter_store(a, idx, r, g, b);
    else a.cout[idx] = make_float4(r, g, b, (r + g) + b);
}

}  // namespace

hipError_t launch_filter_pack(const FilterPack &a, hipStream_t stream) {
    if (a.npix == 0 || a.npix >= 0x80000000u || (!a.rgb && !a.sums) || !a.records || !a.col || !a.g0 || !a.g1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_pack_kernel, dim3((a.npix + kFilterThreads - 1u) / kFilterThreads),
                       dim3(kFilterThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_filter_level(const FilterLevel &a, hipStream_t stream) {
    const uint64_t npix = (uint64_t)a.width * a.height;
    const bool last = a.cout == nullptr;
    if (npix == 0 || npix >= (1ull << 31) || !a.cin || a.step > 128u || (last && !a.out_rgb && !a.out_rgba))
        return hipErrorInvalidValue;
    if (a.step == 0) {
        if (!last) return hipErrorInvalidValue;
        hipLaunchKernelGGL(filter_store_kernel, dim3((uint32_t)((npix + kFilterThreads - 1u) / kFilterThreads)),
                           dim3(kFilterThreads), 0, stream, a);
        return hipGetLastError();
    }
    if (!a.g0 || !a.g1 || (a.step & (a.step - 1u)) != 0u) return hipErrorInvalidValue;
    const uint64_t tiles = (uint64_t)((a.width + kTile - 1u) / kTile) * ((a.height + kTile - 1u) / kTile);
    const uint64_t per_block = kFilterThreads / kWave;
    const uint64_t blocks = (tiles + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (last) hipLaunchKernelGGL(filter_level_kernel<true>, dim3((uint32_t)blocks), dim3(kFilterThreads), 0, stream, a);
    else hipLaunchKernelGGL(filter_level_kernel<false>, dim3((uint32_t)blocks), dim3(kFilterThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtamd
