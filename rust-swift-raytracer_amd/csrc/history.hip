// history.hip -- temporal reprojection of an accumulator's resolved view into
// the next one (include/raytracer_amd.h rt_history_*).
//
// One lane per pixel, a wave per 8 x 8 tile as filter_level_kernel: the lane
// projects its first-hit position into prev's view, gathers the 2 x 2 pixels
// of prev around it, keeps the taps on its own primitive and plane, and blends
// what they carry with the pixel's mean.  Neighbouring lanes land on
// neighbouring pixels of prev, so a wave's four gathers fall on a few 128-byte
// rows of each of prev's two arrays.
//
// Every step of the contract is one rounded f32 operation: this unit compiles
// without contraction, `/` and sqrt are the correctly rounded ones, and no
// reciprocal shortcut appears.  A tap that is skipped adds nothing; the four
// accumulations keep their order (j outer, i inner) in every lane.  A float
// becomes an index only after the range test that also rejects NaN.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exactdiv.h"
#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

#include "device_math.h"

namespace rtamd {
namespace {

constexpr uint32_t kHistoryThreads = 256;
constexpr uint32_t kTile = 8;  // a wave's pixels: kTile x kTile

__device__ __forceinline__ uint32_t gamma_u8(float c) { return sat_u8(__builtin_sqrtf(c) * 255.999f); }

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return ((ax * bx) + (ay * by)) + (az * bz);
}

__global__ __launch_bounds__(kHistoryThreads) void history_resolve_kernel(HistoryResolve a) {
    // the lane's pixel: wave -> tile, lane -> pixel of the tile
    const uint32_t wave = blockIdx.x * (kHistoryThreads / kWave) + threadIdx.x / kWave;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t tiles_x = (a.width + kTile - 1u) / kTile;
    const uint32_t ty = wave / tiles_x, tx = wave - ty * tiles_x;
    const uint32_t x = tx * kTile + (lane & (kTile - 1u)), y = ty * kTile + lane / kTile;
    if (x >= a.width || y >= a.height) return;
    const uint32_t idx = y * a.width + x;

    // the mean and its sample count
    uint32_t n;
    float mr, mg, mb;
    if (a.rgb) {
        const float *c = a.rgb + 3u * (size_t)idx;
        n = a.n[idx];
        mr = c[0];
        mg = c[1];
        mb = c[2];
    } else {
        // what the frame's resolve takes the square root of (chunk_resolve.h)
        n = a.count ? a.count[idx] : a.held;
        const float inv = 1.0f / (float)n;
        mr = a.sums[idx] * inv;
        mg = a.sums[a.plane + idx] * inv;
        mb = a.sums[2 * a.plane + idx] * inv;
    }
    const float nf = (float)n;
    // RtFirstHit: prim, t, normal[3], position[3]
    const float4 r0 = a.records[2u * (size_t)idx], r1 = a.records[2u * (size_t)idx + 1u];
    const uint32_t prim_p = __float_as_uint(r0.x);
    const float Px = r1.y, Py = r1.z, Pz = r1.w;

    float outr = mr, outg = mg, outb = mb, len = nf;
    if (a.prev_col && prim_p != 0u) {
        const float dx = Px - a.org[0], dy = Py - a.org[1], dz = Pz - a.org[2];
        const float s = dot3(dx, dy, dz, a.n0[0], a.n0[1], a.n0[2]);
        const float pa = dot3(dx, dy, dz, a.n1[0], a.n1[1], a.n1[2]);
        const float pb = dot3(dx, dy, dz, a.n2[0], a.n2[1], a.n2[2]);
        const bool front = (s > 0.0f && a.det > 0.0f) || (s < 0.0f && a.det < 0.0f);
        const float u = pa / s, v = pb / s;
        const float wf = (float)a.width, hf = (float)a.height;
        const float fx = u * (float)(a.width - 1u) - 0.5f, fy = v * (float)(a.height - 1u) - 0.5f;
        // (false for NaN; inside it both floors are -1 .. size - 1)
        const bool inside = front && fx > -1.0f && fx < wf && fy > -1.0f && fy < hf;
        const float x0f = __builtin_floorf(fx), y0f = __builtin_floorf(fy);
        const float tfx = fx - x0f, tfy = fy - y0f;
        const int x0 = (int)(inside ? x0f : 0.0f), y0 = (int)(inside ? y0f : 0.0f);
        const float zlim = a.sigma_z * r0.y;
        float cr = 0.0f, cg = 0.0f, cb = 0.0f, ls = 0.0f, ws = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            // (unsigned: column or row -1 wraps far past the size)
            const uint32_t qrow = (uint32_t)(y0 + j);  // from the bottom
            const float wy = j ? tfy : 1.0f - tfy;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint32_t qcol = (uint32_t)(x0 + i);
                const float wx = i ? tfx : 1.0f - tfx;
                const bool in = inside && qcol < a.width && qrow < a.height;
                // (a tap outside the frame reads the centre and is dropped below)
                const uint32_t qi = in ? (a.height - 1u - qrow) * a.width + qcol : idx;
                const float4 cq = a.prev_col[qi], gq = a.prev_guide[qi];
                const float vx = gq.x - Px, vy = gq.y - Py, vz = gq.z - Pz;
                const float e = __builtin_fabsf(dot3(vx, vy, vz, r0.z, r0.w, r1.x));
                const float w = wx * wy;
                if (in && cq.w > 0.0f && __float_as_uint(gq.w) == prim_p && e <= zlim && w > 0.0f) {
                    cr = cr + w * cq.x;
                    cg = cg + w * cq.y;
                    cb = cb + w * cq.z;
                    ls = ls + w * cq.w;
                    ws = ws + w;
                }
            }
        }
        if (ws > 0.0f) {
            const float hr = cr / ws, hg = cg / ws, hb = cb / ws, hl = ls / ws;
            const float cap = a.max_history > nf ? a.max_history : nf;
            float tl = hl + nf;
            tl = tl > cap ? cap : tl;
            const float alpha = nf / tl;
            outr = hr + (mr - hr) * alpha;
            outg = hg + (mg - hg) * alpha;
            outb = hb + (mb - hb) * alpha;
            len = tl;
        }
    }

    a.cur_col[idx] = make_float4(outr, outg, outb, len);
    if (a.cur_guide) a.cur_guide[idx] = make_float4(Px, Py, Pz, r0.x);
    if (a.out_rgb) {
        float *o = a.out_rgb + 3u * (size_t)idx;
        o[0] = outr;
        o[1] = outg;
        o[2] = outb;
    }
    if (a.out_rgba)
        a.out_rgba[idx] = gamma_u8(outr) | (gamma_u8(outg) << 8) | (gamma_u8(outb) << 16) | (255u << 24);
}

}  // namespace

hipError_t launch_history_resolve(const HistoryResolve &a, hipStream_t stream) {
    const uint64_t npix = (uint64_t)a.width * a.height;
    if (npix == 0 || npix >= (1ull << 31) || (!a.rgb && !a.sums) || (a.rgb && !a.n) || !a.records || !a.cur_col ||
        (a.prev_col && !a.prev_guide) || a.prev_col == a.cur_col)
        return hipErrorInvalidValue;
    const uint64_t tiles = (uint64_t)((a.width + kTile - 1u) / kTile) * ((a.height + kTile - 1u) / kTile);
    const uint64_t per_block = kHistoryThreads / kWave;
    const uint64_t blocks = (tiles + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(history_resolve_kernel, dim3((uint32_t)blocks), dim3(kHistoryThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtamd
