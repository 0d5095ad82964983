// sky.hip -- the frame's sky rows (bvh.h classify_sky_rows):
// image rows none of whose primary rays can hit a sphere, rendered without a
// search.  Every sample of such a pixel is the background of its primary ray
// (common.rs:276-281), so a lane takes one pixel, runs its spp samples in
// order -- the seed, the two draws, the camera ray, the two normalisations and
// the lerp, through the frame kernels' own helpers (device_math.h), each one
// f32 operation as there -- folds them in registers (common.rs:333-341) and
// stores the pixel's RGBA8 word (chunk_resolve.h resolve_channel).  No ring, no
// job counter, no LDS; a wave's lanes are 64 neighbouring pixels of a row.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exactdiv.h"
#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

#include "chunk_resolve.h"
#include "device_math.h"

namespace rtamd {
namespace {

// The argument block: the frame's TraceParams (no field added), then the rows.
struct SkyParams {
    TraceParams p;
    uint32_t top, bottom;
};

constexpr uint32_t kSkyThreads = 256;

__global__ __launch_bounds__(kSkyThreads) void sky_rows_kernel(SkyParams a) {
    const TraceParams &p = a.p;
    const uint32_t i = blockIdx.x * kSkyThreads + threadIdx.x;  // pixel of the two blocks, the top one first
    if (i >= (a.top + a.bottom) * p.width) return;
    const uint32_t q = fdiv(i, p.div_width);
    const uint32_t col = i - q * p.width;
    const uint32_t trow = q < a.top ? q : p.height - a.bottom + (q - a.top);  // image row from the top
    const uint32_t row = p.height - 1u - trow;                                // reference row, 0 = bottom
    // the reference's job index of the pixel's sample 0 (common.rs:327-336)
    const uint64_t gjob0 = ((uint64_t)row * p.width + col) * p.spp;
    const F3 h = f3(p.cam[6], p.cam[7], p.cam[8]);
    const F3 vv = f3(p.cam[9], p.cam[10], p.cam[11]);
    const F3 org = f3(p.cam[0], p.cam[1], p.cam[2]);
    const F3 llc = f3(p.cam[3], p.cam[4], p.cam[5]);
    const bool xd = p.xdiv_uv != 0;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    for (uint32_t s = 0; s < p.spp; ++s) {
        uint32_t rng = counter_seed(p.seed, gjob0 + s);
        const float un = draw_plus(rng, (float)col);  // u drawn before v (common.rs:335-337)
        const float vn = draw_plus(rng, (float)row);
        const float u = xd ? xdiv(un, p.wden, p.wrcp) : un / p.wden;
        const float v = xd ? xdiv(vn, p.hden, p.hrcp) : vn / p.hden;
        const F3 vdir = ((llc + scale(h, u)) + scale(vv, v)) - org;
        const F3 dir = unit<true>(vdir);  // the ray's direction ...
        const F3 un3 = unit<true>(dir);   // ... normalised again by the miss branch (common.rs:277)
        const float t = 0.5f * (un3.y + 1.0f);
        const float w = 1.0f - t;
        // (the path's throughput is exactly 1.0f: its product is dropped)
        acc_r = acc_r + (1.0f * w + 0.5f * t);
        acc_g = acc_g + (1.0f * w + 0.7f * t);
        acc_b = acc_b + (1.0f * w + 1.0f * t);
    }
    p.out[(size_t)trow * p.width + col] = resolve_channel(p, acc_r) | (resolve_channel(p, acc_g) << 8) |
                                          (resolve_channel(p, acc_b) << 16) | (p.alpha_u8 << 24);
}

}  // namespace

hipError_t launch_sky_rows(const TraceParams &p, uint32_t top, uint32_t bottom, hipStream_t stream) {
    if (p.out == nullptr || p.width == 0 || (uint64_t)top + bottom > p.height || p.mode != kRngCounter ||
        p.depth < 1 || p.nranks != 1)
        return hipErrorInvalidValue;
    const uint64_t npix = ((uint64_t)top + bottom) * p.width;
    if (npix == 0) return hipSuccess;
    const uint64_t blocks = (npix + kSkyThreads - 1) / kSkyThreads;
    if (npix > 0xFFFFFFFFull || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    SkyParams a{p, top, bottom};
    void *args[] = {(void *)&a};
    return hipLaunchKernel((const void *)sky_rows_kernel, dim3((uint32_t)blocks), dim3(kSkyThreads), args, 0, stream);
}

}  // namespace rtamd
