// device_math.h -- device maths of the render path: F3, the exact divisions, the reference's RNG
// draws, the counter seed, `as u8`, wave-uniform loads.
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "exactdiv.h"
#include "render.h"

namespace rtamd {
namespace {

// ------------------------------------------------------------ device maths
struct F3 { float x, y, z; };

__device__ __forceinline__ F3 f3(float x, float y, float z) { return F3{x, y, z}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return F3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 operator-(F3 a) { return F3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ F3 scale(F3 a, float s) { return F3{a.x * s, a.y * s, a.z * s}; }
// (x*x' + y*y') + z*z'  (maths.rs:82)
__device__ __forceinline__ float dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 cross(F3 a, F3 b) {  // maths.rs:88-94
    return F3{a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x};
}
// The divisions go through exactdiv.h (one shared correctly rounded
// reciprocal, three corrected quotients: the same bits as `/`) whenever the
// operands are in its guarded range; HIP's divide otherwise (never taken by
// lanes of ordinary scenes: one wave-wide test skips it, see exactdiv.h).
// RT_NO_XDIV builds the plain-divide variant (A/B only).
// kWaveGuard (exactdiv.h): true in every kernel but the triangle-mesh ones
// (kMesh >= 2), which keep the per-lane fallbacks.
template <bool kWaveGuard>
__device__ __forceinline__ F3 divide_by(F3 a, float b) {
#ifndef RT_NO_XDIV
    xdivide3<kWaveGuard>(a.x, a.y, a.z, b);
    return a;
#else
    return F3{a.x / b, a.y / b, a.z / b};
#endif
}
template <bool kWaveGuard>
__device__ __forceinline__ F3 unit(F3 a) {  // NVec3::new, maths.rs:111-118
#ifndef RT_NO_XDIV
    xunit3<kWaveGuard>(a.x, a.y, a.z);
    return a;
#else
    const float len = xsqrt<kWaveGuard>((a.x * a.x + a.y * a.y) + a.z * a.z);
    return F3{a.x / len, a.y / len, a.z / len};
#endif
}

// xorshift32 (random.rs:22-30); `x as f32 / u32::MAX as f32` == RN(x) * 2^-32.
__device__ __forceinline__ uint32_t xorshift(uint32_t &s) {
    uint32_t x = s;
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    s = x;
    return x;
}
// `random_f32() * 2.0 - 1.0` (common.rs:32-38, random.rs:27-30): RN(RN(x) 2^-32 2
// - 1) with an exact product (a power-of-two scaling of RN(x), >= 2^-31), so
// one fma gives the same bits.
__device__ __forceinline__ float draw11(uint32_t &s) {
    return __builtin_fmaf((float)xorshift(s), 0x1p-31f, -1.0f);
}
// `n + random_f32()` (camera u, v numerators, common.rs:335-336): the same
// exact product, one rounding
__device__ __forceinline__ float draw_plus(uint32_t &s, float n) {
    return __builtin_fmaf((float)xorshift(s), 0x1p-32f, n);
}
// common.rs:32-38 -- three draws x, y, z, normalised (no rejection sampling).
template <bool kWaveGuard>
__device__ __forceinline__ F3 draw_unit(uint32_t &s) {
    float x = draw11(s);
    float y = draw11(s);
    float z = draw11(s);
    return unit<kWaveGuard>(F3{x, y, z});
}

// (a one-multiply seed in its place, which renders no valid frame, bounds
// what a cheaper hash could save at 1.1 % of a C2 frame: DESIGN.md round 4)
__device__ __forceinline__ uint32_t counter_seed(uint32_t seed, uint64_t job) {
    uint64_t z = job + (uint64_t)seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uint32_t r = (uint32_t)(z ^ (z >> 32));
    return r ? r : 2547549u;
}

// Rust `f32 as u8`: saturating, NaN -> 0, truncating.
__device__ __forceinline__ uint32_t sat_u8(float x) {
    if (!(x > 0.0f)) return 0u;
    if (x >= 255.0f) return 255u;
    return (uint32_t)x;
}

// Wave-uniform read of scene data through the constant address space, so the
// backend emits s_load (scalar cache -> SGPRs) instead of 64 lane loads.
__device__ __forceinline__ float4 uniform_load(const float4 *base, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float *cfloat_ptr;
    const cfloat_ptr q = (cfloat_ptr)(const void *)base + 4u * i;
    return make_float4(q[0], q[1], q[2], q[3]);
#else
    return base[i];
#endif
}

__device__ __forceinline__ uint32_t uniform_load_u32(const uint32_t *base, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t *cu32_ptr;
    return ((cu32_ptr)(const void *)base)[i];
#else
    return base[i];
#endif
}

__device__ __forceinline__ uint4 uniform_load_u4(const uint4 *base, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint32_t *cu32_ptr;
    const cu32_ptr q = (cu32_ptr)(const void *)base + 4u * i;
    return make_uint4(q[0], q[1], q[2], q[3]);
#else
    return base[i];
#endif
}

__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) { return fastdiv_apply(n, f); }
// kGeneral: the divisor is known to be above 1 (f.one == 0, render.h
// trace_plain_ok), so the flag is neither loaded nor tested
template <bool kGeneral>
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f) {
    if (!kGeneral) return fastdiv_apply(n, f);
    const uint32_t t = __umulhi(n, f.m);
    return (t + ((n - t) >> 1)) >> f.s;
}

constexpr uint32_t kNodeEndDev = 0xFFFFFFFFu;  // bvh.h kNodeEnd
constexpr uint32_t kLeafBitDev = 0x80000000u;  // bvh.h kLeafBit
constexpr uint32_t kBatch = 8;  // spheres per scalar-load batch (sphere count padded to it)

}  // namespace
}  // namespace rtamd
