// kernels.h -- what the HIP units (render.hip, serial.hip) share beside
// render.h: device-side constants and helpers, each defined once.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtamd {

constexpr uint32_t kWave = 64;
constexpr uint32_t kSphListWalk = 0xFFFFu;  // bvh.h kSphListWalk
constexpr uint32_t kSphListMaxDev = 3u;     // bvh.h kSphListMax

// SERIAL walks (serial.hip) and the coalescing search (serial_coalesce.h, in render.hip's unit)
constexpr uint32_t kWalkLeft = 0x80000000u;  // bend: the walk left a window (offsets stay below 2^31)
// (the iteration's candidates per sample: ctrl[5] when set, else the launch's K)
__device__ __forceinline__ uint32_t serial_k(const uint32_t *ctrl, uint32_t K) {
    const uint32_t k = ctrl[5];
    return k != 0u && k < K ? k : K;
}

}  // namespace rtamd
