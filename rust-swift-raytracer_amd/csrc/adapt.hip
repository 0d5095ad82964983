// adapt.hip -- the adaptive accumulator's list kernels: the
// per-pixel convergence decision (select) and the order-preserving compaction
// of the active list (compact).  None of them traces a ray; the adaptive trace
// instances (adapt::trace_kernel) are in render.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

namespace rtamd {
namespace {

constexpr uint32_t kAdaptWaves = kAdaptBlock / kWave;
constexpr uint32_t kScanBlock = 1024;

__global__ __launch_bounds__(kAdaptBlock) void adapt_iota_kernel(uint32_t *list, uint32_t n) {
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    if (i < n) list[i] = i;
}

// The decision of DESIGN.md 5.7, every step one rounded f32 operation:
//   m = ((R + G) + B) inv, v = max0(q inv - m m) (NaN stays NaN), e = v inv,
//   lim = tolerance (m + bias); converged iff e <= lim lim (false for NaN).
__global__ __launch_bounds__(kAdaptBlock) void adapt_select_kernel(
    const uint32_t *__restrict__ list, uint32_t n, const float *__restrict__ sums,
    const float *__restrict__ sumsq, size_t plane, uint32_t *__restrict__ count, uint32_t *__restrict__ keep,
    uint32_t N, float inv, float tolerance, float bias, uint32_t decide) {
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t idx = list[i];
    count[idx] = N;
    uint32_t k = 1u;
    if (decide) {
        const float R = sums[idx], G = sums[plane + idx], B = sums[2 * plane + idx], q = sumsq[idx];
        const float m = ((R + G) + B) * inv;
        const float qm = q * inv;
        const float mm = m * m;
        float v = qm - mm;
        v = v < 0.0f ? 0.0f : v;
        const float e = v * inv;
        const float lim = tolerance * (m + bias);
        k = e <= lim * lim ? 0u : 1u;
    }
    keep[i] = k;
}

// A lane's rank among its wave's set flags and the wave's number of them.
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t &total) {
    const uint64_t b = __ballot(flag);
    total = (uint32_t)__popcll(b);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// totals[block] = kept entries of the block's kAdaptBlock entries
__global__ __launch_bounds__(kAdaptBlock) void adapt_count_kernel(const uint32_t *__restrict__ keep, uint32_t n,
                                                                   uint32_t *__restrict__ totals) {
    __shared__ uint32_t wsum[kAdaptWaves];
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    uint32_t total;
    (void)wave_rank(i < n && keep[i < n ? i : 0u] != 0u, total);
    if (threadIdx.x % kWave == 0) wsum[threadIdx.x / kWave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kAdaptWaves; ++w) t += wsum[w];
        totals[blockIdx.x] = t;
    }
}

// One workgroup: totals[0, nblocks) become their exclusive prefix sums, tile
// by tile with a carried base (a fixed shape: the result does not depend on
// timing), and *len the sum of all.
__global__ __launch_bounds__(kScanBlock) void adapt_scan_kernel(uint32_t *totals, uint32_t nblocks, uint32_t *len) {
    __shared__ uint32_t wsum[kScanBlock / kWave];
    __shared__ uint32_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (tid == 0) carry_s = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += kScanBlock) {
        const uint32_t i = base + tid;
        const uint32_t v = i < nblocks ? totals[i] : 0u;
        uint32_t x = v;  // inclusive scan inside the wave
        for (uint32_t off = 1; off < kWave; off <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)x, off);
            if (lane >= off) x += t;
        }
        if (lane == kWave - 1) wsum[wave] = x;
        __syncthreads();
        uint32_t before = carry_s;  // the tiles before this one, then this tile's waves before this one
        uint32_t tile = 0;
        for (uint32_t w = 0; w < kScanBlock / kWave; ++w) {
            before += w < wave ? wsum[w] : 0u;
            tile += wsum[w];
        }
        if (i < nblocks) totals[i] = before + x - v;
        __syncthreads();
        if (tid == 0) carry_s += tile;
        __syncthreads();
    }
    if (tid == 0) *len = carry_s;
}

// out[totals[block] + rank inside the block] = list[i] for the kept entries
__global__ __launch_bounds__(kAdaptBlock) void adapt_scatter_kernel(
    const uint32_t *__restrict__ list, const uint32_t *__restrict__ keep, uint32_t n,
    const uint32_t *__restrict__ totals, uint32_t *__restrict__ out) {
    __shared__ uint32_t wsum[kAdaptWaves];
    const uint32_t i = blockIdx.x * kAdaptBlock + threadIdx.x;
    const bool kept = i < n && keep[i < n ? i : 0u] != 0u;
    uint32_t total;
    const uint32_t rank = wave_rank(kept, total);
    const uint32_t wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) wsum[wave] = total;
    __syncthreads();
    uint32_t pos = totals[blockIdx.x] + rank;
    for (uint32_t w = 0; w < kAdaptWaves; ++w) pos += w < wave ? wsum[w] : 0u;
    if (kept) out[pos] = list[i];
}

}  // namespace

hipError_t launch_adapt_iota(uint32_t *list, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(adapt_iota_kernel, dim3((uint32_t)adapt_compact_blocks(n)), dim3(kAdaptBlock), 0, stream,
                       list, n);
    return hipGetLastError();
}

hipError_t launch_adapt_select(const uint32_t *list, uint32_t n, const float *sums, const float *sumsq,
                               size_t plane, uint32_t *count, uint32_t *keep, uint32_t N, float inv,
                               float tolerance, float bias, bool decide, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(adapt_select_kernel, dim3((uint32_t)adapt_compact_blocks(n)), dim3(kAdaptBlock), 0, stream,
                       list, n, sums, sumsq, plane, count, keep, N, inv, tolerance, bias, decide ? 1u : 0u);
    return hipGetLastError();
}

hipError_t launch_adapt_compact(const uint32_t *list, const uint32_t *keep, uint32_t n, uint32_t *totals,
                                uint32_t *out, uint32_t *len, hipStream_t stream) {
    if (n == 0) return hipMemsetAsync(len, 0, sizeof(uint32_t), stream);
    const uint32_t blocks = (uint32_t)adapt_compact_blocks(n);
    hipLaunchKernelGGL(adapt_count_kernel, dim3(blocks), dim3(kAdaptBlock), 0, stream, keep, n, totals);
    hipLaunchKernelGGL(adapt_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, totals, blocks, len);
    hipLaunchKernelGGL(adapt_scatter_kernel, dim3(blocks), dim3(kAdaptBlock), 0, stream, list, keep, n, totals, out);
    return hipGetLastError();
}

}  // namespace rtamd
