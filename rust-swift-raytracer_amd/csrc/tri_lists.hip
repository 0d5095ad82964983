// tri_lists.hip -- the primary triangle strip lists built on the device
// (DESIGN.md 5.3a): the twin of bvh.cpp build_primary_tri_lists, as
// serial.hip's spl_rect_kernel / spl_fill_kernel are the twin of
// build_primary_sphere_lists.  Same double operations in the same order
// (-ffp-contract=off), so offsets, items and the trailing `always` records hold
// the host build's bytes.  No atomic and no sort decides a position: records
// are culled 256 at a time and compacted in record order (ballot + mbcnt), a
// cell's count pass and fill pass run the same loop, and the offsets come from
// a fixed-shape scan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "render.h"

namespace rtamd {

namespace {

struct PtlConst { double Mi[9], o[3], wden, hden; };

// A record's span: strips [x, y] of bottom-counted rows [z, w].  Dropped
// records and `always` records carry spans that every tile culls (lo above any
// strip, hi below); y tells them apart.
__device__ __forceinline__ int4 ptl_dropped() { return make_int4(0x7FFFFFFF, -1, 0x7FFFFFFF, -1); }
__device__ __forceinline__ int4 ptl_always() { return make_int4(0x7FFFFFFF, -2, 0x7FFFFFFF, -1); }

// One thread per camera-origin record: its padded phantom box (6 floats)
// projected through the inverse camera map (bvh.cpp build_primary_tri_lists,
// the loop over i).
__global__ __launch_bounds__(256) void ptl_rect_kernel(const float *__restrict__ boxes, uint32_t n, PtlConst k,
                                                       uint32_t W, uint32_t H, int4 *__restrict__ rects) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *b = boxes + (size_t)i * 6;
    const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
    double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
    int front = 0, behind = 0;
    for (int c = 0; c < 8; ++c) {
        const double P[3] = {(c & 1 ? hi[0] : lo[0]) - k.o[0], (c & 2 ? hi[1] : lo[1]) - k.o[1],
                             (c & 4 ? hi[2] : lo[2]) - k.o[2]};
        double w[3];
        for (int r = 0; r < 3; ++r) w[r] = k.Mi[3 * r] * P[0] + k.Mi[3 * r + 1] * P[1] + k.Mi[3 * r + 2] * P[2];
        const double wn = fabs(w[0]) + fabs(w[1]) + fabs(w[2]);
        if (w[2] > 1e-6 * wn) {
            ++front;
            umin = fmin(umin, w[0] / w[2]); umax = fmax(umax, w[0] / w[2]);
            vmin = fmin(vmin, w[1] / w[2]); vmax = fmax(vmax, w[1] / w[2]);
        } else if (w[2] < -1e-6 * wn) {
            ++behind;
        }
    }
    int4 rect = ptl_dropped();
    if (behind != 8 && front < 8) {
        rect = ptl_always();
    } else if (front == 8) {
        const double cl = floor(umin * k.wden) - 2, ch = floor(umax * k.wden) + 1;
        const double rl = floor(vmin * k.hden) - 2, rh = floor(vmax * k.hden) + 1;
        if (!(ch < 0 || cl > (double)(W - 1) || rh < 0 || rl > (double)(H - 1))) {
            const int c0 = cl < 0 ? 0 : (int)cl, c1 = ch > (double)(W - 1) ? (int)(W - 1) : (int)ch;
            const int r0 = rl < 0 ? 0 : (int)rl, r1 = rh > (double)(H - 1) ? (int)(H - 1) : (int)rh;
            rect = make_int4(c0 / (int)kPrimaryTriStripW, c1 / (int)kPrimaryTriStripW, r0, r1);
        }
    }
    rects[i] = rect;
}

// One thread per cell (a strip of one bottom-counted row) of a 16 x 16 tile of
// cells.  Spans are culled against the tile 256 at a time and compacted, in
// record order, into LDS; each cell then takes the survivors that cover it.
// kFill = false: count[cell] = its records.  kFill = true: the same loop
// writes them to items from offsets[cell] on (ascending records; `cap` bounds
// every store).
template <bool kFill>
__global__ __launch_bounds__(256) void ptl_cell_kernel(const int4 *__restrict__ rects, uint32_t n, uint32_t spr,
                                                       uint32_t H, uint32_t *__restrict__ count,
                                                       const uint32_t *__restrict__ offsets,
                                                       uint32_t *__restrict__ items, uint32_t cap) {
    __shared__ int4 rl[256];
    __shared__ uint32_t ri[256];
    __shared__ uint32_t wc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int st = (int)(blockIdx.x * 16 + (tid & 15u)), row = (int)(blockIdx.y * 16 + (tid >> 4));
    const bool on = st < (int)spr && row < (int)H;
    const int ts0 = (int)(blockIdx.x * 16), ts1 = min(ts0 + 15, (int)spr - 1);
    const int tr0 = (int)(blockIdx.y * 16), tr1 = min(tr0 + 15, (int)H - 1);
    const size_t cell = (size_t)row * spr + (uint32_t)st;
    uint32_t cnt = 0;
    const uint32_t base = kFill && on ? offsets[cell] : 0u;
    for (uint32_t b0 = 0; b0 < n; b0 += 256) {
        const uint32_t i = b0 + tid;
        int4 r = ptl_dropped();
        if (i < n) r = rects[i];
        const bool keep = r.x <= ts1 && r.y >= ts0 && r.z <= tr1 && r.w >= tr0;
        const uint64_t m = __ballot(keep);
        if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            off += w < wave ? wc[w] : 0u;
            total += wc[w];
        }
        if (keep) {
            const uint32_t pos = off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            rl[pos] = r;
            ri[pos] = i;
        }
        __syncthreads();
        for (uint32_t j = 0; j < total; ++j) {
            const int4 q = rl[j];
            if (st >= q.x && st <= q.y && row >= q.z && row <= q.w) {
                if (kFill && on) {
                    const uint32_t pos = base + cnt;
                    if (pos < cap) items[pos] = ri[j];
                }
                ++cnt;
            }
        }
        // (no third barrier: wc was last read before the second one, and rl / ri
        // are rewritten only after the next batch's first)
    }
    if (!kFill && on) count[cell] = cnt;
}

// offsets[0] = 0, offsets[c + 1] = count[0] + ... + count[c] (u32, as the host's
// running sum), one workgroup of 1024 walking the cells in chunks with a carry:
// the same shape whatever the data.  meta[0] = the total; meta[2] = 1 when the
// 64-bit total does not fit the host's u32.
__global__ __launch_bounds__(1024) void ptl_scan_kernel(const uint32_t *__restrict__ count, uint32_t ncells,
                                                        uint32_t *__restrict__ offsets, uint32_t *__restrict__ meta) {
    __shared__ unsigned long long ws[16];
    __shared__ unsigned long long carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) { carry_s = 0; offsets[0] = 0; }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < ncells; b0 += 1024) {
        const uint32_t c = b0 + tid;
        unsigned long long v = c < ncells ? count[c] : 0u;
        // inclusive scan inside the wave
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d, 64);
            if (lane >= d) v += t;
        }
        if (lane == 63) ws[wave] = v;
        __syncthreads();
        unsigned long long before = carry_s, all = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wave ? ws[w] : 0ull;
            all += ws[w];
        }
        if (c < ncells) offsets[c + 1] = (uint32_t)(before + v);
        __syncthreads();
        if (tid == 0) carry_s += all;
        __syncthreads();
    }
    if (tid == 0) {
        meta[0] = (uint32_t)carry_s;
        meta[2] = carry_s > 0x7FFFFFFFull ? 1u : 0u;
    }
}

// The `always` records, ascending, to alw (n u32 of scratch); meta[1] = their
// number.  One workgroup, 256 records at a time, compacted in record order.
__global__ __launch_bounds__(256) void ptl_always_kernel(const int4 *__restrict__ rects, uint32_t n,
                                                         uint32_t *__restrict__ alw, uint32_t *__restrict__ meta) {
    __shared__ uint32_t wc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t done = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 256) {
        const uint32_t i = b0 + tid;
        const bool keep = i < n && rects[i].y == -2;
        const uint64_t m = __ballot(keep);
        if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (uint32_t w = 0; w < 4; ++w) {
            off += w < wave ? wc[w] : 0u;
            total += wc[w];
        }
        if (keep)
            alw[done + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = i;
        done += total;
        __syncthreads();
    }
    if (tid == 0) meta[1] = done;
}

}  // namespace

hipError_t launch_tri_list_counts(const float *boxes, uint32_t n, const double *Mi, const double *o, double wden,
                                  double hden, uint32_t width, uint32_t height, int4 *rects, uint32_t *count,
                                  uint32_t *offsets, uint32_t *alw, uint32_t *meta, hipStream_t stream) {
    PtlConst k;
    for (int i = 0; i < 9; ++i) k.Mi[i] = Mi[i];
    for (int i = 0; i < 3; ++i) k.o[i] = o[i];
    k.wden = wden;
    k.hden = hden;
    const uint32_t spr = (width + kPrimaryTriStripW - 1) / kPrimaryTriStripW;
    const dim3 tiles((spr + 15) / 16, (height + 15) / 16);
    if (n == 0 || tiles.y > 65535u || (uint64_t)spr * height >= 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ptl_rect_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, boxes, n, k, width, height,
                       rects);
    hipLaunchKernelGGL(ptl_cell_kernel<false>, tiles, dim3(256), 0, stream, rects, n, spr, height, count,
                       (const uint32_t *)nullptr, (uint32_t *)nullptr, 0u);
    hipLaunchKernelGGL(ptl_scan_kernel, dim3(1), dim3(1024), 0, stream, count, spr * height, offsets, meta);
    hipLaunchKernelGGL(ptl_always_kernel, dim3(1), dim3(256), 0, stream, rects, n, alw, meta);
    return hipGetLastError();
}

hipError_t launch_tri_list_fill(const int4 *rects, uint32_t n, uint32_t width, uint32_t height,
                                const uint32_t *offsets, const uint32_t *alw, uint32_t total, uint32_t nalways,
                                uint32_t *items, hipStream_t stream) {
    const uint32_t spr = (width + kPrimaryTriStripW - 1) / kPrimaryTriStripW;
    const dim3 tiles((spr + 15) / 16, (height + 15) / 16);
    if (n == 0 || tiles.y > 65535u) return hipErrorInvalidValue;
    if (total)
        hipLaunchKernelGGL(ptl_cell_kernel<true>, tiles, dim3(256), 0, stream, rects, n, spr, height,
                           (uint32_t *)nullptr, offsets, items, total);
    if (nalways) {
        hipError_t e = hipMemcpyAsync(items + total, alw, (size_t)nalways * 4, hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

}  // namespace rtamd
