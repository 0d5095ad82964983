// serial.hip -- the kernels of the render path that never trace a ray: the
// SERIAL mode's stream machinery (window, block walks, superblocks, finish,
// states; the estimate reduction and its scans; reach, check count, table reuse
// and gather), the primary sphere lists built on the device, and the
// multi-device frame assembly.  The kernels that trace (trace_kernel,
// serial_coalesce_kernel) are in render.hip's unit (serial_coalesce.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

namespace rtamd {

// ------------------------------------------------------------ SERIAL mode
// The reference draws every sample from ONE xorshift32 stream (common.rs:321):
// sample j starts at stream position P_j = 2j + 3B_j, B_j = the diffuse/metal
// scatters of all earlier samples.  serial_states.cpp render_frame_serial finds
// every P_j chunk by chunk: trace_kernel (kRngSerialCount) traces each sample
// of the chunk from K candidate positions around its predicted one,
// the walk kernels follow the true path through that table, and the frame
// is then rendered in REPLAY mode from the start states found.

// xorshift32^(2^i) as 32 columns (GF(2) matrix): y = XOR of columns c with bit c of x set
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t *cols, uint32_t x) {
    uint32_t y = 0;
#pragma unroll 8
    for (uint32_t c = 0; c < 32u; ++c) y ^= (x >> c & 1u) ? cols[c] : 0u;
    return y;
}

// the same from a matrix in global memory (tabulated powers), 16-B loads
__device__ __forceinline__ uint32_t gf2_apply_g(const uint32_t *cols, uint32_t x) {
    const uint4 *c4 = reinterpret_cast<const uint4 *>(cols);
    uint32_t y = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8u; ++q) {
        const uint4 m = c4[q];
        y ^= (x >> (4u * q) & 1u) ? m.x : 0u;
        y ^= (x >> (4u * q + 1u) & 1u) ? m.y : 0u;
        y ^= (x >> (4u * q + 2u) & 1u) ? m.z : 0u;
        y ^= (x >> (4u * q + 3u) & 1u) ? m.w : 0u;
    }
    return y;
}

// Window: thread t writes win[4t, 4t + 4): one jump to 4t (two tabulated
// matrices), then plain xorshift steps.  (16 states per thread and one
// matrix apply per set bit of 16t until round 5: a few dozen workgroups of
// long jumps, 16 us per iteration on world.txt 960x540x16.)
constexpr uint32_t kWinPerThread = kSerialWinPerThread;
// It also tabulates the iteration's window bases lo[jl] = serial_lo(a, jl) for
// jl < L (a = ctrl[4], K = the iteration's candidates), which the count pass
// and the walks then load instead of evaluating M twice per step.
// pix_spp != 0 (the pixel table pass follows): ctrl[7] = max over the
// iteration's pixels of the stream positions their samples' windows span.
__global__ __launch_bounds__(256) void serial_window_kernel(uint32_t *__restrict__ ctrl,
                                                            const uint32_t *__restrict__ jump,
                                                            uint32_t *__restrict__ win, uint32_t n,
                                                            SerialPred M, uint32_t *__restrict__ lo,
                                                            uint32_t L, uint32_t Kmax, uint32_t depth,
                                                            uint32_t nserial, uint32_t pix_spp, uint32_t pix_emax,
                                                            uint32_t *__restrict__ counters, uint32_t ncounters,
                                                            uint4 *__restrict__ spix, uint32_t pix_chunk,
                                                            const uint4 *__restrict__ spix_prev) {
    if (ctrl[0] != 0u) return;
    // the following trace pass's job counters (instead of a fill launch)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ncounters; i += gridDim.x * blockDim.x)
        counters[32u * i] = 0u;
    if (lo != nullptr) {
        const uint32_t k = ctrl[5];
        const uint32_t K = k != 0u && k < Kmax ? k : Kmax;  // (serial_k)
        const uint32_t a = ctrl[4];
        for (uint32_t jl = blockIdx.x * blockDim.x + threadIdx.x; jl < L; jl += gridDim.x * blockDim.x)
            lo[jl] = serial_lo(M, a, jl, K, depth, nserial);
        if (pix_spp != 0u) {
            // local pixel q: samples [jf, jz] of the iteration, windows from
            // 2 jf + 3 lo(jf) to 2 jz + 3 (lo(jz) + K - 1)
            const uint32_t ln = min(L, nserial - a);
            const uint32_t p0 = a / pix_spp, npq = (a + ln - 1u) / pix_spp - p0 + 1u;
            // the previous iteration (serial_walk_finish_kernel: its first sample
            // ctrl[10], its table's row stride ctrl[11], this iteration's window
            // at its stream offset ctrl[8]; ctrl[9] set once one has run)
            const bool reuse = spix_prev != nullptr && ctrl[9] != 0u && ctrl[11] != 0u;
            const uint32_t ap = ctrl[10], D = ctrl[8], Ep = ctrl[11];
            const uint32_t p0p = ap / pix_spp;
            const uint32_t npqp = reuse ? (ap + min(L, nserial - ap) - 1u) / pix_spp - p0p + 1u : 0u;
            uint32_t span = 0;
            for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < npq; q += gridDim.x * blockDim.x) {
                const uint32_t jf = q == 0u ? 0u : (p0 + q) * pix_spp - a;
                const uint32_t jz = min((p0 + q + 1u) * pix_spp - a, ln) - 1u;
                const uint32_t lf = serial_lo(M, a, jf, K, depth, nserial);
                const uint32_t lz = serial_lo(M, a, jz, K, depth, nserial);
                const uint32_t hi = 2u * jz + 3u * (lz + K - 1u), lo0 = 2u * jf + 3u * lf;
                span = max(span, hi >= lo0 ? hi - lo0 + 1u : 1u);
                if (spix != nullptr) {
                    // the positions of this pixel the previous table holds: its
                    // traced range [plo', min(phi', plo' + E' - 1)] at offset -D,
                    // inside [lo0, hi] (relative to lo0; empty: z > w)
                    uint32_t r0 = 1u, r1 = 0u;
                    const uint32_t pix = p0 + q;
                    if (reuse && pix >= p0p && pix - p0p < npqp) {
                        const uint4 so = spix_prev[pix - p0p];
                        if (so.y >= so.x) {
                            const int64_t olo = (int64_t)so.x - D;
                            const int64_t ohi = (int64_t)min(so.y, so.x + Ep - 1u) - D;
                            const int64_t l = olo > (int64_t)lo0 ? olo : (int64_t)lo0;
                            const int64_t h = ohi < (int64_t)hi ? ohi : (int64_t)hi;
                            if (l <= h) {
                                r0 = (uint32_t)(l - lo0);
                                r1 = (uint32_t)(h - lo0);
                            }
                        }
                    }
                    spix[q] = make_uint4(lo0, hi, r0, r1);
                }
            }
            // (rounded up to whole chunks of the pass's job queue (pix_chunk,
            // spix: rows of one pixel per chunk) and clamped to the table's row
            // stride, a multiple of it: every reader takes ctrl[7] as is, and a
            // position past it reads as "left the window")
            if (spix != nullptr && pix_chunk > 1u) span = (span + pix_chunk - 1u) / pix_chunk * pix_chunk;
            span = min(span, pix_emax);
            if (span) atomicMax(ctrl + 7, span);
        }
    }
    // the jump matrices this workgroup's threads need (bits of i0 below 32),
    // staged in LDS: the jumps then read no global memory
    __shared__ uint32_t jl_lds[32 * 32];
    for (uint32_t i = threadIdx.x; i < 32u * 32u; i += blockDim.x) jl_lds[i] = jump[i];
    __syncthreads();
    const uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * kWinPerThread;
    if (i0 >= n) return;
    uint32_t x = ctrl[1];
    // the jump to i0: M^(4096 j) M^(4 j') from the tabulated powers (two
    // applies; were one per set bit of i0, ~7 on average), higher bits by
    // powers of two
    x = gf2_apply_g(jump + 32u * (64u + kSerialJumpT1 + ((i0 >> 12) & 255u)), x);
    x = gf2_apply_g(jump + 32u * (64u + ((i0 & 4095u) / kWinPerThread)), x);
    for (uint32_t b = 20; (i0 >> b) != 0u; ++b)
        if ((i0 >> b) & 1u) x = gf2_apply(jl_lds + 32u * b, x);
    for (uint32_t q = 0; q < kWinPerThread && i0 + q < n; ++q) {
        win[i0 + q] = x;
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
    }
}

// The walk through an iteration's candidate table (b of chunk sample jl at
// candidate k = table[jl * K + k]; candidate k means B = lo[jl] + k scatters
// since sample a, lo = serial_lo tabulated by serial_window_kernel) in short
// dependent-load chains instead of one of L:
//   blocks: for every block of R samples and every candidate of its first
//     sample, follow R samples: its end offset, or kWalkLeft | the samples
//     walked before one left its window (the path of every walk recorded);
//   super: for every group of kSuperBlocks blocks and every candidate of its
//     first block, chain through the group's block ends (recording each
//     block's start offset);
//   finish: one lane chains the superblock ends from B = 0 as far as they
//     are valid, the workgroup fills the full blocks' path columns from the
//     recorded starts, and serial_states_kernel gathers the start states
//     (win[2 jl + 3 B]) of every resolved sample from the recorded paths; ctrl
//     advances past the resolved samples (>= 1: sample a's own window always
//     holds B = 0).
constexpr uint32_t kWalkInvalid = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t walk_step(const float *table, const SerialPred &M, uint32_t a,
                                              uint32_t K, uint32_t depth, uint32_t nserial, uint32_t jl,
                                              uint32_t B, const uint32_t *lo = nullptr) {
    const uint32_t l = lo ? lo[jl] : serial_lo(M, a, jl, K, depth, nserial);
    const float b = (B >= l && B - l < K) ? table[(size_t)jl * K + (B - l)] : -1.0f;
    return b >= 0.0f ? B + (uint32_t)b : kWalkInvalid;
}

// path (optional): the offset B at the start of each of the block's samples,
// sample-major (path[(jl - j0) * nb * K + t], coalesced), so that the states
// of the true path are a gather (serial_states_kernel), not a re-walk
// ptab (the pixel table pass, kRngSerialPixel): b is read from the traced
// (pixel, position) table itself -- b of sample jl at offset B is
// ptab[q E + (2 jl + 3 B - plo(q))], q its local pixel -- instead of a
// gathered L x K count table (a 16 MB table instead of an 80 MB one at 32 k x
// 617, and no gather pass); ppix: the frame's spp as a divider.
__global__ __launch_bounds__(256) void serial_walk_blocks_kernel(
    const uint32_t *__restrict__ ctrl, const float *__restrict__ table, SerialPred M,
    uint32_t *__restrict__ bend, uint32_t *__restrict__ path, const uint32_t *__restrict__ lo, uint32_t L,
    uint32_t K, uint32_t R, uint32_t depth, uint32_t nserial, const float *__restrict__ ptab, FastDiv ppix) {
    if (ctrl[0] != 0u) return;
    K = serial_k(ctrl, K);
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nb = (n + R - 1) / R;
    if (t >= nb * K) return;
    const uint32_t blk = t / K, k0 = t - blk * K;
    const uint32_t j0 = blk * R, j1 = min(j0 + R, n);
    const size_t stride = (size_t)nb * K;
    uint32_t B = (lo ? lo[j0] : serial_lo(M, a, j0, K, depth, nserial)) + k0;
    uint32_t jl = j0;
    if (ptab != nullptr) {
        const uint32_t E = ctrl[7], spp = ppix.d;
        const uint32_t p0 = fastdiv_apply(a, ppix);
        uint32_t q = fastdiv_apply(a + j0, ppix) - p0;  // local pixel of sample jl
        uint32_t jf = q == 0u ? 0u : (p0 + q) * spp - a;  // its first sample in the iteration
        uint32_t jnext = (p0 + q + 1u) * spp - a;        // the next pixel's
        uint32_t plo = 2u * jf + 3u * lo[jf];
        for (; jl < j1; ++jl) {
            if (path) path[(size_t)(jl - j0) * stride + t] = B;
            if (jl == jnext) {
                ++q;
                plo = 2u * jnext + 3u * lo[jnext];
                jnext += spp;
            }
            const uint32_t l = lo[jl];
            const uint32_t pos = 2u * jl + 3u * B;
            const float b = (B >= l && B - l < K && pos >= plo && pos - plo < E)
                                ? ptab[(size_t)q * E + (pos - plo)]
                                : -1.0f;
            if (!(b >= 0.0f)) break;
            B += (uint32_t)b;
        }
    } else {
#pragma unroll 4
        for (; jl < j1; ++jl) {
            if (path) path[(size_t)(jl - j0) * stride + t] = B;
            const uint32_t nB = walk_step(table, M, a, K, depth, nserial, jl, B, lo);
            if (nB == kWalkInvalid) break;
            B = nB;
        }
    }
    // the block's end offset, or kWalkLeft | the samples whose end was found
    // (the path then holds the start offset of the sample that left)
    bend[t] = jl == j1 ? B : kWalkLeft | (jl - j0);
}

// ---- pixel table walks with the rows in LDS (kRngSerialPixel, depth < 255)
// One workgroup per block of R samples stages the pixel-table rows of the
// block's pixels -- positions [plo(q), phi(q)] of each local pixel q, the span
// its samples' windows cover (serial_pixel_span), as u8 scatter counts -- and
// then walks from LDS: the per-step reads that were dependent L2 loads (and
// the path of every candidate, 64 stores per lane) become LDS reads.  A
// position outside its pixel's traced span reads as "left the window" (the
// span, not the launch's widest one: positions past a narrower pixel's span
// were not traced).
struct WalkRowsLds {
    uint32_t lo[kMaxWalkR];              // lo[j0 .. j1)
    uint32_t plo[kWalkLdsMaxPix], span[kWalkLdsMaxPix], off[kWalkLdsMaxPix];
    uint32_t qa, nq;
};
// stages the rows of samples [j0, j1) of the iteration (whole workgroup; E:
// the pass's positions per pixel, ctrl[7])
__device__ __forceinline__ void walk_stage_rows(WalkRowsLds &w, uint8_t *rows, uint32_t E, const float *ptab,
                                                const uint32_t *lo, uint32_t a, uint32_t n, uint32_t j0,
                                                uint32_t j1, uint32_t K, FastDiv ppix) {
    const uint32_t spp = ppix.d;
    const uint32_t p0 = fastdiv_apply(a, ppix);
    const uint32_t qa = fastdiv_apply(a + j0, ppix) - p0, qb = fastdiv_apply(a + j1 - 1u, ppix) - p0;
    const uint32_t nq = qb - qa + 1u;
    for (uint32_t i = threadIdx.x; i < j1 - j0; i += blockDim.x) w.lo[i] = lo[j0 + i];
    if (threadIdx.x == 0) {
        w.qa = qa;
        w.nq = nq;
        uint32_t off = 0;
        for (uint32_t i = 0; i < nq; ++i) {
            const uint32_t q = qa + i;
            const uint32_t jf = q == 0u ? 0u : (p0 + q) * spp - a;
            const uint32_t jz = min((p0 + q + 1u) * spp - a, n) - 1u;
            const uint32_t plo = 2u * jf + 3u * lo[jf];
            const uint32_t phi = 2u * jz + 3u * (lo[jz] + K - 1u);
            // the traced positions: plo + e for e < E and plo + e <= phi
            const uint32_t sp = min(phi >= plo ? phi - plo + 1u : 0u, E);
            w.plo[i] = plo;
            w.span[i] = sp;
            w.off[i] = off;
            off += sp;
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < nq; ++i) {
        const float *src = ptab + (size_t)(qa + i) * E;
        uint8_t *dst = rows + w.off[i];
        for (uint32_t e = threadIdx.x; e < w.span[i]; e += blockDim.x) dst[e] = (uint8_t)src[e];
    }
    __syncthreads();
}

// b of sample jl (local pixel i = q - qa of the rows) at offset B, or -1
__device__ __forceinline__ int walk_lds_b(const WalkRowsLds &w, const uint8_t *rows, uint32_t i, uint32_t jl,
                                          uint32_t j0, uint32_t B, uint32_t K) {
    const uint32_t l = w.lo[jl - j0];
    const uint32_t pos = 2u * jl + 3u * B;
    const uint32_t e = pos - w.plo[i];
    return (B >= l && B - l < K && pos >= w.plo[i] && e < w.span[i]) ? (int)rows[w.off[i] + e] : -1;
}

// Block walks from LDS rows: bend and path as serial_walk_blocks_kernel (one
// workgroup of kWalkLdsThreads per block; the pixel's span and row offset stay
// in registers between pixel changes, so a step is one dependent LDS read).
constexpr uint32_t kWalkLdsThreads = 1024;
__global__ __launch_bounds__(kWalkLdsThreads) void serial_walk_blocks_lds_kernel(
    const uint32_t *__restrict__ ctrl, uint32_t *__restrict__ bend, uint32_t *__restrict__ path,
    const uint32_t *__restrict__ lo, uint32_t L, uint32_t Kmax, uint32_t R, uint32_t nserial,
    const float *__restrict__ ptab, FastDiv ppix) {
    if (ctrl[0] != 0u) return;
    const uint32_t K = serial_k(ctrl, Kmax);
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t nb = (n + R - 1) / R;
    const uint32_t blk = blockIdx.x;
    if (blk >= nb) return;  // (whole workgroups)
    __shared__ WalkRowsLds w;
    extern __shared__ uint8_t rows[];
    const uint32_t j0 = blk * R, j1 = min(j0 + R, n);
    walk_stage_rows(w, rows, ctrl[7], ptab, lo, a, n, j0, j1, K, ppix);
    const uint32_t spp = ppix.d, p0 = fastdiv_apply(a, ppix);
    const size_t stride = (size_t)nb * K;
    for (uint32_t k0 = threadIdx.x; k0 < K; k0 += blockDim.x) {
        const size_t t = (size_t)blk * K + k0;
        uint32_t B = w.lo[0] + k0;
        uint32_t i = 0;                                     // local pixel of sample jl, - qa
        uint32_t jnext = (p0 + w.qa + 1u) * spp - a;        // the next pixel's first sample
        uint32_t plo = w.plo[0], span = w.span[0], off = w.off[0];
        uint32_t jl = j0;
        for (; jl < j1; ++jl) {
#ifndef RT_DIAG_NO_PATH  // (timing-only diagnostic build: no path records, wrong states)
            path[(size_t)(jl - j0) * stride + t] = B;
#endif
            if (jl == jnext) {
                ++i;
                jnext += spp;
                plo = w.plo[i];
                span = w.span[i];
                off = w.off[i];
            }
            const uint32_t l = w.lo[jl - j0];
            const uint32_t pos = 2u * jl + 3u * B;
            const uint32_t e = pos - plo;
            if (!(B >= l && B - l < K && pos >= plo && e < span)) break;
            B += rows[off + e];
        }
        bend[t] = jl == j1 ? B : kWalkLeft | (jl - j0);
    }
}

// Superblocks of kSuperBlocks blocks: for every candidate start of a
// superblock's first block, the chain through its blocks' ends (bend), so that
// the finish kernel's chain is one dependent load per superblock.  sbend[sb *
// K + k]: the superblock's end offset, or kWalkLeft | the block (within it)
// where the chain stopped; sB[blk * K + k]: the offset at the start of its
// block blk (nb * K u32, coalesced over k).
constexpr uint32_t kSuperBlocks = 16;
constexpr size_t kSuperLdsBytes = 48 * 1024;  // serial_walk_super_lds_kernel's staged block ends
__global__ __launch_bounds__(256) void serial_walk_super_kernel(
    const uint32_t *__restrict__ ctrl, const uint32_t *__restrict__ bend, const uint32_t *__restrict__ lo,
    uint32_t *__restrict__ sbend, uint32_t *__restrict__ sB, uint32_t L, uint32_t Kmax, uint32_t R,
    uint32_t nserial) {
    if (ctrl[0] != 0u) return;
    const uint32_t K = serial_k(ctrl, Kmax);
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t nb = (n + R - 1) / R;
    const uint32_t ns = (nb + kSuperBlocks - 1) / kSuperBlocks;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ns * K) return;
    const uint32_t sb = t / K, k0 = t - sb * K;
    const uint32_t b0 = sb * kSuperBlocks, b1 = min(nb, b0 + kSuperBlocks);
    uint32_t B = lo[b0 * R] + k0;
    uint32_t blk = b0;
    for (; blk < b1; ++blk) {
        sB[(size_t)blk * K + k0] = B;
        const uint32_t l = lo[blk * R];
        if (!(B >= l && B - l < K)) break;
        const uint32_t e = bend[(size_t)blk * K + (B - l)];
        if (e & kWalkLeft) break;
        B = e;
    }
    sbend[t] = blk == b1 ? B : kWalkLeft | (blk - b0);
}

// The same with the superblock's block ends staged in LDS (one workgroup per
// superblock, kSuperBlocks * K u32 <= kSuperLdsBytes): the chain's dependent
// reads come from LDS instead of L2.
__global__ __launch_bounds__(1024) void serial_walk_super_lds_kernel(
    const uint32_t *__restrict__ ctrl, const uint32_t *__restrict__ bend, const uint32_t *__restrict__ lo,
    uint32_t *__restrict__ sbend, uint32_t *__restrict__ sB, uint32_t L, uint32_t Kmax, uint32_t R,
    uint32_t nserial) {
    if (ctrl[0] != 0u) return;
    const uint32_t K = serial_k(ctrl, Kmax);
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t nb = (n + R - 1) / R;
    const uint32_t ns = (nb + kSuperBlocks - 1) / kSuperBlocks;
    const uint32_t sb = blockIdx.x;
    if (sb >= ns) return;  // (whole workgroups)
    extern __shared__ uint32_t be[];  // bend of the superblock's blocks, [blk - b0][k]
    __shared__ uint32_t blo[kSuperBlocks];
    const uint32_t b0 = sb * kSuperBlocks, b1 = min(nb, b0 + kSuperBlocks);
    for (uint32_t i = threadIdx.x; i < (b1 - b0) * K; i += blockDim.x) be[i] = bend[(size_t)b0 * K + i];
    if (threadIdx.x < b1 - b0) blo[threadIdx.x] = lo[(b0 + threadIdx.x) * R];
    __syncthreads();
    for (uint32_t k0 = threadIdx.x; k0 < K; k0 += blockDim.x) {
        uint32_t B = blo[0] + k0;
        uint32_t blk = b0;
        for (; blk < b1; ++blk) {
            sB[(size_t)blk * K + k0] = B;
            const uint32_t l = blo[blk - b0];
            if (!(B >= l && B - l < K)) break;
            const uint32_t e = be[(blk - b0) * K + (B - l)];
            if (e & kWalkLeft) break;
            B = e;
        }
        sbend[(size_t)sb * K + k0] = blk == b1 ? B : kWalkLeft | (blk - b0);
    }
}

__global__ __launch_bounds__(256) void serial_walk_finish_kernel(
    uint32_t *__restrict__ ctrl, const float *__restrict__ table, SerialPred M,
    const double *__restrict__ V, uint32_t npix, uint32_t spp, const uint32_t *__restrict__ win,
    const uint32_t *__restrict__ bend, const uint32_t *__restrict__ path, uint32_t *__restrict__ states,
    uint32_t *__restrict__ fin, const uint32_t *__restrict__ lo, const uint32_t *__restrict__ sbend,
    const uint32_t *__restrict__ sB, uint32_t L, uint32_t Lw, uint32_t Kmax, uint32_t R, uint32_t depth,
    uint32_t nserial, float z, float sfloor) {
    __shared__ uint32_t bstart[kMaxWalkBlocks];
    __shared__ uint32_t blo[kMaxWalkBlocks];
    __shared__ uint32_t nfull;
    __shared__ uint32_t scol[kMaxWalkBlocks / kSuperBlocks + 1];  // the chain's column in each superblock
    __shared__ uint32_t cB, cblk, cleft;
    if (ctrl[0] != 0u) {
        if (fin && threadIdx.x == 0) fin[1] = fin[3] = 0u;  // (the states kernels: nothing)
        return;
    }
    const uint32_t K = serial_k(ctrl, Kmax);
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t nb = (n + R - 1) / R;
    const uint32_t ns = (nb + kSuperBlocks - 1) / kSuperBlocks;
    for (uint32_t blk = threadIdx.x; blk < nb; blk += blockDim.x)
        blo[blk] = lo ? lo[blk * R] : serial_lo(M, a, blk * R, K, depth, nserial);
    __syncthreads();
    // The chain through the superblock ends: one dependent load per
    // superblock (the block-by-block chain was 256 dependent L2 loads, 98 us
    // per iteration on c_raytracer 960x540x16); where it stops, the block and
    // its start offset come from the superblock's recorded block starts.
    if (threadIdx.x == 0) {
        uint32_t B = 0, sb = 0, blk = nb, left = 0;
        for (; sb < ns; ++sb) {
            const uint32_t b0 = sb * kSuperBlocks, l = blo[b0];
            if (!(B >= l && B - l < K)) {  // outside the first block's window
                blk = b0;
                break;
            }
            const uint32_t col = sb * K + (B - l);
            scol[sb] = col;
            const uint32_t e = sbend[col];
            if (e & kWalkLeft) {
                blk = b0 + (e & ~kWalkLeft);
                B = sB[(size_t)blk * K + (col - sb * K)];
                const uint32_t lb = blo[blk];
                if (B >= lb && B - lb < K) {
                    const uint32_t eb = bend[(size_t)blk * K + (B - lb)];
                    left = eb == kWalkInvalid ? 0u : eb & ~kWalkLeft;  // samples resolved in blk
                }
                break;
            }
            B = e;
        }
        cB = B;
        cblk = blk;
        cleft = left;
    }
    __syncthreads();
    // the full blocks' start offsets and path columns, in parallel
    for (uint32_t blk = threadIdx.x; blk < cblk; blk += blockDim.x) {
        const uint32_t sb = blk / kSuperBlocks;
        const uint32_t Bb = sB[(size_t)blk * K + (scol[sb] - sb * K)];
        bstart[blk] = Bb;
        if (fin) fin[4 + blk] = blk * K + (Bb - blo[blk]);  // the block's path column
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t B = cB, blk = cblk;
        nfull = blk;
        uint32_t done = min(blk * R, n);
        if (fin) {
            if (blk < nb && cleft > 0u) {
                // the path leaves a window inside this block, after cleft
                // samples whose states the block walk's path holds, as it
                // holds the start offset of the sample that left
                const uint32_t col = blk * K + (B - blo[blk]);
                fin[4 + blk] = col;
                B = path[(size_t)cleft * nb * K + col];
                done = blk * R + cleft;
            }
            fin[0] = a;
            fin[1] = blk;
            fin[2] = nb * K;
            fin[3] = done;  // the states to gather: samples [0, done) of the iteration
        }
        if (blk < nb && fin) {
            ctrl[6] += 1u;
        } else if (blk < nb) {
            // the path leaves a window inside this block: resolve it lane-serially
            // up to that sample (the window of the block's first sample holds B:
            // it was the previous block's valid end, or 0)
            const uint32_t j1 = min(blk * R + R, n);
            for (uint32_t jl = blk * R; jl < j1; ++jl) {
                const uint32_t nB = walk_step(table, M, a, K, depth, nserial, jl, B, lo);
                if (nB == kWalkInvalid) break;
                states[a + jl] = win[2u * jl + 3u * B];
                B = nB;
                done = jl + 1;
            }
            ctrl[6] += 1u;
        }
        ctrl[1] = win[2u * done + 3u * B];
        ctrl[2] += B;
        ctrl[3] += 1u;
        ctrl[4] = a + done;
        // (the next iteration's reuse of this one's pixel table: its window
        // starts at offset D = 2 done + 3 B of this one's; the first sample and
        // the row stride of this one's table)
        ctrl[8] = 2u * done + 3u * B;
        ctrl[9] = 1u;
        ctrl[10] = a;
        ctrl[11] = ctrl[7];
        ctrl[7] = 0u;  // (the next window kernel's pixel span, atomicMax)
        if (a + done >= nserial) ctrl[0] = 1u;
        if (V != nullptr) {
            // the next iteration's windows: +-z sigma of the scatter-count
            // deviation its samples can accumulate (V: prefix sums of the
            // per-sample variances from the estimate pass), plus the spread of
            // one sample; never more than the launch's Kmax
            // V: per-pixel prefix sums P (npix + 1) then variances (npix); the
            // variance of samples [0, j) is P[p] + (j - p spp) var[p], p = j / spp
            auto vsum = [&](uint32_t j) {
                const uint32_t q = min(j / spp, npix);
                return q < npix ? V[q] + (double)(j - q * spp) * V[npix + 1 + q] : V[npix];
            };
            const uint32_t a2 = min(a + done, nserial), e = min(a2 + Lw, nserial);
            const double v = vsum(e) - vsum(a2);
            const double w = ceil(2.0 * (double)z * (sqrt(v > 0.0 ? v : 0.0) + (double)sfloor * sqrt((double)(e - a2)))) +
                             (double)(2u * depth + 2u);
            ctrl[5] = w >= (double)Kmax ? Kmax : (uint32_t)w;
        }
    }
    __syncthreads();
    if (fin) return;  // the full blocks' states: serial_states_kernel (a gather)
    for (uint32_t blk = threadIdx.x; blk < nfull; blk += blockDim.x) {
        uint32_t B = bstart[blk];
        const uint32_t j1 = min(blk * R + R, n);
        for (uint32_t jl = blk * R; jl < j1; ++jl) {
            states[a + jl] = win[2u * jl + 3u * B];
            B = walk_step(table, M, a, K, depth, nserial, jl, B, lo);
        }
    }
}

// The start states of the iteration's full blocks, one thread per sample:
// the path the block walk recorded for the block's true start (fin, written by
// serial_walk_finish_kernel: {a, full blocks, path stride, samples of the
// iteration, column per block}).
__global__ __launch_bounds__(256) void serial_states_kernel(const uint32_t *__restrict__ fin,
                                                            const uint32_t *__restrict__ path,
                                                            const uint32_t *__restrict__ win,
                                                            uint32_t *__restrict__ states, uint32_t R) {
    const uint32_t jl = blockIdx.x * blockDim.x + threadIdx.x;
    if (jl >= fin[3]) return;
    const uint32_t blk = jl / R;
    const uint32_t B = path[(size_t)(jl - blk * R) * fin[2] + fin[4 + blk]];
    states[fin[0] + jl] = win[2u * jl + 3u * B];
}

// ---- the estimate reduction (render.h serial_tab_doubles for the layout)
// One thread per pixel: its spp * R scatter counts (contiguous) summed in
// double; a negative or NaN count (a lost draw count) raises the flag.
__global__ __launch_bounds__(256) void serial_moments_kernel(const float *__restrict__ est, uint32_t pix0,
                                                             uint32_t n, uint32_t spp, uint32_t R,
                                                             double scale, double *__restrict__ tab,
                                                             uint32_t npix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t per = spp * R;
    const float *src = est + (size_t)i * per;
    double s = 0.0, sq = 0.0;
    bool bad = false;
    for (uint32_t k = 0; k < per; ++k) {
        const float b = src[k];
        bad |= !(b >= 0.0f);
        s += (double)b;
        sq += (double)b * (double)b;
    }
    const uint32_t p = pix0 + i;
    const double mu = s / (double)per;
    const double v = sq / (double)per - mu * mu;
    tab[npix + 1 + p] = mu;
    tab[3 * (size_t)npix + 2 + p] = (v > 0.0 ? v : 0.0) * scale;
    tab[4 * (size_t)npix + 2 + p] = sq - s * mu;
    if (bad) tab[5 * (size_t)npix + 5] = 1.0;
}

// Prefix sums over pixels of (spp mu, spp var, ss) in tiles of kScanTile:
// tile totals, one workgroup's exclusive scan of the totals, then each tile's
// own scan from its offset.  The shape is fixed, so the sums are the same
// bits on every call.
constexpr uint32_t kScanTile = 1024;
__device__ __forceinline__ void scan_inputs(const double *tab, uint32_t npix, uint32_t spp, uint32_t p,
                                            double v[3]) {
    if (p >= npix) { v[0] = v[1] = v[2] = 0.0; return; }
    v[0] = (double)spp * tab[npix + 1 + p];
    v[1] = (double)spp * tab[3 * (size_t)npix + 2 + p];
    v[2] = tab[4 * (size_t)npix + 2 + p];
}

// inclusive scan of 256 values x 3 across the workgroup (Hillis-Steele in LDS)
__device__ __forceinline__ void block_scan3(double (*sh)[256], double v[3]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) sh[c][t] = v[c];
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        double a[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = t >= off ? sh[c][t - off] : 0.0;
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) sh[c][t] += a[c];
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = sh[c][t];
    __syncthreads();
}

__global__ __launch_bounds__(256) void serial_scan_tiles_kernel(const double *__restrict__ tab, uint32_t npix,
                                                                uint32_t spp, double *__restrict__ tsum) {
    __shared__ double sh[3][256];
    const uint32_t p0 = blockIdx.x * kScanTile + threadIdx.x * 4u;
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = 0; k < 4; ++k) {
        double v[3];
        scan_inputs(tab, npix, spp, p0 + k, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += v[c];
    }
    block_scan3(sh, acc);
    if (threadIdx.x == 255)
#pragma unroll
        for (int c = 0; c < 3; ++c) tsum[3 * blockIdx.x + c] = acc[c];
}

// one workgroup: exclusive scan of the ntiles totals in place
__global__ __launch_bounds__(256) void serial_scan_totals_kernel(double *__restrict__ tsum, uint32_t ntiles) {
    __shared__ double sh[3][256];
    const uint32_t per = (ntiles + 255u) / 256u;
    const uint32_t b = threadIdx.x * per, e = min(b + per, ntiles);
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = b; i < e; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += tsum[3 * i + c];
    double inc[3] = {acc[0], acc[1], acc[2]};
    block_scan3(sh, inc);
    double run[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) run[c] = inc[c] - acc[c];  // (exclusive: the sum before b)
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) run[c] = 0.0;
    for (uint32_t i = b; i < e; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double x = tsum[3 * i + c];
            tsum[3 * i + c] = run[c];
            run[c] += x;
        }
}

__global__ __launch_bounds__(256) void serial_scan_apply_kernel(double *__restrict__ tab, uint32_t npix,
                                                                uint32_t spp, const double *__restrict__ tsum) {
    __shared__ double sh[3][256];
    const uint32_t p0 = blockIdx.x * kScanTile + threadIdx.x * 4u;
    double v[4][3], acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t k = 0; k < 4; ++k) {
        scan_inputs(tab, npix, spp, p0 + k, v[k]);
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += v[k][c];
    }
    double inc[3] = {acc[0], acc[1], acc[2]};
    block_scan3(sh, inc);
    double run[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) run[c] = tsum[3 * blockIdx.x + c] + (inc[c] - acc[c]);
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < 3; ++c) run[c] = tsum[3 * blockIdx.x + c];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        tab[0] = 0.0;                         // P[0]
        tab[2 * (size_t)npix + 1] = 0.0;      // PV[0]
    }
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t p = p0 + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) run[c] += v[k][c];
        if (p < npix) {
            tab[p + 1] = run[0];
            tab[2 * (size_t)npix + 2 + p] = run[1];
            if (p + 1 == npix) tab[5 * (size_t)npix + 2] = run[2];  // sum of ss
        }
    }
}

// dmax over the window starts a = i q, q = max(1, L / 4) (atomicMax on the
// bits of a non-negative double orders like the doubles), plus V(n0).
__global__ __launch_bounds__(256) void serial_reach_kernel(double *__restrict__ tab, uint32_t npix, uint32_t spp,
                                                           uint32_t L, uint32_t n0) {
    const SerialPred m{tab, tab + npix + 1, spp, npix};
    const uint32_t N = npix * spp;  // (< 2^32, serial_states.cpp)
    const uint32_t q = max(1u, L / 4u);
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long *dmax = reinterpret_cast<unsigned long long *>(tab + 5 * (size_t)npix + 3);
    if (i * q < N) {
        const uint32_t a = (uint32_t)(i * q);
        const uint64_t e = (uint64_t)a + L + L / 4u;
        const double d = serial_M(m, e < N ? (uint32_t)e : N) - serial_M(m, a);
        atomicMax(dmax, (unsigned long long)__double_as_longlong(d > 0.0 ? d : 0.0));
    }
    if (i == 0) {
        const double *PV = tab + 2 * (size_t)npix + 1, *var = tab + 3 * (size_t)npix + 2;
        const uint32_t p = n0 / spp;
        tab[5 * (size_t)npix + 4] = p < npix ? PV[p] + (double)(n0 - p * spp) * var[p] : PV[npix];
    }
}

__global__ __launch_bounds__(256) void serial_check_count_kernel(const float *__restrict__ flags, uint32_t n,
                                                                 unsigned long long *__restrict__ count) {
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        c += flags[i] != 0.0f ? 1u : 0u;
    for (uint32_t off = kWave / 2; off > 0; off >>= 1) c += __shfl_xor(c, (int)off);
    if ((threadIdx.x & (kWave - 1u)) == 0 && c != 0) atomicAdd(count, (unsigned long long)c);
}

hipError_t launch_serial_check_count(const float *flags, uint32_t n, unsigned long long *count,
                                     hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint32_t want = (n + 255) / 256, blocks = want < 2048 ? want : 2048;
    hipLaunchKernelGGL(serial_check_count_kernel, dim3(blocks), dim3(256), 0, stream, flags, n, count);
    return hipGetLastError();
}

size_t serial_tab_doubles(uint32_t npix) { return 5 * (size_t)npix + 10; }

size_t serial_scan_scratch(uint32_t npix) { return 3 * (size_t)((npix + kScanTile - 1) / kScanTile) + 3; }

hipError_t launch_serial_moments(const float *est, uint32_t pix0, uint32_t n, uint32_t spp, uint32_t R,
                                 double scale, double *tab, uint32_t npix, hipStream_t stream) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(serial_moments_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, est, pix0, n, spp,
                       R, scale, tab, npix);
    return hipGetLastError();
}

hipError_t launch_serial_tables(double *tab, double *scratch, uint32_t npix, uint32_t spp, uint32_t L,
                                uint32_t n0, hipStream_t stream) {
    if (!npix) return hipSuccess;
    const uint32_t ntiles = (npix + kScanTile - 1) / kScanTile;
    hipLaunchKernelGGL(serial_scan_tiles_kernel, dim3(ntiles), dim3(256), 0, stream, tab, npix, spp, scratch);
    hipLaunchKernelGGL(serial_scan_totals_kernel, dim3(1), dim3(256), 0, stream, scratch, ntiles);
    hipLaunchKernelGGL(serial_scan_apply_kernel, dim3(ntiles), dim3(256), 0, stream, tab, npix, spp, scratch);
    const uint32_t N = npix * spp, q = L / 4u > 1u ? L / 4u : 1u;
    const uint64_t pts = ((uint64_t)N + q - 1) / q;
    hipLaunchKernelGGL(serial_reach_kernel, dim3((uint32_t)((pts + 255) / 256)), dim3(256), 0, stream, tab,
                       npix, spp, L, n0);
    return hipGetLastError();
}

hipError_t launch_serial_window(uint32_t *ctrl, const uint32_t *jump, uint32_t *win, uint32_t n,
                                SerialPred M, uint32_t *lo, uint32_t L, uint32_t K, uint32_t depth,
                                uint32_t nserial, uint32_t pix_spp, uint32_t pix_emax, uint32_t *counters,
                                uint32_t ncounters, uint4 *spix, uint32_t pix_chunk, const uint4 *spix_prev,
                                hipStream_t stream) {
    if (!n) return hipSuccess;
    const uint32_t threads = std::max((n + kWinPerThread - 1) / kWinPerThread, lo ? std::min(L, 1u << 16) : 0u);
    hipLaunchKernelGGL(serial_window_kernel, dim3((threads + 255) / 256), dim3(256), 0, stream, ctrl,
                       jump, win, n, M, lo, L, K, depth, nserial, pix_spp, pix_emax, counters,
                       counters ? ncounters : 0u, pix_spp != 0u ? spix : nullptr, pix_chunk,
                       pix_spp != 0u && spix != nullptr ? spix_prev : nullptr);
    return hipGetLastError();
}

// One workgroup per local pixel q of the iteration: the table entries of its
// reused range (spix[q].zw, serial_window_kernel) from the previous table.
// Entry e of pixel q is stream position plo(q) + e of this iteration's window,
// i.e. position plo(q) + e + D of the previous one, entry plo(q) + e + D -
// plo'(q') of its pixel's row there: b of a (pixel, stream position) pair is
// the same whichever iteration traced it.
__global__ __launch_bounds__(256) void serial_reuse_kernel(const uint32_t *__restrict__ ctrl,
                                                           const uint4 *__restrict__ spix,
                                                           const uint4 *__restrict__ spix_prev,
                                                           float *__restrict__ ptab,
                                                           const float *__restrict__ ptab_prev, uint32_t spp,
                                                           uint32_t L, uint32_t nserial) {
    if (ctrl[0] != 0u || ctrl[9] == 0u) return;
    const uint32_t a = ctrl[4];
    const uint32_t ln = min(L, nserial - a);
    const uint32_t p0 = a / spp, npq = (a + ln - 1u) / spp - p0 + 1u;
    const uint32_t q = blockIdx.x;
    if (q >= npq) return;
    const uint4 s = spix[q];
    if (s.z > s.w) return;
    const uint32_t E = ctrl[7], Ep = ctrl[11], D = ctrl[8];
    const uint4 so = spix_prev[p0 + q - ctrl[10] / spp];
    const uint32_t e1 = min(s.w, E - 1u);
    for (uint32_t e = s.z + threadIdx.x; e <= e1; e += blockDim.x)
        ptab[(size_t)q * E + e] = ptab_prev[(size_t)(p0 + q - ctrl[10] / spp) * Ep + (s.x + e + D - so.x)];
}

hipError_t launch_serial_reuse(const uint32_t *ctrl, const uint4 *spix, const uint4 *spix_prev, float *ptab,
                               const float *ptab_prev, uint32_t npq_max, uint32_t spp, uint32_t L,
                               uint32_t nserial, hipStream_t stream) {
    if (!npq_max) return hipSuccess;
    hipLaunchKernelGGL(serial_reuse_kernel, dim3(npq_max), dim3(256), 0, stream, ctrl, spix, spix_prev, ptab,
                       ptab_prev, spp, L, nserial);
    return hipGetLastError();
}

// table[jl * K + k] = b of sample jl at offset lo[jl] + k, i.e. at stream
// position 2 jl + 3 (lo[jl] + k) of the iteration, which the pixel table pass
// traced for the sample's pixel q at ptab[q * E + (position - plo(q))]
__global__ __launch_bounds__(256) void serial_pixtab_gather_kernel(const uint32_t *__restrict__ ctrl,
                                                                   const float *__restrict__ ptab,
                                                                   const uint32_t *__restrict__ lo,
                                                                   float *__restrict__ table, uint32_t L,
                                                                   uint32_t Kmax, uint32_t spp, uint32_t nserial) {
    if (ctrl[0] != 0u) return;
    const uint32_t K = serial_k(ctrl, Kmax);
    const uint32_t E = ctrl[7];
    const uint32_t a = ctrl[4];
    const uint32_t n = min(L, nserial - a);
    const uint32_t p0 = a / spp;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n * K; t += gridDim.x * blockDim.x) {
        const uint32_t jl = t / K, k = t - jl * K;
        const uint32_t q = (a + jl) / spp - p0;
        const uint32_t jf = q == 0u ? 0u : (p0 + q) * spp - a;
        const uint32_t plo = 2u * jf + 3u * lo[jf];
        const uint32_t pos = 2u * jl + 3u * (lo[jl] + k);
        // (lo is non-decreasing up to a rounding tie of the double prediction:
        // a position outside the traced span reads as "left the window")
        table[t] = (pos >= plo && pos - plo < E) ? ptab[(size_t)q * E + (pos - plo)] : -1.0f;
    }
}

hipError_t launch_serial_pixtab_gather(const uint32_t *ctrl, const float *ptab, const uint32_t *lo, float *table,
                                       uint32_t L, uint32_t K, uint32_t spp, uint32_t nserial, hipStream_t stream) {
    const uint64_t n = (uint64_t)L * K;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(serial_pixtab_gather_kernel, dim3(std::max(blocks, 1u)), dim3(256), 0, stream, ctrl, ptab,
                       lo, table, L, K, spp, nserial);
    return hipGetLastError();
}

uint32_t serial_super_words(uint32_t L, uint32_t K, uint32_t R) {
    const uint32_t nb = (L + R - 1) / R;
    return (nb + kSuperBlocks - 1) / kSuperBlocks * K;
}

uint32_t serial_walk_block(uint32_t L) {
    const uint32_t R = (L + 255) / 256;
    return R < 32u ? 32u : R;
}

hipError_t launch_serial_walk(uint32_t *ctrl, const float *table, SerialPred M, const double *V,
                              uint32_t npix, uint32_t spp, float z, float sfloor, const uint32_t *win,
                              uint32_t *states, uint32_t *bend, uint32_t *path, uint32_t *fin,
                              const uint32_t *lo, uint32_t *sbend, uint32_t *sB, uint32_t L, uint32_t Lw,
                              uint32_t K, uint32_t R, uint32_t depth, uint32_t nserial, const float *ptab,
                              uint32_t lds_rows, hipStream_t stream) {
    if (!L || !R) return hipSuccess;
    const uint32_t nb = (L + R - 1) / R;
    if (nb > kMaxWalkBlocks) return hipErrorInvalidValue;
    const uint64_t nt = (uint64_t)nb * K;
    const uint64_t nst = (uint64_t)((nb + kSuperBlocks - 1) / kSuperBlocks) * K;
    if (!fin) path = nullptr;
    // (the coalescing search and the pixel table need the recorded paths: the
    // finish kernel's lane-serial fallback reads a count table)
    if ((table == nullptr || ptab != nullptr) && !path) return hipErrorInvalidValue;
    const FastDiv ppix = make_fastdiv(spp ? spp : 1u);
    // the pixel table's walks from LDS rows (lds_rows bytes per workgroup)
    if (ptab != nullptr && lds_rows != 0) {
        if (R > kMaxWalkR) return hipErrorInvalidValue;
        hipLaunchKernelGGL(serial_walk_blocks_lds_kernel, dim3(nb), dim3(kWalkLdsThreads), lds_rows, stream, ctrl,
                           bend, path, lo, L, K, R, nserial, ptab, ppix);
    } else if (table != nullptr || ptab != nullptr) {
        hipLaunchKernelGGL(serial_walk_blocks_kernel, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, stream,
                           ctrl, table, M, bend, path, lo, L, K, R, depth, nserial, ptab, ppix);
    }
    const uint32_t ns = (nb + kSuperBlocks - 1) / kSuperBlocks;
    if ((size_t)kSuperBlocks * K * 4 <= kSuperLdsBytes)
        hipLaunchKernelGGL(serial_walk_super_lds_kernel, dim3(ns), dim3(1024), (size_t)kSuperBlocks * K * 4, stream,
                           ctrl, bend, lo, sbend, sB, L, K, R, nserial);
    else
        hipLaunchKernelGGL(serial_walk_super_kernel, dim3((uint32_t)((nst + 255) / 256)), dim3(256), 0, stream,
                           ctrl, bend, lo, sbend, sB, L, K, R, nserial);
    hipLaunchKernelGGL(serial_walk_finish_kernel, dim3(1), dim3(256), 0, stream, ctrl, table, M, V, npix,
                       spp ? spp : 1u, win, bend, path, states, path ? fin : nullptr, lo, sbend, sB, L, Lw, K,
                       R, depth, nserial, z, sfloor);
    if (path)
        hipLaunchKernelGGL(serial_states_kernel, dim3((L + 255) / 256), dim3(256), 0, stream, fin, path, win,
                           states, R);
    return hipGetLastError();
}

// ------------------------------------------------------------ primary sphere lists
// Device twin of bvh.cpp build_primary_sphere_lists (same double operations in
// the same order, -ffp-contract=off): per tree sphere, the box of its inflated
// ball projected through the inverse camera map to a pixel rectangle (rows
// counted from the bottom, common.rs:327), empty if behind the camera; flag
// bit 0: some ball straddles the camera plane or is not finite (every pixel
// walks).
struct SplConst { double Mi[9], o[3], e_abs, wden, hden; };
// an empty rectangle that every tile culls (lo above any pixel, hi below)
__device__ __forceinline__ int4 spl_empty() { return make_int4(0x7FFFFFFF, -1, 0x7FFFFFFF, -1); }

__global__ __launch_bounds__(256) void spl_rect_kernel(const float4 *__restrict__ prims, uint32_t n,
                                                       SplConst k, uint32_t W, uint32_t H,
                                                       int4 *__restrict__ rects, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 s = prims[i];
    const double c[3] = {s.x, s.y, s.z};
    const double r = sqrt((double)s.w) * (1 + 1e-6);
    const double a = sqrt((c[0] - k.o[0]) * (c[0] - k.o[0]) + (c[1] - k.o[1]) * (c[1] - k.o[1]) +
                          (c[2] - k.o[2]) * (c[2] - k.o[2]));
    const double R = r + 2 * 3e-3 * (a + r) * 1.01 + 2 * k.e_abs;
    int4 rect = spl_empty();
    if (!isfinite(R) || !isfinite(a)) {
        atomicOr(flag, 1u);
        rects[i] = rect;
        return;
    }
    double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
    int front = 0, behind = 0;
    for (int q = 0; q < 8; ++q) {
        const double P[3] = {c[0] + (q & 1 ? R : -R) - k.o[0], c[1] + (q & 2 ? R : -R) - k.o[1],
                             c[2] + (q & 4 ? R : -R) - k.o[2]};
        double w[3];
        for (int t = 0; t < 3; ++t) w[t] = k.Mi[3 * t] * P[0] + k.Mi[3 * t + 1] * P[1] + k.Mi[3 * t + 2] * P[2];
        const double wn = fabs(w[0]) + fabs(w[1]) + fabs(w[2]);
        if (w[2] > 1e-6 * wn) {
            ++front;
            umin = fmin(umin, w[0] / w[2]); umax = fmax(umax, w[0] / w[2]);
            vmin = fmin(vmin, w[1] / w[2]); vmax = fmax(vmax, w[1] / w[2]);
        } else if (w[2] < -1e-6 * wn) {
            ++behind;
        }
    }
    if (behind != 8 && front < 8) atomicOr(flag, 1u);  // straddles the camera plane
    if (front == 8) {
        const double cl = floor(umin * k.wden) - 2, ch = floor(umax * k.wden) + 1;
        const double rl = floor(vmin * k.hden) - 2, rh = floor(vmax * k.hden) + 1;
        if (!(ch < 0 || cl > (double)(W - 1) || rh < 0 || rl > (double)(H - 1)))
            rect = make_int4(cl < 0 ? 0 : (int)cl, ch > (double)(W - 1) ? (int)(W - 1) : (int)ch,
                             rl < 0 ? 0 : (int)rl, rh > (double)(H - 1) ? (int)(H - 1) : (int)rh);
    }
    rects[i] = rect;
}

// One thread per pixel of a 16 x 16 tile (record row 0 = the top image row):
// the first three tree spheres whose rectangle covers it, or "walk" past three
// (bvh.h PrimarySphereLists).  Rectangles are culled against the tile 256 at a
// time and compacted, in tree order, into LDS; a tile whose pixels have all
// overflowed stops early.
__global__ __launch_bounds__(256) void spl_fill_kernel(const int4 *__restrict__ rects, uint32_t n,
                                                       const uint32_t *__restrict__ flag, uint32_t W, uint32_t H,
                                                       uint2 *__restrict__ rec) {
    __shared__ int4 rl[256];
    __shared__ uint32_t ri[256];
    __shared__ uint32_t wc[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int col = (int)(blockIdx.x * 16 + (tid & 15u)), row = (int)(blockIdx.y * 16 + (tid >> 4));
    const bool on = col < (int)W && row < (int)H;
    const int rb = (int)H - 1 - row;  // counted from the bottom
    // the tile's extent: columns [tc0, tc1], bottom-counted rows [tr0, tr1]
    const int tc0 = (int)(blockIdx.x * 16), tc1 = min(tc0 + 15, (int)W - 1);
    const int tr1 = (int)H - 1 - (int)(blockIdx.y * 16), tr0 = max(tr1 - 15, 0);
    uint32_t cnt = flag[0] != 0u ? kSphListMaxDev + 1u : 0u, w0 = 0, w1 = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 256) {
        const uint32_t i = b0 + tid;
        int4 r = spl_empty();
        if (i < n) r = rects[i];
        const bool keep = r.x <= tc1 && r.y >= tc0 && r.z <= tr1 && r.w >= tr0;
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
        for (uint32_t j = 0; j < total && cnt <= kSphListMaxDev; ++j) {
            const int4 q = rl[j];
            if (col >= q.x && col <= q.y && rb >= q.z && rb <= q.w) {
                const uint32_t idx = ri[j];
                if (cnt == 0) w0 = idx;
                else if (cnt == 1) w0 |= idx << 16;
                else if (cnt == 2) w1 = idx;
                ++cnt;
            }
        }
        if (__syncthreads_and(!on || cnt > kSphListMaxDev)) break;
    }
    if (!on) return;
    const uint32_t c = cnt > kSphListMaxDev ? kSphListWalk : cnt;
    rec[(size_t)row * W + (uint32_t)col] = make_uint2(w0, (w1 & 0xFFFFu) | (c << 16));
}

hipError_t launch_sphere_lists(const float4 *prims, uint32_t n, const double *Mi, const double *o,
                               double e_abs, double wden, double hden, uint32_t width, uint32_t height,
                               int4 *rects, uint32_t *flag, uint2 *rec, hipStream_t stream) {
    SplConst k;
    for (int i = 0; i < 9; ++i) k.Mi[i] = Mi[i];
    for (int i = 0; i < 3; ++i) k.o[i] = o[i];
    k.e_abs = e_abs;
    k.wden = wden;
    k.hden = hden;
    hipError_t e = hipMemsetAsync(flag, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spl_rect_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, prims, n, k, width, height,
                       rects, flag);
    hipLaunchKernelGGL(spl_fill_kernel, dim3((width + 15) / 16, (height + 15) / 16), dim3(256), 0, stream, rects, n,
                       flag, width, height, rec);
    return hipGetLastError();
}

// Multi-device frames (multi.cpp render_frame_multi): rank g's tile holds
// the image rows of its row blocks (tile row k = image row tile_row(k)); the
// root's gather buffer holds nranks tiles of max_rows rows each.  One thread
// per RGBA8 word of the frame reads its word from its rank's tile: the frame
// is written once, coalesced, and the gathered tiles are read once.
__global__ __launch_bounds__(256) void assemble_kernel(const uint32_t *__restrict__ gathered,
                                                       uint32_t *__restrict__ out, uint32_t width,
                                                       uint32_t height, uint32_t row_block,
                                                       uint32_t nranks, uint32_t max_rows) {
    const uint64_t n = (uint64_t)width * height;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i / width), col = (uint32_t)(i - (uint64_t)row * width);
        const uint32_t b = row / row_block;
        const uint32_t g = b % nranks;
        const uint32_t k = (b / nranks) * row_block + row % row_block;
        out[i] = gathered[((uint64_t)g * max_rows + k) * width + col];
    }
}

hipError_t launch_assemble(const uint32_t *gathered, uint32_t *out, uint32_t width, uint32_t height,
                           uint32_t row_block, uint32_t nranks, uint32_t max_rows,
                           hipStream_t stream) {
    const uint64_t n = (uint64_t)width * height;
    if (!n) return hipSuccess;
    const uint64_t want = (n + 255) / 256, blocks = want < 256 * 64 ? want : 256 * 64;
    hipLaunchKernelGGL(assemble_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, gathered, out,
                       width, height, row_block ? row_block : 1, nranks ? nranks : 1, max_rows);
    return hipGetLastError();
}

}  // namespace rtamd
