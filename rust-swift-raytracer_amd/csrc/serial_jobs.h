// serial_jobs.h -- job -> pixel maps and the SERIAL passes' start states (render.h kRngSerial*).
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include "device_math.h"

namespace rtamd {
namespace {

// Job -> (sample, column, row): job = local pixel * spp + s (pixel-major);
// local rows map to image rows through the rank's row blocks (tiles.py);
// row counts from the bottom as ray_trace does (common.rs:327-331).
template <bool kSerial>
__device__ __forceinline__ void job_pixel(const TraceParams &p, uint32_t job, uint32_t &s,
                                          uint32_t &col, uint32_t &row) {
    if (kSerial && p.mode == kRngSerialPixel) {
        // job = local pixel q * E + position: pixel p0 + q (s is not used)
        const uint32_t pix = fdiv(p.cbase, p.div_sspp) + fdiv(job, p.div_spp);
        s = 0;
        row = fdiv(pix, p.div_width);
        col = pix - row * p.width;
        return;
    }
    if (kSerial) {
        // SERIAL passes: job = launch sample * V + variant; frame sample j =
        // (row * W + col) * spp + s in the reference's loop order (common.rs:327-336)
        const uint32_t jl = fdiv(job, p.div_spp);
        const uint32_t j = p.cbase + jl < p.nserial ? p.cbase + jl : p.nserial - 1u;
        const uint32_t pix = fdiv(j, p.div_sspp);
        s = j - pix * p.sspp;
        row = fdiv(pix, p.div_width);
        col = pix - row * p.width;
        return;
    }
    const uint32_t lp = fdiv(job, p.div_spp);
    s = job - lp * p.spp;
    const uint32_t q = fdiv(lp, p.div_width);
    col = lp - q * p.width;
    const uint32_t lr = p.slab_row0 + q;
    const uint32_t blk = fdiv(lr, p.div_rowblock);
    const uint32_t ir = (blk * p.nranks + p.rank) * p.row_block + (lr - blk * p.row_block);
    row = p.height - 1u - ir;
}

// kRngSerialPixel: the stream positions (window indices) local pixel q's
// samples' windows cover: from 2 jf + 3 lo(jf) to 2 jz + 3 (lo(jz) + K - 1),
// jf / jz its first / last sample in the iteration
__device__ __forceinline__ void serial_pixel_span(const TraceParams &p, uint32_t q, uint32_t &plo,
                                                  uint32_t &phi) {
    if (p.spix != nullptr) {  // tabulated by the window kernel: one load
        const uint4 s = p.spix[q];
        plo = s.x;
        phi = s.y;
        return;
    }
    const uint32_t a = p.cbase, ss = p.sspp;
    const uint32_t ln = min(p.sL, p.nserial - a);
    const uint32_t p0 = fdiv(a, p.div_sspp);
    const uint32_t jf = q == 0u ? 0u : (p0 + q) * ss - a;
    const uint32_t jz = min((p0 + q + 1u) * ss - a, ln) - 1u;
    plo = 2u * jf + 3u * p.slo[jf];
    phi = 2u * jz + 3u * (p.slo[jz] + p.sK - 1u);
}

// SERIAL passes: the start state of job (launch sample jl, variant k).
__device__ __forceinline__ uint32_t serial_start(const TraceParams &p, uint32_t job) {
    const uint32_t jl = fdiv(job, p.div_spp);
    const uint32_t k = job - jl * p.spp;
    if (p.mode == kRngSerialCount)
        return p.win[2u * jl + 3u * ((p.slo ? p.slo[jl]
                                            : serial_lo(p.sM, p.cbase, jl, p.spp, (p.max_draws - 2u) / 3u,
                                                        p.nserial)) + k)];
    if (p.mode == kRngSerialCheck) return p.win[p.cbase + jl];
    if (p.mode == kRngSerialPixel) {
        // local pixel q = jl, position plo(q) + k (kept inside the pixel's span:
        // the launch's E is the widest pixel's; jobs past a narrower pixel's
        // span are not traced, serial_pixel_job)
        uint32_t plo, phi;
        serial_pixel_span(p, jl, plo, phi);
        return p.win[min(plo + k, max(phi, plo))];
    }
    return counter_seed(p.seed, (uint64_t)(p.cbase + jl) * p.spp + k);
}

// kRngSerialPixel: false for a job past its pixel's span (the lane stays idle)
__device__ __forceinline__ bool serial_pixel_job(const TraceParams &p, uint32_t job) {
    const uint32_t q = fdiv(job, p.div_spp);
    uint32_t plo, phi;
    serial_pixel_span(p, q, plo, phi);
    return plo + (job - q * p.spp) <= phi;
}

}  // namespace
}  // namespace rtamd
