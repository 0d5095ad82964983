// serial_states.cpp -- RT_RNG_SERIAL: the search for every sample's start
// state in the reference's one stream (serial_find_states), and the frame
// rendered from them (render_frame_serial).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>

#include "runtime_internal.h"

namespace rtamd {

// ------------------------------------------------------------ SERIAL mode
// The reference draws every sample from one xorshift32 stream seeded 2547549
// (common.rs:321, random.rs:8-30): sample j (reference order (row * W + col)
// * spp + s) starts at stream position P_j = 2j + 3 B_j, where B_j counts the
// diffuse/metal scatters of all earlier samples (2 draws for u, v, 3 per
// random_unit_sphere).  That is a sequential dependency, resolved here on the
// device chunk by chunk:
//   1. estimate: each sample traced R times from counter seeds gives every
//      pixel's mean scatter count (kRngSerialEstimate);
//   2. per chunk of L samples, whose first sample's B is known exactly:
//      window: the stream states from that sample's start on (jump matrices);
//      count: every sample traced from K candidate positions centred on its
//        predicted offset (kRngSerialCount), a table of scatter counts;
//      walk: one lane follows the true path through the table, writing each
//        sample's start state and the next chunk's start state;
//      a walk that leaves its window cancels the remaining launches and the
//      host resumes from that chunk with a window twice as wide;
//   3. the frame is rendered in REPLAY mode from the start states.
// The result is the reference's own frame, bit for bit (tests/test_gpu_serial.py).
namespace {
uint32_t xorshift32(uint32_t x) {
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}

// columns of M^(2^i), i < 64, M the xorshift32 step as a GF(2) matrix
// xorshift32 jump matrices (GF(2), 32 columns each; render.h
// kSerialJumpWords): M^(2^i) for i < 64, then M^(w j) for j < 4096 / w (w =
// kSerialWinPerThread) and M^(4096 j) for j < 256 (serial_window_kernel: two
// applies reach any multiple of w below 2^20)
std::vector<uint32_t> xorshift_jump_table() {
    std::vector<uint32_t> t(kSerialJumpWords);
    for (uint32_t c = 0; c < 32; ++c) t[c] = xorshift32(1u << c);
    auto apply = [&](const uint32_t *cols, uint32_t x) {
        uint32_t y = 0;
        for (uint32_t c = 0; c < 32; ++c)
            if (x >> c & 1u) y ^= cols[c];
        return y;
    };
    for (int i = 1; i < 64; ++i)
        for (uint32_t c = 0; c < 32; ++c) t[32 * i + c] = apply(&t[32 * (i - 1)], t[32 * (i - 1) + c]);
    static_assert((kSerialWinPerThread & (kSerialWinPerThread - 1)) == 0, "a power of two");
    int wlog = 0;
    while ((1u << wlog) < kSerialWinPerThread) ++wlog;
    for (int lvl = 0; lvl < 2; ++lvl) {
        uint32_t *T = &t[(size_t)32 * (64 + (lvl ? kSerialJumpT1 : 0))];
        const uint32_t *step = &t[32 * (lvl == 0 ? wlog : 12)];  // M^w, M^4096
        const uint32_t cnt = lvl == 0 ? kSerialJumpT1 : 256u;
        for (uint32_t c = 0; c < 32; ++c) T[c] = 1u << c;  // M^0
        for (uint32_t j = 1; j < cnt; ++j)
            for (uint32_t c = 0; c < 32; ++c) T[32 * j + c] = apply(step, T[32 * (j - 1) + c]);
    }
    return t;
}
}  // namespace

// sigma floor of a sample's scatter count (the frame-wide K adds 0.05 to its
// sigma), scaled for the means' estimation error from `per` traces a pixel
static double serial_floor(uint64_t per) { return 0.05 * std::sqrt(1.0 + 1.0 / (double)per); }

int serial_check_args(size_t width, size_t height, const RtRenderOptions &o) {
    const uint64_t N = (uint64_t)width * height * (uint64_t)std::max(o.samples_per_pixel, 0);
    if (N >= 0xFFFFFFFFull) {
        set_error("RT_RNG_SERIAL: width * height * spp must be below 2^32");
        return -1;
    }
    if (o.max_ray_bounces > 100000) {
        set_error("RT_RNG_SERIAL: max_ray_bounces above 100000");
        return -1;
    }
    return 0;
}

// Steps 1 and 2 of SERIAL mode on device d, stream s: every sample's start
// state of the whole width x height frame into d->sstates (frame sample
// order), the events sev[0] (start), sev[2] (tables done) and sev[1] (states
// found) recorded on s; with RT_FLAG_SERIAL_CHECK the chain is checked after
// sev[1].  stats (optional) gets the serial_* fields.
int serial_find_states(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                       const RtRenderOptions &o, DeviceState *d, hipStream_t s, RtRenderStats *stats) {
    const uint64_t spp = (uint64_t)std::max(o.samples_per_pixel, 0);
    const uint64_t N = (uint64_t)width * height * spp;
    const uint32_t depth = (uint32_t)std::max(o.max_ray_bounces, 0);
    int rc = 0;
    HIP_TRY(d->done.wait(s));
    HIP_TRY(hipEventRecord(d->sev[0].get(), s));
    HIP_TRY(d->sstates.grow(std::max<uint64_t>(N, 1)));
    RtRenderOptions ob = o;
    // the inner passes read and write d's buffers (d->samples, d->stab, ...):
    // pin them to d's device rather than to whichever device is current
    ob.device = d->device;
    ob.ndevices = 0;
    ob.rng_mode = RT_RNG_COUNTER;
    ob.rank = 0;
    ob.nranks = 1;
    ob.flags = 0;
    uint32_t final_state = o.seed;  // the stream state after the last sample
    if (N > 0) {
        const auto tp0 = std::chrono::steady_clock::now();  // (RT_AMD_SERIAL_DEBUG)
        // 1. per-pixel mean scatter counts from R counter-seeded traces per
        // sample, reduced on the device (per-pixel moments, then prefix sums
        // over pixels): no per-sample table and no host pass over the samples
        // (RT_AMD_SERIAL_EST traces per pixel: the means' error adds to every
        // window's deviation, sweep on the 960x540x16 frames at z 1.5:
        // c_raytracer / RTOW / world.txt 32 -> 457 / 315 / - ms, 128 -> 418 /
        // 281 / 364, 256 -> 416 / 285 / 360, 512 -> 427 / 281 / -; z 1.2 and
        // 1.0 cost more at every EST, 1.8 and 2.1 as much or more)
        // (round 5, with the pixel table: x2 per x4 samples per pixel from 16 spp,
        // like the iteration length -- profiles/round5_serial/sweep_estimate_
        // traces*.jsonl: world.txt 960x540x16 64 / 96 / 128 / 192 -> 84.7 / 84.0 /
        // 83.2 / 84.2 ms; RTOW at C2 settings 128 / 192 / 256 / 320 / 384 -> 639 /
        // 604 / 591 / 588 / 594 ms)
        uint64_t est_def = 128;
        for (uint64_t q = 64; q <= spp; q *= 4) est_def *= 2;
        const uint64_t est = std::max<uint64_t>(1, env_u64("RT_AMD_SERIAL_EST", est_def));
        const uint64_t R = std::max<uint64_t>(
            1, std::min<uint64_t>({(est + spp - 1) / spp, 64, 0x7FFFFFFFull / N}));
        const uint64_t npix = (uint64_t)width * height;
        const double per = (double)(spp * R);
        // The coalescing block search (serial_coalesce_kernel) or the count
        // pass over every (sample, candidate) pair + block walks.  Coalescing
        // traces 0.33-0.45 of the count pass's traces but runs each block's
        // samples in sequence: it wins where a trace is short -- brute-force
        // scenes, i.e. no sphere or triangle tree (< 16 of each: render()'s
        // scenes; 960x540x16 c_raytracer 338 -> 308 ms, world.txt 301 -> 233
        // ms) -- and loses on tree walks (RTOW 238 -> 620 ms).
        // RT_AMD_SERIAL_COALESCE: 0 off, 1 on, unset: that rule.  The rule
        // keys on the scene's size (trees are built for >= 16 spheres or
        // triangles), not on o.accel: a large scene forced to RT_ACCEL_BRUTE
        // has even longer traces and takes the count pass too.
        const bool trees = d->nnodes > 0 || d->tnodes > 0;
        // The pixel table pass (round 4, the default from 4 samples per pixel):
        // a sample's scatter count depends only on its pixel and its start
        // position (the samples of one pixel trace the same camera ray from
        // the same draws), so the count table of an iteration is gathered from
        // one trace per (pixel, stream position) that any of the pixel's
        // samples' windows covers -- about L (3K / spp + 2 + 3 mu) traces
        // instead of the count pass's L K, and independent ones, unlike the
        // coalescing search's chains.  RT_AMD_SERIAL_PIXTAB=0: the searches below.
        bool pixtab = spp >= 4 && env_u64("RT_AMD_SERIAL_PIXTAB", 1) != 0;
        // the pixel pass's per-pixel spans (one load per refill, whole-chunk rows)
        const bool use_spix = env_u64("RT_AMD_SERIAL_SPIX", 1) != 0;
        // ... and an iteration's reuse of the previous one's table (the positions
        // both windows cover, after a stop: DESIGN.md 3.4); two tables, alternating
        const bool reuse = use_spix && env_u64("RT_AMD_SERIAL_REUSE", 1) != 0;
        const uint64_t pchunk = std::max<uint64_t>(1, env_u64("RT_AMD_SERIAL_PCHUNK", 128));
        bool coalesce = false;
        // (iterations of 128 k samples in blocks of 32 for the coalescing search,
        // profiles/round3_serial/coalesce_sweep*.log; 16 k for the count pass;
        // the pixel table: 32 k at 16 spp, x sqrt(spp / 16) in powers of two --
        // its traces per sample grow as K / spp ~ sqrt(L) / spp, its fixed cost
        // per iteration as 1 / L; profiles/round4_serial/pixtab_sweep*.log:
        // world.txt 960x540x16 16 k / 32 k / 64 k -> 141 / 114 / 121 ms, RTOW
        // 1920x1080x64 64 k / 128 k / 256 k -> 1.01 / 1.07 / 1.24 s)
        uint64_t L = 1, Lw = 1, n0 = 1;
        // the iteration length for the search chosen (planned again, without the
        // pixel table, when its table turns out too large below)
        auto plan = [&]() {
            coalesce = !pixtab && env_u64("RT_AMD_SERIAL_COALESCE", trees ? 0 : 1) != 0 && depth < 1024;
            uint64_t Ldef = coalesce ? 131072 : 16384;
            if (pixtab) {
                // (round 5, after the iterations' fixed cost fell from ~90 to ~54
                // us: 48 k at 16 spp, profiles/round5_serial/iteration_length_*.log:
                // world.txt 960x540x16 32 k / 48 k / 64 k / 96 k -> 92.5 / 91.3 /
                // 94.3 / 102.5 ms, 1920x1080x16 400 / 368 / 385 / 425 ms; RTOW
                // 1920x1080x64 64 k / 96 k / 128 k -> 732 / 683 / 689 ms)
                Ldef = 49152;
                for (uint64_t q = 64; q <= spp; q *= 4) Ldef *= 2;        // 64 spp: 96 k, 256 spp: 192 k
                for (uint64_t q = spp; q < 16 && Ldef > 8192; q *= 4) Ldef /= 2;  // 4 spp: 24 k
            }
            L = std::max<uint64_t>(1, std::min<uint64_t>(env_u64("RT_AMD_SERIAL_CHUNK", Ldef), N));
            // windows are sized for the deviation over Lw samples (default L; a
            // longer Lw widens them, a shorter iteration stops less often)
            Lw = std::max<uint64_t>(1, env_u64("RT_AMD_SERIAL_WLEN", L));
            n0 = std::min(N, Lw);
        };
        plan();
        HIP_TRY(d->stab.grow(serial_tab_doubles((uint32_t)npix)));
        HIP_TRY(d->sscan.grow(serial_scan_scratch((uint32_t)npix)));
        double *const sums = d->stab.get() + 5 * npix + 2;  // {sum ss, dmax, V(n0), lost count}
        HIP_TRY(hipMemsetAsync(sums, 0, 8 * sizeof(double), s));
        {
            // launches of whole pixels, <= 2^28 traces each
            const uint64_t step_pix = std::max<uint64_t>(1, ((1ull << 28) / R) / spp);
            for (uint64_t p0 = 0; p0 < npix; p0 += step_pix) {
                const uint64_t np = std::min(step_pix, npix - p0);
                const SerialPass sp{kRngSerialEstimate, (uint32_t)(p0 * spp), (uint32_t)(np * spp), (uint32_t)R,
                                    nullptr, SerialPred{}, nullptr};
                rc = render_frame(w, cam, width, height, ob, nullptr, s, nullptr, &sp);
                if (rc) return rc;
                HIP_TRY(launch_serial_moments(d->samples.get(), (uint32_t)p0, (uint32_t)np, (uint32_t)spp, (uint32_t)R,
                                              1.0 + 1.0 / per, d->stab.get(), (uint32_t)npix, s));
            }
        }
        const SerialPred pred{d->stab.get(), d->stab.get() + npix + 1, (uint32_t)spp, (uint32_t)npix};
        const double z = (double)env_u64("RT_AMD_SERIAL_Z10", 15) / 10.0;
        double dmax = 0.0;  // largest predicted offset within L + L/4 samples: the window
        uint64_t K = 0, npq_max = 0, emax = 0;
        double sm[4] = {0.0, 0.0, 0.0, 0.0};  // {sum ss, dmax bits, V(n0), lost-count flag}
        double sigma = 0.0;
        for (;;) {
            HIP_TRY(launch_serial_tables(d->stab.get(), d->sscan.get(), (uint32_t)npix, (uint32_t)spp, (uint32_t)L,
                                         (uint32_t)n0, s));
            HIP_TRY(hipEventRecord(d->sev[2].get(), s));
            HIP_TRY(hipMemcpyAsync(sm, sums, sizeof(sm), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (sm[3] != 0.0) {
                set_error("RT_RNG_SERIAL: estimate pass lost a sample's draw count");
                return -5;
            }
            {
                uint64_t bits;
                std::memcpy(&bits, &sm[1], 8);
                std::memcpy(&dmax, &bits, 8);
            }
            sigma = std::sqrt(std::max(sm[0], 0.0) / (double)(N * R)) + 0.05;
            // 2. iterations of L samples from the first unresolved one (ctrl[4]),
            // K candidates per sample, spanning +-z sigma of the deviation of the
            // true offset from the predicted one at the end of L samples.  Narrow
            // windows trade progress for work: an iteration resolves samples up
            // to where the path leaves a window, and the next one starts there
            // with its windows re-centred (no host round trip).
            // (tools/serial_sweep.sh on the c_raytracer, C1 and RTOW frames: L 2048
            // -> 103 / 9 / 126 ms, 4096 -> 71 / 7 / 85, 16384 -> 56 / 6 / 61, 65536 ->
            // 72 / 6 / 64; z 1.0 / 1.5 / 2.0 within 5 %: short iterations pay the
            // launch tail, long ones the sqrt(L) wider windows)
            const double spread = std::sqrt((double)Lw * (1.0 + 1.0 / (double)(spp * R)));
            K = (uint64_t)std::ceil(2.0 * z * sigma * spread) + 2 * (uint64_t)depth + 2;
            if (const uint64_t k = env_u64("RT_AMD_SERIAL_K", 0)) K = k;  // (tests: narrow windows)
            // sample a + 1's window must hold every b of sample a: K >= 2 depth + 2
            K = std::min<uint64_t>(std::max<uint64_t>(K, 2 * (uint64_t)depth + 2), (uint64_t)depth * L + 1);
            if (L * K > 0x7FFFFFFFull) {
                set_error("RT_RNG_SERIAL: candidate table too large");
                return -5;
            }
            // (the coalescing workgroup keeps K candidates' u16 slots and K + depth
            // + 1 live offsets in LDS, <= 64 KB: wider windows take the count pass)
            if (K > 4096 || serial_coalesce_search_lds((uint32_t)K, depth) > 64 * 1024) coalesce = false;
            // the pixel table's bounds (64-bit: no wrap before the checks): pixels an
            // iteration touches x the widest span of positions one pixel's windows cover
            npq_max = L / spp + 2;
            emax = pixtab ? serial_pixtab_emax64(spp, K, depth) : 0;
            // (rows padded to whole job chunks of the pixel pass: render_frame's chunk)
            if (pixtab && use_spix) emax = (emax + pchunk - 1) / pchunk * pchunk;
            if (!pixtab || (npq_max * emax <= (1ull << 28) && emax <= 0x7FFFFFFFull)) break;
            // too large: plan the iterations as without the pixel table (L, and
            // with it K and the reach; the coalescing search where the rule picks it)
            pixtab = false;
            plan();
            HIP_TRY(hipMemsetAsync(sums + 1, 0, sizeof(double), s));  // (the reach: atomicMax)
        }
        // the block walks read the pixel table directly (RT_AMD_SERIAL_PGATHER=1:
        // through a gathered L x K count table instead, the first build: 27 us per
        // iteration more at 32 k x 617)
        const bool pgather = pixtab && env_u64("RT_AMD_SERIAL_PGATHER", 0) != 0;
        if (pixtab) {
            HIP_TRY(d->sptab.grow(npq_max * emax));
            HIP_TRY(d->sspix.grow(2 * npq_max));
            if (reuse) HIP_TRY(d->sptab2.grow(npq_max * emax));
            if (pgather) HIP_TRY(d->samples.grow(L * K));
        }
        // The walks size each iteration's windows from the per-pixel variances
        // (V: prefix sums over pixels of spp var, then var; the variance of
        // samples [0, j) is PV[p] + (j - p spp) var[p]): 2 z (sqrt(V) + 0.05
        // sqrt(n scale)) + 2 depth + 2 for n samples -- the frame-wide K above
        // where every pixel has the frame's sigma, narrower over sky and other
        // constant-count pixels
        const bool adapt = env_u64("RT_AMD_SERIAL_ADAPT", 1) != 0;
        const double *Vdev = d->stab.get() + 2 * npix + 1;
        const uint64_t wlen = 2 * L + 3 * ((uint64_t)std::ceil(dmax) + K + (uint64_t)depth) + 8;
        if (wlen >= 0xFFFFFFFFull) {
            set_error("RT_RNG_SERIAL: candidate window too large");
            return -5;
        }
        // block length: the count pass's walks use serial_walk_block(L) (256
        // blocks); the coalescing search RT_AMD_SERIAL_R samples (default 32,
        // <= kMaxWalkBlocks blocks per iteration)
        // (the pixel table's walks: blocks of 64 samples up to 48 k-sample
        // iterations, then about 768 blocks per iteration -- 128 samples at 64
        // spp's 96 k: RTOW at C2 settings 665 -> 645 ms, world.txt unchanged)
        uint64_t walk_r_def = 64;
        while (walk_r_def < kMaxWalkR && L > walk_r_def * 768) walk_r_def *= 2;
        const uint64_t R_walk =
            coalesce ? std::min<uint64_t>(L, std::max<uint64_t>({env_u64("RT_AMD_SERIAL_R", 32), 1,
                                                                 (L + kMaxWalkBlocks - 1) / kMaxWalkBlocks}))
            : pixtab ? std::min<uint64_t>(L, std::max<uint64_t>({env_u64("RT_AMD_SERIAL_WALKR", walk_r_def), 1,
                                                                 (L + kMaxWalkBlocks - 1) / kMaxWalkBlocks}))
                     : serial_walk_block((uint32_t)L);
        // the pixel table's walks read each block's rows from LDS (as u8 counts:
        // depth < 255) when a block's pixels x the row stride fit the budget
        // (RT_AMD_SERIAL_WALK_LDS=0: the walks read the table in global memory)
        uint32_t walk_lds = 0;
        if (pixtab && !pgather && depth < 255 && R_walk <= kMaxWalkR &&
            env_u64("RT_AMD_SERIAL_WALK_LDS", 1) != 0) {
            const uint64_t maxpix = (R_walk - 1) / spp + 2;
            if (maxpix <= kWalkLdsMaxPix && maxpix * emax <= kWalkLdsRowBytes) walk_lds = (uint32_t)(maxpix * emax);
        }
        uint32_t K0 = 0;  // the first iteration's candidates (later ones: the walks)
        if (adapt) {
            const double w0 = 2.0 * z * (std::sqrt(std::max(sm[2], 0.0)) + serial_floor(spp * R) * std::sqrt((double)n0));
            K0 = (uint32_t)std::min<double>((double)K, std::ceil(w0) + 2.0 * depth + 2.0);
        }
        HIP_TRY(d->swin.grow(wlen));
        HIP_TRY(d->slo.grow(L));
        HIP_TRY(d->sbend.grow((L + R_walk - 1) / R_walk * K));
        HIP_TRY(d->ssb.grow((L + R_walk - 1) / R_walk * K));
        HIP_TRY(d->ssbend.grow(serial_super_words((uint32_t)L, (uint32_t)K, (uint32_t)R_walk)));
        // recorded block paths: the states of resolved samples become a gather
        // (the coalescing search has no count table to re-walk: always)
        const bool gather = coalesce || pixtab || env_u64("RT_AMD_SERIAL_GATHER", 1) != 0;
        if (gather) {
            HIP_TRY(d->spath.grow((L + R_walk - 1) / R_walk * R_walk * K));
            HIP_TRY(d->sfin.grow(kWalkFinWords));
        }
        if (!d->sjump) HIP_TRY(d->sjump.upload(xorshift_jump_table()));
        HIP_TRY(d->sctrl.grow(16));
        // Random::new() (random.rs:8-10); words 8-11: the previous iteration (reuse)
        const uint32_t ctrl0[16] = {0u, o.seed, 0u, 0u, 0u, K0, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        HIP_TRY(hipMemcpyAsync(d->sctrl.get(), ctrl0, 64, hipMemcpyHostToDevice, s));
        uint64_t iter_q = 0;  // iterations queued (table / span buffers alternate)
        // iterations are queued in batches sized by the expected progress;
        // those queued past the end exit at once (ctrl[0])
        uint32_t ctrl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        double t_enqueue = 0, t_wait = 0;  // (RT_AMD_SERIAL_DEBUG)
        DevEvent dbg_ev[2];
        DevBuf<unsigned long long> dbg_cnt;  // (coalescing search counters)
        if (env_u64("RT_AMD_SERIAL_DEBUG", 0)) {
            for (auto &e : dbg_ev) HIP_TRY(e.create(true));
            HIP_TRY(hipEventRecord(dbg_ev[0].get(), s));
            HIP_TRY(dbg_cnt.grow(4));
            HIP_TRY(hipMemsetAsync(dbg_cnt.get(), 0, 4 * 8, s));
        }
        const double t_prep = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count();
        uint64_t queued = 0;
        while (!ctrl[0]) {
            const uint64_t left = N - ctrl[4];
            const uint64_t it = std::max<uint64_t>(2, (uint64_t)std::ceil((double)left / (0.8 * (double)L)));
            if ((queued += it) > N + 64) {  // (every iteration resolves >= 1 sample)
                set_error("RT_RNG_SERIAL: start states not resolved");
                return -5;
            }
            const auto t0 = std::chrono::steady_clock::now();
            for (uint64_t q = 0; q < it; ++q, ++iter_q) {
                // this iteration's table and spans, and the previous iteration's
                // (reuse: the two alternate)
                const bool odd = reuse && (iter_q & 1u);
                float *const ptab = odd ? d->sptab2.get() : d->sptab.get();
                float *const ptab_prev = reuse ? (odd ? d->sptab.get() : d->sptab2.get()) : nullptr;
                uint4 *const spix = d->sspix.get() + (odd ? npq_max : 0);
                const uint4 *const spix_prev = reuse ? d->sspix.get() + (odd ? 0 : npq_max) : nullptr;
                // (the pixel table pass's job counters are zeroed by the window kernel)
                HIP_TRY(launch_serial_window(d->sctrl.get(), d->sjump.get(), d->swin.get(), (uint32_t)wlen, pred,
                                             d->slo.get(),
                                             (uint32_t)L, (uint32_t)K, depth, (uint32_t)N,
                                             pixtab ? (uint32_t)spp : 0u, (uint32_t)emax,
                                             pixtab ? d->counter.get() : nullptr, kPixtabParts,
                                             pixtab && use_spix ? spix : nullptr,
                                             (uint32_t)pchunk, spix_prev, s));
                if (pixtab) {
                    if (reuse)
                        HIP_TRY(launch_serial_reuse(d->sctrl.get(), spix, spix_prev, ptab, ptab_prev, (uint32_t)npq_max,
                                                    (uint32_t)spp, (uint32_t)L, (uint32_t)N, s));
                    SerialPass sp{kRngSerialPixel, 0u, (uint32_t)npq_max, (uint32_t)emax, d->swin.get(), pred,
                                  d->sctrl.get(), d->slo.get()};
                    sp.ptab = ptab;
                    sp.spix = use_spix ? spix : nullptr;
                    sp.L = (uint32_t)L;
                    sp.Kmax = (uint32_t)K;
                    rc = render_frame(w, cam, width, height, ob, nullptr, s, nullptr, &sp);
                    if (rc) return rc;
                    if (pgather)
                        HIP_TRY(launch_serial_pixtab_gather(d->sctrl.get(), ptab, d->slo.get(), d->samples.get(), (uint32_t)L,
                                                           (uint32_t)K, (uint32_t)spp, (uint32_t)N, s));
                } else {
                    SerialPass sp{coalesce ? kRngSerialCoalesce : kRngSerialCount, 0u, (uint32_t)L, (uint32_t)K,
                                  d->swin.get(), pred, d->sctrl.get(), d->slo.get()};
                    sp.path = d->spath.get();
                    sp.bend = d->sbend.get();
                    sp.R = (uint32_t)R_walk;
                    sp.dbg = dbg_cnt.get();
                    rc = render_frame(w, cam, width, height, ob, nullptr, s, nullptr, &sp);
                    if (rc) return rc;
                }
                HIP_TRY(launch_serial_walk(d->sctrl.get(),
                                           (coalesce || (pixtab && !pgather)) ? nullptr : d->samples.get(), pred,
                                           adapt ? Vdev : nullptr, (uint32_t)npix, (uint32_t)spp, (float)z,
                                           (float)serial_floor(spp * R), d->swin.get(), d->sstates.get(),
                                           d->sbend.get(), gather ? d->spath.get() : nullptr,
                                           gather ? d->sfin.get() : nullptr, d->slo.get(), d->ssbend.get(),
                                           d->ssb.get(), (uint32_t)L, (uint32_t)Lw, (uint32_t)K,
                                           (uint32_t)R_walk, depth, (uint32_t)N,
                                           (pixtab && !pgather) ? ptab : nullptr, walk_lds, s));
            }
            const auto t1 = std::chrono::steady_clock::now();
            HIP_TRY(hipMemcpyAsync(ctrl, d->sctrl.get(), 32, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const auto t2 = std::chrono::steady_clock::now();
            t_enqueue += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t_wait += std::chrono::duration<double, std::milli>(t2 - t1).count();
        }
        if (stats) {
            stats->serial_retries = ctrl[6];
            stats->serial_iterations = ctrl[3];
        }
        final_state = ctrl[1];
        if (dbg_ev[0]) {
            HIP_TRY(hipEventRecord(dbg_ev[1].get(), s));
            HIP_TRY(hipEventSynchronize(dbg_ev[1].get()));
            float a = 0, b = 0;
            HIP_TRY(hipEventElapsedTime(&a, d->sev[0].get(), dbg_ev[0].get()));
            HIP_TRY(hipEventElapsedTime(&b, dbg_ev[0].get(), dbg_ev[1].get()));
            std::fprintf(stderr, "serial debug: GPU estimate + tables %.1f ms, iterations %.1f ms\n", a, b);
            unsigned long long c[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpy(c, dbg_cnt.get(), sizeof(c), hipMemcpyDeviceToHost));
            if (coalesce && c[2])
                std::fprintf(stderr, "serial debug: coalesce %llu traces in %llu blocks (%.3f of the count pass's "
                             "%llu), %.1f trace passes per block\n", c[0], c[2], (double)c[0] / std::max(1.0, (double)c[3]),
                             c[3], (double)c[1] / (double)c[2]);
        }
        if (env_u64("RT_AMD_SERIAL_DEBUG", 0) && pixtab) {
            // the pixel table pass's idle jobs: per iteration every pixel's row is E
            // (the widest span) long, a pixel's own span ~ 2 (spp - 1) + 3 (K - 1) +
            // 3 (spp - 1) mu (its predicted scatters)
            std::vector<double> mu(npix);
            HIP_TRY(hipMemcpy(mu.data(), d->stab.get() + npix + 1, npix * sizeof(double), hipMemcpyDeviceToHost));
            const uint64_t npq = std::max<uint64_t>(1, L / spp);
            double used = 0, padded = 0;
            for (uint64_t q0 = 0; q0 < npix; q0 += npq) {
                double mx = 0, sum = 0;
                const uint64_t q1 = std::min(npix, q0 + npq);
                for (uint64_t q = q0; q < q1; ++q) {
                    const double sp = 2.0 * (spp - 1) + 3.0 * (K - 1) + 3.0 * (spp - 1) * mu[q] + 1;
                    mx = std::max(mx, sp);
                    sum += sp;
                }
                used += sum;
                padded += mx * (double)(q1 - q0);
            }
            std::fprintf(stderr, "serial debug: pixel table spans use %.3f of the npq x E jobs (K %llu)\n",
                         used / std::max(padded, 1.0), (unsigned long long)K);
        }
        if (env_u64("RT_AMD_SERIAL_DEBUG", 0)) {
            std::fprintf(stderr, "serial debug: %s N %llu L %llu R %llu K %llu sigma %.3f: %u iterations (%u "
                         "stopped short), %llu queued, estimate + tables %.1f ms, enqueue %.1f ms, wait %.1f ms\n",
                         pixtab ? "pixel table" : coalesce ? "coalesce" : "count", (unsigned long long)N,
                         (unsigned long long)L,
                         (unsigned long long)R_walk, (unsigned long long)K, sigma,
                         ctrl[3], ctrl[6], (unsigned long long)queued, t_prep, t_enqueue, t_wait);
        }
    }
    HIP_TRY(hipEventRecord(d->sev[1].get(), s));
    if (N > 0 && (o.flags & RT_FLAG_SERIAL_CHECK)) {
        // the chain the reference's one stream forms (common.rs:321-341):
        // sample 0 starts at the seed, sample j ends where j + 1 starts,
        // the last one where the search ended (ctrl[1])
        // the states the check traces: d->sstates, or (test hook) a scratch
        // copy with one state corrupted, so the check must see the links into
        // and out of that sample break while the frame still renders from the
        // states the search found
        const uint32_t *checked = d->sstates.get();
        DevBuf<uint32_t> broken;
        if (const char *brk = std::getenv("RT_AMD_SERIAL_BREAK")) {
            const uint64_t j = std::strtoull(brk, nullptr, 10);
            if (j < N) {
                HIP_TRY(broken.grow(N));
                HIP_TRY(hipMemcpyAsync(broken.get(), d->sstates.get(), N * 4, hipMemcpyDeviceToDevice, s));
                uint32_t x = 0;
                HIP_TRY(hipMemcpyAsync(&x, broken.get() + j, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                x = x == 1u ? 2u : 1u;
                HIP_TRY(hipMemcpyAsync(broken.get() + j, &x, 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipStreamSynchronize(s));
                checked = broken.get();
            }
        }
        uint32_t first = 0;
        HIP_TRY(hipMemcpyAsync(&first, checked, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(d->scheck.grow(1));
        HIP_TRY(hipMemsetAsync(d->scheck.get(), 0, 8, s));
        const uint64_t step = 1ull << 28;
        for (uint64_t c0 = 0; c0 < N; c0 += step) {
            const uint32_t n = (uint32_t)std::min(step, N - c0);
            const SerialPass sp{kRngSerialCheck, (uint32_t)c0, n, 1u, checked, SerialPred{}, nullptr};
            RtRenderOptions oc = ob;
            oc.seed = final_state;
            rc = render_frame(w, cam, width, height, oc, nullptr, s, nullptr, &sp);
            if (rc) return rc;
            HIP_TRY(launch_serial_check_count(d->samples.get(), n, d->scheck.get(), s));
        }
        unsigned long long breaks = 0;
        HIP_TRY(hipMemcpyAsync(&breaks, d->scheck.get(), 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (stats) {
            stats->serial_checked = N;
            stats->serial_chain_breaks = breaks + (first != o.seed ? 1u : 0u);
        }
    }
    return 0;
}

int render_frame_serial(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                        const RtRenderOptions &o, uint32_t *d_out, hipStream_t stream,
                        RtRenderStats *stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (width == 0 || height == 0) return 0;
    int rc = serial_check_args(width, height, o);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lock(w.mu);
    DeviceState *d = nullptr;
    rc = device_for(w, o.device, d);
    if (rc) return rc;
    hipStream_t s = stream ? stream : d->stream.get();
    rc = serial_find_states(w, cam, width, height, o, d, s, stats);
    if (rc) return rc;
    const uint64_t N = (uint64_t)width * height * (uint64_t)std::max(o.samples_per_pixel, 0);
    // 3. the frame (or rank's tile) from the start states
    RtRenderOptions orp = o;
    orp.rng_mode = RT_RNG_REPLAY;
    orp.replay_states = nullptr;
    RtRenderStats keep{};
    if (stats) keep = *stats;
    rc = render_frame(w, cam, width, height, orp, d_out, s, stats, nullptr, d->sstates.get());
    if (rc) return rc;
    if (stats) {
        stats->serial_retries = keep.serial_retries;
        stats->serial_iterations = keep.serial_iterations;
        stats->serial_checked = keep.serial_checked;
        stats->serial_chain_breaks = keep.serial_chain_breaks;
        float ms = 0.0f;
        HIP_TRY(hipEventSynchronize(d->sev[1].get()));
        HIP_TRY(hipEventElapsedTime(&ms, d->sev[0].get(), d->sev[1].get()));
        stats->serial_ms = ms;
        if (N > 0) {
            HIP_TRY(hipEventElapsedTime(&ms, d->sev[0].get(), d->sev[2].get()));
            stats->serial_setup_ms = ms;
        }
    }
    return 0;
}

}  // namespace rtamd
