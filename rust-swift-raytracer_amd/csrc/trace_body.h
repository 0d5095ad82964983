// trace_body.h -- the persistent trace loop every trace_kernel instance runs, with the workgroup
// and occupancy constants it was tuned with.
// Part of render.hip's translation unit (the only unit that compiles these kernels).
#pragma once

#include <type_traits>

#include "chunk_resolve.h"
#include "device_math.h"
#include "serial_jobs.h"
#include "sphere_search.h"
#include "tri_search.h"

namespace rtamd {
namespace {

// ------------------------------------------------------------ trace kernel
// kBvh: sphere search through the exact BVH (else brute force).  kLds: the
// tree is copied into the workgroup's LDS once (persistent grid), so every
// traversal step is a ds_read instead of an L2 round trip.  kStep: the BVH
// walks are cut into slices of p.steps nodes, so lanes that finish early are
// shaded and refilled while the wave's long walks continue (triangle scenes:
// walk lengths vary by 10-100x); without it a lane walks to the end in one
// iteration (cheaper per node: sphere-only scenes).
// 6 waves per SIMD = 80 VGPRs: 3 LDS workgroups of 512 per CU (A/B: 5 waves ->
// 2 workgroups costs ~6% at C2)
#ifndef RT_WAVES_PER_EU
#define RT_WAVES_PER_EU 6
#endif
// Waves per SIMD of the lean (uncounted) triangle-scene kernels.  A/B on C5:
// with 256-node walk slices 8 waves beat 6 (264 vs 272 ms; 7: 274), with
// 128- or 96-node slices 6 waves win again (242 / 240 vs 248 / 251 ms at 8).
// The counting variants use RT_WAVES_PER_EU; the host queries occupancy per
// variant (trace_occupancy).
#ifndef RT_WAVES_PER_EU_MESH
#define RT_WAVES_PER_EU_MESH 6
#endif
// LDS workgroup of the sphere-only kernel: 1024 threads, 2 per CU (8 waves
// per SIMD, RT_WAVES_PER_EU_SPHERES).  History (A/B, one process): round 1,
// 512 -> 6.77 ms, 768 -> 6.73, 896 -> 8.41, 1024 -> 7.78 (then the per-wave ray
// state thrashed the L1); round 2, 256 -> 7.90, 384 -> 6.15, 512 -> 5.42 = 768,
// and on the 8-rank tile 768 beat 512 by 3 %.  Round 4, after the kernarg
// reloads freed the SGPRs (profiles/round4_occ/ab_occ_*.log, rank_occ_*.log):
// 768 -> 1024 at 8 waves: C2 4.449 -> 4.444 ms, C3 66.86 -> 62.23 ms, C2 tiles
// of 2 / 8 ranks 2.389 -> 2.336 / 0.772 -> 0.781 ms, C3 8-rank tile 8.78 ->
// 8.33 ms; 896 (7 waves) -> one workgroup per CU, 6.0 ms.  The counting and
// SERIAL sphere variants keep 768 threads at RT_WAVES_PER_EU: at 8 waves their
// extra state spills VGPRs to scratch.
#ifndef RT_WAVES_PER_EU_SPHERES
#define RT_WAVES_PER_EU_SPHERES 8
#endif
#ifndef RT_LDS_BLOCK_SPHERES
#define RT_LDS_BLOCK_SPHERES 1024
#endif
// (the sphere kernels without the LDS tree, 256 threads: A/B 8 vs 6 waves,
// global-memory tree at C2 6.01 vs 5.99 ms, brute force 2.39 vs 2.32 ms)
#ifndef RT_WAVES_PER_EU_SPHERES_GLOBAL
#define RT_WAVES_PER_EU_SPHERES_GLOBAL 6
#endif
#ifndef RT_LDS_BLOCK_SPHERES_AUX
#define RT_LDS_BLOCK_SPHERES_AUX 768
#endif
// LDS workgroup of the triangle-scene kernels (A/B on C5: 256 -> 223 ms,
// 512 -> 221, 768 -> 225)
#ifndef RT_LDS_BLOCK_MESH
#define RT_LDS_BLOCK_MESH 512
#endif
// kMesh: the scene has triangles (else the whole Mesh::hit stage compiles
// away, which keeps the sphere-only kernel's register allocation small).
// kSerial: the SERIAL-mode passes (render.h kRngSerial*): jobs are (sample,
// variant) pairs and store scatter counts -- a separate instance, so the frame
// kernels carry none of its registers.
// kind: 0 lean frame kernel, 1 counting frame kernel, 2 SERIAL pass
// Waves per SIMD of the wide triangle walk (kMesh 3; 80 VGPRs at 6)
#ifndef RT_WAVES_PER_EU_WIDE
#define RT_WAVES_PER_EU_WIDE 6
#endif
#ifndef RT_LDS_BLOCK_WIDE
#define RT_LDS_BLOCK_WIDE 512
#endif
constexpr uint32_t trace_threads(bool lds, int mesh, int kind) {
    return !lds ? 256u : mesh == 3 ? (uint32_t)RT_LDS_BLOCK_WIDE : mesh ? (uint32_t)RT_LDS_BLOCK_MESH
                       : kind == 0 ? (uint32_t)RT_LDS_BLOCK_SPHERES : (uint32_t)RT_LDS_BLOCK_SPHERES_AUX;
}
constexpr int trace_waves_per_eu(bool lds, int mesh, int kind) {
    return kind != 0 ? RT_WAVES_PER_EU : mesh == 3 ? RT_WAVES_PER_EU_WIDE : mesh ? RT_WAVES_PER_EU_MESH
                       : lds ? RT_WAVES_PER_EU_SPHERES : RT_WAVES_PER_EU_SPHERES_GLOBAL;
}
// kCorner: the LDS tree is the corner-record image `corner` (sphere-only frame
// kernels, corner::trace_kernel below); every other instance is trace_kernel.
// kAccum: one pass of a progressive accumulation (accum::trace_kernel below):
// the refill's global job and the chunk resolve's fold read `tail`.
// The accumulation kernels' argument block: it begins with the TraceParams
// (kargs() re-reads them from offset 0; TraceParams itself gets no field, its
// offsets are those the frame kernels' kernarg loads were tuned with), then
// the corner image (nullptr for the other searches) and the tail (render.h
// TraceTail's fields for this kind).
struct AccumTail {
    float *sums;
    uint32_t n0, stride;
};
struct AccumParams {
    TraceParams p;
    const uint4 *image;
    AccumTail tail;
};
// kAdapt: one pass of an adaptive accumulation (adapt::trace_kernel below):
// the pass's pixels are those of a list (render.h TraceTail).  The refill maps
// the job's launch-local pixel through it, and so does the chunk resolve
// (resolve_chunk_adapt); nothing else changes.
struct AdaptTail {
    float *sums;
    float *sumsq;
    const uint32_t *list;
    uint32_t n0, stride;
};
struct AdaptParams {
    TraceParams p;
    const uint4 *image;
    AdaptTail tail;
};
// The kernel's argument block, or a prefix of it (TraceParams; AccumParams /
// AdaptParams for their tails), re-read from the kernarg segment through a
// pointer the compiler must treat as changed each time (see trace_body).
template <class Block>
__device__ __forceinline__ const Block &kernarg() {
#if defined(__HIP_DEVICE_COMPILE__)
    const __attribute__((address_space(4))) Block *kp =
        (const __attribute__((address_space(4))) Block *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const Block *)kp;
#else
    static const Block host_pass{};  // (the host pass only parses the callers)
    return host_pass;
#endif
}
// kDefer (the lean whole-walk corner kernel only): the corner walk records
// the leaves it enters, at most kDefer per lane, and the wave tests them in
// shared leaf passes (DESIGN.md 5.2 "deferred leaves"); 0: each lane tests a
// leaf where it enters it.
#ifndef RT_LEAF_DEFER_C
#define RT_LEAF_DEFER_C 2  // pending leaves per lane (2 or 3)
#endif
// (re-culling pending leaves by their stored t_near, an entry dropped at the
// flush when it exceeds the best_t of then: A/B slower, C2 +1.0 %)
constexpr int kLeafDeferC = RT_LEAF_DEFER_C;
static_assert(kLeafDeferC == 2 || kLeafDeferC == 3, "pending leaves per lane: 2 or 3");
// kPlain (the deferred-leaf kernel only): the launch satisfies render.h
// trace_plain_ok, so the loop's wave-uniform tests of launch constants are
// decided here, at compile time: COUNTER seeds, 32-bit global jobs, u and v
// through xdiv, primary sphere lists, gated walks, no ablation, the ring, a
// tree of more than one node, both dividers in their general form and
// plane-lane chunks only.  Each was an s_load -> s_waitcnt -> s_cmp ->
// s_cbranch chain per iteration with the alternative's code behind it
// (DESIGN.md 5.4 "scalar audit"; measured there and dropped: one copy of the
// resolve with the slot's chunk selected into scalars, C2 +0.6 %, C3 +0.4 %,
// and the refill's reads grouped under one wait, no change).  Values (depth,
// camera, bounds, chunk, counters) are still read through kargs().  Every
// test is written `kPlain || <the run-time test>`: the other instances
// compile to the code they were.  RT_PLAIN_STEPS (diagnostic builds, the
// per-step A/B): 1 the refill's tests, 2 the set-up, gate and ablation tests,
// 4 the resolve's.
// The instance's shading paths (DESIGN.md 5.1 "the shading block"; a frame asks
// for the instance only with depth >= 1, render.h TraceRequest), bits of the same macro: 8 a path ends in the
// shading block and nowhere else -- the depth test sits where ++bounce is and
// the sample store inside the block, so the set-up has no depth chain and the
// colour no default; 16 a shading lane is sky or sphere (kMesh == 0: no
// triangle can win), so the sphere's records have no defaults either; 32 the
// first big sphere's record and id are read together, unconditionally (both
// arrays hold an entry even when there is no big sphere); 64 the sample store
// takes the wave's base and a 32-bit byte offset per lane.
#ifndef RT_PLAIN_STEPS
#define RT_PLAIN_STEPS 127
#endif
// The plain instance's sample store (RT_PLAIN_STEPS 64): the ring holds
// 3 kTraceRing << ring_shift floats per wave, so a lane's byte offset into it
// fits 32 bits.  The three stores take the wave's one scalar base and a per-lane
// offset, the plane stride added per plane (three scalar bases cost 5 more SGPR
// spills in the instance).
__device__ __forceinline__ void store_planes(float *sbase, uint32_t pstride, uint32_t slot, float r, float g,
                                             float b) {
    char *const base = reinterpret_cast<char *>(sbase);
    const uint32_t pb = pstride << 2;
    const uint32_t off = slot << 2;
    *reinterpret_cast<float *>(base + (size_t)off) = r;
    *reinterpret_cast<float *>(base + (size_t)(off + pb)) = g;
    *reinterpret_cast<float *>(base + (size_t)(off + 2u * pb)) = b;
}
// One instance's configuration: every k... above by name.  trace_body takes a
// type Cfg derived from it whose constexpr default constructor sets the
// fields (each kernel entry point in render.hip spells one, field by field).
struct TraceConfig {
    bool bvh = false, lds = false, step = false;
    int mesh = 0;
    bool count = false, serial = false, corner = false, accum = false, adapt = false;
    int defer = 0;
    bool plain = false;
};
template <class Cfg>
__device__ __forceinline__ void trace_body(TraceParams p, const uint4 *corner) {
    constexpr TraceConfig kCfg = Cfg();
    constexpr bool kBvh = kCfg.bvh, kLds = kCfg.lds, kStep = kCfg.step, kCount = kCfg.count, kSerial = kCfg.serial;
    constexpr bool kCorner = kCfg.corner, kAccum = kCfg.accum, kAdapt = kCfg.adapt, kPlain = kCfg.plain;
    constexpr int kMesh = kCfg.mesh, kDefer = kCfg.defer;
    static_assert(!(kAccum && kAdapt), "an adaptive pass is an instance of its own");
    static_assert(!kPlain || (kDefer != 0 && !kCount), "the plain instance: the lean deferred-leaf kernel");
    constexpr bool kPlainRefill = kPlain && (RT_PLAIN_STEPS & 1) != 0;
    constexpr bool kPlainWalk = kPlain && (RT_PLAIN_STEPS & 2) != 0;
    constexpr bool kPlainResolve = kPlain && (RT_PLAIN_STEPS & 4) != 0;
    constexpr bool kPlainEnd = kPlain && (RT_PLAIN_STEPS & 8) != 0;
    constexpr bool kPlainShade = kPlain && (RT_PLAIN_STEPS & 16) != 0;
    constexpr bool kPlainBig = kPlain && (RT_PLAIN_STEPS & 32) != 0;
    constexpr bool kPlainStore = kPlain && kPlainResolve && (RT_PLAIN_STEPS & 64) != 0;
    static_assert(!kPlainShade || kCfg.mesh == 0, "two kinds of shading lane: the sphere-only kernels");
    constexpr bool kWaveGuard = kMesh < 2;  // (exactdiv.h; the mesh kernels keep the per-lane fallbacks)
#ifndef RT_COUNT_DEFER  // (diagnostic build: the counting corner instance with the deferred walk)
    static_assert(kDefer == 0 || (kCorner && !kCount && !kStep && !kSerial && kMesh == 0),
                  "deferred leaves: the lean whole-walk corner kernel");
#endif
    // SERIAL count passes: the walk of the previous pass set the first sample
    // and this iteration's candidates per sample (ctrl[5], <= the launch's K)
    if (kSerial && p.ctrl != nullptr) {
        if (p.ctrl[0] != 0u) return;
        p.cbase = p.ctrl[4];  // (the walks advance it)
        const uint32_t K = p.ctrl[5];
        if (p.mode == kRngSerialCount && K != 0u && K < p.spp) {
            // (chunks of whole samples stay whole samples, about as many jobs per atomic)
            if (p.chunk % p.spp == 0u) p.chunk = (p.chunk / K) * K;
            p.spp = K;
            p.div_spp = make_fastdiv(K);
            p.njobs = p.npix * K;
        }
        if (p.mode == kRngSerialPixel) {
            // this iteration's pixels and positions per pixel (the launch was
            // sized for their bounds): job = local pixel q * E + e
            p.sK = K != 0u && K < p.sK ? K : p.sK;  // (serial_k)
            const uint32_t E = min(p.ctrl[7], p.spp);
            const uint32_t ln = min(p.sL, p.nserial - p.cbase);
            const uint32_t p0 = fdiv(p.cbase, p.div_sspp);
            const uint32_t npq = E ? fdiv(p.cbase + ln - 1u, p.div_sspp) - p0 + 1u : 0u;
            p.spp = max(E, 1u);
            p.div_spp = make_fastdiv(p.spp);
            p.npix = npq;
            p.njobs = npq * E;
        }
    }
    // frames: zero the other job-counter set for the launch after this one
    // (stream order: it starts once this grid has finished)
    if (!kSerial && p.job_counter_next != nullptr && blockIdx.x == 0)
        for (uint32_t i = threadIdx.x; i < kMaxJobParts; i += blockDim.x) p.job_counter_next[32u * i] = 0u;
    const uint32_t lane = __lane_id();
    // Each section of the loop (ray setup, sphere walk, triangle setup and
    // walk, shading, the chunk resolve, the refill) re-reads the parameters it
    // needs from the kernarg segment (scalar loads through a pointer the
    // compiler must treat as changed each time) instead of holding all of
    // them in SGPRs across the whole loop: the lean C2 kernel spilled 92 SGPRs
    // to VGPR lanes (252 v_readlane / v_writelane in its code), the C5 kernel
    // 191 plus 13 VGPRs to scratch; now 7 and 0 (+3 VGPRs).  A/B in one
    // process (tools/ab.py, lean frames): C2 4.638 -> 4.451 ms, C3 69.61 ->
    // 66.86 ms, C5 175.1 -> 170.9 ms (profiles/round4_kargs/).
    // (SERIAL passes rewrite fields of their copy of p at entry -- cbase, spp,
    // the divider, njobs -- so they keep reading that copy)
    auto kargs = [&]() -> const TraceParams & {
        if (kSerial) return p;
        return kernarg<TraceParams>();
    };
    // (kAccum, kAdapt) the tail of the argument block, re-read the same way
    auto atail = []() -> const AccumTail & { return kernarg<AccumParams>().tail; };
    auto xtail = []() -> const AdaptTail & { return kernarg<AdaptParams>().tail; };
    extern __shared__ float4 lds[];
    BvhView view;
    const uint32_t sph_root = stage_tree<kLds, kCorner>(p, corner, lds, view);  // the sphere walk's first node
    // kMesh 3: the lane's stack of wide-node indices (u16, entry k at
    // tstack[k * blockDim.x]) after the sphere tree's LDS copy
    uint16_t *const tstack = reinterpret_cast<uint16_t *>(
                                 reinterpret_cast<char *>(lds) +
                                 (kLds ? (trace_tree_lds(p.nnodes, p.nprims, p.nsph_padded) + 15u) & ~(size_t)15u
                                       : 0u)) + threadIdx.x;
    uint32_t tsp = 0;  // (kMesh 3) entries on the stack

    F3 org = f3(0, 0, 0), dir = f3(0, 0, 0), inv = f3(0, 0, 0);
    float thr_r = 1.0f, thr_g = 1.0f, thr_b = 1.0f;  // ray_color's final_color
    uint32_t rng = 0, slot = ~0u, bounce = 0;  // slot ~0: no finished sample to count
    uint32_t nscat = 0;  // (kSerial) the sample's diffuse/metal scatters so far
    uint32_t spl0 = 0, spl1 = kSphListWalk << 16;  // the pixel's primary sphere list (p.spl)
    // lane state between loop iterations (see the bounce loop below)
    enum : uint32_t { kSetup = 0, kSph = 1, kTriInit = 2, kTri = 3, kShade = 4 };
    uint32_t phase = kSetup, node = 0, oct = 0;
    // Sphere-only kernels whose walk is not sliced read inv, oct and node only
    // inside the sphere walk, which starts and ends in one iteration: they are
    // derived there (not loop-carried, and not at all for rays that do not
    // walk).  Sliced walks resume at `node`, the triangle walks read inv.
    constexpr bool kWalkState = kMesh == 0 && !kStep;
    float best_t = 0.0f, tri_t = 0.0f, e = 0.0f;  // e: the triangle walk's margin rho
    int best_i = -1, tri_i = -1;
    bool active = false;
    uint32_t rays = 0, tri_in = 0, sph_tests = 0, node_tests = 0, tnode_tests = 0,
             tri_done = 0;
    // iteration mix (counting variant, lane 0's view; wave-uniform): loop
    // iterations, iterations that walked the sphere tree, active lanes summed
    // over all iterations and over the walking ones (RT_AMD_ITER_DEBUG)
    uint32_t it_all = 0, it_walk = 0, lanes_all = 0, lanes_walk = 0;
#ifdef RT_WALK_MIX
    // diagnostic build only (counting variant): per sphere walk, the walk
    // loop's iterations, those in which some lane tested a leaf, and the leaf
    // loop's sphere trips (each the longest-active lane's view)
    uint32_t wm_iters = 0, wm_leaf_iters = 0, wm_leaf_trips = 0, wm_walks = 0;
#endif

    uint32_t pool_next = 0, pool_end = 0;  // wave-uniform job pool
    // (kSerial pixel pass) jobs [gap_lo, gap_lo + gap_len) of the pool are not
    // handed out: the pool counts jobs without them (copied table entries)
    uint32_t gap_lo = ~0u, gap_len = 0;
    bool exhausted = false;

    // Where a finished sample goes: the slab (slot = job) or, with the fused
    // resolve, the wave's ring (slot = ring offset = (k << ring_shift) + job -
    // rbase[k] for the chunk in ring slot k).  All wave-uniform.
    const bool fused = kPlainResolve || p.ring != nullptr;
    const uint32_t wave_id = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / kWave) +
                                                            threadIdx.x / kWave);
    float *const sbase = fused ? p.ring + (size_t)wave_id * (3u * kTraceRing << p.ring_shift)
                               : p.samples;
    const uint32_t pstride = fused ? (kTraceRing << p.ring_shift) : p.njobs;
    uint32_t rfree = (1u << kTraceRing) - 1u;  // ring slots not holding a chunk
    uint32_t rbase[kTraceRing], rlen[kTraceRing], rleft[kTraceRing];  // chunk jobs, samples not done
#pragma unroll
    for (uint32_t k = 0; k < kTraceRing; ++k) rbase[k] = rlen[k] = rleft[k] = 0;
    uint32_t cur_off = 0;  // slot - job for the pool's chunk
    // a lane's job from its slot (tri_primary_list needs the pixel)
    auto lane_job = [&](uint32_t sl) -> uint32_t {
        if (!fused) return sl;
        const uint32_t k = sl >> p.ring_shift;
        uint32_t b = rbase[0];
#pragma unroll
        for (uint32_t i = 1; i < kTraceRing; ++i) b = k == i ? rbase[i] : b;
        return b + (sl & ((1u << p.ring_shift) - 1u));
    };

#ifdef RT_WAVE_TIMES
    // diagnostic build only: per-wave timeline on the 100 MHz constant clock
    // (start, last chunk pulled, queue found empty, exit; tools/tail_probe.py)
    const uint64_t wt_start = __builtin_amdgcn_s_memrealtime();
    uint64_t wt_pull = wt_start, wt_exh = wt_start;
    uint32_t wt_jobs_tail = 0;  // jobs claimed in the wave's last chunk
#endif
#ifdef RT_STAMPS
    // diagnostic build only: wave cycles per loop segment (s_memtime deltas):
    // 0 direction normalisation + loop back, 1 ray setup, 2 walks, 3 shading,
    // 4 sample store, 5 fused resolve, 6 refill, 7 (unused)
    uint64_t stamp_acc[kStampSegs] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t stamp_prev = __builtin_amdgcn_s_memtime();
#define RT_STAMP(k)                                                       \
    do {                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();                 \
        __builtin_amdgcn_sched_barrier(0);                                \
        stamp_acc[k] += t_ - stamp_prev;                                  \
        stamp_prev = t_;                                                  \
    } while (0)
#else
#define RT_STAMP(k) \
    do {            \
    } while (0)
#endif
    // Job queue: the launch's jobs are split into p.nparts equal partitions,
    // each with its own counter on its own 128-B line (one shared counter
    // serialises at ~12 ns per atomic: 6 ms per C2 frame).  A wave starts on
    // its home partition and moves on when that one is drained.
    uint32_t part = (blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) % p.nparts;
    uint32_t tries = 0;  // partitions found drained (wave-uniform)
    // (pixel-aligned, so every chunk holds whole pixels: the fused resolve)
    auto part_begin = [&](uint32_t k) -> uint32_t {
        return (uint32_t)(((uint64_t)k * p.npix) / p.nparts) * p.spp;
    };
    uint32_t pbegin = part_begin(part), pend = part_begin(part + 1);
    uint32_t prefetch = 0;          // lane 0: counter value of the next chunk, fetched early
    bool prefetch_pending = false;  // wave-uniform
    for (;;) {
        // Directions that need NVec3::new (maths.rs:111-118) this iteration: the
        // scattered rays' and the new primary rays' share one normalisation.
        F3 vdir = dir;
        bool renorm = false;
        bool done = false;
        bool walked = false;  // (kCount: the iteration mix)
        const uint32_t nact = kCount ? (uint32_t)__popcll(__ballot(active)) : 0u;
        if (active) {
            // ---- ray_color's bounce loop (common.rs:267-282) as a lane state
            // machine: setup -> sphere walk -> triangle walk -> shade.  The walks
            // advance at most p.steps nodes per loop iteration, so lanes whose
            // search ends early are shaded and refilled while the others walk on.
            float out_r = 0.0f, out_g = 0.0f, out_b = 0.0f;
            if (phase == kSetup) {
                const TraceParams &p = kargs();  // (ray setup: see kargs)
                // (kPlainEnd: a path that reaches the depth ends where ++bounce was, below)
                if (!kPlainEnd && (int32_t)bounce >= p.depth) {
                    done = true;  // depth exhausted -> (0, 0, 0) (common.rs:284)
                } else {
                    ++rays;
                    // slab-test reciprocals only (not reference arithmetic): v_rcp_f32's
                    // 1-ulp error moves a slab face by <= 4u|b - lo|, inside e_abs and
                    // rho.  Clamped to +-1e20 (+-0 -> +-1e20, sign kept)
                    // so slab products stay finite: an axis with |d| < 1e-20 gets its
                    // t values scaled by 1e20|d| < 1, which keeps its interval's sign
                    // pattern -- the ray lies inside that (inflated) slab for any
                    // finite hit, and the scaled interval still spans [0, >1e9].
                    // (kWalkState: derived at the sphere walk instead, see there)
                    if (!kWalkState) {
                        inv = f3(slab_rcp(dir.x), slab_rcp(dir.y), slab_rcp(dir.z));
                        oct = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
                    }
                    // World::hit, spheres in order with shrinking t_max (common.rs:241-247)
                    best_t = __builtin_inff();
                    best_i = -1;
                    if (kBvh) {
                        spheres_big<kWaveGuard, kPlainBig>(p, org, dir, best_t, best_i);
                        if (!kWalkState)
                            node = kCorner ? sphere_corner_entry(sph_root, oct, kPlainWalk ? 2u : p.nnodes)
                                           : sphere_walk_entry<kLds>(sph_root, oct, p.nnodes);
                        // (RT_AMD_ABLATE=1: timing-only diagnostic, results are wrong)
                        phase = (!kPlainWalk && (p.ablate & 1u)) ? kTriInit : kSph;
                        if (!kMesh && bounce == 0 && (spl1 >> 16) != kSphListWalk) {
                            // primary ray: the pixel's candidate spheres instead of
                            // the walk (bvh.h PrimarySphereLists; same candidate
                            // arithmetic and (t, index) argmin as sphere_leaf)
                            const uint32_t nc = spl1 >> 16;
                            sph_tests += nc;
                            if (nc > 0) sphere_candidate<kWaveGuard>(view.prims[spl0 & 0xFFFFu], org, dir,
                                                         (int)view.ids[spl0 & 0xFFFFu], best_t, best_i);
                            if (nc > 1) sphere_candidate<kWaveGuard>(view.prims[spl0 >> 16], org, dir,
                                                         (int)view.ids[spl0 >> 16], best_t, best_i);
                            if (nc > 2) sphere_candidate<kWaveGuard>(view.prims[spl1 & 0xFFFFu], org, dir,
                                                         (int)view.ids[spl1 & 0xFFFFu], best_t, best_i);
                            phase = kTriInit;
                        }
                    } else {
                        spheres_brute<kWaveGuard>(p, org, dir, best_t, best_i);
                        phase = kTriInit;
                    }
                }
            }
            RT_STAMP(1);
            // kStep: at most p.steps node visits per lane per iteration
            uint32_t budget = p.steps;
            // walk_min (sphere-only scenes): while fewer than walk_min lanes wait
            // for a walk and other lanes can advance without one (fresh samples
            // whose primary sphere list replaced the walk), skip this
            // iteration's walk: those lanes are shaded now and join the next
            // walk, so fewer walk segments run with lanes idle in them
            bool walk_now = true;
            if (!kMesh && (kPlainWalk || p.walk_min != 0)) {
                const uint32_t nwalk = (uint32_t)__popcll(__ballot(phase == kSph));
                const uint32_t nother = (uint32_t)__popcll(__ballot(phase != kSph && !done));
                walk_now = nwalk >= p.walk_min || nother == 0;
            }
            if (kBvh && phase == kSph && walk_now) {
                const TraceParams &p = kargs();  // (see kargs)
                walked = true;
                constexpr uint32_t kEnd = kLds ? 0xFFFFu : kNodeEndDev;
                const SphBound bnd = sph_bound(p, org);
                if (kWalkState) {
                    // the walk's own inputs, with its other per-ray values: an
                    // unsliced walk ends in this iteration, so they are derived
                    // once per walking ray and never for a ray whose primary
                    // sphere list replaces the walk (the clamp and the sign
                    // rule of the ray setup above, the same operations)
                    inv = f3(slab_rcp(dir.x), slab_rcp(dir.y), slab_rcp(dir.z));
                    oct = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
                    node = kCorner ? sphere_corner_entry(sph_root, oct, kPlainWalk ? 2u : p.nnodes)
                                   : sphere_walk_entry<kLds>(sph_root, oct, p.nnodes);
                }
                if (kCorner) {
                    // corner records: the same nodes in the same order with the
                    // same skip decisions (sphere_node_corner), fewer VALU per node
                    F3 nn, nf;
                    sphere_corner_slabs(org, inv, sph_inflation(p, bnd, best_t), oct, nn, nf);
                    const uint32_t offn = sph_root + 16u * oct, offf = sph_root + 112u - 16u * oct;
                    if constexpr (kDefer != 0) {  // (constexpr: kDefer - 1 below is a shift count)
                        // Deferred leaves: a lane that enters a leaf records it
                        // and walks on; the walking lanes test their recorded
                        // leaves together once one of them holds kDefer, and
                        // the whole wave tests what is left when no lane can
                        // step (a lane whose walk ended keeps its entries until
                        // then).  `pend` holds the upper halves of the leaves'
                        // link words (kCornerLeaf | leaf word) in 16-bit fields,
                        // the latest lowest; 0 = no entry.
                        typedef typename std::conditional<(kDefer > 2), uint64_t, uint32_t>::type Pend;
                        Pend pend = 0;
                        // every lane's r-th entry in one pass
                        auto flush = [&]() {
#pragma unroll
                            for (int r = 0; r < kDefer; ++r) {
                                const uint32_t ent = (uint32_t)(pend >> 16 * r) & 0xFFFFu;
                                if (ent != 0u)
                                    sphere_leaf<kWaveGuard, true>(view, org, dir, ent & 0x7FFFu, best_t, best_i,
                                                             sph_tests);
                            }
                            pend = 0;
                        };
                        do {
                            uint32_t leaf, lw;
                            float tn;
                            bool any_leaf;
                            const bool lf = sphere_node_corner(offn, offf, inv, best_t, nn, nf, node, leaf,
                                                               node_tests, tn, lw, any_leaf);
                            // (both branches wave-uniform, on masks the compares
                            // produce: a trip in which no lane enters a leaf runs
                            // the immediate walk's VALU)
                            if (any_leaf) {
                                if (lf) pend = pend << 16 | (lw >> 16);
                                if (__builtin_amdgcn_ballot_w64((pend >> 16 * (kDefer - 1)) != 0) != 0) flush();
                            }
                        } while (node != 0xFFFFu);
                        flush();
                    } else
                    do {
                        uint32_t leaf;
                        if (sphere_node_corner(offn, offf, inv, best_t, nn, nf, node, leaf, node_tests))
                            sphere_leaf<kWaveGuard, true>(view, org, dir, leaf, best_t, best_i, sph_tests);
                    } while (node != 0xFFFFu && (!kStep || --budget != 0));
                } else {
                    F3 nlo, nhi;
                    sphere_slabs(org, inv, sph_inflation(p, bnd, best_t), nlo, nhi);
                    const uint32_t ooff = kLds ? 4u * oct : oct;
#ifdef RT_WALK_MIX
                    uint32_t wi = 0, wl = 0, wt = 0;
#endif
                    do {
                        uint32_t leaf;
                        const bool lf = sphere_node<kLds>(view, inv, ooff, best_t, nlo, nhi, node, leaf, node_tests);
#ifdef RT_WALK_MIX
                        if (kCount) {
                            ++wi;
                            const bool any1 = __ballot(lf) != 0;
                            const bool any2 = __ballot(lf && (leaf & 7u) >= 2u) != 0;
                            wl += any1 ? 1u : 0u;
                            wt += any2 ? 2u : any1 ? 1u : 0u;
                        }
#endif
                        if (lf) sphere_leaf<kWaveGuard, kLds>(view, org, dir, leaf, best_t, best_i, sph_tests);
                    } while (node != kEnd && (!kStep || --budget != 0));
#ifdef RT_WALK_MIX
                    if (kCount) {
                        // (wave maxima over the walking lanes: the longest-active lane saw every iteration)
                        for (uint32_t off = 1; off < kWave; off <<= 1) {
                            wi = max(wi, (uint32_t)__shfl_xor((int)wi, (int)off));
                            wl = max(wl, (uint32_t)__shfl_xor((int)wl, (int)off));
                            wt = max(wt, (uint32_t)__shfl_xor((int)wt, (int)off));
                        }
                        wm_iters += wi;
                        wm_leaf_iters += wl;
                        wm_leaf_trips += wt;
                        wm_walks += 1u;
                    }
#endif
                }
                if (node == kEnd) phase = kTriInit;
            }
            if (phase == kTriInit) {
                const TraceParams &p = kargs();  // (see kargs)
                // Mesh::hit with t_max = best_t, own closest from +inf (common.rs:178-223)
                tri_t = __builtin_inff();
                tri_i = -1;
                phase = kShade;
                if (kMesh == 0) {
                    // no triangles: Mesh::hit finds nothing
                } else if (kMesh >= 2) {  // (p.tnodes != 0)
                    // (kMesh 3: every lane walks the static tree's wide image)
                    const bool cam = kMesh == 2 && bounce == 0 && p.cam_nnodes != 0;
                    if (tri_begin(p, org, dir, best_t, cam, e, tri_t, tri_i, tri_in, tri_done)) {
                        // (the lists index the camera-origin records, which exist
                        // without the camera tree's nodes: primary_lists.cpp prepare_camera)
                        if (kAdapt && bounce == 0 && p.ptl_off != nullptr) {
                            tri_primary_list_adapt(p, xtail().list, lane_job(slot), org, dir, best_t, tri_t, tri_i,
                                                   tri_in, tri_done);
                        } else if (bounce == 0 && p.ptl_off != nullptr) {
                            tri_primary_list<kSerial>(p, lane_job(slot), org, dir, best_t, tri_t, tri_i, tri_in,
                                             tri_done);
                        } else {
                            node = 0;
                            tsp = 0;
                            phase = kTri;
                        }
                    }
                } else {
                    triangles_brute(p, org, dir, best_t, tri_t, tri_i, tri_in);
                }
            }
            bool tri_now = true;
            if (kMesh >= 2 && p.tri_walk_min != 0) {
                const uint32_t nwalk = (uint32_t)__popcll(__ballot(phase == kTri));
                const uint32_t nother = (uint32_t)__popcll(__ballot(phase != kTri && !done));
                tri_now = nwalk >= p.tri_walk_min || nother == 0;
            }
            if (kMesh == 2 && phase == kTri && tri_now) {
                const TraceParams &p = kargs();  // (see kargs)
                if (kStep) budget = max(budget, p.steps / 2u);  // a lane that just left the sphere walk
                const bool cam = bounce == 0 && p.cam_nnodes != 0;
                const F3 dlt2 = f3(2.0f * (org.x - p.tbvh_oc[0]), 2.0f * (org.y - p.tbvh_oc[1]),
                                   2.0f * (org.z - p.tbvh_oc[2]));
                // rho (e; 0 on the camera tree) folded into the slab offsets
                F3 nlo, nhi;
                sphere_slabs(org, inv, e, nlo, nhi);
                float cap = fminf(best_t, tri_t);
                do {
                    uint32_t leaf;
                    if (tri_node(p, nlo, nhi, inv, dlt2, cam, cap, node, leaf, tnode_tests)) {
                        tri_leaf(p, org, dir, cam, leaf, best_t, tri_t, tri_i, tri_in, tri_done);
                        cap = fminf(best_t, tri_t);
                    }
                } while (node != kNodeEndDev && (!kStep || --budget != 0));
                if (node == kNodeEndDev) phase = kShade;
            }
            if (kMesh == 3 && phase == kTri && tri_now) {
                // The static tree's 4-wide image: one 128-B record per step
                // holds four children's boxes (one round trip where the binary
                // walk takes about four; tools/tbvh_sim.cpp SIM_WIDE=4: 584 ->
                // 146 dependent node loads per secondary ray, the same box
                // tests).  Leaf children are tested at once; of the internal
                // children that are entered, the nearest is walked next and the
                // others are pushed on the lane's LDS stack (A/B on C5 against
                // the lowest slot next: 151.0 -> 150.5 ms).  Any order is exact
                // (tri_merge keeps the (t, index) argmin).
                const TraceParams &p = kargs();  // (see kargs)
                uint32_t wbudget = p.wsteps;
                // Per-origin-cell trees (RT_AMD_TRI_CELLS, off by default): the
                // tree whose phantoms were built for the centre of the cell the
                // origin lies in (the static tree, tc_ncells, outside every cell).
                // The origin does not change during the walk, so every slice
                // picks the same tree.  Any tree is exact for any origin: the
                // widening below covers o - oc (bvh.h TriangleCells).
                F3 oc = f3(p.tbvh_oc[0], p.tbvh_oc[1], p.tbvh_oc[2]);
                uint32_t tree = 0;  // (one register across the walk: the bases follow from it)
                if (p.tc_ncells != 0u) {
                    const float fx = floorf((org.x - p.tc_lo[0]) * p.tc_inv_size);
                    const float fy = floorf((org.y - p.tc_lo[1]) * p.tc_inv_size);
                    const float fz = floorf((org.z - p.tc_lo[2]) * p.tc_inv_size);
                    tree = p.tc_ncells;
                    if (fx >= 0.0f && fx < (float)p.tc_n[0] && fy >= 0.0f && fy < (float)p.tc_n[1] && fz >= 0.0f &&
                        fz < (float)p.tc_n[2]) {
                        tree = ((uint32_t)fz * p.tc_n[1] + (uint32_t)fy) * p.tc_n[0] + (uint32_t)fx;
                        // (bvh.cpp build_triangle_cells' centre, the same operations)
                        oc = f3(p.tc_lo[0] + (fx + 0.5f) * p.tc_size, p.tc_lo[1] + (fy + 0.5f) * p.tc_size,
                                p.tc_lo[2] + (fz + 0.5f) * p.tc_size);
                    }
                }
                const F3 dlt2 = f3(2.0f * (org.x - oc.x), 2.0f * (org.y - oc.y), 2.0f * (org.z - oc.z));
                F3 nlo, nhi;
                sphere_slabs(org, inv, e, nlo, nhi);
                // (the grid base folded in: tri_wide_child)
                nlo = f3(__builtin_fmaf(p.tq_base[0], inv.x, nlo.x), __builtin_fmaf(p.tq_base[1], inv.y, nlo.y),
                         __builtin_fmaf(p.tq_base[2], inv.z, nlo.z));
                nhi = f3(__builtin_fmaf(p.tq_base[0], inv.x, nhi.x), __builtin_fmaf(p.tq_base[1], inv.y, nhi.y),
                         __builtin_fmaf(p.tq_base[2], inv.z, nhi.z));
                float cap = fminf(best_t, tri_t);
                do {
                    const uint4 *wn = p.tw_nodes + 8u * (tree * p.tw_stride + node);
                    tnode_tests += 4;
                    float tn[4];
                    bool in[4];
                    // two halves: the first brings the 128-B line into the L1,
                    // the second (after a compiler barrier, so that the node
                    // never occupies 28 VGPRs at once) hits it there
                    {
                        const uint4 q0 = wn[0], q1 = wn[1], q2 = wn[2];
                        in[0] = tri_wide_child(p, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, nlo, nhi, inv, dlt2, cap, tn[0]);
                        in[1] = tri_wide_child(p, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, nlo, nhi, inv, dlt2, cap, tn[1]);
                    }
                    asm volatile("" ::: "memory");
                    {
                        const uint4 q3 = wn[3], q4 = wn[4], q5 = wn[5];
                        in[2] = tri_wide_child(p, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, nlo, nhi, inv, dlt2, cap, tn[2]);
                        in[3] = tri_wide_child(p, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, nlo, nhi, inv, dlt2, cap, tn[3]);
                    }
                    const uint4 qa = wn[6];
                    const uint32_t a[4] = {qa.x, qa.y, qa.z, qa.w};
                    // entered leaf children, one copy of the leaf test for all four
                    uint32_t lmask = 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) lmask |= (in[c] && (a[c] & kLeafBitDev)) ? 1u << c : 0u;
                    while (lmask != 0) {
                        const uint32_t c = (uint32_t)__builtin_ctz(lmask);
                        lmask &= lmask - 1u;
                        const uint32_t lw = c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3];
                        tri_leaf(p, org, dir, false, lw & ~kLeafBitDev, best_t, tri_t, tri_i, tri_in, tri_done,
                                 p.tw_tris);
                    }
                    cap = fminf(best_t, tri_t);
                    uint32_t nxt = 0xFFFFu;
                    float ntn = 0.0f;
#pragma unroll
                    for (int c = 3; c >= 0; --c) {
                        if (in[c] && !(a[c] & kLeafBitDev) && __float_as_int(tn[c]) <= __float_as_int(cap)) {
                            if (nxt != 0xFFFFu) {
                                // the nearer one next, the other on the stack
                                const bool closer = tn[c] < ntn;
                                tstack[tsp * blockDim.x] = (uint16_t)(closer ? nxt : a[c]);
                                ++tsp;
                                if (closer) { nxt = a[c]; ntn = tn[c]; }
                            } else {
                                nxt = a[c];
                                ntn = tn[c];
                            }
                        }
                    }
                    if (nxt == 0xFFFFu && tsp != 0) {
                        --tsp;
                        nxt = tstack[tsp * blockDim.x];
                    }
                    node = nxt;
                } while (node != 0xFFFFu && (!kStep || --wbudget != 0));
                if (node == 0xFFFFu) phase = kShade;
            }
            RT_STAMP(2);
            if (phase == kShade) {
                const TraceParams &p = kargs();  // (see kargs)
                phase = kSetup;
                // One NVec3::new for both kinds of lane that need one here: a
                // missed ray re-normalises its direction (common.rs:277), a
                // sphere hit normalises (pos - c) / r (common.rs:95), so the
                // wave runs one copy of the sqrt / divide sequence, not two
                // (kPlainShade: no triangle wins, a lane is sky or sphere; the
                // sphere's values are then set on every path that reads them
                // and get no default)
                const bool sky = kPlainShade ? best_i < 0 : tri_i < 0 && best_i < 0;
                const bool sph = kPlainShade ? !sky : tri_i < 0 && best_i >= 0;
                F3 un = dir, spos;
                float4 SS, SM;
                uint32_t skind;
                if (!kPlainShade) {
                    spos = dir;
                    SS = SM = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    skind = 0;
                }
                if (sph) {
                    // one round trip: centre/radius, colour/param and kind together
                    SS = view.shade[2 * best_i];
                    SM = view.shade[2 * best_i + 1];
                    skind = view.kinds[best_i];
                    // (kPlainShade: the hit point replaces the origin here.  A
                    // sphere lane either scatters from it or ends, and a lane
                    // that ended reads no origin before its refill sets one)
                    if (kPlainShade) spos = org = org + scale(dir, best_t);
                    else spos = org + scale(dir, best_t);
                    un = divide_by<kWaveGuard>(spos - f3(SS.x, SS.y, SS.z), SS.w);
                }
                if (kPlainShade || sky || sph) un = unit<kWaveGuard>(un);
                if (sky) {
                    // background (common.rs:276-281): re-normalise, lerp to sky blue
                    const float t = 0.5f * (un.y + 1.0f);
                    const float w = 1.0f - t;
                    out_r = thr_r * (1.0f * w + 0.5f * t);
                    out_g = thr_g * (1.0f * w + 0.7f * t);
                    out_b = thr_b * (1.0f * w + 1.0f * t);
                    done = true;
                } else {
                    F3 pos, nrm;
                    uint32_t kind;
                    float cr, cg, cb, param;
                    if (!kPlainShade && tri_i >= 0) {  // a triangle wins a tie against a sphere
                        pos = org + scale(dir, tri_t);
                        const float4 *g = p.tri_geo + 4u * (uint32_t)tri_i;
                        const float4 A = g[0], Nn = g[3];
                        nrm = f3(Nn.x, Nn.y, Nn.z);
                        const float *m = p.mats + 8u * __float_as_uint(A.w);
                        kind = __float_as_uint(m[0]);
                        cr = m[1]; cg = m[2]; cb = m[3]; param = m[4];
                    } else {
                        kind = skind;
                        pos = kPlainShade ? org : spos;
                        nrm = un;  // common.rs:95, normalised above
                        cr = SM.x; cg = SM.y; cb = SM.z; param = SM.w;
                    }
                    // Each scatter builds an un-normalised direction `v`; the draws
                    // of diffuse and metal (random_unit_sphere, common.rs:32-38) and
                    // the final normalisation are shared code so divergent lanes do
                    // not execute three copies of the divide/sqrt sequences.
                    bool next = true, keep_normal = false;
                    F3 v = nrm;
                    if (kind == kMatDiffuse || kind == kMatMetal) {
                        const F3 ru = draw_unit<kWaveGuard>(rng);
                        if (kSerial) ++nscat;
                        if (kind == kMatDiffuse) {  // materials.rs:42-52
                            v = nrm + ru;
                            const float eps = 1e-8f;
                            keep_normal = fabsf(v.x) < eps && fabsf(v.y) < eps && fabsf(v.z) < eps;
                        } else {  // materials.rs:54-63 (reflect, maths.rs:26-28)
                            const F3 refl = dir - scale(nrm, 2.0f * dot(dir, nrm));
                            v = refl + scale(ru, param);
                            next = dot(v, nrm) >= 0.0f;
                        }
                    } else if (kind == kMatDielectric) {  // materials.rs:65-97
                        F3 n2 = nrm;
                        float eta = param;
                        if (dot(dir, nrm) >= 0.0f) { n2 = -nrm; eta = 1.0f / param; }
                        const float cos_t = dot(-dir, n2);  // maths.rs:31-36
                        const F3 perp = scale(dir + scale(n2, cos_t), eta);
                        const F3 par = scale(n2, -xsqrt<kWaveGuard>(fabsf(1.0f - dot(perp, perp))));
                        v = perp + par;
                        cr = cg = cb = 1.0f;
                    } else {  // Emission (materials.rs:100-102)
                        next = false;
                    }
                    // (kPlainEnd: the scattered ray would be bounce + 1, which the
                    // set-up's depth test turned into (0, 0, 0), common.rs:284)
                    if (next && !(kPlainEnd && (int32_t)(bounce + 1u) >= p.depth)) {
                        thr_r = thr_r * cr;
                        thr_g = thr_g * cg;
                        thr_b = thr_b * cb;
                        org = pos;
                        if (keep_normal) {
                            dir = nrm;
                        } else {
                            vdir = v;  // normalised below, with the new rays' directions
                            renorm = true;
                        }
                        ++bounce;
                    } else {
                        if (!kPlainEnd || !next) {  // common.rs:273-274: final * colour
                            out_r = thr_r * cr;
                            out_g = thr_g * cg;
                            out_b = thr_b * cb;
                        }
                        done = true;
                    }
                }
                if constexpr (kPlainEnd) {
                    // every path ends here: the store of below, inside the block
                    if (done) {
                        if constexpr (kPlainStore) {
                            store_planes(sbase, pstride, slot, out_r, out_g, out_b);
                        } else {
                            sbase[slot] = out_r;
                            sbase[pstride + slot] = out_g;
                            sbase[2 * pstride + slot] = out_b;
                        }
                        active = false;
                    }
                }
            }
            RT_STAMP(3);
            if (!kPlainEnd && done) {
                if (kSerial && p.mode == kRngSerialCheck) {
                    // the chain check: this sample's end state must be the next
                    // sample's start state (one variant: slot = launch sample)
                    const uint32_t j = p.cbase + slot;
                    out_r = rng == (j + 1u < p.nserial ? p.win[j + 1u] : p.seed) ? 0.0f : 1.0f;
                } else if (kSerial) {
                    // SERIAL passes: the sample's scatter count b instead of its
                    // colour -- it drew 2 + 3b numbers (common.rs:335-336 and one
                    // random_unit_sphere per diffuse/metal scatter, common.rs:32-38),
                    // counted as they were drawn
                    out_r = (float)nscat;
                }
                // planar (R, G, B planes): 12 B per sample, to the slab or the
                // ring (SERIAL passes: plane 0 only)
                if constexpr (kPlainStore) {
                    store_planes(sbase, pstride, slot, out_r, out_g, out_b);
                } else {
                    sbase[slot] = out_r;
                    if (!kSerial) {
                        sbase[pstride + slot] = out_g;
                        sbase[2 * pstride + slot] = out_b;
                    }
                }
                active = false;
            }
        }
        RT_STAMP(4);
        if (kCount && nact != 0) {  // (wave-uniform: every lane counts the same)
            const bool wk = __ballot(walked) != 0;
            ++it_all;
            lanes_all += nact;
            it_walk += wk ? 1u : 0u;
            lanes_walk += wk ? nact : 0u;
        }
        const uint64_t dead = __ballot(!active);
        const uint32_t ndead = (uint32_t)__popcll(dead);
        const bool refill = dead != 0 && (ndead >= p.refill_min || ndead == kWave);
        // ---- fused resolve, at refill points: lanes that finished since the
        // last one (slot != ~0) are counted against their chunk's ring slot; a
        // chunk with no samples left is summed now, by this wave, while its
        // samples are still in the cache.  (Every lane is idle in the last
        // iteration, so every chunk is resolved before the wave exits.)
        if (fused && refill) {
            const bool fin = !active && slot != ~0u;
            if (__ballot(fin) != 0) {
                const uint32_t lk = slot >> p.ring_shift;
                // (measured and dropped, DESIGN.md 5.4: the first finished lane's
                // slot read with v_readlane and the other slots passed by on a
                // scalar compare when no finished lane has another, C2 +2.4 %)
#pragma unroll
                for (uint32_t k = 0; k < kTraceRing; ++k) {
                    if (rfree & (1u << k)) continue;
                    const uint32_t n = (uint32_t)__popcll(__ballot(fin && lk == k));
                    rleft[k] -= n;
                    if (n != 0 && rleft[k] == 0) {
                        const TraceParams &pc = kargs();
                        if (kAdapt) {
                            const AdaptTail &t = xtail();
                            resolve_chunk_adapt<RT_PLANE_LANES(kMesh)>(pc, sbase, pstride, k << pc.ring_shift,
                                                                       rbase[k], rlen[k], lane, t.sums, t.sumsq,
                                                                       t.list);
                        } else if (kAccum)
                            resolve_chunk<RT_PLANE_LANES(kMesh), true>(pc, sbase, pstride, k << pc.ring_shift,
                                                                       rbase[k], rlen[k], lane, atail().sums);
                        else if (kPlainResolve)
                            resolve_chunk<true, false, true>(pc, sbase, pstride, k << pc.ring_shift, rbase[k],
                                                             rlen[k], lane);
                        else if (!(pc.ablate & 2u))
                            resolve_chunk<RT_PLANE_LANES(kMesh)>(pc, sbase, pstride, k << pc.ring_shift, rbase[k],
                                                  rlen[k], lane);
                        rfree |= 1u << k;
                    }
                }
                if (fin) slot = ~0u;
            }
        }
        RT_STAMP(5);
        // ---- refill lanes whose path ended (active-ray compaction) -------
        // (with the fused resolve a new chunk needs a free ring slot: with all
        // kTraceRing slots waiting on unfinished samples the lanes stay idle)
        if (refill && !exhausted && !(fused && rfree == 0 && pool_next >= pool_end)) {
            const TraceParams &pc = kargs();  // (the refill's parameters: see kargs)
            // (a wave-uniform loop only in the pixel table pass, which skips
            // chunks that hold no position of its pixel's span)
            while (pool_next >= pool_end) {
                uint32_t base = 0;
                if (lane == 0) {
                    base = pbegin + (prefetch_pending ? prefetch
                                                      : atomicAdd(pc.job_counter + 32u * part, pc.chunk));
                    while (base >= pend && ++tries < pc.nparts) {
                        part = part + 1 == pc.nparts ? 0 : part + 1;
                        pbegin = part_begin(part);
                        pend = part_begin(part + 1);
                        base = pbegin + atomicAdd(pc.job_counter + 32u * part, pc.chunk);
                    }
                }
                prefetch_pending = false;
                base = __builtin_amdgcn_readfirstlane(base);
                part = __builtin_amdgcn_readfirstlane(part);
                tries = __builtin_amdgcn_readfirstlane(tries);
                pbegin = __builtin_amdgcn_readfirstlane(pbegin);
                pend = __builtin_amdgcn_readfirstlane(pend);
                if (base >= pend) {
                    exhausted = true;
#ifdef RT_WAVE_TIMES
                    wt_exh = __builtin_amdgcn_s_memrealtime();
#endif
                    break;
                } else {
                    pool_next = base;
                    pool_end = min(base + pc.chunk, pend);
                    if (kSerial && pc.mode == kRngSerialPixel && pc.spix != nullptr) {
                        // pixel rows are padded to whole chunks (the row stride E
                        // is a multiple of the chunk: serial_window_kernel), so a
                        // chunk lies in one pixel's row: hand out only its
                        // positions inside the pixel's span (the rest would leave
                        // lanes idle, serial_pixel_job) and skip chunks past it
                        const uint32_t q = fdiv(base, pc.div_spp);
                        const uint4 sq = uniform_load_u4(pc.spix, q);
                        const uint32_t rowb = q * pc.spp;
                        const uint32_t live_end = rowb + (sq.y >= sq.x ? sq.y - sq.x + 1u : 0u);
                        pool_end = min(pool_end, live_end);
                        // the positions the previous iteration traced were copied
                        // (serial_reuse_kernel): the pool skips them
                        gap_lo = ~0u;
                        gap_len = 0;
                        if (sq.z <= sq.w && pool_next < pool_end) {
                            const uint32_t g0 = max(rowb + sq.z, pool_next);
                            const uint32_t g1 = min(rowb + sq.w + 1u, pool_end);
                            if (g0 < g1) {
                                gap_lo = g0;
                                gap_len = g1 - g0;
                                pool_end -= gap_len;
                            }
                        }
                        if (pool_next >= pool_end) continue;
                    }
#ifdef RT_WAVE_TIMES
                    wt_pull = __builtin_amdgcn_s_memrealtime();
                    wt_jobs_tail = pool_end - pool_next;
#endif
                    if (fused) {
                        const uint32_t k = (uint32_t)__builtin_ctz(rfree);
                        rfree &= ~(1u << k);
#pragma unroll
                        for (uint32_t i = 0; i < kTraceRing; ++i)
                            if (i == k) rbase[i] = base, rlen[i] = rleft[i] = pool_end - base;
                        cur_off = (k << pc.ring_shift) - base;
                    }
                }
                if (!kSerial) break;  // (frames: one pass, as the plain `if` it replaces)
            }
            // (the pixel pass's skipped chunks may leave pool_end below pool_next)
            const uint32_t avail = kSerial && exhausted ? 0u : pool_end - pool_next;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
                (uint32_t)(dead >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dead, 0u));
            if (!active && rank < avail) {
                uint32_t job = pool_next + rank;
                if (kSerial && job >= gap_lo) job += gap_len;
                // Jobs are enumerated pixel-major (job = pixel*spp + s): the
                // lanes refilled together trace samples of one pixel (or of
                // neighbours), so their primary walks visit the same nodes
                // (A/B: C2 trace -5.5 %, C5 -5 % against sample-major), and
                // they store to consecutive slab slots.  Seeds and replay
                // states use the reference's job index below, so the
                // enumeration order changes no bits.
                uint32_t s, col, row;
                uint64_t gjob = 0;
                if (kAdapt) {
                    // the pass's pixel lp is frame pixel list[lp] (top row first);
                    // its job as in an accumulation pass
                    const AdaptTail &t = xtail();
                    const uint32_t lp = fdiv(job, pc.div_spp);
                    const uint32_t idx = t.list[lp];
                    const uint32_t q = fdiv(idx, pc.div_width);
                    s = job - lp * pc.spp;
                    col = idx - q * pc.width;
                    row = pc.height - 1u - q;
                    const uint32_t pix = row * pc.width + col;
                    if (pc.gj32) gjob = pix * t.stride + (t.n0 + s);  // (W H S < 2^32)
                    else gjob = (uint64_t)pix * t.stride + (t.n0 + s);
                } else if (kAccum) {
                    // sample N0 + s of the pixel, its job at the accumulator's
                    // sample stride (whole frames of one rank: tile row = image row)
                    const AccumTail &t = atail();
                    const uint32_t lp = fdiv(job, pc.div_spp);
                    const uint32_t q = fdiv(lp, pc.div_width);
                    s = job - lp * pc.spp;
                    col = lp - q * pc.width;
                    row = pc.height - 1u - (pc.slab_row0 + q);
                    const uint32_t pix = row * pc.width + col;
                    if (pc.gj32) gjob = pix * t.stride + (t.n0 + s);  // (W H S < 2^32)
                    else gjob = (uint64_t)pix * t.stride + (t.n0 + s);
                } else if (!kSerial && (kPlainRefill || pc.gj32)) {
                    // one rank, 32-bit global jobs (TraceParams::gj32)
                    const uint32_t lp = fdiv<kPlainRefill>(job, pc.div_spp);
                    const uint32_t q = fdiv<kPlainRefill>(lp, pc.div_width);
                    col = lp - q * pc.width;
                    row = pc.height - 1u - (pc.slab_row0 + q);
                    gjob = job + pc.gj_c0 - q * pc.gj_2p;
                } else {
                    job_pixel<kSerial>(pc, job, s, col, row);
                    gjob = ((uint64_t)row * pc.width + col) * pc.spp + s;
                }
                slot = job + cur_off;
                bool take = true;
                if (kSerial) {
                    nscat = 0;
                    rng = serial_start(pc, job);
                    if (pc.mode == kRngSerialPixel) take = serial_pixel_job(pc, job);
                } else {
                    rng = (!kPlainRefill && pc.mode == kRngReplay) ? pc.replay[gjob] : counter_seed(pc.seed, gjob);
                }
                // common.rs:335-337: u drawn before v; camera.rs:84-89
                // numerators are in [2^-32, 2^24]: exactdiv.h with the host's
                // reciprocals whenever the denominators are in range
                const float un = draw_plus(rng, (float)col);
                const float vn = draw_plus(rng, (float)row);
#ifndef RT_NO_XDIV
                const bool xd = kPlainRefill || pc.xdiv_uv != 0;
#else
                const bool xd = false;
#endif
                const float u = xd ? xdiv(un, pc.wden, pc.wrcp) : un / pc.wden;
                const float v = xd ? xdiv(vn, pc.hden, pc.hrcp) : vn / pc.hden;
                const F3 h = f3(pc.cam[6], pc.cam[7], pc.cam[8]);
                const F3 vv = f3(pc.cam[9], pc.cam[10], pc.cam[11]);
                org = f3(pc.cam[0], pc.cam[1], pc.cam[2]);
                const F3 llc = f3(pc.cam[3], pc.cam[4], pc.cam[5]);
                vdir = ((llc + scale(h, u)) + scale(vv, v)) - org;  // normalised below
                renorm = true;
                if (kBvh && !kMesh && (kPlainRefill || pc.spl != nullptr)) {
                    // issued after the seed's (replay) load, so nothing waits on it
                    // before the ray's setup in the next iteration
                    if (!kPlainRefill && (pc.ablate & 4u)) {  // timing-only diagnostic: no record load
                        spl0 = 0;
                        spl1 = 0;
                    } else {
                        // (32-bit index: a frame's pixel count fits)
                        const uint2 r = pc.spl[(pc.height - 1u - row) * pc.width + col];
                        spl0 = r.x;
                        spl1 = r.y;
                    }
                }
                thr_r = thr_g = thr_b = 1.0f;
                bounce = 0;
                phase = kSetup;
                active = take;
            }
            pool_next += min(ndead, avail);
            // ask for the next chunk now; the reply is only waited for when the
            // pool runs dry (hides the ~1-3 us atomic round trip)
            if (!exhausted && !prefetch_pending && pool_end - pool_next < kWave) {
                if (lane == 0) prefetch = atomicAdd(p.job_counter + 32u * part, p.chunk);
                prefetch_pending = true;
            }
        }
        RT_STAMP(6);
        if (renorm) dir = unit<kWaveGuard>(vdir);
        RT_STAMP(0);
        if (__ballot(active) == 0 && exhausted) break;
    }

    // ---- per-wave statistics (stats requested only): each wave adds its
    // counters to its own 16-slot record, no atomics -- 6144 waves' atomics on
    // the same six words serialised at the end of every launch (~0.4 ms, most
    // of a multi-GPU tile's overhead); the host sums the records
    if (!kCount || p.stats == nullptr) return;  // (!kCount: the counters compile away)
    uint64_t c[6] = {rays, tri_in, sph_tests, node_tests, tnode_tests, tri_done};
    const uint64_t mix[4] = {it_all, it_walk, lanes_all, lanes_walk};  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (uint32_t off = kWave / 2; off > 0; off >>= 1) c[k] += __shfl_xor(c[k], (int)off);
    if (lane == 0) {
        unsigned long long *w = p.stats + (size_t)wave_id * kStatSlots;
#pragma unroll
        for (int k = 0; k < 6; ++k) w[k < 4 ? k : k + 4] += c[k];
        for (int k = 0; k < 4; ++k) w[10 + k] += mix[k];
#ifdef RT_WALK_MIX
        w[4] += wm_iters; w[5] += wm_leaf_iters; w[6] += wm_leaf_trips; w[7] += wm_walks;
#endif
#ifdef RT_STAMPS
        // coarse shares (stamp_cycles): refill + store + resolve + loop, setup, walks, shade
        w[4] += stamp_acc[0] + stamp_acc[4] + stamp_acc[5] + stamp_acc[6];
        for (int k = 1; k < 4; ++k) w[4 + k] += stamp_acc[k];
        for (uint32_t k = 0; k < kStampSegs; ++k) w[16 + k] += stamp_acc[k];
#endif
#ifdef RT_WAVE_TIMES
        w[4] = wt_start;
        w[5] = wt_pull;
        w[6] = wt_exh;
        w[7] = __builtin_amdgcn_s_memrealtime();
        w[14] = wt_jobs_tail;
#endif
    }
}

}  // namespace
}  // namespace rtamd
