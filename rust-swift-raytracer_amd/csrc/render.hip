// render.hip -- the MI355X render path: a persistent path-regenerating trace
// kernel and an ordered resolve kernel, hand-written for gfx950 (CDNA4).
//
// Replaces the reference's ray_trace pixel loop and everything under it
// (Naxaes/Rust-Swift-Raytracer raytracer/src/common.rs:263-361 ray_color /
// ray_trace, common.rs:59-258 Sphere/Triangle/Mesh/World::hit,
// materials.rs:30-102 scatter, camera.rs:84-89 cast_ray, random.rs:15-30).
//
// Numerics: every operation is one IEEE binary32 op in the reference's order
// (-ffp-contract=off, correctly rounded divide/sqrt), so a sample started
// from the same xorshift32 state produces the same bits as the reference.
//
// Work decomposition: one job = one pixel sample.  Each wave
// is persistent: its 64 lanes trace one bounce per loop iteration; a lane
// whose path ends writes the sample colour to a per-sample slab in HBM and
// takes the next job (ballot + mbcnt prefix, one atomic per chunk per wave on
// one of 16-64 partitioned counters), so lanes never idle behind the longest path
// of their wave.  World::hit goes through exact BVHs (spheres: staged in LDS;
// triangles: phantom-aware static and camera-origin trees, primary strip
// lists) whose visiting order provably returns the reference's hit; the
// brute-force loops keep the reference order (RT_ACCEL_BRUTE, small scenes).
// The resolve kernel sums each pixel's samples in sample order (the
// reference's sequential add_with_alpha, common.rs:338-340), applies the
// gamma/`as u8` epilogue (:344-356) and stores RGBA8 rows top-first (:351).
//
// This unit holds everything that traces a ray (the SERIAL mode's coalescing
// block search included); the kernels that do not are in serial.hip.  The
// device code is in headers by concern, compiled here and nowhere else (in a
// unit of their own the coalescing kernels come out as other code): this file
// keeps the kernel entry points, the resolve kernel, the instance table and
// the host launchers (one for every trace kernel: launch_trace).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "exactdiv.h"
#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

#include "device_math.h"      // F3, exact divisions, RNG draws, seeds, uniform loads
#include "sphere_search.h"    // sphere search: brute force, the three tree walks' steps, stage_tree
#include "serial_jobs.h"      // job -> pixel maps, SERIAL start states
#include "tri_search.h"       // triangle search: brute force, tree steps, primary strip lists
#include "chunk_resolve.h"    // in-kernel resolve of a finished chunk
#include "trace_body.h"       // the trace loop and its occupancy constants
#include "serial_coalesce.h"  // SERIAL coalescing block search

namespace rtamd {
namespace {

// Each entry point spells its trace_body configuration by field name, as a
// local type Cfg (trace_body.h TraceConfig; a field left alone keeps its default).
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCount, bool kSerial = false>
__global__ __launch_bounds__(trace_threads(kLds, kMesh, kSerial ? 2 : kCount ? 1 : 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(kLds, kMesh, kSerial ? 2 : kCount ? 1 : 0), 8)))
void trace_kernel(TraceParams p) {
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = kBvh, lds = kLds, step = kStep, mesh = kMesh, count = kCount, serial = kSerial; }
    };
    trace_body<Cfg>(p, nullptr);
}

// The sphere-only frame kernels over the corner records: instances of their
// own, so that the box-record kernels above stay the code they were (one
// kernel with both walks behind a launch flag ran its box walk 1.5 % slower:
// the compiler placed it out of line).  The argument block begins with the
// TraceParams (trace_body's kargs() re-reads them from offset 0).  They keep
// trace_kernel's name and parameter list, so tools that parse
// `trace_kernel<...>` names (tools/pmc_summary.py) tell lean from counting.
struct CornerParams {
    TraceParams p;
    const uint4 *image;  // bvh.h SphereBVH::corner: 8 uint4 per node
};
namespace corner {
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCount, bool kSerial = false>
__global__ __launch_bounds__(trace_threads(true, 0, kCount ? 1 : 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(true, 0, kCount ? 1 : 0), 8)))
void trace_kernel(CornerParams c) {
    static_assert(kBvh && kLds && kMesh == 0 && !kSerial, "corner records: sphere-only LDS frame kernels");
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = lds = corner = true, step = kStep, count = kCount; }
    };
    trace_body<Cfg>(c.p, c.image);
}
// The lean whole-walk kernel with deferred leaf tests (trace_body's kDefer):
// an instance of its own beside the immediate walk above, which stays the code
// it was (RT_AMD_LEAF_DEFER=0 runs it).  Same name and parameter list again.
namespace deferred {
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCount, bool kSerial = false>
__global__ __launch_bounds__(trace_threads(true, 0, kCount ? 1 : 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(true, 0, kCount ? 1 : 0), 8)))
void trace_kernel(CornerParams c) {
    static_assert(kBvh && kLds && !kStep && kMesh == 0 && !kSerial, "deferred leaves: whole corner walks");
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = lds = corner = true, count = kCount, defer = kLeafDeferC; }
    };
    trace_body<Cfg>(c.p, c.image);
}
}  // namespace deferred
// The deferred-leaf kernel with the launch's constants compiled in
// (trace_body's kPlain; launches that satisfy render.h trace_plain_ok): an
// instance of its own beside the one above, which stays the code it was and
// runs every other launch (RT_AMD_PLAIN=0: all of them).  Same name and
// parameter list again.
namespace plain {
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCount, bool kSerial = false>
__global__ __launch_bounds__(trace_threads(true, 0, 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(true, 0, 0), 8)))
void trace_kernel(CornerParams c) {
    static_assert(kBvh && kLds && !kStep && kMesh == 0 && !kCount && !kSerial, "plain: the lean deferred-leaf kernel");
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = lds = corner = plain = true, defer = kLeafDeferC; }
    };
    trace_body<Cfg>(c.p, c.image);
}
}  // namespace plain
}  // namespace corner

// Accumulation passes (kKindAccum): the lean frame kernels' twins with
// trace_body's kAccum changes, one per (search, step, mesh) a lean frame can
// run, at their twins' workgroup size and waves per SIMD.  Entry points of
// their own in a namespace of their own, as the corner-record kernels are: the
// frame kernels above stay the code they were, and their names and parameter
// types stay what tools/kernel_hash.py looks for.
namespace accum {
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCorner>
__global__ __launch_bounds__(trace_threads(kLds, kMesh, 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(kLds, kMesh, 0), 8)))
void trace_kernel(AccumParams a) {
    static_assert(!kCorner || (kBvh && kLds && kMesh == 0), "corner records: sphere-only LDS kernels");
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = kBvh, lds = kLds, step = kStep, mesh = kMesh, corner = kCorner, accum = true; }
    };
    trace_body<Cfg>(a.p, a.image);
}
}  // namespace accum

// Adaptive accumulation passes (kKindAdapt): the accumulation kernels' twins
// with trace_body's kAdapt changes, one per (search, step, mesh) an
// accumulation pass can run, at the same workgroup size and waves per SIMD.
namespace adapt {
template <bool kBvh, bool kLds, bool kStep, int kMesh, bool kCorner>
__global__ __launch_bounds__(trace_threads(kLds, kMesh, 0))
__attribute__((amdgpu_waves_per_eu(trace_waves_per_eu(kLds, kMesh, 0), 8)))
void trace_kernel(AdaptParams a) {
    static_assert(!kCorner || (kBvh && kLds && kMesh == 0), "corner records: sphere-only LDS kernels");
    struct Cfg : TraceConfig {
        constexpr Cfg() { bvh = kBvh, lds = kLds, step = kStep, mesh = kMesh, corner = kCorner, adapt = true; }
    };
    trace_body<Cfg>(a.p, a.image);
}
}  // namespace adapt

// ------------------------------------------------------------ resolve kernel
// Sums each pixel's samples in order (common.rs:333-341), gamma + `as u8`
// (:344-356), one RGBA8 word per pixel.  The slab is planar and pixel-major,
// so one wave's 64 pixels own a contiguous run of 64*spp floats per plane:
// the wave copies it through LDS in chunks of 64 samples (float4 loads
// across the run, coalesced), padded to 65 floats per pixel so that the
// in-order per-lane sums read LDS without bank conflicts.
constexpr uint32_t kResolveWaves = 4;
constexpr uint32_t kResolveChunk = 64;
constexpr uint32_t kResolvePad = kResolveChunk + 1;
__global__ __launch_bounds__(kResolveWaves * 64) void resolve_kernel(
    const float *__restrict__ samples, uint32_t *__restrict__ out, uint32_t npix, uint32_t spp,
    float inv, uint32_t width, uint32_t slab_row0) {
    __shared__ float lds[kResolveWaves][kWave * kResolvePad];
    const uint32_t lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const uint32_t lp0 = (blockIdx.x * kResolveWaves + wave) * kWave;
    if (lp0 >= npix) return;  // whole waves only: no workgroup barrier below
    const uint32_t n = min(kWave, npix - lp0);
    const size_t plane = (size_t)npix * spp;
    float *L = lds[wave];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    float a = 1.0f;  // Color::new(0,0,0): alpha 1
    for (uint32_t k0 = 0; k0 < spp; k0 += kResolveChunk) {
        const uint32_t kc = min(kResolveChunk, spp - k0);
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) {
            const float *src = samples + c * plane + (size_t)lp0 * spp + k0;
            if (kc == kResolveChunk && spp % 4 == 0) {
                // 16 lanes per pixel, 4 pixels per float4 wave load
                for (uint32_t e = lane; e < n * 16; e += kWave) {
                    const uint32_t pix = e >> 4, k = (e & 15u) * 4;
                    const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)pix * spp + k);
                    float *d = L + pix * kResolvePad + k;
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                }
            } else {
                for (uint32_t e = lane; e < n * kc; e += kWave) {
                    const uint32_t pix = e / kc, k = e - pix * kc;
                    L[pix * kResolvePad + k] = src[(size_t)pix * spp + k];
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            float x = acc[c];
            if (lane < n)
                for (uint32_t k = 0; k < kc; ++k) x = x + L[lane * kResolvePad + k];
            acc[c] = x;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        for (uint32_t k = 0; k < kc; ++k) a = a + 1.0f;  // every sample's alpha is exactly 1.0
    }
    if (lane >= n) return;
    const uint32_t lp = lp0 + lane;
    const uint32_t R = sat_u8(__builtin_sqrtf(acc[0] * inv) * 255.999f);
    const uint32_t G = sat_u8(__builtin_sqrtf(acc[1] * inv) * 255.999f);
    const uint32_t B = sat_u8(__builtin_sqrtf(acc[2] * inv) * 255.999f);
    const uint32_t A = sat_u8(a * inv * 255.999f);
    const uint32_t q = lp / width;
    const uint32_t col = lp - q * width;
    out[(size_t)(slab_row0 + q) * width + col] = R | (G << 8) | (B << 16) | (A << 24);
}

}  // namespace

// ------------------------------------------------------------ the instances
// Every trace_kernel / corner::trace_kernel / accum:: / adapt::trace_kernel instance is
// spelled here and nowhere else, in one table by render.h trace_key: the launch,
// the occupancy queries and the LDS opt-in look it up by its TraceVariant.
struct TraceInstance {
    const void *fn;    // nullptr: no such instance
    uint32_t threads;  // per workgroup (the kernel's __launch_bounds__)
};
template <class Kernel>
static TraceInstance instance_of(Kernel *kernel, uint32_t threads) {
    return {reinterpret_cast<const void *>(kernel), threads};
}

// the instance of the variant with table key kKey
template <int kKey>
static TraceInstance trace_instance_at() {
    constexpr TraceVariant kV = trace_variant_at(kKey);
    constexpr bool kBvh = kV.search != kSearchBrute, kLds = kV.lds(), kCorner = kV.search == kSearchLdsCorner,
                   kStep = kV.step, kCount = kV.kind == kKindCounting, kSerial = kV.kind == kKindSerial,
                   kAccum = kV.kind == kKindAccum, kAdapt = kV.kind == kKindAdapt;
    // (an accumulation pass runs at its lean twin's workgroup size)
    constexpr uint32_t threads = trace_threads(kLds, kV.mesh, kAccum || kAdapt ? (int)kKindLean : kV.kind);
    if constexpr (kV.leaf == TraceLeaf::Plain) {  // the deferred-leaf kernel's plain twin (render.h trace_plain_ok)
        return instance_of(&corner::plain::trace_kernel<true, true, false, 0, false, false>, threads);
    } else if constexpr (kV.leaf == TraceLeaf::Deferred) {  // deferred leaves: the lean whole-walk corner kernel
        return instance_of(&corner::deferred::trace_kernel<true, true, false, 0, false, false>, threads);
    } else if constexpr (kKey == kTraceNoKey || trace_key(normalise_trace_variant(kV)) != kKey) {
        return {nullptr, 0};  // not its own normal form: another instance serves it (render.h)
    } else if constexpr (kAdapt) {
        return instance_of(&adapt::trace_kernel<kBvh, kLds, kStep, kV.mesh, kCorner>, threads);
    } else if constexpr (kAccum) {
        return instance_of(&accum::trace_kernel<kBvh, kLds, kStep, kV.mesh, kCorner>, threads);
    } else if constexpr (!kCorner) {
        return instance_of(&trace_kernel<kBvh, kLds, kStep, kV.mesh, kCount, kSerial>, threads);
#ifdef RT_COUNT_DEFER
    } else if constexpr (kCount && !kStep) {  // diagnostic build: the deferred walk, counted
        return instance_of(&corner::deferred::trace_kernel<true, true, false, 0, true, false>, threads);
#endif
    } else {  // corner records: the sphere-only frame kernels
        return instance_of(&corner::trace_kernel<true, true, kStep, 0, kCount, false>, threads);
    }
}
template <int... kKey>
static const TraceInstance *trace_table(std::integer_sequence<int, kKey...>) {
    static const TraceInstance table[] = {trace_instance_at<kKey>()...};
    return table;
}
static const TraceInstance &trace_instance(TraceVariant v) {
    return trace_table(std::make_integer_sequence<int, kTraceKeys>{})[trace_key(v)];
}

uint32_t trace_block_threads(TraceVariant v) { return trace_instance(v).threads; }

bool trace_instance_exists(int key) {
    return key >= 0 && key < kTraceKeys && trace_instance(trace_variant_at(key)).fn != nullptr;
}

size_t trace_lds_bytes(const TraceParams &p, bool corner) {
    // (shading records in global memory instead, which would allow 8 waves per
    // SIMD: A/B +1.7 % at 6 waves, +8 % at 8 waves per SIMD)
    // (the corner records do exactly that: twice the node bytes, still two
    // workgroups of 8 waves per SIMD per CU)
    return corner ? trace_corner_lds(p.nnodes, p.nprims) : trace_tree_lds(p.nnodes, p.nprims, p.nsph_padded);
}

size_t trace_dyn_lds(const TraceParams &p, TraceVariant v) {
    const size_t tree = v.lds() ? (trace_lds_bytes(p, v.search == kSearchLdsCorner) + 15u) & ~(size_t)15u : 0u;
    return tree + (v.mesh == 3 ? (size_t)p.tw_depth * trace_block_threads(v) * 2u : 0u);
}

hipError_t launch_trace(TraceVariant v, const TraceParams &p, const TraceTail &tail, uint32_t blocks,
                        hipStream_t stream) {
    const TraceInstance &k = trace_instance(v);
    if (k.fn == nullptr || (v.kind == kKindCounting) != (p.stats != nullptr) ||
        (v.kind == kKindSerial) != (p.mode >= kRngSerialCount))
        return hipErrorInvalidValue;
    const uint4 *image = v.search == kSearchLdsCorner ? tail.corner : nullptr;
    auto launch = [&](void *block) {
        void *args[] = {block};
        return hipLaunchKernel(k.fn, dim3(blocks), dim3(k.threads), args, trace_dyn_lds(p, v), stream);
    };
    if (v.kind == kKindAccum || v.kind == kKindAdapt) {
        // (the passes resolve in-kernel: without a ring the samples would go to the slab)
        if (p.ring == nullptr || tail.sums == nullptr) return hipErrorInvalidValue;
        if (v.kind == kKindAccum) {
            AccumParams block{p, image, AccumTail{tail.sums, tail.n0, tail.stride}};
            return launch(&block);
        }
        if (tail.sumsq == nullptr || tail.list == nullptr) return hipErrorInvalidValue;
        AdaptParams block{p, image, AdaptTail{tail.sums, tail.sumsq, tail.list, tail.n0, tail.stride}};
        return launch(&block);
    }
    CornerParams block{p, image};  // (begins with the TraceParams: either frame kernel's argument block)
    return launch(&block);
}

hipError_t trace_occupancy(int *blocks_per_cu, TraceVariant v, size_t lds_bytes) {
    const TraceInstance &k = trace_instance(v);
    if (k.fn == nullptr) return hipErrorInvalidValue;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k.fn, (int)k.threads, lds_bytes);
}

int trace_leaf_defer(TraceVariant v) {
    return v.leaf != TraceLeaf::Immediate && trace_instance(v).fn != nullptr ? kLeafDeferC : 0;
}

hipError_t trace_lds_opt_in() {
    hipError_t e = hipSuccess;
    for (int key = 0; key < kTraceKeys && e == hipSuccess; ++key) {
        const TraceVariant v = trace_variant_at(key);
        if (v.lds() && trace_instance(v).fn != nullptr)
            e = hipFuncSetAttribute(trace_instance(v).fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsPerCu);
    }
    return e;
}

hipError_t launch_resolve_ex(const float *samples, uint32_t *out, uint32_t npix, uint32_t spp,
                             float inv_spp, uint32_t width, uint32_t slab_row0,
                             hipStream_t stream) {
    const uint32_t per_block = kResolveWaves * kWave;
    const uint32_t blocks = (npix + per_block - 1) / per_block;
    hipLaunchKernelGGL(resolve_kernel, dim3(blocks), dim3(per_block), 0, stream, samples, out, npix,
                       spp, inv_spp, width, slab_row0);
    return hipGetLastError();
}

template <bool kBvh, bool kLds>
static void launch_coalesce_m(const TraceParams &p, uint32_t *path, uint32_t *bend, uint32_t L, uint32_t Kmax,
                              uint32_t R, size_t tree_bytes, size_t lds, unsigned long long *dbg,
                              hipStream_t stream) {
    const uint32_t nb = (L + R - 1) / R;
    const int mesh = trace_mesh_kind(p.ntri != 0, p.tnodes != 0);
    if (mesh == 2)
        hipLaunchKernelGGL((serial_coalesce_kernel<kBvh, kLds, 2>), dim3(nb), dim3(kCoalesceThreads), lds, stream, p,
                           path, bend, L, Kmax, R, (uint32_t)tree_bytes, dbg);
    else if (mesh == 1)
        hipLaunchKernelGGL((serial_coalesce_kernel<kBvh, kLds, 1>), dim3(nb), dim3(kCoalesceThreads), lds, stream, p,
                           path, bend, L, Kmax, R, (uint32_t)tree_bytes, dbg);
    else
        hipLaunchKernelGGL((serial_coalesce_kernel<kBvh, kLds, 0>), dim3(nb), dim3(kCoalesceThreads), lds, stream, p,
                           path, bend, L, Kmax, R, (uint32_t)tree_bytes, dbg);
}

size_t serial_coalesce_search_lds(uint32_t K, uint32_t depth) { return coalesce_lds_bytes(K, depth); }

size_t serial_coalesce_lds(const TraceParams &p, uint32_t K, bool tree_lds) {
    const size_t tb = tree_lds ? (trace_lds_bytes(p) + 15) & ~(size_t)15 : 0;
    return tb + coalesce_lds_bytes(K, p.depth > 0 ? (uint32_t)p.depth : 0u);
}

hipError_t launch_serial_coalesce(const TraceParams &p, uint32_t *path, uint32_t *bend, uint32_t L, uint32_t Kmax,
                                  uint32_t R, bool tree_lds, unsigned long long *dbg, hipStream_t stream) {
    if (!L || !R) return hipSuccess;
    const size_t tb = tree_lds ? (trace_lds_bytes(p) + 15) & ~(size_t)15 : 0;
    const size_t lds = serial_coalesce_lds(p, Kmax, tree_lds);
    if (p.nnodes && tree_lds) launch_coalesce_m<true, true>(p, path, bend, L, Kmax, R, tb, lds, dbg, stream);
    else if (p.nnodes) launch_coalesce_m<true, false>(p, path, bend, L, Kmax, R, tb, lds, dbg, stream);
    else launch_coalesce_m<false, false>(p, path, bend, L, Kmax, R, tb, lds, dbg, stream);
    return hipGetLastError();
}

}  // namespace rtamd
