// first_hit.hip -- the first World::hit of every pixel's deterministic primary
// ray: records (primitive, t, normal, position) or a view of them as RGBA8
// (include/raytracer_amd.h rt_first_hit_*).
//
// The ray of the pixel at reference (row, col) is the frame's primary ray with
// its two draws replaced by the constants su, sv (common.rs:335-337,
// camera.rs:84-89); the search is World::hit (common.rs:237-258) through the
// frame kernels' own tests and walks (sphere_search.h, tri_search.h): the sphere
// tree walked whole from global memory after the spheres kept out of it; the
// primary triangle strip lists where the host bound them (made current for
// this camera and frame size first), else the static triangle tree; brute
// force where the scene has no tree or RT_ACCEL_BRUTE asks for it.
//
// One lane per pixel of the rectangle in a plain grid: a wave covers an 8 x 8
// tile (neighbouring rays walk the same nodes), a lane stores its 32-byte
// record with two 16-byte stores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "exactdiv.h"
#include "kernels.h"
#include "render.h"

#pragma clang fp contract(off)

#include "device_math.h"
#include "sphere_search.h"
#include "tri_search.h"

namespace rtamd {
namespace {

// The argument block: the frame kernels' TraceParams (no field added), then
// the tail (render.h FirstHitTail).
struct FirstHitParams {
    TraceParams p;
    FirstHitTail tail;
};

constexpr uint32_t kFirstHitThreads = 256;
constexpr uint32_t kTile = 8;  // a wave's pixels: kTile x kTile

// kBvh: the sphere tree (p.nnodes != 0).  kMesh: render.h trace_mesh_kind.
// kView: write the view's RGBA8 instead of the record.
template <bool kBvh, int kMesh, bool kView>
__global__ __launch_bounds__(kFirstHitThreads) void first_hit_kernel(FirstHitParams a) {
    constexpr bool kWaveGuard = kMesh < 2;  // (exactdiv.h, as the frame kernels)
    const TraceParams &p = a.p;
    const FirstHitTail &q = a.tail;
    // the lane's pixel: wave -> tile, lane -> pixel of the tile
    const uint32_t wave = blockIdx.x * (kFirstHitThreads / kWave) + threadIdx.x / kWave;
    const uint32_t lane = threadIdx.x % kWave;
    const uint32_t tiles_x = (q.w + kTile - 1u) / kTile;
    const uint32_t ty = wave / tiles_x, tx = wave - ty * tiles_x;
    const uint32_t rx = tx * kTile + (lane & (kTile - 1u)), ry = ty * kTile + lane / kTile;
    if (rx >= q.w || ry >= q.h) return;
    const uint32_t col = q.x0 + rx;
    const uint32_t row = p.height - 1u - (q.y0 + ry);  // reference row, 0 = bottom

    // common.rs:335-337 with the draws replaced by su, sv; camera.rs:84-89
    const float u = ((float)col + q.su) / p.wden;
    const float v = ((float)row + q.sv) / p.hden;
    const F3 org = f3(p.cam[0], p.cam[1], p.cam[2]);
    const F3 llc = f3(p.cam[3], p.cam[4], p.cam[5]);
    const F3 hor = f3(p.cam[6], p.cam[7], p.cam[8]);
    const F3 ver = f3(p.cam[9], p.cam[10], p.cam[11]);
    const F3 dir = unit<kWaveGuard>(((llc + scale(hor, u)) + scale(ver, v)) - org);

    // World::hit, spheres with shrinking t_max (common.rs:241-247)
    float best_t = __builtin_inff();
    int best_i = -1;
    uint32_t unused = 0;  // (the frame kernels' work counters)
    // slab-test reciprocals, clamped (trace_body.h's ray setup)
    const F3 inv = f3(slab_rcp(dir.x), slab_rcp(dir.y), slab_rcp(dir.z));
    if (kBvh) {
        spheres_big<kWaveGuard>(p, org, dir, best_t, best_i);
        BvhView view;
        stage_tree<false, false>(p, nullptr, nullptr, view);
        const uint32_t oct = (inv.x < 0.0f ? 1u : 0u) | (inv.y < 0.0f ? 2u : 0u) | (inv.z < 0.0f ? 4u : 0u);
        F3 nlo, nhi;
        sphere_slabs(org, inv, sph_inflation(p, sph_bound(p, org), best_t), nlo, nhi);
        uint32_t node = sphere_walk_entry<false>(0u, oct, p.nnodes);
        do {
            uint32_t leaf;
            if (sphere_node<false>(view, inv, oct, best_t, nlo, nhi, node, leaf, unused))
                sphere_leaf<kWaveGuard, false>(view, org, dir, leaf, best_t, best_i, unused);
        } while (node != kNodeEndDev);
    } else {
        spheres_brute<kWaveGuard>(p, org, dir, best_t, best_i);
    }

    // Mesh::hit with t_max = best_t, its own closest from +inf (common.rs:178-223)
    float tri_t = __builtin_inff();
    int tri_i = -1;
    if (kMesh == 2) {
        float rho = 0.0f;
        if (!tri_begin(p, org, dir, best_t, false, rho, tri_t, tri_i, unused, unused)) {
            // (a far or non-finite origin: every record was tested there)
        } else if (p.ptl_off != nullptr) {
            // the frame's primary strip lists, current for this camera and frame
            // size (first_hit.cpp): the pixel's strip from its job, top row first
            tri_primary_list<false>(p, (q.y0 + ry) * p.width + col, org, dir, best_t, tri_t, tri_i, unused, unused);
        } else {
            const F3 dlt2 = f3(2.0f * (org.x - p.tbvh_oc[0]), 2.0f * (org.y - p.tbvh_oc[1]),
                               2.0f * (org.z - p.tbvh_oc[2]));
            F3 nlo, nhi;
            sphere_slabs(org, inv, rho, nlo, nhi);
            float cap = fminf(best_t, tri_t);
            uint32_t node = 0;
            do {
                uint32_t leaf;
                if (tri_node(p, nlo, nhi, inv, dlt2, false, cap, node, leaf, unused)) {
                    tri_leaf(p, org, dir, false, leaf, best_t, tri_t, tri_i, unused, unused);
                    cap = fminf(best_t, tri_t);
                }
            } while (node != kNodeEndDev);
        }
    } else if (kMesh == 1) {
        triangles_brute(p, org, dir, best_t, tri_t, tri_i, unused);
    }

    // the hit record (common.rs:95 for a sphere; a triangle wins a tie)
    uint32_t prim = 0;
    float t = __builtin_inff();
    F3 nrm = f3(0.0f, 0.0f, 0.0f), pos = nrm;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f;  // (kView) the primitive's material colour
    if (kMesh != 0 && tri_i >= 0) {
        prim = 1u + p.nsph + (uint32_t)tri_i;
        t = tri_t;
        pos = org + scale(dir, tri_t);
        const float4 *g = p.tri_geo + 4u * (uint32_t)tri_i;
        const float4 Nn = g[3];
        nrm = f3(Nn.x, Nn.y, Nn.z);
        if (kView) {
            const float *m = p.mats + 8u * __float_as_uint(g[0].w);
            const bool glass = __float_as_uint(m[0]) == kMatDielectric;  // materials.rs:96
            cr = glass ? 1.0f : m[1];
            cg = glass ? 1.0f : m[2];
            cb = glass ? 1.0f : m[3];
        }
    } else if (best_i >= 0) {
        prim = 1u + (uint32_t)best_i;
        t = best_t;
        pos = org + scale(dir, best_t);
        const float4 SS = p.sph_shade[2 * best_i];
        nrm = unit<kWaveGuard>(divide_by<kWaveGuard>(pos - f3(SS.x, SS.y, SS.z), SS.w));
        if (kView) {
            const float4 SM = p.sph_shade[2 * best_i + 1];
            const bool glass = p.sph_kind[best_i] == kMatDielectric;
            cr = glass ? 1.0f : SM.x;
            cg = glass ? 1.0f : SM.y;
            cb = glass ? 1.0f : SM.z;
        }
    }

    const size_t idx = (size_t)ry * q.w + rx;
    if (!kView) {
        float4 *out = reinterpret_cast<float4 *>(q.out) + 2u * idx;
        out[0] = make_float4(__uint_as_float(prim), t, nrm.x, nrm.y);
        out[1] = make_float4(nrm.z, pos.x, pos.y, pos.z);
        return;
    }
    uint32_t R = 0, G = 0, B = 0;
    if (prim != 0u) {
        if (q.view == kViewNormal) {
            R = sat_u8(((nrm.x * 0.5f) + 0.5f) * 255.999f);
            G = sat_u8(((nrm.y * 0.5f) + 0.5f) * 255.999f);
            B = sat_u8(((nrm.z * 0.5f) + 0.5f) * 255.999f);
        } else if (q.view == kViewDepth) {
            R = G = B = sat_u8((1.0f / (1.0f + t)) * 255.999f);
        } else if (q.view == kViewAlbedo) {
            R = sat_u8(cr * 255.999f);
            G = sat_u8(cg * 255.999f);
            B = sat_u8(cb * 255.999f);
        } else {
            const uint32_t h = prim * 2654435761u;
            R = h >> 24;
            G = (h >> 16) & 255u;
            B = (h >> 8) & 255u;
        }
    }
    reinterpret_cast<uint32_t *>(q.out)[idx] = R | (G << 8) | (B << 16) | (255u << 24);
}

template <bool kView>
const void *first_hit_instance(bool bvh, int mesh) {
#define RT_FH(B, M) reinterpret_cast<const void *>(&first_hit_kernel<B, M, kView>)
    if (bvh) return mesh == 2 ? RT_FH(true, 2) : mesh == 1 ? RT_FH(true, 1) : RT_FH(true, 0);
    return mesh == 2 ? RT_FH(false, 2) : mesh == 1 ? RT_FH(false, 1) : RT_FH(false, 0);
#undef RT_FH
}

}  // namespace

hipError_t launch_first_hit(const TraceParams &p, const FirstHitTail &tail, hipStream_t stream) {
    if (tail.out == nullptr || tail.w == 0 || tail.h == 0 || tail.x0 + (uint64_t)tail.w > p.width ||
        tail.y0 + (uint64_t)tail.h > p.height || (tail.view != kViewNone && tail.view > kViewPrim))
        return hipErrorInvalidValue;
    const int mesh = trace_mesh_kind(p.ntri != 0, p.tnodes != 0);
    const bool view = tail.view != kViewNone;
    const void *fn = view ? first_hit_instance<true>(p.nnodes != 0, mesh) : first_hit_instance<false>(p.nnodes != 0, mesh);
    const uint64_t tiles = (uint64_t)((tail.w + kTile - 1u) / kTile) * ((tail.h + kTile - 1u) / kTile);
    const uint64_t per_block = kFirstHitThreads / kWave;
    const uint64_t blocks = (tiles + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    FirstHitParams a{p, tail};
    void *args[] = {(void *)&a};
    return hipLaunchKernel(fn, dim3((uint32_t)blocks), dim3(kFirstHitThreads), args, 0, stream);
}

}  // namespace rtamd
