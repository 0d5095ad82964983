// corner_image_check.cpp -- the sphere tree's corner records (bvh.h
// SphereBVH::corner) against the tree they are built from (CPU test driver for
// tests/test_corner_image.py; compiled with g++ against csrc/bvh.cpp).
//
//   corner_image_check scene.txt [budget]   the scene in the file
//   corner_image_check --random             random sets of 20-480 spheres
//
// Per tree:
//   * slot o of every node is the box's near corner for octant o (per axis lo
//     where the direction is positive, hi where it is negative) and slot 7 - o
//     its far corner;
//   * every link index is below the node count or the end marker;
//   * every leaf word decodes to the leaf's (first, count);
// and for a few thousand rays (among them directions with one or two
// components exactly +0 or -0, components below 1e-20, origins inside leaf
// boxes), each with an infinite and a finite best t and with the full and the
// smallest inflation: a host emulation of the kernel's corner step
// (sphere_search.h sphere_node_corner) visits the same nodes in the same order,
// takes the same skip decisions and enters the same leaves as an emulation of
// the box step (sphere_node, LDS form).  float arithmetic, fmaf, slab_rcp's
// clamp; both emulations share the reciprocal.
// `budget`: the image, prims and ids fit the 81,920 B a workgroup of the lean
// sphere kernel may take.
// Prints "OK <counts>" or the first failures and exits non-zero.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "bvh.h"
#include "scene.h"

using namespace rtamd;

static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (fails++ < 10) std::printf(__VA_ARGS__); \
        }                                               \
    } while (0)

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static float fbits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static int32_t ibits(float f) { return (int32_t)bits(f); }

struct Rng {  // xorshift64*
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    float uni() { return (float)(next() >> 40) * 0x1p-24f; }            // [0, 1)
    float range(float a, float b) { return a + (b - a) * uni(); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() >> 33) % n; }
};

static float slab_rcp(float d) {  // sphere_search.h: med3(rcp(d), -1e20, 1e20)
    const float r = 1.0f / d;
    return r < -1e20f ? -1e20f : r > 1e20f ? 1e20f : r;
}

struct Step { uint32_t node; bool skip; uint32_t leaf; };  // leaf: entered leaf's word, else 0

struct Ray { float o[3], d[3]; };

// the walk's per-ray inputs (sphere_search.h sph_bound / sph_inflation)
static float inflation(const SphereBVH &bv, const Ray &r, float best_t, bool full) {
    const float e_abs = 2e-6f * ((std::fabs(r.o[0]) + std::fabs(r.o[1])) + std::fabs(r.o[2]) + bv.mag);
    if (!full) return e_abs;
    const float ax = r.o[0] - bv.centre[0], ay = r.o[1] - bv.centre[1], az = r.o[2] - bv.centre[2];
    const float A = std::sqrt((ax * ax + ay * ay) + az * az) * 1.00001f + bv.radius;
    const float K = 3.0e-3f, Kq = 40.5f * 0x1p-24f;
    const float s = std::fmin(A, best_t + bv.rmax) * (1.0f + 3.0f * K) + bv.rmax;
    return std::fmin(K * s, (Kq * s) * (s * bv.inv_rmin)) + e_abs;
}

static bool skip_test(float tn, float tf, float best_t) {
    return tn > tf || tf < 0.001f || ibits(tn) > ibits(best_t);
}

// sphere_node<true> with sphere_walk_entry and sphere_slabs
static std::vector<Step> walk_box(const SphereBVH &bv, const Ray &r, const float inv[3], uint32_t oct, float e,
                                  float best_t) {
    const size_t nn = bv.nodes.size() / 8;
    float nlo[3], nhi[3];
    for (int k = 0; k < 3; ++k) {
        nlo[k] = -((r.o[k] + e) * inv[k]);
        nhi[k] = -((r.o[k] - e) * inv[k]);
    }
    auto next_of = [&](uint32_t n) -> uint32_t {  // the record's `next` link for oct
        const uint32_t a = bits(bv.nodes[n * 8 + 3]), b = bits(bv.nodes[n * 8 + 7]);
        return (a & kLeafBit) ? bv.miss[n * 8 + oct] : a + ((oct >> b) & 1u);
    };
    std::vector<Step> out;
    uint32_t node = nn > 1 ? next_of(0) : 0;
    while (node != kNodeEnd && out.size() <= 4 * nn) {
        const float *B = &bv.nodes[node * 8];
        float t0[3], t1[3];
        for (int k = 0; k < 3; ++k) {
            t0[k] = std::fmaf(B[k], inv[k], nlo[k]);
            t1[k] = std::fmaf(B[4 + k], inv[k], nhi[k]);
        }
        const float tn = std::fmax(std::fmax(std::fmin(t0[0], t1[0]), std::fmin(t0[1], t1[1])), std::fmin(t0[2], t1[2]));
        const float tf = std::fmin(std::fmin(std::fmax(t0[0], t1[0]), std::fmax(t0[1], t1[1])), std::fmax(t0[2], t1[2]));
        const bool skip = skip_test(tn, tf, best_t);
        const uint32_t a = bits(B[3]), b = bits(B[7]);
        const uint32_t leaf = (a & kLeafBit) ? ((a & ~kLeafBit) << 3) | b : 0u;
        out.push_back({node, skip, skip ? 0u : leaf});
        node = skip ? bv.miss[node * 8 + oct] : next_of(node);
    }
    return out;
}

// sphere_node_corner with sphere_corner_entry and sphere_corner_slabs
static std::vector<Step> walk_corner(const SphereBVH &bv, const Ray &r, const float inv[3], uint32_t oct, float e,
                                     float best_t) {
    const size_t nn = bv.corner.size() / 32;
    float nnr[3], nf[3];
    for (int k = 0; k < 3; ++k) {
        const float ek = ((oct >> k) & 1u) ? -e : e;
        nnr[k] = -((r.o[k] + ek) * inv[k]);
        nf[k] = -((r.o[k] - ek) * inv[k]);
    }
    std::vector<Step> out;
    uint32_t node = nn > 1 ? bv.corner[oct * 4 + 3] >> 16 : 0;
    while (node != kCornerEnd && out.size() <= 4 * nn) {
        if (node >= nn) { CHECK(false, "corner walk left the image (node %u)\n", node); break; }
        const uint32_t *N = &bv.corner[(size_t)node * 32 + oct * 4];
        const uint32_t *F = &bv.corner[(size_t)node * 32 + (7 - oct) * 4];
        float a[3], b[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = std::fmaf(fbits(N[k]), inv[k], nnr[k]);
            b[k] = std::fmaf(fbits(F[k]), inv[k], nf[k]);
        }
        const float tn = std::fmax(std::fmax(a[0], a[1]), a[2]);
        const float tf = std::fmin(std::fmin(b[0], b[1]), b[2]);
        const bool skip = skip_test(tn, tf, best_t);
        const uint32_t lw = N[3];
        const bool is_leaf = (int32_t)lw < 0;
        out.push_back({node, skip, !skip && is_leaf ? (lw >> 16) & 0x7FFFu : 0u});
        node = (skip || is_leaf) ? (lw & 0xFFFFu) : (lw >> 16);
    }
    return out;
}

static void check_image(const SphereBVH &bv, const char *what) {
    const size_t nn = bv.nodes.size() / 8;
    CHECK(bv.corner.size() == nn * 32, "%s: image holds %zu words for %zu nodes\n", what, bv.corner.size(), nn);
    if (bv.corner.size() != nn * 32) return;
    for (size_t n = 0; n < nn; ++n) {
        const float *B = &bv.nodes[n * 8];
        const uint32_t a = bits(B[3]), b = bits(B[7]);
        const bool leaf = (a & kLeafBit) != 0;
        for (uint32_t o = 0; o < 8; ++o) {
            const uint32_t *S = &bv.corner[n * 32 + o * 4], *Fc = &bv.corner[n * 32 + (7 - o) * 4];
            for (int k = 0; k < 3; ++k) {
                const bool neg = (o >> k) & 1u;
                CHECK(S[k] == bits(neg ? B[4 + k] : B[k]), "%s: node %zu slot %u axis %d is not the near corner\n",
                      what, n, o, k);
                CHECK(Fc[k] == bits(neg ? B[k] : B[4 + k]), "%s: node %zu slot %u axis %d is not the far corner\n",
                      what, n, 7 - o, k);
            }
            const uint32_t miss = S[3] & 0xFFFFu, next = S[3] >> 16;
            CHECK(miss < nn || miss == kCornerEnd, "%s: node %zu oct %u miss link %u\n", what, n, o, miss);
            CHECK(miss == (bv.miss[n * 8 + o] == kNodeEnd ? kCornerEnd : bv.miss[n * 8 + o]),
                  "%s: node %zu oct %u miss link differs from the tree's\n", what, n, o);
            if (leaf) {
                CHECK((next & kCornerLeaf) != 0 && ((next & 0x7FFFu) >> 3) == (a & ~kLeafBit) && (next & 7u) == b,
                      "%s: leaf %zu oct %u word %#x is not (first %u, count %u)\n", what, n, o, next,
                      a & ~kLeafBit, b);
            } else {
                CHECK(next < nn && next == a + ((o >> b) & 1u), "%s: node %zu oct %u next link %u\n", what, n, o, next);
            }
        }
    }
}

static size_t check_rays(const SphereBVH &bv, uint64_t seed, size_t nrays, const char *what) {
    const size_t nn = bv.nodes.size() / 8;
    Rng g{seed | 1};
    std::vector<uint32_t> leaves;
    for (size_t n = 0; n < nn; ++n)
        if (bits(bv.nodes[n * 8 + 3]) & kLeafBit) leaves.push_back((uint32_t)n);
    const float *R = &bv.nodes[0];  // the root box
    size_t steps = 0;
    const float tiny[] = {1e-25f, -3e-30f, 1e-40f, -1e-44f, 9e-21f};
    for (size_t i = 0; i < nrays; ++i) {
        Ray r;
        if (i % 4 == 3) {  // inside a leaf box
            const float *B = &bv.nodes[(size_t)leaves[g.below((uint32_t)leaves.size())] * 8];
            for (int k = 0; k < 3; ++k) r.o[k] = B[k] + (B[4 + k] - B[k]) * g.range(0.05f, 0.95f);
        } else {
            for (int k = 0; k < 3; ++k) {
                const float w = R[4 + k] - R[k] + 1.0f;
                r.o[k] = g.range(R[k] - 0.5f * w, R[4 + k] + 0.5f * w);
            }
        }
        float len = 0;
        for (int k = 0; k < 3; ++k) { r.d[k] = g.range(-1.0f, 1.0f); len += r.d[k] * r.d[k]; }
        len = std::sqrt(len) > 0 ? std::sqrt(len) : 1.0f;
        for (int k = 0; k < 3; ++k) r.d[k] /= len;
        const uint32_t kind = (uint32_t)(i % 8);
        const int k0 = (int)g.below(3), k1 = (k0 + 1 + (int)g.below(2)) % 3;
        if (kind == 1) r.d[k0] = g.below(2) ? 0.0f : -0.0f;
        if (kind == 2) { r.d[k0] = g.below(2) ? 0.0f : -0.0f; r.d[k1] = g.below(2) ? 0.0f : -0.0f; }
        if (kind == 5) r.d[k0] = tiny[g.below(5)];
        if (kind == 6) { r.d[k0] = tiny[g.below(5)]; r.d[k1] = g.below(2) ? 0.0f : -0.0f; }
        float inv[3];
        for (int k = 0; k < 3; ++k) inv[k] = slab_rcp(r.d[k]);
        const uint32_t oct = (inv[0] < 0.0f ? 1u : 0u) | (inv[1] < 0.0f ? 2u : 0u) | (inv[2] < 0.0f ? 4u : 0u);
        const float bts[2] = {INFINITY, g.range(0.002f, 2.0f * (R[4] - R[0] + 1.0f))};
        for (float best_t : bts)
            for (int full = 0; full < 2; ++full) {
                const float e = inflation(bv, r, best_t, full != 0);
                const std::vector<Step> a = walk_box(bv, r, inv, oct, e, best_t);
                const std::vector<Step> b = walk_corner(bv, r, inv, oct, e, best_t);
                CHECK(a.size() == b.size(), "%s: ray %zu visits %zu nodes (box) vs %zu (corner)\n", what, i, a.size(),
                      b.size());
                CHECK(a.size() <= nn, "%s: ray %zu walks %zu nodes of %zu\n", what, i, a.size(), nn);
                for (size_t k = 0; k < a.size() && k < b.size(); ++k) {
                    const bool same = a[k].node == b[k].node && a[k].skip == b[k].skip && a[k].leaf == b[k].leaf;
                    CHECK(same, "%s: ray %zu step %zu: box (node %u skip %d leaf %#x) corner (node %u skip %d leaf %#x)\n",
                          what, i, k, a[k].node, (int)a[k].skip, a[k].leaf, b[k].node, (int)b[k].skip, b[k].leaf);
                    if (!same) break;
                }
                steps += a.size();
            }
    }
    return steps;
}

static std::vector<Sphere> random_set(uint64_t seed, uint32_t n, float spread, float radius, const float off[3],
                                      uint32_t dup, bool big) {
    Rng g{seed * 0x9E3779B97F4A7C15ull | 1};
    std::vector<Sphere> s;
    if (big) s.push_back({{off[0], off[1] - 1000.0f, off[2]}, 999.0f, 0});
    const size_t first = s.size();
    for (uint32_t i = 0; i < n; ++i) {
        Sphere q;
        q.center = {off[0] + g.range(-spread, spread), off[1] + g.range(-spread, spread),
                    off[2] + g.range(-spread, spread) - spread - 2.0f};
        q.radius = radius * g.range(0.3f, 1.0f);
        q.material = 0;
        s.push_back(q);
    }
    for (uint32_t i = 0; i < dup; ++i) s.push_back(s[first + i]);  // exact duplicates
    return s;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: corner_image_check scene.txt [budget] | --random\n"); return 2; }
    size_t trees = 0, steps = 0;
    if (std::strcmp(argv[1], "--random") != 0) {
        std::ifstream fh(argv[1]);
        std::stringstream ss;
        ss << fh.rdbuf();
        SceneModel s;
        if (parse_scene(ss.str(), s) != kParseOk) { std::printf("parse error\n"); return 2; }
        const SphereBVH bv = build_sphere_bvh(s.spheres, 2);
        CHECK(!bv.corner.empty(), "file: no corner image\n");
        if (bv.corner.empty()) return 1;
        check_image(bv, "file");
        steps += check_rays(bv, 0x2547549, 4000, "file");
        ++trees;
        const size_t bytes = bv.corner.size() * 4 + bv.prim_id.size() * 20;
        std::printf("nodes %zu prims %zu image+prims+ids %zu B\n", bv.nodes.size() / 8, bv.prim_id.size(), bytes);
        if (argc > 2 && std::strcmp(argv[2], "budget") == 0)
            CHECK(bytes <= 81920, "file: %zu B do not fit 81,920 B\n", bytes);
    } else {
        const float zero[3] = {0, 0, 0}, far[3] = {3000.0f, -2000.0f, 1500.0f};
        struct Case { uint32_t n; float spread, radius; const float *off; uint32_t dup; bool big; };
        const Case cases[] = {
            {20, 2.0f, 0.5f, zero, 0, true},     {77, 4.0f, 0.4f, zero, 0, false},
            {200, 5.0f, 0.4f, far, 0, true},     {300, 3.0f, 0.6f, zero, 40, true},
            {333, 6.0f, 0.3f, zero, 333, false}, {480, 20.0f, 0.05f, zero, 0, true},
        };
        uint64_t seed = 1;
        for (const Case &c : cases) {
            const std::vector<Sphere> s = random_set(seed, c.n, c.spread, c.radius, c.off, c.dup, c.big);
            const SphereBVH bv = build_sphere_bvh(s, 2);
            char what[64];
            std::snprintf(what, sizeof what, "random n=%u dup=%u", c.n, c.dup);
            CHECK(!bv.corner.empty(), "%s: no corner image\n", what);
            if (bv.corner.empty()) continue;
            check_image(bv, what);
            steps += check_rays(bv, 77 * seed, 2500, what);
            ++trees;
            ++seed;
        }
    }
    if (fails) { std::printf("FAILED: %d checks\n", fails); return 1; }
    std::printf("OK trees %zu node visits %zu\n", trees, steps);
    return 0;
}
