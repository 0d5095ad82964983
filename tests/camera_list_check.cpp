// camera_list_check.cpp -- host check of both primary-ray list builders under
// an arbitrary camera (bvh.cpp build_primary_sphere_lists and
// build_primary_tri_lists; CPU test driver for tests/test_camera_lists_host.py,
// the oriented-camera companion of sphere_list_check.cpp).
//
// For every pixel of a W x H frame and eight sub-pixel offsets (the extremes
// 2^-32 and 1.0 of random_f32 included) the primary ray is built with the
// reference's f32 arithmetic (common.rs:335-336, camera.rs:84-89,
// maths.rs:111-118).  Spheres: every tree sphere that yields a candidate root
// (common.rs:74-92) must be on the pixel's list, unless the pixel walks.
// Triangles: every camera-origin record whose padded phantom box the ray meets
// (a slab test in double, t >= 0) must be on the pixel's strip list or on
// `always`.  Prints one line per builder, "spheres OK ..." / "spheres no lists"
// and "triangles OK ..." / "triangles no lists" / "triangles no tree", or the
// first failures, and exits non-zero on a failure.
// usage: camera_list_check scene.txt W H c0 ... c11
//        (rt_camera_get's 12 floats, each as the 8 hex digits of its bits)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <vector>

#include "bvh.h"
#include "scene.h"

#pragma STDC FP_CONTRACT OFF

using namespace rtamd;

static uint32_t xs32(uint32_t &s) {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}

struct Ray { float o[3], d[3]; };

// the k-th test ray of pixel (col, row counted from the bottom)
static Ray primary_ray(const CameraModel &cam, size_t col, size_t row, float wden, float hden, int k, uint32_t &seed) {
    const float offs[3] = {0x1p-32f, 1.0f, 0.5f};
    const float r1 = k < 3 ? offs[k] : (float)xs32(seed) * 0x1p-32f;
    const float r2 = k < 3 ? offs[2 - k] : (float)xs32(seed) * 0x1p-32f;
    const float u = ((float)col + r1) / wden, v = ((float)row + r2) / hden;
    const Vec3 o = cam.origin, l = cam.lower_left, h = cam.horizontal, vv = cam.vertical;
    float dx = ((l.x + h.x * u) + vv.x * v) - o.x;
    float dy = ((l.y + h.y * u) + vv.y * v) - o.y;
    float dz = ((l.z + h.z * u) + vv.z * v) - o.z;
    const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
    return Ray{{o.x, o.y, o.z}, {dx / len, dy / len, dz / len}};
}

// does the ray o + t d, t >= 0, meet the box [lo, hi]?  (double slabs; a NaN
// direction meets everything: such a pixel must not lose a record)
static bool meets(const Ray &r, const float *b) {
    double t0 = 0.0, t1 = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const double o = r.o[a], d = r.d[a], lo = b[a], hi = b[3 + a];
        if (std::isnan(d)) return true;
        if (d == 0.0) {
            if (o < lo || o > hi) return false;
            continue;
        }
        double ta = (lo - o) / d, tb = (hi - o) / d;
        if (ta > tb) std::swap(ta, tb);
        t0 = std::max(t0, ta);
        t1 = std::min(t1, tb);
    }
    return t0 <= t1;
}

static int check_spheres(const SceneModel &scene, const CameraModel &cam, size_t W, size_t H) {
    const SphereBVH bv = build_sphere_bvh(scene.spheres, 2);
    const PrimarySphereLists L = build_primary_sphere_lists(bv, cam, W, H);
    if (L.rec.empty()) {
        std::printf("spheres no lists\n");
        return 0;
    }
    const size_t n = bv.prims.size() / 4;
    const float wden = (float)(W - 1), hden = (float)(H - 1);
    uint32_t seed = 2547549u;
    size_t rays = 0, hits = 0, walk = 0, listed = 0, fails = 0;
    for (size_t ir = 0; ir < H; ++ir) {
        const size_t row = H - 1 - ir;  // rows count from the bottom (common.rs:327)
        for (size_t col = 0; col < W; ++col) {
            const uint32_t a = L.rec[2 * (ir * W + col)], b = L.rec[2 * (ir * W + col) + 1];
            const uint32_t cnt = b >> 16;
            if (cnt == kSphListWalk) { ++walk; continue; }
            listed += cnt;
            const uint32_t item[3] = {a & 0xFFFFu, a >> 16, b & 0xFFFFu};
            for (int k = 0; k < 8; ++k) {
                const Ray r = primary_ray(cam, col, row, wden, hden, k, seed);
                ++rays;
                for (size_t i = 0; i < n; ++i) {
                    const float *s = &bv.prims[4 * i];
                    const float ox = r.o[0] - s[0], oy = r.o[1] - s[1], oz = r.o[2] - s[2];
                    const float hb = (ox * r.d[0] + oy * r.d[1]) + oz * r.d[2];
                    const float cc = ((ox * ox + oy * oy) + oz * oz) - s[3];
                    const float disc = hb * hb - cc;
                    if (!(disc >= 0.0f)) continue;
                    const float sq = std::sqrt(disc);
                    if (!(0.001f < -hb - sq) && !(0.001f < -hb + sq)) continue;
                    ++hits;
                    bool in = false;
                    for (uint32_t j = 0; j < cnt; ++j) in |= item[j] == i;
                    if (!in && fails++ < 10)
                        std::printf("pixel (%zu, %zu) offset %d: tree sphere %zu has a candidate but is not listed\n",
                                    col, ir, k, i);
                }
            }
        }
    }
    if (fails) return 1;
    std::printf("spheres OK rays %zu candidates %zu walk-pixels %zu listed %zu\n", rays, hits, walk, listed);
    return 0;
}

static int check_triangles(const SceneModel &scene, const CameraModel &cam, size_t W, size_t H) {
    const PackedScene packed = pack_scene(scene, 8, 1);
    const TriangleBVH tb = build_triangle_bvh(scene.triangles, packed.tri_hot, 1);
    if (tb.nodes.empty()) {
        std::printf("triangles no tree\n");
        return 0;
    }
    const float o[3] = {cam.origin.x, cam.origin.y, cam.origin.z};
    const CameraTriangleBVH ct = build_camera_triangle_bvh(scene.triangles, packed.tri_hot, tb, o, 2, false);
    const PrimaryTriLists L = build_primary_tri_lists(ct, cam, W, H);
    if (L.offsets.empty()) {
        std::printf("triangles no lists\n");
        return 0;
    }
    const size_t n = ct.rec_box.size() / 6, spr = L.strips_per_row;
    if (L.offsets.size() != spr * H + 1 || L.offsets.back() > L.items.size()) {
        std::printf("triangles: offsets of %zu entries for %zu strips\n", L.offsets.size(), spr * H);
        return 1;
    }
    size_t fails = 0;
    // the shape the device build must reproduce: ascending within a strip and in `always`
    for (size_t c = 0; c < spr * H; ++c)
        for (uint32_t j = L.offsets[c] + 1; j < L.offsets[c + 1]; ++j)
            if (L.items[j - 1] >= L.items[j] && fails++ < 10) std::printf("strip %zu is not ascending\n", c);
    for (size_t j = L.offsets.back() + 1; j < L.items.size(); ++j)
        if (L.items[j - 1] >= L.items[j] && fails++ < 10) std::printf("`always` is not ascending\n");
    std::vector<uint8_t> always(n, 0), in(n, 0);
    for (size_t j = L.offsets.back(); j < L.items.size(); ++j) always[L.items[j]] = 1;
    const float wden = (float)(W - 1), hden = (float)(H - 1);
    uint32_t seed = 2547549u;
    size_t rays = 0, met = 0;
    for (size_t row = 0; row < H; ++row) {  // counted from the bottom, as the lists' rows are
        for (size_t col = 0; col < W; ++col) {
            const size_t cell = row * spr + col / kTriStripW;
            for (uint32_t j = L.offsets[cell]; j < L.offsets[cell + 1]; ++j) in[L.items[j]] = 1;
            for (int k = 0; k < 8; ++k) {
                const Ray r = primary_ray(cam, col, row, wden, hden, k, seed);
                ++rays;
                for (size_t i = 0; i < n; ++i) {
                    if (in[i] || always[i] || !meets(r, &ct.rec_box[i * 6])) continue;
                    if (fails++ < 10)
                        std::printf("pixel (%zu, bottom row %zu) offset %d: the ray meets record %zu's box, "
                                    "which is not listed\n", col, row, k, i);
                }
                for (size_t i = 0; i < n; ++i) met += (in[i] || always[i]) && meets(r, &ct.rec_box[i * 6]);
            }
            for (uint32_t j = L.offsets[cell]; j < L.offsets[cell + 1]; ++j) in[L.items[j]] = 0;
        }
    }
    if (fails) return 1;
    std::printf("triangles OK rays %zu met %zu records %zu listed %u always %zu\n", rays, met, n, L.offsets.back(),
                L.items.size() - L.offsets.back());
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 16) return 2;
    std::ifstream fh(argv[1]);
    std::stringstream ss;
    ss << fh.rdbuf();
    SceneModel scene;
    if (parse_scene(ss.str(), scene) != kParseOk) return 2;
    const size_t W = (size_t)std::atoi(argv[2]), H = (size_t)std::atoi(argv[3]);
    float c[12];
    for (int k = 0; k < 12; ++k) {  // the floats' bits, as 8 hex digits each
        const uint32_t u = (uint32_t)std::strtoul(argv[4 + k], nullptr, 16);
        std::memcpy(&c[k], &u, 4);
    }
    CameraModel cam;
    cam.origin = {c[0], c[1], c[2]};
    cam.lower_left = {c[3], c[4], c[5]};
    cam.horizontal = {c[6], c[7], c[8]};
    cam.vertical = {c[9], c[10], c[11]};
    int rc = check_spheres(scene, cam, W, H);
    rc |= check_triangles(scene, cam, W, H);
    return rc;
}
