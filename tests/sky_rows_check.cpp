// sky_rows_check.cpp -- host check of the sky-row classifier (bvh.cpp
// classify_sky_rows; CPU test driver for tests/test_sky_rows_host.py).  For
// every pixel of every row the classifier calls sky, primary rays are built
// with the reference's f32 arithmetic (common.rs:335-336, camera.rs:84-89,
// maths.rs:111-118) at the pixel's corners, along its edges and at 1000 random
// positions -- the extremes 2^-32 and 1.0 of random_f32 included, the latter
// rounding to the next column or row -- and tested against every sphere of the
// scene with Sphere::hit (common.rs:74-92, t in (0.001, inf)).  No ray of a
// sky row may hit.  Prints "OK top <n> bottom <n> rays <n>" or the first
// failures and exits non-zero.
// usage: sky_rows_check scene.txt W H [12 camera floats: origin, lower_left, horizontal, vertical]
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// Sphere::hit with t_min = 0.001, t_max = inf (the direction is an NVec3: a = 1.0)
static bool sphere_hit(const Sphere &s, const Vec3 &o, float dx, float dy, float dz) {
    const float ox = o.x - s.center.x, oy = o.y - s.center.y, oz = o.z - s.center.z;
    const float a = 1.0f;
    const float hb = (ox * dx + oy * dy) + oz * dz;
    const float c = ((ox * ox + oy * oy) + oz * oz) - s.radius * s.radius;
    const float disc = hb * hb - a * c;
    if (disc < 0.0f) return false;
    const float sq = std::sqrt(disc);
    const float r1 = (-hb - sq) / a, r2 = (-hb + sq) / a;
    return (0.001f < r1 && r1 < INFINITY) || (0.001f < r2 && r2 < INFINITY);
}

int main(int argc, char **argv) {
    if (argc != 4 && argc != 16) return 2;
    std::ifstream fh(argv[1]);
    std::stringstream ss;
    ss << fh.rdbuf();
    SceneModel scene;
    if (parse_scene(ss.str(), scene) != kParseOk) return 2;
    const size_t W = (size_t)std::atoi(argv[2]), H = (size_t)std::atoi(argv[3]);
    CameraModel cam = scene.camera;
    if (argc == 16) {
        float c[12];
        for (int k = 0; k < 12; ++k) c[k] = std::strtof(argv[4 + k], nullptr);
        cam = CameraModel{{c[0], c[1], c[2]}, {c[3], c[4], c[5]}, {c[6], c[7], c[8]}, {c[9], c[10], c[11]}};
    }
    const SphereBVH bv = build_sphere_bvh(scene.spheres, 2);
    const SkyRows sky = classify_sky_rows(bv, scene.spheres, cam, W, H);
    if ((size_t)sky.top + sky.bottom > H) {
        std::printf("top %u + bottom %u rows of %zu\n", sky.top, sky.bottom, H);
        return 1;
    }
    const float wden = (float)(W - 1), hden = (float)(H - 1);
    // positions: 4 corners, 4 x 16 along the edges, 1000 random
    const float lo = 0x1p-32f, hi = 1.0f;
    std::vector<float> pu, pv;
    for (float a : {lo, hi})
        for (float b : {lo, hi}) pu.push_back(a), pv.push_back(b);
    for (int k = 1; k <= 16; ++k) {
        const float m = (float)k / 17.0f;
        pu.push_back(m); pv.push_back(lo);
        pu.push_back(m); pv.push_back(hi);
        pu.push_back(lo); pv.push_back(m);
        pu.push_back(hi); pv.push_back(m);
    }
    const size_t fixed = pu.size();
    uint32_t seed = 2547549u;
    size_t rays = 0, fails = 0;
    for (size_t ir = 0; ir < H; ++ir) {
        if (!(ir < sky.top || ir >= H - sky.bottom)) continue;  // ir counts from the top
        const size_t row = H - 1 - ir;                          // rows count from the bottom (common.rs:327)
        for (size_t col = 0; col < W; ++col)
            for (size_t k = 0; k < fixed + 1000; ++k) {
                const float r1 = k < fixed ? pu[k] : (float)xs32(seed) * 0x1p-32f;
                const float r2 = k < fixed ? pv[k] : (float)xs32(seed) * 0x1p-32f;
                const float u = ((float)col + r1) / wden, v = ((float)row + r2) / hden;
                const Vec3 o = cam.origin, l = cam.lower_left, h = cam.horizontal, vv = cam.vertical;
                float dx = ((l.x + h.x * u) + vv.x * v) - o.x;
                float dy = ((l.y + h.y * u) + vv.y * v) - o.y;
                float dz = ((l.z + h.z * u) + vv.z * v) - o.z;
                const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
                dx = dx / len; dy = dy / len; dz = dz / len;
                ++rays;
                for (size_t i = 0; i < scene.spheres.size(); ++i)
                    if (sphere_hit(scene.spheres[i], o, dx, dy, dz) && fails++ < 10)
                        std::printf("sky row %zu (from the top), col %zu, position %zu: sphere %zu is hit\n", ir, col,
                                    k, i);
            }
    }
    if (fails) return 1;
    std::printf("OK top %u bottom %u rays %zu\n", sky.top, sky.bottom, rays);
    return 0;
}
