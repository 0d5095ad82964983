// guard_mix_check.hip -- csrc/exactdiv.h's xdivide3, xunit3 and xsqrt in waves
// whose lanes mix guard outcomes, on gfx950.
//
// Each helper computes its fast sequence in every lane and reaches HIP's
// divide / sqrtf through one wave-wide test, selecting per lane inside that
// block.  A wave where some lanes are inside the guards and some outside is
// the case an all-or-nothing check (tools/exactdiv_check.hip) never runs.
//
// One wave (a 64-thread block) per (lane pattern, edge value) pair:
//   lane patterns: no lane out of range; exactly one, at lane 0, 31, 32, 63;
//                  alternating lanes; every lane;
//   xdivide3:      denominator 2^-41, 2^41, 0, -0, +inf, NaN; a numerator
//                  component of 2^-61 beside ordinary ones; a numerator sum
//                  >= 2^60;
//   xunit3:        the same eight as vectors (length 2^-41, 2^41, 0 from +0 and
//                  from -0 components, +inf, NaN, a 2^-61 component, a sum of
//                  magnitudes >= 2^60);
//   xsqrt:         0, -0, 2^-97, 2^-96, the smallest normal, a denormal, a
//                  negative value, NaN.
// Lanes inside the guards hold random finite operands.  Every result is
// compared on raw bits (NaN equal to NaN) with the plain form on the device
// (`/`, sqrtf, no contraction) and with IEEE float division and sqrtf on the
// host.  Prints the mismatch counts and exits 1 on any.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -I../rust-swift-raytracer_amd/csrc
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exactdiv.h"

#pragma clang fp contract(off)

using namespace rtamd;

#define CHECK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(2);                                                                  \
        }                                                                             \
    } while (0)

constexpr uint32_t kLanes = 64, kPatterns = 7, kEdges = 8;
constexpr uint32_t kWaves = kPatterns * kEdges, kN = kWaves * kLanes;

// in:  div (x, y, z, b) | unit (x, y, z, -) | sqrt (a, -, -, -), 4 floats each, per element
// out: fast and plain results, 7 floats each: div xyz, unit xyz, sqrt
__global__ void __launch_bounds__(64) mix_kernel(const float4 *din, const float4 *uin, const float *sin,
                                                 float *fast, float *plain, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;  // (n is a multiple of 64: whole waves)
    const float4 d = din[i], u = uin[i];
    const float a = sin[i];
    float dx = d.x, dy = d.y, dz = d.z;
    xdivide3(dx, dy, dz, d.w);
    float ux = u.x, uy = u.y, uz = u.z;
    xunit3(ux, uy, uz);
    float *f = fast + 7u * i, *p = plain + 7u * i;
    f[0] = dx; f[1] = dy; f[2] = dz;
    f[3] = ux; f[4] = uy; f[5] = uz;
    f[6] = xsqrt(a);
    p[0] = d.x / d.w; p[1] = d.y / d.w; p[2] = d.z / d.w;
    const float len = __builtin_sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z);
    p[3] = u.x / len; p[4] = u.y / len; p[5] = u.z / len;
    p[6] = __builtin_sqrtf(a);
}

static uint32_t xs32(uint32_t &s) {
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}
// a finite value of random sign with magnitude in [2^lo, 2^hi)
static float rnd(uint32_t &s, int lo, int hi, bool positive = false) {
    const uint32_t e = (uint32_t)(127 + lo) + xs32(s) % (uint32_t)(hi - lo);
    const uint32_t bits = (positive ? 0u : (xs32(s) & 0x80000000u)) | (e << 23) | (xs32(s) & 0x7FFFFFu);
    float f;
    memcpy(&f, &bits, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits_of(a) == bits_of(b); }

static bool lane_out(uint32_t pattern, uint32_t lane) {
    switch (pattern) {
        case 0: return false;
        case 1: return lane == 0;
        case 2: return lane == 31;
        case 3: return lane == 32;
        case 4: return lane == 63;
        case 5: return (lane & 1u) != 0;
        default: return true;
    }
}

int main() {
    const float inf = INFINITY, nan = NAN;
    const float den_edge[6] = {0x1p-41f, 0x1p41f, 0.0f, -0.0f, inf, nan};
    const float unit_edge[kEdges][3] = {
        {0x1p-41f, 0.0f, 0.0f}, {0.0f, -0x1p41f, 0.0f}, {0.0f, 0.0f, 0.0f}, {-0.0f, -0.0f, -0.0f},
        {1.0f, inf, -2.0f},     {0.5f, 1.0f, nan},      {0x1p-61f, 1.0f, -2.0f}, {0x1p60f, -0x1p59f, 1.0f}};
    float denormal, min_normal;
    {
        const uint32_t d = 0x00012345u, m = 0x00800000u;
        memcpy(&denormal, &d, 4);
        memcpy(&min_normal, &m, 4);
    }
    const float sqrt_edge[kEdges] = {0.0f, -0.0f, 0x1p-97f, 0x1p-96f, min_normal, denormal, -2.25f, nan};

    std::vector<float> din(4 * kN), uin(4 * kN), sin(kN);
    uint32_t s = 2547549u, nout = 0;
    for (uint32_t w = 0; w < kWaves; ++w) {
        const uint32_t pattern = w / kEdges, edge = w % kEdges;
        for (uint32_t l = 0; l < kLanes; ++l) {
            const uint32_t i = w * kLanes + l;
            // ordinary operands: inside every guard
            float *d = &din[4 * i], *u = &uin[4 * i];
            d[0] = rnd(s, -10, 10); d[1] = rnd(s, -10, 10); d[2] = rnd(s, -10, 10);
            d[3] = rnd(s, -20, 20, true);
            u[0] = rnd(s, -10, 10); u[1] = rnd(s, -10, 10); u[2] = rnd(s, -10, 10);
            u[3] = 0.0f;
            sin[i] = rnd(s, -96, 100, true);
            if (!lane_out(pattern, l)) continue;
            ++nout;
            if (edge < 6) d[3] = den_edge[edge];
            else if (edge == 6) d[l % 3] = 0x1p-61f;
            else d[l % 3] = 0x1p60f;
            // (the edge component takes each position in turn)
            for (uint32_t k = 0; k < 3; ++k) u[(k + l) % 3] = unit_edge[edge][k];
            sin[i] = sqrt_edge[edge];
        }
    }

    float4 *ddin, *duin;
    float *dsin, *dfast, *dplain;
    CHECK(hipMalloc(&ddin, kN * 16));
    CHECK(hipMalloc(&duin, kN * 16));
    CHECK(hipMalloc(&dsin, kN * 4));
    CHECK(hipMalloc(&dfast, kN * 28));
    CHECK(hipMalloc(&dplain, kN * 28));
    CHECK(hipMemcpy(ddin, din.data(), kN * 16, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(duin, uin.data(), kN * 16, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dsin, sin.data(), kN * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(dfast, 0xEE, kN * 28));
    CHECK(hipMemset(dplain, 0xDD, kN * 28));
    hipLaunchKernelGGL(mix_kernel, dim3(kWaves), dim3(kLanes), 0, 0, ddin, duin, dsin, dfast, dplain, kN);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<float> fast(7 * kN), plain(7 * kN);
    CHECK(hipMemcpy(fast.data(), dfast, kN * 28, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(plain.data(), dplain, kN * 28, hipMemcpyDeviceToHost));

    static const char *names[3] = {"divide_by", "unit", "xsqrt"};
    unsigned long long bad_plain[3] = {0, 0, 0}, bad_host[3] = {0, 0, 0};
    long first = -1;
    for (uint32_t i = 0; i < kN; ++i) {
        const float *d = &din[4 * i], *u = &uin[4 * i];
        float host[7];
        // volatile: each operation rounds to float on its own
        volatile float n = u[0] * u[0];
        volatile float t = u[1] * u[1];
        n = n + t;
        t = u[2] * u[2];
        n = n + t;
        const float len = sqrtf(n);
        for (int k = 0; k < 3; ++k) {
            host[k] = d[k] / d[3];
            host[3 + k] = u[k] / len;
        }
        host[6] = sqrtf(sin[i]);
        for (int k = 0; k < 7; ++k) {
            const int op = k < 3 ? 0 : k < 6 ? 1 : 2;
            const bool okp = same(fast[7 * i + k], plain[7 * i + k]);
            const bool okh = same(fast[7 * i + k], host[k]);
            bad_plain[op] += !okp;
            bad_host[op] += !okh;
            if ((!okp || !okh) && first < 0) {
                first = (long)i;
                printf("first mismatch: element %u (wave %u = pattern %u edge %u, lane %u) %s[%d]: helper 0x%08x "
                       "device plain 0x%08x host 0x%08x\n", i, i / kLanes, i / kLanes / kEdges, i / kLanes % kEdges,
                       i % kLanes, names[op], k - 3 * op, bits_of(fast[7 * i + k]), bits_of(plain[7 * i + k]),
                       bits_of(host[k]));
            }
        }
    }
    printf("%u waves (%u lane patterns x %u edge values), %u of %u lanes outside the guards\n", kWaves, kPatterns,
           kEdges, nout, kN);
    bool ok = true;
    for (int op = 0; op < 3; ++op) {
        printf("%s: %llu mismatches with the device's plain form, %llu with the host\n", names[op], bad_plain[op],
               bad_host[op]);
        ok = ok && bad_plain[op] == 0 && bad_host[op] == 0;
    }
    printf("%s\n", ok ? "guard_mix OK" : "guard_mix FAILED");
    return ok ? 0 : 1;
}
