// sbvh_sim.cpp -- host emulation of the sphere-tree walk (tuning tool).
// Walks the stackless octant-linked sphere BVH (bvh.h SphereBVH) the way
// render.hip does for rays of a scene -- primary rays of a W x H grid and
// diffuse bounces from their hits -- and reports the distribution of node
// visits per walk and what a 64-lane wave pays for it: a walk loop runs until
// its longest walk ends, so the wave's cost is the max over its lanes.
// Not product code, not a parity check (double arithmetic, no inflation).
//   g++ -O2 -std=c++17 -I../rust-swift-raytracer_amd/csrc sbvh_sim.cpp \
//       ../rust-swift-raytracer_amd/csrc/{bvh,scene}.cpp -o sbvh_sim -lpthread
//   ./sbvh_sim ../scenes/rtow.txt [W H [S]] (S samples per pixel, pixel-major like
//   the kernel's jobs, default 1; RT_AMD_LEAF: leaf size, default 3;
//   SIM_BVH4=1: node fetches and box tests of the tree collapsed to 4-wide nodes)
// SIM_WAVE=1: lock-step wave cost of the walk loop.  The walks of one bounce
// (SIM_WAVE_BOUNCE, default 1) are recorded visit by visit -- started at the
// root's near child like the LDS walks -- and replayed 64 consecutive walks
// per wave the way the kernel's loop runs them: one node step per trip for
// the lanes still walking, and in trips where some lane entered a leaf the
// leaf code, sphere by sphere: a discriminant for the lanes whose leaf holds
// that sphere, a root-and-merge pass when one of them is >= 0.  Reports trips,
// leaf trips, lanes per leaf trip, root passes and a VALU estimate per wave
// walk from per-step costs read off the compiled kernel (SIM_COST_NODE 16,
// SIM_COST_LEAF 19 per discriminant, SIM_COST_ROOT 22 per root-and-merge
// pass, SIM_COST_SELECT 4), for the loop as it is and for two variants:
//   merged roots: all of a leaf's discriminants first, then one root pass for
//     each lane's first sphere with a root (+ the selects) and further passes
//     only while some lane has another;
//   gated leaf tests (SIM_WAVE_GATE=T, default 1 2 4 8 16 32): lanes that
//     entered a leaf wait until T lanes have or no lane can step without one;
//     every loop trip then also pays the gate's own VALU (SIM_COST_GATE 3:
//     two selects that hold the leaf word and the pending flag, the compare
//     behind the ballot).
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

using namespace rtamd;

struct V { double x, y, z; };
static V add(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V sub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V mul(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V unit(V a) { return mul(a, 1.0 / std::sqrt(dot(a, a))); }

struct Hit { double t = INFINITY; int id = -1; };

static double sphere_t(V o, V d, const float *s) {  // (cx, cy, cz, r^2), |d| = 1
    V oc = sub(o, V{s[0], s[1], s[2]});
    const double hb = dot(oc, d), c = dot(oc, oc) - s[3], disc = hb * hb - c;
    if (disc < 0) return INFINITY;
    const double q = std::sqrt(disc), r1 = -hb - q, r2 = -hb + q;
    return r1 > 1e-3 ? r1 : r2 > 1e-3 ? r2 : INFINITY;
}

// the kernel's walk: big spheres, then the tree from the root along the
// octant links; returns node visits
// ev (SIM_WAVE): one byte per visit, the entered leaf's sphere count (0: none)
// | a bit per sphere with a discriminant >= 0 << 3; the walk then starts at
// the root's near child
static int walk(const SphereBVH &b, const std::vector<float> &hot, V o, V d, Hit &h,
                std::vector<uint8_t> *ev = nullptr) {
    for (uint32_t i : b.big) {
        const double t = sphere_t(o, d, &hot[(size_t)i * 4]);
        if (t < h.t) { h.t = t; h.id = (int)i; }
    }
    const double inv[3] = {1 / d.x, 1 / d.y, 1 / d.z}, ov[3] = {o.x, o.y, o.z};
    const uint32_t oct = (inv[0] < 0 ? 1u : 0u) | (inv[1] < 0 ? 2u : 0u) | (inv[2] < 0 ? 4u : 0u);
    int visits = 0;
    uint32_t node = 0;
    if (ev && b.nodes.size() > 8) {
        uint32_t a, ax;
        std::memcpy(&a, &b.nodes[3], 4);
        std::memcpy(&ax, &b.nodes[7], 4);
        if (!(a & kLeafBit)) node = a + ((oct >> ax) & 1u);
    }
    while (node != kNodeEnd) {
        ++visits;
        const float *n = &b.nodes[(size_t)node * 8];
        double tn = -INFINITY, tf = INFINITY;
        for (int k = 0; k < 3; ++k) {
            const double t0 = (n[k] - ov[k]) * inv[k], t1 = (n[4 + k] - ov[k]) * inv[k];
            tn = std::max(tn, std::min(t0, t1));
            tf = std::min(tf, std::max(t0, t1));
        }
        uint32_t a, bb;
        std::memcpy(&a, &n[3], 4);
        std::memcpy(&bb, &n[7], 4);
        const bool skip = tn > tf || tf < 1e-3 || tn > h.t;
        const bool leaf = a & kLeafBit;
        uint8_t e = 0;
        if (!skip && leaf) {
            e = (uint8_t)std::min(bb, 5u);
            for (uint32_t j = a & ~kLeafBit; j < (a & ~kLeafBit) + bb; ++j) {
                const float *sp = &b.prims[(size_t)j * 4];
                const V oc = sub(o, V{sp[0], sp[1], sp[2]});
                const double hb = dot(oc, d);
                if (hb * hb - (dot(oc, oc) - sp[3]) >= 0 && j - (a & ~kLeafBit) < 5) e |= 8u << (j - (a & ~kLeafBit));
                const double t = sphere_t(o, d, sp);
                if (t < h.t) { h.t = t; h.id = (int)b.prim_id[j]; }
            }
        }
        if (ev) ev->push_back(e);
        node = (skip || leaf) ? b.miss[(size_t)node * 8 + oct] : a + ((oct >> bb) & 1u);
    }
    return visits;
}

// SIM_BVH4=1: the same tree collapsed to 4 children per node (each internal
// child replaced by its two children), walked with a stack, nearest child
// first.  Returns node fetches; box tests (children tested) go to *tests.
static int walk4(const SphereBVH &b, const std::vector<float> &hot, V o, V d, Hit &h, int *tests) {
    for (uint32_t i : b.big) {
        const double t = sphere_t(o, d, &hot[(size_t)i * 4]);
        if (t < h.t) { h.t = t; h.id = (int)i; }
    }
    const double inv[3] = {1 / d.x, 1 / d.y, 1 / d.z}, ov[3] = {o.x, o.y, o.z};
    auto box = [&](uint32_t n, double &tn) {
        const float *f = &b.nodes[(size_t)n * 8];
        double a = -INFINITY, z = INFINITY;
        for (int k = 0; k < 3; ++k) {
            const double t0 = (f[k] - ov[k]) * inv[k], t1 = (f[4 + k] - ov[k]) * inv[k];
            a = std::max(a, std::min(t0, t1));
            z = std::min(z, std::max(t0, t1));
        }
        tn = a;
        return !(a > z || z < 1e-3 || a > h.t);
    };
    auto word = [&](uint32_t n, int k) { uint32_t w; std::memcpy(&w, &b.nodes[(size_t)n * 8 + k], 4); return w; };
    auto leaf = [&](uint32_t n) {
        const uint32_t a = word(n, 3), cnt = word(n, 7);
        for (uint32_t j = a & ~kLeafBit; j < (a & ~kLeafBit) + cnt; ++j) {
            const double t = sphere_t(o, d, &b.prims[(size_t)j * 4]);
            if (t < h.t) { h.t = t; h.id = (int)b.prim_id[j]; }
        }
    };
    int fetches = 0;
    double t0;
    std::vector<std::pair<double, uint32_t>> st;
    if (!box(0, t0)) return 0;
    if (word(0, 3) & kLeafBit) { leaf(0); return 1; }
    st.push_back({t0, 0});
    while (!st.empty()) {
        auto [tn, n] = st.back();
        st.pop_back();
        if (tn > h.t) continue;
        ++fetches;
        uint32_t kids[4], nk = 0;
        const uint32_t a = word(n, 3);
        for (uint32_t c = a; c < a + 2; ++c) {
            if (word(c, 3) & kLeafBit) kids[nk++] = c;
            else { const uint32_t g = word(c, 3); kids[nk++] = g; kids[nk++] = g + 1; }
        }
        std::pair<double, uint32_t> hit[4];
        int nh = 0;
        for (uint32_t k = 0; k < nk; ++k) {
            ++*tests;
            double t;
            if (box(kids[k], t)) hit[nh++] = {t, kids[k]};
        }
        std::sort(hit, hit + nh, [](auto &x, auto &y) { return x.first > y.first; });  // nearest last
        for (int k = 0; k < nh; ++k) {
            if (word(hit[k].second, 3) & kLeafBit) continue;
            st.push_back(hit[k]);
        }
        for (int k = nh - 1; k >= 0; --k)  // leaves now, nearest first
            if (word(hit[k].second, 3) & kLeafBit) leaf(hit[k].second);
    }
    return fetches;
}

// SIM_WAVE: replays the recorded walks 64 per wave.  merged: the merged-roots
// leaf code; gate: lanes that entered a leaf wait for `gate` such lanes.
struct WaveCost { double trips = 0, leaf_trips = 0, leaf_lanes = 0, roots = 0, valu = 0; size_t waves = 0; };
static WaveCost wave_cost(const std::vector<std::vector<uint8_t>> &w, bool merged, int gate, const double c[5]) {
    WaveCost r;
    for (size_t g = 0; g + 64 <= w.size(); g += 64) {
        size_t pos[64] = {0};
        bool pend[64] = {false};
        ++r.waves;
        for (;;) {
            int act = 0, step = 0, npend = 0;
            for (int l = 0; l < 64; ++l) {
                if (pos[l] >= w[g + l].size()) continue;
                ++act;
                if (pend[l]) continue;
                ++step;
                if (w[g + l][pos[l]] & 7) pend[l] = true; else ++pos[l];
            }
            if (!act) break;
            ++r.trips;
            if (step) r.valu += c[0];
            if (gate) r.valu += c[4];
            for (int l = 0; l < 64; ++l) npend += pend[l] ? 1 : 0;
            // (the loop as it is: gate 0, every entered leaf is tested in its trip)
            if (!npend || (npend < gate && npend < act)) continue;
            ++r.leaf_trips;
            r.leaf_lanes += npend;
            int maxn = 0, maxroots = 0;
            bool root_at[5] = {false, false, false, false, false};
            for (int l = 0; l < 64; ++l) {
                if (!pend[l]) continue;
                const uint8_t e = w[g + l][pos[l]];
                maxn = std::max(maxn, e & 7);
                int nr = 0;
                for (int k = 0; k < 5; ++k)
                    if (e & (8u << k)) { root_at[k] = true; ++nr; }
                maxroots = std::max(maxroots, nr);
                pend[l] = false;
                ++pos[l];
            }
            r.valu += c[1] * maxn;
            int passes = 0;
            if (merged) {
                passes = maxroots;
                if (maxn > 1) r.valu += c[3];
            } else {
                for (int k = 0; k < maxn; ++k) passes += root_at[k] ? 1 : 0;
            }
            r.roots += passes;
            r.valu += c[2] * passes;
        }
    }
    return r;
}

// SIM_WAVE_DEFER: deferred leaf tests (trace_body.h trace_body kDefer), a true
// lock-step run of 64 consecutive walks on their own geometry -- deferral
// changes best_t and with it the cull decisions, so the recorded events do
// not do.  A lane that enters a leaf records (leaf, t_near) and walks on, at
// most C entries per lane.  The lanes flush -- test their entries pass by
// pass, every lane's r-th entry together -- as soon as one of them holds C,
// and once more when no lane can step.  join = false (the kernel): a lane
// whose walk has ended keeps its entries until that last flush; join = true:
// it takes part in every flush.  recull: at the flush an entry whose t_near
// is now > best_t is dropped untested.  A pass costs like the leaf code as it
// is (leaf cost x the largest leaf among its lanes + root cost per sphere
// position at which some lane has a discriminant >= 0) + `round`; a trip in
// which some lane records a leaf costs `push` more.  C = 1 at push = round = 0
// is the loop as it is: its line must equal wave_cost's, digit for digit.
struct DeferCost { double trips = 0, passes = 0, pass_lanes = 0, flushes = 0, roots = 0, valu = 0, visits = 0,
                   tests = 0; size_t waves = 0, walks = 0; };
struct DeferRay { V o, d; };
static DeferCost defer_cost(const SphereBVH &b, const std::vector<float> &hot, const std::vector<DeferRay> &rays,
                            int C, bool recull, bool join, const double c[5], double push, double round) {
    DeferCost r;
    struct Lane {
        V o, d; double inv[3], ov[3]; uint32_t oct, node; Hit h;
        int n; uint32_t leaf[8]; double tn[8];
    };
    for (size_t g = 0; g + 64 <= rays.size(); g += 64) {
        Lane L[64];
        ++r.waves;
        r.walks += 64;
        for (int l = 0; l < 64; ++l) {
            Lane &x = L[l];
            x.o = rays[g + l].o; x.d = rays[g + l].d; x.h = Hit{}; x.n = 0;
            for (uint32_t i : b.big) {
                const double t = sphere_t(x.o, x.d, &hot[(size_t)i * 4]);
                if (t < x.h.t) { x.h.t = t; x.h.id = (int)i; }
            }
            x.inv[0] = 1 / x.d.x; x.inv[1] = 1 / x.d.y; x.inv[2] = 1 / x.d.z;
            x.ov[0] = x.o.x; x.ov[1] = x.o.y; x.ov[2] = x.o.z;
            x.oct = (x.inv[0] < 0 ? 1u : 0u) | (x.inv[1] < 0 ? 2u : 0u) | (x.inv[2] < 0 ? 4u : 0u);
            x.node = 0;
            if (b.nodes.size() > 8) {  // (the walk starts at the root's near child, as walk() with ev)
                uint32_t a, ax;
                std::memcpy(&a, &b.nodes[3], 4);
                std::memcpy(&ax, &b.nodes[7], 4);
                if (!(a & kLeafBit)) x.node = a + ((x.oct >> ax) & 1u);
            }
        }
        // tests every taking-part lane's entries, pass by pass
        auto flush = [&](const bool *part) {
            ++r.flushes;
            for (int k = 0; k < C; ++k) {
                int lanes = 0, maxn = 0;
                bool root_at[5] = {false, false, false, false, false};
                for (int l = 0; l < 64; ++l) {
                    Lane &x = L[l];
                    if (!part[l] || k >= x.n) continue;
                    if (recull && x.tn[k] > x.h.t) continue;
                    ++lanes;
                    uint32_t bb;
                    std::memcpy(&bb, &b.nodes[(size_t)x.leaf[k] * 8 + 7], 4);
                    uint32_t a;
                    std::memcpy(&a, &b.nodes[(size_t)x.leaf[k] * 8 + 3], 4);
                    const uint32_t first = a & ~kLeafBit;
                    maxn = std::max(maxn, (int)std::min(bb, 5u));
                    for (uint32_t j = first; j < first + bb; ++j) {
                        const float *sp = &b.prims[(size_t)j * 4];
                        const V oc = sub(x.o, V{sp[0], sp[1], sp[2]});
                        const double hb = dot(oc, x.d);
                        if (hb * hb - (dot(oc, oc) - sp[3]) >= 0 && j - first < 5) root_at[j - first] = true;
                        const double t = sphere_t(x.o, x.d, sp);
                        if (t < x.h.t) { x.h.t = t; x.h.id = (int)b.prim_id[j]; }
                        ++r.tests;
                    }
                }
                if (!lanes) continue;
                ++r.passes;
                r.pass_lanes += lanes;
                int passes = 0;
                for (int q = 0; q < maxn; ++q) passes += root_at[q] ? 1 : 0;
                r.roots += passes;
                r.valu += c[1] * maxn + c[2] * passes + round;
            }
            for (int l = 0; l < 64; ++l)
                if (part[l]) L[l].n = 0;
        };
        for (;;) {
            bool part[64];
            int step = 0;
            bool rec = false, full = false;
            for (int l = 0; l < 64; ++l) {
                Lane &x = L[l];
                part[l] = join || x.node != kNodeEnd;  // (a lane that ends in this trip still takes part in its flush)
                if (x.node == kNodeEnd) continue;
                ++step;
                ++r.visits;
                const float *n = &b.nodes[(size_t)x.node * 8];
                double tn = -INFINITY, tf = INFINITY;
                for (int k = 0; k < 3; ++k) {
                    const double t0 = (n[k] - x.ov[k]) * x.inv[k], t1 = (n[4 + k] - x.ov[k]) * x.inv[k];
                    tn = std::max(tn, std::min(t0, t1));
                    tf = std::min(tf, std::max(t0, t1));
                }
                uint32_t a, bb;
                std::memcpy(&a, &n[3], 4);
                std::memcpy(&bb, &n[7], 4);
                const bool skip = tn > tf || tf < 1e-3 || tn > x.h.t;
                const bool leaf = a & kLeafBit;
                if (!skip && leaf) {
                    x.leaf[x.n] = x.node; x.tn[x.n] = tn; ++x.n;
                    rec = true;
                    full = full || x.n >= C;
                }
                x.node = (skip || leaf) ? b.miss[(size_t)x.node * 8 + x.oct] : a + ((x.oct >> bb) & 1u);
            }
            if (!step) break;
            ++r.trips;
            r.valu += c[0];
            if (rec) r.valu += push;
            if (full) flush(part);
        }
        bool all[64], any = false;
        for (int l = 0; l < 64; ++l) { all[l] = true; any = any || L[l].n; }
        if (any) flush(all);
    }
    return r;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: sbvh_sim scene.txt [W H [S]]\n"); return 2; }
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    SceneModel s;
    if (parse_scene(ss.str(), s) != kParseOk) { std::fprintf(stderr, "parse error\n"); return 1; }
    const int W = argc > 3 ? std::atoi(argv[2]) : 192, H = argc > 3 ? std::atoi(argv[3]) : 108;
    const int S = argc > 4 ? std::atoi(argv[4]) : 1;
    const char *lf = std::getenv("RT_AMD_LEAF");
    const SphereBVH b = build_sphere_bvh(s.spheres, lf ? (uint32_t)std::atoi(lf) : 3u);
    std::vector<float> hot(s.spheres.size() * 4);
    for (size_t i = 0; i < s.spheres.size(); ++i) {
        hot[i * 4] = s.spheres[i].center.x; hot[i * 4 + 1] = s.spheres[i].center.y;
        hot[i * 4 + 2] = s.spheres[i].center.z; hot[i * 4 + 3] = s.spheres[i].radius * s.spheres[i].radius;
    }
    const CameraModel &cm = s.camera;
    const V org{cm.origin.x, cm.origin.y, cm.origin.z};
    uint32_t rng = 2547549u;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5; return rng * 0x1p-32; };
    std::vector<int> vis[3];  // bounce 0, 1, 2
    const bool bvh4 = std::getenv("SIM_BVH4") != nullptr;
    std::vector<int> box4[3];  // SIM_BVH4: children tested per walk
    const bool wave = std::getenv("SIM_WAVE") != nullptr;
    const int wave_bounce = std::getenv("SIM_WAVE_BOUNCE") ? std::atoi(std::getenv("SIM_WAVE_BOUNCE")) : 1;
    std::vector<std::vector<uint8_t>> events;  // SIM_WAVE: the recorded walks
    std::vector<DeferRay> wave_rays;           // ... and their rays (SIM_WAVE_DEFER)
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W * S; ++i) {
            const int px = i / S;
            const double u = (px + rnd()) / (W - 1), v = (j + rnd()) / (H - 1);
            V o = org;
            V d = unit(sub(add(add(V{cm.lower_left.x, cm.lower_left.y, cm.lower_left.z},
                                   mul(V{cm.horizontal.x, cm.horizontal.y, cm.horizontal.z}, u)),
                               mul(V{cm.vertical.x, cm.vertical.y, cm.vertical.z}, v)), o));
            for (int bounce = 0; bounce < 3; ++bounce) {
                Hit h;
                if (bvh4) {
                    Hit h2;
                    int tests = 0;
                    vis[bounce].push_back(walk4(b, hot, o, d, h2, &tests));
                    box4[bounce].push_back(tests);
                }
                const bool rec = wave && bounce == wave_bounce;
                if (rec) events.emplace_back();
                if (rec) wave_rays.push_back({o, d});
                const int v2 = walk(b, hot, o, d, h, rec ? &events.back() : nullptr);
                if (!bvh4) vis[bounce].push_back(v2);
                if (h.id < 0) break;
                const float *c = &hot[(size_t)h.id * 4];
                const V p = add(o, mul(d, h.t));
                const V n = unit(sub(p, V{c[0], c[1], c[2]}));
                const V r = unit(V{rnd() * 2 - 1, rnd() * 2 - 1, rnd() * 2 - 1});
                o = p;
                d = unit(add(n, r));
            }
        }
    std::printf("nodes %zu leaves<=%s big %zu\n", b.nodes.size() / 8, lf ? lf : "3", b.big.size());
    if (wave) {
        auto envd = [](const char *k, double dflt) { const char *v = std::getenv(k); return v ? std::atof(v) : dflt; };
        const double c[5] = {envd("SIM_COST_NODE", 16), envd("SIM_COST_LEAF", 19), envd("SIM_COST_ROOT", 22),
                             envd("SIM_COST_SELECT", 4), envd("SIM_COST_GATE", 3)};
        double visits = 0;
        for (auto &e : events) visits += e.size();
        std::printf("wave cost, bounce %d: %zu walks, %.1f visits per walk; costs node %.0f leaf %.0f root %.0f select %.0f gate %.0f\n",
                    wave_bounce, events.size(), events.empty() ? 0.0 : visits / events.size(), c[0], c[1], c[2], c[3],
                    c[4]);
        auto line = [&](const char *name, const WaveCost &r, double base) {
            const double n = r.waves ? (double)r.waves : 1.0;
            std::printf("  %-16s trips %.1f, leaf trips %.2f with %.1f lanes, root passes %.2f, VALU %.0f per wave walk"
                        " (%+.1f%%)\n", name, r.trips / n, r.leaf_trips / n, r.leaf_trips ? r.leaf_lanes / r.leaf_trips : 0.0,
                        r.roots / n, r.valu / n, base > 0 ? 100.0 * (r.valu / n / base - 1.0) : 0.0);
        };
        const WaveCost base = wave_cost(events, false, 0, c);
        const double bv = base.waves ? base.valu / base.waves : 0.0;
        line("as it is", base, bv);
        line("merged roots", wave_cost(events, true, 0, c), bv);
        const char *gs = std::getenv("SIM_WAVE_GATE");
        for (int t : {1, 2, 4, 8, 16, 32}) {
            const int T = gs ? std::max(1, std::atoi(gs)) : t;
            char name[32];
            std::snprintf(name, sizeof name, "gated, T = %d", T);
            line(name, wave_cost(events, false, T, c), bv);
            if (gs) break;
        }
        // SIM_WAVE_DEFER=1: deferred leaf tests; SIM_DEFER_C (default: 1 2 3),
        // SIM_DEFER_RECULL (default: both), SIM_DEFER_JOIN=1 (ended lanes take
        // part in every flush), SIM_COST_PUSH / SIM_COST_ROUND (default 0)
        if (std::getenv("SIM_WAVE_DEFER")) {
            const double push = envd("SIM_COST_PUSH", 0), round = envd("SIM_COST_ROUND", 0);
            const bool join = envd("SIM_DEFER_JOIN", 0) != 0;
            const char *cs = std::getenv("SIM_DEFER_C"), *rs = std::getenv("SIM_DEFER_RECULL");
            std::printf("deferred leaves (%s), push %.0f round %.0f\n",
                        join ? "ended lanes join every flush" : "ended lanes keep their entries to the last flush",
                        push, round);
            for (int C : {1, 2, 3}) {
                if (cs && std::atoi(cs) != C) continue;
                for (int rc = 0; rc < 2; ++rc) {
                    if ((rs && (std::atoi(rs) != 0) != (rc != 0)) || (C == 1 && rc)) continue;
                    const DeferCost r = defer_cost(b, hot, wave_rays, C, rc != 0, join, c, push, round);
                    const double n = r.waves ? (double)r.waves : 1.0, w = r.walks ? (double)r.walks : 1.0;
                    std::printf("  C = %d%-8s trips %.1f, leaf passes %.2f with %.1f lanes, flushes %.2f, root passes %.2f, "
                                "VALU %.0f per wave walk (%+.1f%%); per ray: %.2f node visits, %.2f sphere tests\n",
                                C, rc ? " recull" : "", r.trips / n, r.passes / n,
                                r.passes ? r.pass_lanes / r.passes : 0.0, r.flushes / n, r.roots / n, r.valu / n,
                                bv > 0 ? 100.0 * (r.valu / n / bv - 1.0) : 0.0, r.visits / w, r.tests / w);
                }
            }
        }
    }
    for (int k = 0; k < 3; ++k) {
        std::vector<int> v = vis[k];
        if (v.empty()) continue;
        double mean = 0;
        for (int x : v) mean += x;
        mean /= v.size();
        // consecutive groups of 64 (neighbouring pixels) and shuffled groups
        double gmax = 0, rmax = 0;
        size_t ng = v.size() / 64;
        for (size_t g = 0; g < ng; ++g) gmax += *std::max_element(v.begin() + g * 64, v.begin() + g * 64 + 64);
        std::vector<int> sh = v;
        for (size_t i = sh.size() - 1; i > 0; --i) std::swap(sh[i], sh[(size_t)(rnd() * (i + 1)) % (i + 1)]);
        for (size_t g = 0; g < ng; ++g) rmax += *std::max_element(sh.begin() + g * 64, sh.begin() + g * 64 + 64);
        if (bvh4 && !box4[k].empty()) {
            double bt = 0, bmax = 0;
            for (int x : box4[k]) bt += x;
            for (size_t g = 0; g < ng; ++g)
                bmax += *std::max_element(box4[k].begin() + g * 64, box4[k].begin() + g * 64 + 64);
            std::printf("bvh4 bounce %d: box tests mean %.1f, E[max of 64] %.1f\n", k, bt / box4[k].size(),
                        ng ? bmax / ng : 0.0);
        }
        std::sort(v.begin(), v.end());
        std::printf("bounce %d: %zu walks, mean %.1f, p50 %d p90 %d p99 %d max %d; E[max of 64] "
                    "neighbours %.1f, shuffled %.1f (lane use %.0f%% / %.0f%%)\n",
                    k, v.size(), mean, v[v.size() / 2], v[v.size() * 9 / 10], v[v.size() * 99 / 100], v.back(),
                    ng ? gmax / ng : 0.0, ng ? rmax / ng : 0.0, ng ? 100 * mean / (gmax / ng) : 0.0,
                    ng ? 100 * mean / (rmax / ng) : 0.0);
    }
}
