// Host-only check of render.h's trace-instance rules (tests/test_trace_variants_host.py
// builds and runs it): every request a caller can make -- search x step x mesh x
// kind x defer x plain -- is resolved and compared with the rules stated here
// a second time, as independent predicates; the table key is checked for range,
// injectivity and its inverse; trace_plain_ok for its baseline and each of its
// fourteen conditions.  Prints one line and returns the number of failures.
#include <cstdio>
#include <map>

#include "render.h"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            std::printf("FAILED %s: ", #cond); \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

static unsigned long long g_stats;
static float g_ring;
static uint2 g_spl;
static uint4 g_wide;

// A launch that satisfies trace_plain_ok, of a scene searched as `search` in
// family `mesh`, whose stats and mode agree with `kind` as launch_trace demands
static TraceParams params(int search, bool step, int mesh, int kind) {
    TraceParams p{};
    p.nnodes = search == kSearchBrute ? 0u : 7u;
    p.use_lds = search >= kSearchLdsBox;
    p.step = step;
    p.ntri = mesh != 0 ? 20u : 0u;
    p.tnodes = mesh >= 2 ? 5u : 0u;
    p.tw_nodes = mesh == 3 ? &g_wide : nullptr;
    p.mode = kind == kKindSerial ? kRngSerialCount : kRngCounter;
    p.stats = kind == kKindCounting ? &g_stats : nullptr;
    p.ring = &g_ring;
    p.gj32 = 1;
    p.xdiv_uv = 1;
    p.spl = &g_spl;
    p.walk_min = 65;
    p.spp = 16;
    p.chunk = 128;
    return p;
}

static bool same(TraceVariant a, TraceVariant b) {
    return a.search == b.search && a.step == b.step && a.mesh == b.mesh && a.kind == b.kind && a.leaf == b.leaf;
}

int main() {
    std::map<int, TraceVariant> by_key;
    int requests = 0;
    for (int search = 0; search < 4; ++search)
        for (int step = 0; step < 2; ++step)
            for (int mesh = 0; mesh < 4; ++mesh)
                for (int kind = 0; kind < kTraceKinds; ++kind)
                    for (int defer = 0; defer < 2; ++defer)
                        for (int plain = 0; plain < 2; ++plain, ++requests) {
                            // the rules, stated apart from render.h
                            const bool serial = kind == kKindSerial;
                            const int want_mesh = serial && mesh == 3 ? 2 : mesh;  // SERIAL: the binary walk
                            const bool corner_ok = want_mesh == 0 && !serial;      // corner records: sphere-only, not SERIAL
                            const int want_search = search == kSearchLdsCorner && !corner_ok ? kSearchLdsBox : search;
                            const bool want_defer = defer && want_search == kSearchLdsCorner && !step &&
                                                    want_mesh == 0 && kind == kKindLean;
                            const TraceLeaf want_leaf = !want_defer ? TraceLeaf::Immediate
                                                        : plain     ? TraceLeaf::Plain
                                                                    : TraceLeaf::Deferred;
                            const TraceVariant n = normalise_trace_variant(
                                TraceVariant{search, step != 0, mesh, kind, defer ? TraceLeaf::Deferred : TraceLeaf::Immediate});
                            CHECK(n.search == want_search && n.step == (step != 0) && n.mesh == want_mesh && n.kind == kind &&
                                      n.leaf == (want_defer ? TraceLeaf::Deferred : TraceLeaf::Immediate),
                                  "normalise %d %d %d %d %d", search, step, mesh, kind, defer);
                            CHECK(same(normalise_trace_variant(n), n), "idempotent %d %d %d %d %d", search, step, mesh, kind, defer);
                            // the launch's resolution: the same, and plain only on top of defer
                            const TraceParams p = params(search == kSearchLdsCorner ? kSearchLdsBox : search, step != 0, mesh, kind);
                            TraceRequest r;
                            r.corner = search == kSearchLdsCorner;
                            r.kind = kind;
                            r.defer = defer != 0;
                            r.plain = plain != 0;
                            const TraceVariant v = resolve_trace_variant(p, r);
                            CHECK(v.search == want_search && v.step == (step != 0) && v.mesh == want_mesh && v.kind == kind &&
                                      v.leaf == want_leaf,
                                  "resolve %d %d %d %d %d %d", search, step, mesh, kind, defer, plain);
                            CHECK(v.leaf != TraceLeaf::Plain || (defer && plain), "plain without defer");
                            // the table key: in range, one variant per key, trace_variant_at its inverse
                            const int key = trace_key(v);
                            CHECK(key >= 0 && key < kTraceKeys && key != kTraceNoKey, "key %d out of range", key);
                            const auto seen = by_key.find(key);
                            CHECK(seen == by_key.end() || same(seen->second, v), "key %d serves two variants", key);
                            by_key[key] = v;
                            CHECK(same(trace_variant_at(key), v), "trace_variant_at(%d)", key);
                        }
    CHECK(trace_key(TraceVariant{4, false, 0, 0}) == kTraceNoKey && trace_key(TraceVariant{0, false, 0, kTraceKinds}) == kTraceNoKey &&
              trace_key(TraceVariant{0, false, 4, 0}) == kTraceNoKey && trace_key(TraceVariant{-1, false, 0, 0}) == kTraceNoKey,
          "an unknown variant has no key");
    CHECK(trace_key(TraceVariant{kSearchLdsBox, false, 0, kKindLean, TraceLeaf::Deferred}) == kTraceNoKey,
          "deferred leaves off the corner search have no key");
    CHECK(trace_key(trace_variant_at(kTraceNoKey)) == kTraceNoKey, "the empty entry");

    // trace_plain_ok: the baseline, then each condition violated alone
    const TraceParams base = params(kSearchLdsBox, false, 0, kKindLean);
    CHECK(trace_plain_ok(base), "baseline");
    int conditions = 0;
    auto violated = [&](const char *what, auto change) {
        TraceParams p = base;
        change(p);
        ++conditions;
        CHECK(!trace_plain_ok(p), "%s", what);
        TraceRequest r;
        r.corner = r.defer = r.plain = true;
        CHECK(resolve_trace_variant(p, r).leaf != TraceLeaf::Plain, "resolved plain with %s", what);
    };
    violated("mode", [](TraceParams &p) { p.mode = kRngReplay; });
    violated("stats", [](TraceParams &p) { p.stats = &g_stats; });
    violated("ring", [](TraceParams &p) { p.ring = nullptr; });
    violated("gj32", [](TraceParams &p) { p.gj32 = 0; });
    violated("xdiv_uv", [](TraceParams &p) { p.xdiv_uv = 0; });
    violated("spl", [](TraceParams &p) { p.spl = nullptr; });
    violated("walk_min", [](TraceParams &p) { p.walk_min = 0; });
    violated("ablate", [](TraceParams &p) { p.ablate = 1; });
    violated("nnodes", [](TraceParams &p) { p.nnodes = 1; });
    violated("div_spp", [](TraceParams &p) { p.div_spp.one = 1; });
    violated("div_width", [](TraceParams &p) { p.div_width.one = 1; });
    violated("spp % 4", [](TraceParams &p) { p.spp = 6; p.chunk = 126; });
    violated("chunk % spp", [](TraceParams &p) { p.chunk = 130; });
    violated("pixels per chunk", [](TraceParams &p) { p.chunk = 22 * 16; });
    CHECK(conditions == 14, "fourteen conditions");
    {
        TraceRequest r;
        r.corner = r.defer = r.plain = true;
        CHECK(resolve_trace_variant(base, r).leaf == TraceLeaf::Plain, "the baseline resolves to the plain instance");
    }
    std::printf("requests %d keys %zu conditions %d failures %d\n", requests, by_key.size(), conditions, failures);
    return failures;
}
