// history.cpp -- temporal reprojection, host side (rt_history_*).
//
// Keeps an accumulator's two snapshots (which one is cur, what camera and scene
// version each was made under), computes prev's camera constants and enqueues
// history.hip's resolve kernel in front of the outputs or of the edge-aware
// filter.  Ordered on the stream exactly as filter_accum, whose records cache,
// filter state and output staging it shares (runtime_internal.h).  The resolve's
// neighbourhood clamp (rt_clamp_*) is a setting kept beside the
// history's: it picks the kernel's clamped instance and, with
// RT_CLAMP_KEEP_ON_EDIT, lets the snapshots outlive an edit.  After a geometry
// edit (rt_world_set_sphere_geometry) a kept snapshot remembers
// the spheres that have moved since it was made, and a resolve against it runs
// move.hip's kernel with prev's sphere table.
#include <algorithm>
#include <limits>

#include "runtime_internal.h"

namespace rtamd {

namespace {

// a x b as maths.rs:88-94: each product rounded, then the subtraction
void cross(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = -(a[0] * b[2] - a[2] * b[0]);
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// prev's camera constants (this unit compiles without contraction: one rounded
// operation per step, the bits a lane would compute)
void history_camera(const float cam[12], HistoryResolve &k) {
    const float *O = cam, *L = cam + 3, *H = cam + 6, *V = cam + 9;
    const float A[3] = {L[0] - O[0], L[1] - O[1], L[2] - O[2]};
    cross(H, V, k.n0);
    cross(V, A, k.n1);
    cross(A, H, k.n2);
    k.det = ((A[0] * k.n0[0]) + (A[1] * k.n0[1])) + (A[2] * k.n0[2]);
    for (int i = 0; i < 3; ++i) k.org[i] = O[i];
}

void drop_snapshots(AccumState &a) {
    for (auto &h : a.hist) {
        h.valid = false;
        h.moved.clear();
    }
}

// prev's sphere table on the device, enqueued on s: the world's spheres as they
// are, overlaid with what prev remembers of those that moved since.  The host
// waits for the accumulator's last resolve first, which may still be reading the
// staging (and, on another stream, the table).
int upload_prev_spheres(AccumState &a, const WorldState &w, const AccumState::HistorySnap &prev, hipStream_t s) {
    const size_t n = w.scene.spheres.size();
    HIP_TRY(a.done.sync());
    HIP_TRY(a.move_stage.grow(n));
    HIP_TRY(a.move_table.grow(n));
    float4 *t = a.move_stage.get();
    for (size_t i = 0; i < n; ++i) {
        const Sphere &sp = w.scene.spheres[i];
        t[i] = make_float4(sp.center.x, sp.center.y, sp.center.z, sp.radius);
    }
    for (const auto &kv : prev.moved)
        if (kv.first < n) t[kv.first] = make_float4(kv.second[0], kv.second[1], kv.second[2], kv.second[3]);
    HIP_TRY(hipMemcpyAsync(a.move_table.get(), t, n * sizeof(float4), hipMemcpyHostToDevice, s));
    return 0;
}

}  // namespace

int history_check(const RtFilterOptions *filter, const void *out_rgb, const void *out_rgba, const char *who) {
    int rc = filter_check_outputs(out_rgb, out_rgba, who);
    if (rc) return rc;
    RtFilterOptions o;
    return filter ? filter_check_options(filter, who, o) : 0;
}

int history_enable(AccumState &a, const CameraModel &cam, bool on, float max_history, float sigma_z) {
    // (the options were checked by rt_history_enable, before the accumulator)
    std::unique_lock<std::recursive_mutex> lock;
    if (!accum_begin(a, cam, lock)) return -1;
    drop_snapshots(a);
    a.hist_enabled = on;
    if (on) {
        a.hist_max = max_history;
        a.hist_sigma_z = sigma_z;
        return 0;
    }
    // (the last resolve may still use the buffers)
    if (a.device >= 0 && a.done.recorded()) {
        HIP_TRY(hipSetDevice(a.device));
        HIP_TRY(a.done.sync());
    }
    for (auto &h : a.hist) {
        h.col.reset();
        h.guide.reset();
    }
    a.hist_rgb.reset();
    a.move_stage.reset();
    a.move_table.reset();
    return 0;
}

int history_reset(AccumState &a, const CameraModel &cam) {
    std::unique_lock<std::recursive_mutex> lock;
    if (!accum_begin(a, cam, lock)) return -1;
    if (!a.hist_enabled) return fail("rt_history_reset", "the accumulator's history is not enabled");
    drop_snapshots(a);
    return 0;
}

int clamp_enable(AccumState &a, const CameraModel &cam, bool on, const RtClampOptions &o) {
    std::unique_lock<std::recursive_mutex> lock;
    if (!accum_begin(a, cam, lock)) return -1;
    // (no snapshot goes: a resolve is a function of prev, the accumulator's state and the options)
    a.clamp_enabled = on;
    a.clamp_gamma = on ? o.gamma : 0.0f;
    a.clamp_radius = on ? (uint32_t)o.radius : 0u;
    a.clamp_flags = on ? o.flags : 0u;
    return 0;
}

int history_resolve(AccumState *ap, const CameraModel *cam, const RtFilterOptions *filter, float *out_rgb,
                    void *out_rgba, bool on_device, hipStream_t stream, const char *who) {
    if (!ap || !cam) return fail(who, "null accumulator");
    AccumState &a = *ap;
    // (the entry point has been through history_check already: a caller's mistake
    // shows whatever the accumulator's state)
    int rc = history_check(filter, out_rgb, out_rgba, who);
    if (rc) return rc;
    RtFilterOptions fo{};
    if (filter) fo = *filter;
    AccumRead r{a, *cam, who, out_rgb, out_rgba, on_device};
    rc = r.lock_world("a history");
    if (rc) return rc;
    if (!a.hist_enabled) return fail(who, "the accumulator's history is not enabled (rt_history_enable)");
    rc = r.begin(stream);
    if (rc) return rc;
    hipStream_t s = r.s;
    const size_t npix = a.width * a.height;
    for (auto &h : a.hist) {
        HIP_TRY(h.col.grow(npix));
        HIP_TRY(h.guide.grow(npix));
    }
    if (filter) HIP_TRY(a.hist_rgb.grow(3 * npix));

    // a snapshot of another scene: both go; a cur of another camera becomes prev.
    // Under a clamp that keeps history over edits they stay, and a cur of another
    // scene becomes prev too: a material edit leaves the guides true, and a sphere
    // that moved is followed through what prev remembers of it (below)
    const bool keep = a.clamp_enabled && (a.clamp_flags & RT_CLAMP_KEEP_ON_EDIT) != 0;
    for (const auto &h : a.hist)
        if (!keep && h.valid && h.edit != a.edit_version) drop_snapshots(a);
    if (a.hist[a.hist_cur].valid && (std::memcmp(a.hist[a.hist_cur].cam, a.cam, sizeof(a.cam)) != 0 ||
                                     (keep && a.hist[a.hist_cur].edit != a.edit_version)))
        a.hist_cur ^= 1u;
    AccumState::HistorySnap &cur = a.hist[a.hist_cur], &prev = a.hist[a.hist_cur ^ 1u];
    // (valid again once the kernel that fills it is enqueued)
    cur.valid = false;

    HistoryResolve k{};
    k.sums = a.sums.get();
    k.plane = npix;
    k.count = a.adaptive ? a.count.get() : nullptr;
    k.held = a.held;
    k.records = reinterpret_cast<const float4 *>(a.records.get());
    if (prev.valid) {
        k.prev_col = prev.col.get();
        k.prev_guide = prev.guide.get();
        history_camera(prev.cam, k);
    }
    k.max_history = a.hist_max;
    k.sigma_z = a.hist_sigma_z;
    k.cur_col = cur.col.get();
    k.cur_guide = cur.guide.get();
    k.out_rgb = filter ? a.hist_rgb.get() : r.d_rgb;
    k.out_rgba = filter ? nullptr : r.d_rgba;
    k.width = (uint32_t)a.width;
    k.height = (uint32_t)a.height;
    const HistoryClamp clamp{a.clamp_gamma, a.clamp_radius, nullptr};
    // prev saw some sphere elsewhere: the resolve follows it (keep: the clamp is on
    // with the flag; without it no snapshot outlives an edit and no map fills)
    if (keep && prev.valid && !prev.moved.empty()) {
        rc = upload_prev_spheres(a, *r.w, prev, s);
        if (rc) return rc;
        const HistoryMove mv{a.move_table.get(), r.d->sph_shade.get(), 2u, (uint32_t)r.w->scene.spheres.size()};
        HIP_TRY(launch_history_move(k, clamp, mv, s));
    } else {
        HIP_TRY(a.clamp_enabled ? launch_history_clamp(k, clamp, s) : launch_history_resolve(k, s));
    }
    cur.moved.clear();  // (made under the world's present geometry)
    std::memcpy(cur.cam, a.cam, sizeof(a.cam));
    cur.edit = a.edit_version;
    cur.valid = true;
    if (filter) {
        // the filter of the blended image with the same records; the history keeps the unfiltered one
        FilterPack src{};
        src.rgb = a.hist_rgb.get();
        src.records = k.records;
        rc = filter_enqueue(*r.f, fo, src, r.d_rgb, r.d_rgba, s);
        if (rc) return rc;
    } else {
        // (host outputs went to the filter's staging: its next run, on another stream, waits)
        HIP_TRY(r.f->done.record(s));
    }
    return r.finish();
}

int history_read_length(AccumState &a, const CameraModel &cam, float *len) {
    if (!len) return fail("rt_history_read_length", "null output: len");
    std::unique_lock<std::recursive_mutex> lock;
    if (!accum_begin(a, cam, lock)) return -1;
    if (!a.hist_enabled) return fail("rt_history_read_length", "the accumulator's history is not enabled");
    const size_t npix = a.width * a.height;
    const AccumState::HistorySnap &cur = a.hist[a.hist_cur];
    if (!cur.valid) {
        std::fill(len, len + npix, 0.0f);
        return 0;
    }
    HIP_TRY(hipSetDevice(a.device));
    HIP_TRY(a.done.sync());
    std::vector<float4> col(npix);
    HIP_TRY(hipMemcpy(col.data(), cur.col.get(), npix * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npix; ++i) len[i] = col[i].w;
    return 0;
}

int history_run(size_t width, size_t height, float max_history, float sigma_z, const float *prev_cam,
                const float *prev_rgbl, const void *prev_records, const float *rgb, const uint32_t *n,
                const void *records, float *out_rgbl, int device, const RtClampOptions *clamp, float *out_box,
                const HistoryRunMove *move) {
    // (the arguments were checked by rt_history_run, rt_clamp_run or rt_move_run)
    int dev = -1;
    const int rc = select_device(device, dev, move ? "rt_move_run" : clamp ? "rt_clamp_run" : "rt_history_run");
    if (rc) return rc;
    const size_t npix = width * height;
    DevBuf<float> d_rgb;
    DevBuf<uint32_t> d_n, d_rec;
    DevBuf<float4> d_prev_col, d_prev_guide, d_out;
    HIP_TRY(d_rgb.grow(3 * npix));
    HIP_TRY(d_n.grow(npix));
    HIP_TRY(d_rec.grow(npix * (sizeof(RtFirstHit) / 4)));
    HIP_TRY(d_out.grow(npix));
    HIP_TRY(hipMemcpy(d_rgb.get(), rgb, 3 * npix * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_n.get(), n, npix * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_rec.get(), records, npix * sizeof(RtFirstHit), hipMemcpyHostToDevice));
    HistoryResolve k{};
    if (prev_rgbl) {
        // a snapshot's guide: {position, prim bits} of its records
        const RtFirstHit *pr = static_cast<const RtFirstHit *>(prev_records);
        std::vector<float4> guide(npix);
        for (size_t i = 0; i < npix; ++i) {
            guide[i].x = pr[i].position[0];
            guide[i].y = pr[i].position[1];
            guide[i].z = pr[i].position[2];
            std::memcpy(&guide[i].w, &pr[i].prim, sizeof(float));
        }
        HIP_TRY(d_prev_col.grow(npix));
        HIP_TRY(d_prev_guide.grow(npix));
        HIP_TRY(hipMemcpy(d_prev_col.get(), prev_rgbl, npix * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_prev_guide.get(), guide.data(), npix * sizeof(float4), hipMemcpyHostToDevice));
        k.prev_col = d_prev_col.get();
        k.prev_guide = d_prev_guide.get();
        history_camera(prev_cam, k);
    }
    k.rgb = d_rgb.get();
    k.n = d_n.get();
    k.records = reinterpret_cast<const float4 *>(d_rec.get());
    k.max_history = max_history;
    k.sigma_z = sigma_z;
    k.cur_col = d_out.get();
    k.width = (uint32_t)width;
    k.height = (uint32_t)height;
    // (the null stream: the copies above are done, the one below follows the kernel)
    DevBuf<float> d_box;
    HistoryClamp c{};
    if (clamp) {
        c.gamma = clamp->gamma;
        c.radius = (uint32_t)clamp->radius;
        if (out_box) {
            HIP_TRY(d_box.grow(6 * npix));
            c.out_box = d_box.get();
        }
    }
    // rt_move_run's tables: prev's dense, as move_table is; the present one as a
    // device's sph_shade, {centre, r} in the first of two float4 per sphere, the
    // second one NaN: a read that forgets the stride meets poison, not a neighbour.
    // One guard entry stands behind each table, NaN in prev's and zeros in the
    // present one: an index one past the end reads a sphere that moved, to nowhere,
    // and not whatever lies behind the buffer (so the tables exist at nspheres = 0 too)
    DevBuf<float4> d_prev_sph, d_sph;
    HistoryMove mv{};
    if (move) {
        const size_t ns = move->nspheres;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        std::vector<float4> was(ns + 1, make_float4(nan, nan, nan, nan));
        std::vector<float4> shade(2 * (ns + 1), make_float4(nan, nan, nan, nan));
        if (ns) std::memcpy(was.data(), move->prev_spheres, ns * sizeof(float4));
        for (size_t i = 0; i < ns; ++i) std::memcpy(&shade[2 * i], move->spheres + 4 * i, sizeof(float4));
        shade[2 * ns] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        HIP_TRY(d_prev_sph.grow(was.size()));
        HIP_TRY(d_sph.grow(shade.size()));
        HIP_TRY(hipMemcpy(d_prev_sph.get(), was.data(), was.size() * sizeof(float4), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_sph.get(), shade.data(), shade.size() * sizeof(float4), hipMemcpyHostToDevice));
        mv = HistoryMove{d_prev_sph.get(), d_sph.get(), 2u, (uint32_t)ns};
    }
    HIP_TRY(move    ? launch_history_move(k, c, mv, nullptr)
            : clamp ? launch_history_clamp(k, c, nullptr)
                    : launch_history_resolve(k, nullptr));
    HIP_TRY(hipMemcpy(out_rgbl, d_out.get(), npix * sizeof(float4), hipMemcpyDeviceToHost));
    if (c.out_box) HIP_TRY(hipMemcpy(out_box, d_box.get(), 6 * npix * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace rtamd
