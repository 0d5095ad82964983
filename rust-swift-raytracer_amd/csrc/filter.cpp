// filter.cpp -- the edge-aware filter, host side (rt_filter_*).
//
// Checks a request, owns a filter's scratch, and enqueues filter.hip's pack
// and level kernels.  On an accumulator the input is the means of its sums and
// the guides are its cached first-hit records, traced through first_hit.cpp's
// own device path for the camera and scene version the samples were traced
// with.
#include <cmath>

#include "runtime_internal.h"

namespace rtamd {

int filter_check_options(const RtFilterOptions *opts, const char *who, RtFilterOptions &o) {
    if (opts) o = *opts;
    else rt_filter_default_options(&o);
    if (o.levels < 0 || o.levels > 8) return fail(who, "levels must be 0 to 8");
    if (!finite_from(o.sigma_l, 0.0f, true)) return fail(who, "sigma_l must be finite and > 0");
    if (!finite_from(o.sigma_z, 0.0f, true)) return fail(who, "sigma_z must be finite and > 0");
    if (o.normal_squarings < 0 || o.normal_squarings > 8) return fail(who, "normal_squarings must be 0 to 8");
    if (o.flags & ~(uint32_t)RT_FILTER_SAME_PRIM) return fail(who, "flags: unknown bits (RT_FILTER_SAME_PRIM is 1)");
    return 0;
}

int filter_check_outputs(const void *out_rgb, const void *out_rgba, const char *who) {
    if (!out_rgb && !out_rgba) return fail(who, "null output: give out_rgb, the RGBA8 output or both");
    return 0;
}

// The pack and the levels on s, ordered after the filter's last run.  src: the
// input form (rgb, or sums / plane / count / held) and the records.
int filter_enqueue(FilterState &f, const RtFilterOptions &o, FilterPack src, float *d_out_rgb, uint32_t *d_out_rgba,
                   hipStream_t s) {
    const size_t npix = f.width * f.height;
    HIP_TRY(f.col[0].grow(npix));
    if (o.levels >= 2) HIP_TRY(f.col[1].grow(npix));
    HIP_TRY(f.g0.grow(npix));
    HIP_TRY(f.g1.grow(npix));
    HIP_TRY(f.done.wait(s));
    src.sigma_z = o.sigma_z;
    src.col = f.col[0].get();
    src.g0 = f.g0.get();
    src.g1 = f.g1.get();
    src.npix = (uint32_t)npix;
    HIP_TRY(launch_filter_pack(src, s));
    FilterLevel lv{};
    lv.g0 = f.g0.get();
    lv.g1 = f.g1.get();
    lv.width = (uint32_t)f.width;
    lv.height = (uint32_t)f.height;
    lv.squarings = (uint32_t)o.normal_squarings;
    lv.same_prim = o.flags & RT_FILTER_SAME_PRIM;
    for (int l = 0; l < std::max(o.levels, 1); ++l) {
        const bool last = l + 1 >= o.levels;
        lv.cin = f.col[l & 1].get();
        lv.cout = last ? nullptr : f.col[(l + 1) & 1].get();
        lv.out_rgb = last ? d_out_rgb : nullptr;
        lv.out_rgba = last ? d_out_rgba : nullptr;
        lv.step = o.levels == 0 ? 0u : 1u << l;
        lv.sl = std::ldexp(o.sigma_l, -l);  // sigma_l * 2^-l
        HIP_TRY(launch_filter_level(lv, s));
    }
    HIP_TRY(f.done.record(s));
    return 0;
}

// Device staging of the host outputs asked for, and their copies back (waits).
int filter_stage_outputs(FilterState &f, float *out_rgb, void *out_rgba, float *&d_rgb, uint32_t *&d_rgba) {
    const size_t npix = f.width * f.height;
    d_rgb = nullptr;
    d_rgba = nullptr;
    if (out_rgb) {
        HIP_TRY(f.out_rgb.grow(3 * npix));
        d_rgb = f.out_rgb.get();
    }
    if (out_rgba) {
        HIP_TRY(f.out_rgba.grow(npix));
        d_rgba = f.out_rgba.get();
    }
    return 0;
}

int filter_fetch_outputs(FilterState &f, float *out_rgb, void *out_rgba, hipStream_t s) {
    const size_t npix = f.width * f.height;
    if (out_rgb)
        HIP_TRY(hipMemcpyAsync(out_rgb, f.out_rgb.get(), 3 * npix * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_rgba) HIP_TRY(hipMemcpyAsync(out_rgba, f.out_rgba.get(), npix * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

FilterState::~FilterState() {
    // (a filter that never ran makes no HIP call; the last run may still use
    // the buffers that the members free)
    if (device >= 0 && (done.recorded() || stream) && hipSetDevice(device) == hipSuccess) (void)done.sync();
}

FilterState *filter_create(size_t width, size_t height, int device) {
    if (check_image_size(width, height, "image size", "rt_filter_create")) return nullptr;
    FilterState *f = new FilterState();
    f->width = width;
    f->height = height;
    f->device = device;
    return f;
}

int filter_run(FilterState *f, const RtFilterOptions *opts, const float *rgb, const void *records, float *out_rgb,
               void *out_rgba, bool on_device, hipStream_t stream, const char *who) {
    if (!f) return fail(who, "null filter");
    if (!rgb) return fail(who, "null input: rgb");
    if (!records) return fail(who, "null input: records");
    int rc = filter_check_outputs(out_rgb, out_rgba, who);
    if (rc) return rc;
    RtFilterOptions o;
    rc = filter_check_options(opts, who, o);
    if (rc) return rc;

    std::lock_guard<std::mutex> lock(f->mu);
    int dev = -1;
    rc = select_device(f->device, dev, who);
    if (rc) return rc;
    f->device = dev;  // (the scratch lives there from now on)
    hipStream_t s = on_device ? stream : nullptr;
    if (!s) {
        HIP_TRY(f->stream.create());
        s = f->stream.get();
    }
    const size_t npix = f->width * f->height;
    FilterPack src{};
    float *d_rgb = out_rgb;
    uint32_t *d_rgba = static_cast<uint32_t *>(out_rgba);
    if (on_device) {
        src.rgb = rgb;
        src.records = static_cast<const float4 *>(records);
    } else {
        HIP_TRY(f->in_rgb.grow(3 * npix));
        HIP_TRY(f->in_rec.grow(npix * (sizeof(RtFirstHit) / 4)));
        rc = filter_stage_outputs(*f, out_rgb, out_rgba, d_rgb, d_rgba);
        if (rc) return rc;
        // (the staging may still be read by the last run, on another stream)
        HIP_TRY(f->done.wait(s));
        HIP_TRY(hipMemcpyAsync(f->in_rgb.get(), rgb, 3 * npix * sizeof(float), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(f->in_rec.get(), records, npix * sizeof(RtFirstHit), hipMemcpyHostToDevice, s));
        src.rgb = f->in_rgb.get();
        src.records = reinterpret_cast<const float4 *>(f->in_rec.get());
    }
    rc = filter_enqueue(*f, o, src, d_rgb, d_rgba, s);
    if (rc) return rc;
    return on_device ? 0 : filter_fetch_outputs(*f, out_rgb, out_rgba, s);
}

FilterState &accum_filter(AccumState &a) {
    if (!a.filter) {
        a.filter = std::make_unique<FilterState>();
        a.filter->width = a.width;
        a.filter->height = a.height;
        a.filter->device = a.device;
    }
    return *a.filter;
}

int accum_records(AccumState &a, WorldState &w, const CameraModel &cam, FilterState &f, hipStream_t s,
                  const char *who) {
    const size_t npix = a.width * a.height;
    int rc = 0;
    // the records of the camera and scene the held samples were traced with
    // (a.cam is the handle's camera here: the reset rule has just been applied)
    if (!a.rec_valid || std::memcmp(a.rec_cam, a.cam, sizeof(a.cam)) != 0 || a.rec_edit != a.edit_version) {
        a.rec_valid = false;
        HIP_TRY(a.records.grow(npix * (sizeof(RtFirstHit) / 4)));
        // (the last run, on another stream, may still read the old ones)
        HIP_TRY(f.done.wait(s));
        RtFirstHitOptions fo;
        rt_first_hit_default_options(&fo);
        fo.device = a.device;
        fo.accel = a.accel;
        rc = first_hit(w, cam, a.width, a.height, &fo, false, 0, a.records.get(), s, nullptr, who);
        if (rc) return rc;
        std::memcpy(a.rec_cam, a.cam, sizeof(a.cam));
        a.rec_edit = a.edit_version;
        a.rec_valid = true;
    }
    return 0;
}

int filter_accum(AccumState *ap, const CameraModel *cam, const RtFilterOptions *opts, float *out_rgb, void *out_rgba,
                 bool on_device, hipStream_t stream, const char *who) {
    if (!ap || !cam) return fail(who, "null accumulator");
    AccumState &a = *ap;
    int rc = filter_check_outputs(out_rgb, out_rgba, who);
    if (rc) return rc;
    RtFilterOptions o;
    rc = filter_check_options(opts, who, o);
    if (rc) return rc;
    AccumRead r{a, *cam, who, out_rgb, out_rgba, on_device};
    rc = r.lock_world("the filter");
    if (!rc) rc = r.begin(stream);
    if (rc) return rc;

    FilterPack src{};
    src.sums = a.sums.get();
    src.plane = a.width * a.height;
    src.count = a.adaptive ? a.count.get() : nullptr;
    src.held = a.held;
    src.records = reinterpret_cast<const float4 *>(a.records.get());
    rc = filter_enqueue(*r.f, o, src, r.d_rgb, r.d_rgba, r.s);
    return rc ? rc : r.finish();
}

int AccumRead::lock_world(const char *taker) {
    if ((uint64_t)a.width * a.height >= (1ull << 31))
        return fail(who, std::string("the accumulator's frame has 2^31 pixels or more: ") + taker +
                             " takes width * height below 2^31 (an accumulator up to 2^32 - 1)");
    w = accum_begin(a, cam, lock);
    return w ? 0 : fail(who, "the accumulator's world was freed");
}

int AccumRead::begin(hipStream_t stream) {
    if (a.held == 0) return fail(who, "no samples held");
    int rc = device_for(*w, a.device, d);
    if (rc) return rc;
    s = stream ? stream : d->stream.get();
    f = &accum_filter(a);
    flock = std::unique_lock<std::mutex>(f->mu);
    // d->done is recorded again by finish, on s: it must still stand for the frame
    // another stream may be running, which the next frame on s has to wait for ...
    HIP_TRY(d->done.wait(s));
    // ... after the accumulator's last pass, like its other readers, and its last
    // resolve (the snapshots) ...
    HIP_TRY(a.done.wait(s));
    // ... and after the filter's last run (its scratch and staging are written next)
    HIP_TRY(f->done.wait(s));
    rc = accum_records(a, *w, cam, *f, s, who);
    if (rc) return rc;
    d_rgb = out_rgb;
    d_rgba = static_cast<uint32_t *>(out_rgba);
    return on_device ? 0 : filter_stage_outputs(*f, out_rgb, out_rgba, d_rgb, d_rgba);
}

int AccumRead::finish() {
    // the next pass, on whatever stream, writes the sums after this run read them
    HIP_TRY(d->done.record(s));
    HIP_TRY(a.done.record(s));
    return on_device ? 0 : filter_fetch_outputs(*f, out_rgb, out_rgba, s);
}

}  // namespace rtamd
