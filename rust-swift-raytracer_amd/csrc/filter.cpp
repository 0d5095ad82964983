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

namespace {

constexpr float kMaxFloat = 3.4028234663852886e38f;

int fail(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return -1;
}

int check_size(size_t width, size_t height, const char *who) {
    if (width == 0 || height == 0 || (uint64_t)width >= (1ull << 31) || (uint64_t)height >= (1ull << 31) ||
        (uint64_t)width * height >= (1ull << 31))
        return fail(who, "image size: width and height at least 1, width * height below 2^31");
    return 0;
}

}  // namespace

int filter_check_options(const RtFilterOptions *opts, const char *who, RtFilterOptions &o) {
    if (opts) o = *opts;
    else rt_filter_default_options(&o);
    if (o.levels < 0 || o.levels > 8) return fail(who, "levels must be 0 to 8");
    if (!(o.sigma_l > 0.0f) || !(o.sigma_l <= kMaxFloat)) return fail(who, "sigma_l must be finite and > 0");
    if (!(o.sigma_z > 0.0f) || !(o.sigma_z <= kMaxFloat)) return fail(who, "sigma_z must be finite and > 0");
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
    if (!f.done) HIP_TRY(hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
    HIP_TRY(f.col[0].grow(npix));
    if (o.levels >= 2) HIP_TRY(f.col[1].grow(npix));
    HIP_TRY(f.g0.grow(npix));
    HIP_TRY(f.g1.grow(npix));
    if (f.done_stream && f.done_stream != s) HIP_TRY(hipStreamWaitEvent(s, f.done, 0));
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
    HIP_TRY(hipEventRecord(f.done, s));
    f.done_stream = s;
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
    if (device >= 0 && (done || stream) && hipSetDevice(device) == hipSuccess) {
        // (the last run may still use the buffers that the members free)
        if (done_stream) (void)hipEventSynchronize(done);
        if (done) (void)hipEventDestroy(done);
        if (stream) (void)hipStreamDestroy(stream);
    }
}

FilterState *filter_create(size_t width, size_t height, int device) {
    if (check_size(width, height, "rt_filter_create")) return nullptr;
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
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error(std::string(who) + ": no HIP device available: the MI355X render path requires a GPU");
        return -3;
    }
    int dev = f->device;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= count) return fail(who, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
    f->device = dev;  // (the scratch lives there from now on)
    hipStream_t s = on_device ? stream : nullptr;
    if (!s) {
        if (!f->stream) HIP_TRY(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
        s = f->stream;
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
        if (f->done_stream && f->done_stream != s) HIP_TRY(hipStreamWaitEvent(s, f->done, 0));
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
        if (f.done_stream && f.done_stream != s) HIP_TRY(hipStreamWaitEvent(s, f.done, 0));
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
    if ((uint64_t)a.width * a.height >= (1ull << 31))
        return fail(who, "the accumulator's frame has 2^31 pixels or more: the filter takes width * height below "
                         "2^31 (an accumulator up to 2^32 - 1)");

    std::unique_lock<std::recursive_mutex> lock;
    WorldState *wp = accum_begin(a, *cam, lock);
    if (!wp) return fail(who, "the accumulator's world was freed");
    WorldState &w = *wp;
    if (a.held == 0) return fail(who, "no samples held");
    DeviceState *d = nullptr;
    rc = device_for(w, a.device, d);
    if (rc) return rc;
    hipStream_t s = stream ? stream : d->stream;
    const size_t npix = a.width * a.height;
    FilterState &f = accum_filter(a);
    std::lock_guard<std::mutex> flock(f.mu);
    // d->done is recorded again below, on s: it must still stand for the frame
    // another stream may be running, which the next frame on s has to wait for
    if (d->done_stream && d->done_stream != s) HIP_TRY(hipStreamWaitEvent(s, d->done, 0));
    // after the accumulator's last pass, like its other readers
    if (a.done_stream && a.done_stream != s) HIP_TRY(hipStreamWaitEvent(s, a.done, 0));

    rc = accum_records(a, w, *cam, f, s, who);
    if (rc) return rc;

    FilterPack src{};
    src.sums = a.sums.get();
    src.plane = npix;
    src.count = a.adaptive ? a.count.get() : nullptr;
    src.held = a.held;
    src.records = reinterpret_cast<const float4 *>(a.records.get());
    float *d_rgb = out_rgb;
    uint32_t *d_rgba = static_cast<uint32_t *>(out_rgba);
    if (!on_device) {
        rc = filter_stage_outputs(f, out_rgb, out_rgba, d_rgb, d_rgba);
        if (rc) return rc;
    }
    rc = filter_enqueue(f, o, src, d_rgb, d_rgba, s);
    if (rc) return rc;
    // the next pass, on whatever stream, writes the sums after this run read them
    HIP_TRY(hipEventRecord(d->done, s));
    d->done_stream = s;
    HIP_TRY(hipEventRecord(a.done, s));
    a.done_stream = s;
    return on_device ? 0 : filter_fetch_outputs(f, out_rgb, out_rgba, s);
}

}  // namespace rtamd
