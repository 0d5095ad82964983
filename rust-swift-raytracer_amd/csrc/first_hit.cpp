// first_hit.cpp -- first-hit records and views (host side).
//
// Checks a request, binds the device's resident scene with the camera as it
// is now (frame.cpp's binders: the scene, the trees and the primary triangle
// lists as a frame gets them) and launches first_hit.hip's kernel over the
// rectangle.
#include <cmath>

#include "runtime_internal.h"

namespace rtamd {

namespace {

struct Request {
    RtFirstHitOptions o;
    uint32_t x0, y0, w, h;  // the rectangle, resolved
};

// Every argument, with a message, before any device is looked for.
int check_request(size_t width, size_t height, const RtFirstHitOptions *opts, int view, bool views,
                  const void *d_out, const void *host_out, const char *who, const FirstHitPick *pick,
                  Request &r) {
    if (!d_out && !host_out) return fail(who, "null output");
    if (check_image_size(width, height, "frame size", who)) return -1;
    if (opts) r.o = *opts;
    else rt_first_hit_default_options(&r.o);
    const RtFirstHitOptions &o = r.o;
    if (!(o.su >= 0.0f && o.su < 1.0f)) return fail(who, "su must be in [0, 1)");
    if (!(o.sv >= 0.0f && o.sv < 1.0f)) return fail(who, "sv must be in [0, 1)");
    if (o.accel != RT_ACCEL_AUTO && o.accel != RT_ACCEL_BRUTE && o.accel != RT_ACCEL_BVH)
        return fail(who, "accel must be RT_ACCEL_AUTO, RT_ACCEL_BRUTE or RT_ACCEL_BVH");
    if (views && (view < RT_VIEW_NORMAL || view > RT_VIEW_PRIM))
        return fail(who, "view must be RT_VIEW_NORMAL, RT_VIEW_DEPTH, RT_VIEW_ALBEDO or RT_VIEW_PRIM");
    if (pick) {  // (the rectangle in opts is ignored)
        if (pick->col >= width || pick->row >= height) return fail(who, "pick: col, row outside the frame");
        r.x0 = (uint32_t)pick->col; r.y0 = (uint32_t)pick->row; r.w = r.h = 1;
        return 0;
    }
    if (o.x0 == 0 && o.y0 == 0 && o.w == 0 && o.h == 0) {
        r.x0 = r.y0 = 0; r.w = (uint32_t)width; r.h = (uint32_t)height;
        return 0;
    }
    if (o.w == 0 || o.h == 0) return fail(who, "rectangle: w and h must both be nonzero (or x0, y0, w, h all 0)");
    if ((uint64_t)o.x0 + o.w > width || (uint64_t)o.y0 + o.h > height)
        return fail(who, "rectangle: x0, y0, w, h leave the frame");
    r.x0 = o.x0; r.y0 = o.y0; r.w = o.w; r.h = o.h;
    return 0;
}

}  // namespace

int first_hit(WorldState &w, const CameraModel &cam, size_t width, size_t height, const RtFirstHitOptions *opts,
              bool views, int view, void *d_out, hipStream_t stream, void *host_out, const char *who,
              const FirstHitPick *pick) {
    Request r{};
    int rc = check_request(width, height, opts, view, views, d_out, host_out, who, pick, r);
    if (rc) return rc;

    std::lock_guard<std::recursive_mutex> lock(w.mu);
    DeviceState *d = nullptr;
    rc = device_for(w, r.o.device, d);
    if (rc) return rc;
    hipStream_t s = stream ? stream : d->stream.get();
    // ordered against the frames and passes of other streams like a frame
    // (render_frame): the host path's buffer is the device's, and an edit's
    // re-upload must not overtake a launch that reads the old arrays
    HIP_TRY(d->done.wait(s));

    // The scene and the camera as it is now.  The sphere tree and the static
    // triangle tree are exact for any origin; the primary strip lists (what
    // makes a frame's primary rays cheap on a large mesh) are
    // made current for this camera and frame size by the frames' own binder
    // before they are bound, so none can be an earlier camera's.
    TraceParams p{};
    bind_scene_arrays(d, cam, width, height, p);
    if (d->nnodes > 0 && r.o.accel != RT_ACCEL_BRUTE) bind_sphere_tree(w, d, p);
    rc = bind_primary_triangle_search(w, d, cam, width, height, r.o.accel, s, p);
    if (rc) return rc;
    // the lists' strip of a pixel comes from its job (serial_jobs.h job_pixel):
    // one sample per pixel, one rank, job = top row * width + col
    p.spp = 1;
    p.div_spp = make_fastdiv(1);
    p.row_block = (uint32_t)height;
    p.div_rowblock = make_fastdiv((uint32_t)height);
    p.nranks = 1;

    const size_t npix = (size_t)r.w * r.h;
    const size_t words = views ? npix : npix * (sizeof(RtFirstHit) / 4);
    void *out = d_out;
    if (!out) {
        HIP_TRY(d->first_hit.grow(words));
        out = d->first_hit.get();
    }
    const FirstHitTail tail{out, r.o.su, r.o.sv, r.x0, r.y0, r.w, r.h, views ? (uint32_t)view : kViewNone};
    HIP_TRY(launch_first_hit(p, tail, s));
    HIP_TRY(d->done.record(s));
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(host_out, out, words * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

}  // namespace rtamd
