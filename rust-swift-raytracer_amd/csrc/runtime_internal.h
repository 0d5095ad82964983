// runtime_internal.h -- what the host runtime's units share with each other
// (device_state, primary_lists, frame, serial_states, multi, accum) and, of
// this, the argument checks with the C ABI, whose interface is runtime.h.
#pragma once

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <rccl/rccl.h>

#include "../../include/raytracer_amd.h"
#include "runtime.h"

namespace rtamd {

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            set_error(std::string(#expr) + " failed: " + hipGetErrorString(e_));      \
            return -2;                                                                \
        }                                                                             \
    } while (0)

#define NCCL_TRY(expr)                                                                \
    do {                                                                              \
        ncclResult_t r_ = (expr);                                                     \
        if (r_ != ncclSuccess) {                                                      \
            set_error(std::string(#expr) + " failed: " + ncclGetErrorString(r_));     \
            return -4;                                                                \
        }                                                                             \
    } while (0)

// (read at every use: tests and tools change the environment between frames)
inline uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::strtoull(v, nullptr, 10);
}

inline bool same_cam(const CameraModel &a, const CameraModel &b) {
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

// ---- checks, shared with the C ABI: every message reads "<who>: <msg>"
inline int fail(const char *who, const std::string &msg) {
    set_error(std::string(who) + ": " + msg);
    return -1;
}

// a size the filter, the history and the first-hit records take (noun: "image size", "frame size")
inline int check_image_size(size_t width, size_t height, const char *noun, const char *who) {
    if (width == 0 || height == 0 || (uint64_t)width >= (1ull << 31) || (uint64_t)height >= (1ull << 31) ||
        (uint64_t)width * height >= (1ull << 31))
        return fail(who, std::string(noun) + ": width and height at least 1, width * height below 2^31");
    return 0;
}

// v is finite and at least lo (above: more than lo); false for a NaN
inline bool finite_from(float v, float lo, bool above = false) {
    return (above ? v > lo : v >= lo) && v <= 3.4028234663852886e38f;
}

static_assert(kPrimaryTriStripW == kTriStripW, "render.h and bvh.h strip widths");
static constexpr uint64_t kMaxParts = kMaxJobParts;  // job-queue partitions (render.h)
static constexpr uint32_t kPixtabParts = 64;  // the pixel table pass's (zeroed by the window kernel)

// ---- stream capture (raytracer_amd.h, rt_render_device: "Capture")
// s is capturing into a graph (null: no; a query that fails counts as capturing)
inline bool stream_capturing(hipStream_t s) {
    if (!s) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}
// a call that is never captured (stats, SERIAL, several devices, accumulation) -> -1
inline int refuse_capture(const char *who, const char *what) {
    return fail(who, std::string(what) + " cannot be captured into a graph");
}
// a capturing frame that is not warm: it would have to allocate, upload, build
// lists or wait on the host here (what) -> -1, with nothing enqueued or changed
inline int cold_request(const char *what) {
    return fail("capture", std::string(what) + ": render this frame once outside the capture first");
}

// device_state.cpp: device `want` (< 0: the current one) counted, range-checked
// and selected -> dev (who: a prefix for the messages, none for null)
int select_device(int want, int &dev, const char *who = nullptr);
// ... and w's state on it, created on first use -- stream and events, the
// scene upload, the LDS layout and occupancy decisions (capturing: a cold
// request where there is none yet)
int device_for(WorldState &w, int want, DeviceState *&out, bool capturing = false);

// frame.cpp: the parts of a TraceParams that do not depend on the kind of
// launch -- the scene's arrays with the camera and the frame size, the sphere
// tree (global-memory walk) and the static triangle tree
void bind_scene_arrays(const DeviceState *d, const CameraModel &cam, size_t width, size_t height, TraceParams &p);
void bind_sphere_tree(const WorldState &w, const DeviceState *d, TraceParams &p);
void bind_triangle_tree(const WorldState &w, const DeviceState *d, TraceParams &p);
// ... and a frame's whole triangle search for (cam, width, height): that tree
// plus the camera-origin records and primary strip lists, rebuilt when the
// camera, the frame size or the records changed (s: the stream the launch goes to)
int bind_primary_triangle_search(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                                 int32_t accel, hipStream_t s, TraceParams &p);

// primary_lists.cpp
bool gpu_lists();      // RT_AMD_GPU_LISTS
bool gpu_tri_lists();  // RT_AMD_GPU_TRI_LISTS
// (what prepare_camera and prepare_camera_lists would find, without building anything)
bool camera_current(const WorldState &w, const CameraModel &cam, bool tree);
bool camera_lists_current(const WorldState &w, const CameraModel &cam, size_t width, size_t height);
void prepare_camera_lists(WorldState &w, const CameraModel &cam, size_t width, size_t height, bool lists);
// (capturing, in these three: a cold request where something would be built)
int prepare_primary_sphere_lists(WorldState &w, const CameraModel &cam, size_t width, size_t height, bool capturing,
                                 bool &current);
int device_sphere_lists(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                        hipStream_t s, bool capturing, bool &ok);
void classify_pending_sky_rows(WorldState &w, DeviceState *d);
int device_tri_lists(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                     hipStream_t s, bool capturing, bool &ok);

// serial_states.cpp
int serial_check_args(size_t width, size_t height, const RtRenderOptions &o);
int serial_find_states(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                       const RtRenderOptions &o, DeviceState *d, hipStream_t s, RtRenderStats *stats);

// accum.cpp: the accumulator's world, locked, after the reset rule (a moved
// camera or an edited scene drops the held samples); nullptr with the error set
WorldState *accum_begin(AccumState &a, const CameraModel &cam, std::unique_lock<std::recursive_mutex> &lock);

// filter.cpp, for history.cpp: a filter call's checks (who: the entry point, for
// the messages; o: the options checked, the defaults for null) ...
int filter_check_outputs(const void *out_rgb, const void *out_rgba, const char *who);
int filter_check_options(const RtFilterOptions *opts, const char *who, RtFilterOptions &o);
// ... the accumulator's filter state, created on first use ...
FilterState &accum_filter(AccumState &a);
// ... the accumulator's first-hit records made current on s: those of the camera
// and scene version its held samples were traced with, kept until either changes
// (cam: the handle's camera, a.cam's after the reset rule) ...
int accum_records(AccumState &a, WorldState &w, const CameraModel &cam, FilterState &f, hipStream_t s, const char *who);
// ... the pack and the levels on s, ordered after the filter's last run (src:
// the input form and the records) ...
int filter_enqueue(FilterState &f, const RtFilterOptions &o, FilterPack src, float *d_out_rgb, uint32_t *d_out_rgba,
                   hipStream_t s);
// ... and device staging of the host outputs asked for, with their copies back (waits)
int filter_stage_outputs(FilterState &f, float *out_rgb, void *out_rgba, float *&d_rgb, uint32_t *&d_rgba);
int filter_fetch_outputs(FilterState &f, float *out_rgb, void *out_rgba, hipStream_t s);
// A call that reads an accumulator's held samples on a stream (filter_accum,
// history_resolve; the outputs are device memory if on_device, else host).
// lock_world: the frame's size (taker: who takes no more, for the message), the
// world locked, the reset rule.  begin: samples held, the device, s, the filter
// locked, s behind the three fences, the records current, d_rgb / d_rgba where
// the kernels write.  finish: the device's and the accumulator's fences
// recorded, host outputs fetched.
struct AccumRead {
    AccumState &a;
    const CameraModel &cam;
    const char *who;
    float *out_rgb;
    void *out_rgba;
    bool on_device;
    WorldState *w = nullptr;
    DeviceState *d = nullptr;
    hipStream_t s = nullptr;
    FilterState *f = nullptr;
    std::unique_lock<std::recursive_mutex> lock;
    std::unique_lock<std::mutex> flock;
    float *d_rgb = nullptr;
    uint32_t *d_rgba = nullptr;
    int lock_world(const char *taker);
    int begin(hipStream_t stream);
    int finish();
};

// multi.cpp: devices [first, first + n) (first < 0: from the current device), checked
int device_list(int first, int n, std::vector<int> &devs);

}  // namespace rtamd
