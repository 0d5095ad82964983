// primary_lists.cpp -- the per-camera structures of a frame's primary rays:
// the camera-origin triangle records and tree, and the primary sphere and
// triangle-strip lists, built on the host (bvh.cpp) or on the device
// (serial.hip launch_sphere_lists, tri_lists.hip).
#include <chrono>

#include "runtime_internal.h"

namespace rtamd {

static uint32_t cam_leaf() {
    return (uint32_t)env_u64("RT_AMD_CAM_LEAF", 2);  // triangles per camera-tree leaf
}

// prepare_camera below has nothing to build (a capturing frame asks before it calls)
bool camera_current(const WorldState &w, const CameraModel &cam, bool tree) {
    if (w.tbvh.nodes.empty() || env_u64("RT_AMD_CAMERA_TREE", 1) == 0) return true;
    const float o[3] = {cam.origin.x, cam.origin.y, cam.origin.z};
    return w.ctree_version && std::memcmp(o, w.ctree.origin, sizeof(o)) == 0 && (w.ctree_full || !tree);
}

// The camera-origin phantom records (and, with tree, the camera tree over
// them) for cam's origin.  Frames with primary strip lists need only the
// records: the lists replace every bounce-0 walk (C5: ~3 ms instead of the
// tree's ~50 ms after a camera move).
void prepare_camera(WorldState &w, const CameraModel &cam, bool tree) {
    if (camera_current(w, cam, tree)) return;
    const float o[3] = {cam.origin.x, cam.origin.y, cam.origin.z};
    w.ctree = build_camera_triangle_bvh(w.scene.triangles, w.packed.tri_hot, w.tbvh, o, cam_leaf(), tree);
    w.ctree_full = tree;
    ++w.ctree_version;
}

// Primary sphere lists for a new camera or frame size are built on the device
// on the frame's stream, before its trace kernel (RT_AMD_GPU_LISTS, default 1).
// With RT_AMD_GPU_LISTS=0 they are built on a host thread while frames render
// without them (RT_AMD_SYNC_LISTS=1: built before the frame).  Every frame is
// bit-identical either way; only the work per primary ray differs.
static bool sync_lists() { return env_u64("RT_AMD_SYNC_LISTS", 0) != 0; }
bool gpu_lists() { return env_u64("RT_AMD_GPU_LISTS", 1) != 0; }

template <typename T>
static bool job_ready(const std::future<T> &f) {
    return f.valid() && f.wait_for(std::chrono::seconds(0)) == std::future_status::ready;
}

// the host's primary strip lists are those of (cam, width, height) and the camera records
bool camera_lists_current(const WorldState &w, const CameraModel &cam, size_t width, size_t height) {
    return w.ptl_version && w.ptl_w == width && w.ptl_h == height && w.ptl_ctree == w.ctree_version &&
           same_cam(w.ptl_cam, cam);
}

// Camera tree (bounce-0 triangle tree for the camera origin) and the primary
// strip lists for (cam, width, height), rebuilt before the frame when either
// changed.  Unlike the sphere lists these are not deferred to a host thread:
// a C5 frame without them costs ~660 ms instead of ~221 ms, while the
// rebuild takes ~50 + 6 ms (subtrees built on 16 host threads, bvh.cpp).
void prepare_camera_lists(WorldState &w, const CameraModel &cam, size_t width, size_t height, bool lists) {
    prepare_camera(w, cam, !lists);
    if (!lists || !w.ctree_version) return;
    if (camera_lists_current(w, cam, width, height)) return;
    w.ptl = build_primary_tri_lists(w.ctree, cam, width, height);
    w.ptl_cam = cam;
    w.ptl_w = width;
    w.ptl_h = height;
    w.ptl_ctree = w.ctree_version;
    ++w.ptl_version;
}

// Primary sphere candidates per pixel (< 50 ms at 1080p on one host core).
// current: w.spl is current for (cam, width, height) on return.
int prepare_primary_sphere_lists(WorldState &w, const CameraModel &cam, size_t width, size_t height, bool capturing,
                                 bool &current) {
    current = w.spl_version && w.spl_w == width && w.spl_h == height && same_cam(w.spl_cam, cam);
    if (current) return 0;
    if (capturing) return cold_request("the primary sphere lists are not built for this camera and size");
    WorldState::SplJob &j = w.spl_job;
    if (sync_lists()) {
        w.spl = build_primary_sphere_lists(w.bvh, cam, width, height);
    } else {
        if (j.f.valid() && !job_ready(j.f)) return 0;  // (one build at a time)
        if (j.f.valid() && same_cam(j.cam, cam) && j.w == width && j.h == height) {
            w.spl = j.f.get();
        } else {
            if (j.f.valid()) (void)j.f.get();  // a finished build for another camera
            j.cam = cam;
            j.w = width;
            j.h = height;
            j.f = std::async(std::launch::async, [&w, cam, width, height]() {
                return build_primary_sphere_lists(w.bvh, cam, width, height);
            });
            return 0;
        }
    }
    w.spl_cam = cam;
    w.spl_w = width;
    w.spl_h = height;
    ++w.spl_version;
    current = true;
    return 0;
}
// The device build of the primary sphere lists for (cam, width, height),
// enqueued on s when either changed; false = no lists (every primary ray
// walks).  RT_AMD_SPL_CHECK=1 (tests): compare them with the host build.
int device_sphere_lists(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                        hipStream_t s, bool capturing, bool &ok) {
    auto &g = d->gspl;
    if (!g.current(cam, width, height)) {
        if (capturing) return cold_request("the primary sphere lists are not built for this camera and size");
        SphereListParams sp;
        g.ok = sphere_list_params(w.bvh, cam, width, height, sp) && (height + 15) / 16 <= 65535 &&
                     sp.n == d->nprims;
        if (g.ok) {
            d->retire(g.lists);  // (a graph's nodes may name the old camera's lists)
            HIP_TRY(g.lists.grow(width * height));
            HIP_TRY(g.rects.grow((size_t)sp.n));
            HIP_TRY(g.flag.grow(1));
            HIP_TRY(launch_sphere_lists(d->bvh_prims.get(), sp.n, sp.Mi, sp.o, sp.e_abs, sp.wden, sp.hden, sp.width,
                                        sp.height, g.rects.get(), g.flag.get(), g.lists.get(), s));
            if (env_u64("RT_AMD_SPL_CHECK", 0)) {
                const PrimarySphereLists h = build_primary_sphere_lists(w.bvh, cam, width, height);
                std::vector<uint32_t> dev(2 * width * height);
                HIP_TRY(hipMemcpyAsync(dev.data(), g.lists.get(), dev.size() * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                for (size_t px = 0; px < width * height; ++px) {
                    const bool same = h.rec.empty()
                                          ? (dev[2 * px + 1] >> 16) == kSphListWalk
                                          : dev[2 * px] == h.rec[2 * px] && dev[2 * px + 1] == h.rec[2 * px + 1];
                    if (!same) {
                        set_error("RT_AMD_SPL_CHECK: device sphere lists differ from the host build at pixel " +
                                  std::to_string(px));
                        return -2;
                    }
                }
            }
        }
        // the frame's sky rows go with the lists: classified on the host once this
        // frame is enqueued (classify_pending_sky_rows), so its launches do not
        // wait for that; until then there are none
        g.sky = SkyRows{};
        g.sky_pending = g.ok;
        g.remember(cam, width, height);
    }
    ok = g.ok;
    return 0;
}

// The sky rows of the device's current lists (bvh.h classify_sky_rows; some
// tens of microseconds of host arithmetic at 1080p), where a rebuild left them
// to be done: called once a frame's launches are enqueued, so the work hides
// behind the frame and the first frame after a camera move starts no later
// than without it.  The next frame finds them.
void classify_pending_sky_rows(WorldState &w, DeviceState *d) {
    auto &g = d->gspl;
    if (!g.sky_pending) return;
    g.sky = classify_sky_rows(w.bvh, w.scene.spheres, g.cam, g.w, g.h);
    g.sky_pending = false;
}

// Primary triangle strip lists are built on the device too (RT_AMD_GPU_TRI_LISTS,
// default 1; 0: bvh.cpp build_primary_tri_lists on the host, then an upload),
// from the camera-origin records' boxes, which change only with the origin: a
// camera that turns in place uploads nothing.
bool gpu_tri_lists() { return env_u64("RT_AMD_GPU_TRI_LISTS", 1) != 0; }

// The device build of the primary triangle lists for (cam, width, height,
// w.ctree), enqueued on s when any of them changed.  The lengths are read back
// (8 bytes, pinned) to size the items, so the first frame after a change waits
// on the host here, as it waited for the host build.  ok = false: no lists
// (g.host: the sizes are beyond the kernels' range and the host builds).
// RT_AMD_PTL_CHECK=1 (tests): compare the three arrays with the host build.
int device_tri_lists(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                     hipStream_t s, bool capturing, bool &ok) {
    auto &g = d->gptl;
    if (!g.current(cam, width, height, w.ctree_version)) {
        if (capturing) return cold_request("the primary triangle lists are not built for this camera and size");
        const CameraTriangleBVH &ct = w.ctree;
        TriListParams tp;
        g.built = false;
        g.ok = tri_list_params(ct, cam, width, height, tp);
        g.host = g.ok && ((height + 15) / 16 > 65535 ||
                                      (uint64_t)tp.strips_per_row * height >= 0x7FFFFFFFull);
        if (g.host) g.ok = false;
        if (g.ok) {
            const size_t ncells = (size_t)tp.strips_per_row * height;
            if (g.box_version != w.ctree_version) {
                HIP_TRY(g.box.grow(ct.rec_box.size()));
                HIP_TRY(hipMemcpyAsync(g.box.get(), ct.rec_box.data(), ct.rec_box.size() * 4, hipMemcpyHostToDevice,
                                       s));
                // (rec_box is pageable and may be rebuilt by the next origin: wait for the copy)
                HIP_TRY(hipStreamSynchronize(s));
                g.box_version = w.ctree_version;
            }
            HIP_TRY(g.rects.grow((size_t)tp.n));
            HIP_TRY(g.alw.grow((size_t)tp.n));
            HIP_TRY(g.count.grow(ncells));
            d->retire(g.off), d->retire(g.items);  // (a graph's nodes may name the old lists)
            HIP_TRY(g.off.grow(ncells + 1));
            HIP_TRY(g.meta.grow(4));
            HIP_TRY(g.hmeta.grow(4));
            HIP_TRY(launch_tri_list_counts(g.box.get(), tp.n, tp.Mi, tp.o, tp.wden, tp.hden, tp.width, tp.height,
                                           g.rects.get(), g.count.get(), g.off.get(), g.alw.get(), g.meta.get(), s));
            HIP_TRY(hipMemcpyAsync(g.hmeta.get(), g.meta.get(), 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const uint32_t total = g.hmeta.get()[0], nalways = g.hmeta.get()[1];
            if (g.hmeta.get()[2] != 0 || nalways > tp.n) {  // (more items than the host's u32 offsets hold)
                g.ok = false;
                g.host = true;
            } else {
                HIP_TRY(g.items.grow(std::max<size_t>((size_t)total + nalways, 1)));
                HIP_TRY(launch_tri_list_fill(g.rects.get(), tp.n, tp.width, tp.height, g.off.get(), g.alw.get(),
                                             total, nalways, g.items.get(), s));
                g.spr = tp.strips_per_row;
                g.total = total;
                g.nalways = nalways;
            }
        }
        if (g.ok && env_u64("RT_AMD_PTL_CHECK", 0)) {
            const PrimaryTriLists h = build_primary_tri_lists(ct, cam, width, height);
            const size_t nitems = (size_t)g.total + g.nalways;
            std::vector<uint32_t> off(h.offsets.size()), items(nitems);
            const bool shape = h.strips_per_row == g.spr && h.items.size() == nitems &&
                               h.offsets.size() == (size_t)g.spr * height + 1;
            if (shape) {
                HIP_TRY(hipMemcpyAsync(off.data(), g.off.get(), off.size() * 4, hipMemcpyDeviceToHost, s));
                if (nitems)
                    HIP_TRY(hipMemcpyAsync(items.data(), g.items.get(), nitems * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
            }
            if (!shape || off != h.offsets || items != h.items || h.offsets.back() != g.total) {
                set_error("RT_AMD_PTL_CHECK: device triangle lists differ from the host build (" +
                          std::to_string(nitems) + " items, host " + std::to_string(h.items.size()) + ")");
                return -2;
            }
        } else if (!g.ok && !g.host && env_u64("RT_AMD_PTL_CHECK", 0) &&
                   !build_primary_tri_lists(ct, cam, width, height).offsets.empty()) {
            set_error("RT_AMD_PTL_CHECK: the device build gave no lists where the host build has them");
            return -2;
        }
        g.remember(cam, width, height, w.ctree_version);
    }
    ok = g.ok;
    return 0;
}

}  // namespace rtamd
