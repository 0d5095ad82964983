// frame.cpp -- frame driver of the HIP render path (host side).
//
// Uses each world's device-resident scene (device_state.cpp), the per-wave
// sample rings (or the per-sample slab) and the launch sequence: for every
// launch of tile rows, zero the job counters and launch the persistent trace
// kernel, which resolves pixels itself; with RT_FLAG_KEEP_SAMPLES the samples
// go to the slab and the ordered resolve kernel follows.  The reference's
// equivalent is ray_trace's triple loop (common.rs:320-361).
#include <algorithm>
#include <cmath>
#include <cstdio>

#include "runtime_internal.h"

namespace rtamd {

size_t tile_rows(size_t height, uint32_t row_block, uint32_t rank, uint32_t nranks) {
    if (nranks <= 1) return height;
    const size_t B = row_block ? row_block : 1;
    const size_t blocks = (height + B - 1) / B;
    size_t rows = 0;
    for (size_t b = rank; b < blocks; b += nranks) rows += std::min(B, height - b * B);
    return rows;
}

size_t tile_row(size_t k, uint32_t row_block, uint32_t rank, uint32_t nranks) {
    if (nranks <= 1) return k;
    const size_t B = row_block ? row_block : 1;
    return ((k / B) * nranks + rank) * B + k % B;
}

// What every kernel that casts a camera ray reads of a TraceParams, shared by
// the frames (bind_scene below) and the first-hit calls (first_hit.cpp): the
// scene's arrays, the camera's 12 floats, the frame size and its divisions.
void bind_scene_arrays(const DeviceState *d, const CameraModel &cam, size_t width, size_t height, TraceParams &p) {
    p.sph_hot = d->sph_hot.get(); p.sph_cold = d->sph_cold.get();
    p.tri_hot = d->tri_hot.get(); p.tri_geo = d->tri_geo.get();
    p.mats = d->mats.get();
    const Vec3 cv[4] = {cam.origin, cam.lower_left, cam.horizontal, cam.vertical};
    for (int i = 0; i < 4; ++i) { p.cam[3 * i] = cv[i].x; p.cam[3 * i + 1] = cv[i].y; p.cam[3 * i + 2] = cv[i].z; }
    p.wden = (float)(uint64_t)(width - 1);   // (width-1) as f32 (common.rs:335)
    p.hden = (float)(uint64_t)(height - 1);  // (height-1) as f32 (common.rs:336)
    // the camera divisions through exactdiv.h: a denominator in [2^-40, 2^40]
    // and its correctly rounded reciprocal (IEEE division on the host)
    auto den_ok = [](float b) { return b >= 0x1p-40f && b <= 0x1p40f; };
    p.xdiv_uv = den_ok(p.wden) && den_ok(p.hden);
    p.wrcp = p.xdiv_uv ? 1.0f / p.wden : 0.0f;
    p.hrcp = p.xdiv_uv ? 1.0f / p.hden : 0.0f;
    p.nsph = d->nsph; p.nsph_padded = d->nsph_padded; p.ntri = d->ntri;
    p.width = (uint32_t)width; p.height = (uint32_t)height;
    p.sph_shade = d->sph_shade.get();
    p.sph_kind = d->sph_kind.get();
    p.div_width = make_fastdiv((uint32_t)width);
}

// The sphere tree in global memory with its bounds (p.nnodes != 0 from here on)
void bind_sphere_tree(const WorldState &w, const DeviceState *d, TraceParams &p) {
    const SphereBVH &bv = w.bvh;
    p.bvh_nodes = d->bvh_nodes.get(); p.bvh_miss = d->bvh_miss.get();
    p.bvh_prims = d->bvh_prims.get(); p.bvh_prim_id = d->bvh_prim_id.get();
    p.big_hot = d->big_hot.get(); p.big_id = d->big_id.get();
    p.nnodes = d->nnodes; p.nbig = d->nbig; p.nprims = d->nprims;
    p.bvh_miss16 = d->bvh_miss16.get();
    for (int k = 0; k < 3; ++k) p.bvh_c[k] = bv.centre[k];
    p.bvh_r = bv.radius; p.bvh_rmax = bv.rmax; p.bvh_mag = bv.mag;
    p.bvh_inv_rmin = env_u64("RT_AMD_LINEAR_E", 0) ? INFINITY : bv.inv_rmin;
}

// The static triangle tree (binary nodes), its records and grids (p.tnodes != 0)
void bind_triangle_tree(const WorldState &w, const DeviceState *d, TraceParams &p) {
    const TriangleBVH &tb = w.tbvh;
    p.tbvh_nodes = d->tbvh_nodes.get();
    p.tbvh_tris = d->tbvh_tris.get(); p.tbvh_loose = d->tbvh_loose.get();
    p.tnodes = d->tnodes; p.ttris = d->ttris; p.tloose = d->tloose;
    for (int k = 0; k < 3; ++k) {
        p.tbvh_c[k] = tb.centre[k];
        p.tbvh_oc[k] = tb.oc[k];
        p.tq_base[k] = tb.qbox.base[k];
        p.tq_step[k] = tb.qbox.step[k];
    }
    p.tq_nbase = tb.nbase;
    p.tq_nstep = tb.nstep;
    p.tbvh_r = tb.radius; p.tbvh_mag = std::max(tb.mag, w.tcells.mag);
}

namespace {

// The per-camera arrays (camera records, host-built lists) are uploaded again
// under a new version into buffers that frames still in flight may be
// reading: a frame without stats is only enqueued, and the copy below runs on
// the null stream, which orders against neither the library's nor a caller's
// non-blocking stream.  So the host first waits for the device, as
// freeing the old buffer once did implicitly.  (Only when the camera or
// the frame size changed, next to a host rebuild of milliseconds.)
hipError_t wait_for_readers(bool buffer_exists) {
    return buffer_exists ? hipDeviceSynchronize() : hipSuccess;
}

// src into buf after wait_for_readers (synchronously: src is pageable and
// rebuilt by the next camera), at least min_elems elements; an empty buf for
// an empty src with no minimum: a null pointer means "none".  A capturing frame
// can do none of this: it is cold if it gets here.  A buffer that a graph's
// nodes name is moved aside first (DeviceState::retire), and a fresh one filled.
template <typename T, typename U>
int replace_contents(DeviceState *d, DevBuf<T> &buf, const std::vector<U> &src, bool capturing,
                     size_t min_elems = 0) {
    if (capturing) return cold_request("a per-camera array is not on the device yet");
    d->retire(buf);
    HIP_TRY(wait_for_readers((bool)buf));
    if (src.empty() && min_elems == 0) {
        buf.reset();
        return 0;
    }
    HIP_TRY(buf.upload(src, min_elems));
    return 0;
}

// Room for n elements of a scratch buffer; a capturing frame takes it as it is,
// and memory that a graph's nodes name is moved aside, not freed
template <typename T>
int grow_scratch(DeviceState *d, DevBuf<T> &buf, size_t n, bool capturing, const char *what) {
    if (n <= buf.cap()) return 0;
    if (capturing) return cold_request(what);
    d->retire(buf);
    HIP_TRY(buf.grow(n));
    return 0;
}

// what check_frame_request found (negative: an error)
enum { kFrameRender = 0, kFrameNothing = 1, kFrameSerial = 2 };

// One frame launch's schedule for a kernel instance: workgroups, waves, jobs
// per queue pull (chunk) and job-queue partitions
struct LaunchPlan { uint64_t blocks, nwaves, chunk, parts, block_threads; };

// The values of a frame that are derived once, by the steps below in order
struct FrameValues {
    bool capturing = false;            // render_frame: the caller's stream is capturing into a graph
    uint32_t nranks = 1, B = 1;        // check_frame_request: ranks, rows per row block ...
    size_t T = 0;                      // ... and this rank's tile rows
    uint32_t spp = 0;                  // plan_sample_storage
    uint64_t jobs_per_row = 0, slab_jobs = 0;
    size_t rows_per_slab = 0;
    bool fused = false, replay = false;
    size_t replay_upload = 0;          // the caller's REPLAY table goes to d->replay: its states (0: none)
    bool use_bvh = false;              // bind_sphere_search
    const uint4 *corner_img = nullptr; // the LDS tree as corner records (sphere-only frames), else box records
    TraceRequest want;                 // ... and what every launch asks for (render.h; kind: choose_kernel_instance)
    bool primary_lists = false;        // the frame's primary rays use candidate lists (spheres or triangles)
    SkyRows dev_sky;                   // ... and, with the device's lists, the sky rows classified with them
    SkyRows sky;                       // the rows this frame gives the sky kernel (choose_sky_rows; none: all traced)
    bool sky_fork = false;             // ... which may run beside the trace launches, on the device's side stream
    bool use_tbvh = false;             // bind_triangle_search
    int ptl_where = 0;                 // rt_primary_tri_lists: 0 none, 1 host build, 2 device build
    float inv_spp = 0.0f;
    bool timed = false;                // choose_kernel_instance (timed: the caller wants stats)
    TraceVariant tv{};                 // the instance the frame runs, the plain one apart: that is a launch's matter
    uint64_t waves_per_block = 0, full_blocks = 0, max_waves = 0;
};

// What enqueue_launches did, for the pending-stats record
struct LaunchesDone {
    LaunchPlan lean_plan{0, 0, 0, 0, 0};  // the uncounted (timed) kernel's schedule of the last launch
    TraceVariant variant{};               // ... and the instance it ran
    uint32_t launches = 0, waves = 0, nslab = 0;
    uint64_t samples = 0;
};

// Everything before the lock: the request's consistency, the tile's shape.
// (sp: d_out becomes a dummy.)
int check_frame_request(const RtRenderOptions &o, size_t width, size_t height, const SerialPass *sp,
                        const uint32_t *d_replay, const AccumPass *ap, uint32_t *&d_out, FrameValues &f) {
    const uint32_t nranks = o.nranks ? o.nranks : 1;
    if (o.rank >= nranks) { set_error("rank >= nranks"); return -1; }
    if (ap && (sp || nranks != 1 || o.rng_mode == RT_RNG_SERIAL || o.samples_per_pixel < 1 ||
               o.samples_per_pixel > 4096 || (o.flags & RT_FLAG_KEEP_SAMPLES))) {
        set_error("accumulation pass: one rank, COUNTER or REPLAY, 1 to 4096 samples, fused resolve");
        return -1;
    }
    if (o.rng_mode == RT_RNG_SERIAL && !sp && !d_replay)
        return kFrameSerial;
    if (!sp && o.rng_mode != RT_RNG_COUNTER && o.rng_mode != RT_RNG_REPLAY && !d_replay) {
        set_error("rng_mode must be RT_RNG_COUNTER, RT_RNG_REPLAY or RT_RNG_SERIAL");
        return -1;
    }
    if (o.rng_mode == RT_RNG_REPLAY && !o.replay_states && !d_replay) {
        set_error("replay table missing");
        return -1;
    }
    if (sp) d_out = reinterpret_cast<uint32_t *>(1);  // (a pass writes counts, not pixels)
    if (width > 0xFFFFFFu || height > 0xFFFFFFu) { set_error("frame too large"); return -1; }
    const uint32_t B = nranks > 1 ? (o.row_block ? o.row_block : 1) : (uint32_t)std::max<size_t>(height, 1);
    const size_t T = tile_rows(height, B, o.rank, nranks);
    if (width == 0 || T == 0) return kFrameNothing;
    if (!d_out) { set_error("null output"); return -1; }
    f.nranks = nranks;
    f.B = B;
    f.T = T;
    return kFrameRender;
}

// Fused resolve or slab, rows per launch, and room for the REPLAY table
int plan_sample_storage(DeviceState *d, const RtRenderOptions &o, size_t width, size_t height,
                        const SerialPass *sp, const uint32_t *d_replay, const AccumPass *ap, FrameValues &f) {
    const uint32_t spp = o.samples_per_pixel > 0 ? (uint32_t)o.samples_per_pixel : 0u;
    const uint64_t jobs_per_row = (uint64_t)width * spp;
    if (jobs_per_row > 0x7FFFFFFFull) { set_error("width*spp too large"); return -1; }
    // Fused resolve (default): samples live in per-wave rings and the trace
    // kernel writes the RGBA8 pixels.  The slab path (every sample to HBM, then
    // resolve_kernel) serves RT_FLAG_KEEP_SAMPLES and spp above 4096 (a ring
    // slot holds at least one whole pixel).
    // (accumulation passes always resolve in-kernel: the fold continues there)
    const bool fused = spp > 0 && spp <= 4096 && !(o.flags & RT_FLAG_KEEP_SAMPLES) &&
                       (ap != nullptr || env_u64("RT_AMD_FUSED", 1) != 0);
    // jobs per launch: 2^31 (fused: C3 in one launch) or 2^30 (a 12 GB slab)
    const uint64_t slab_jobs = env_u64("RT_AMD_SLAB_JOBS", fused ? (1ull << 31) - 1 : 1ull << 30);
    size_t rows_per_slab = jobs_per_row ? (size_t)std::max<uint64_t>(1, slab_jobs / jobs_per_row) : f.T;
    rows_per_slab = std::min(rows_per_slab, f.T);
    if (jobs_per_row && !fused)
        if (int rc = grow_scratch(d, d->samples, 3 * rows_per_slab * jobs_per_row, f.capturing,
                                  "the sample slab is too small"))
            return rc;

    // (the table's copy is enqueued with the launches: enqueue_launches)
    const bool replay = d_replay != nullptr || o.rng_mode == RT_RNG_REPLAY;
    if (!d_replay && !sp && o.rng_mode == RT_RNG_REPLAY && spp) {
        f.replay_upload = width * height * (size_t)spp;
        if (int rc = grow_scratch(d, d->replay, f.replay_upload, f.capturing,
                                  "the REPLAY table's buffer is too small"))
            return rc;
    }
    f.spp = spp;
    f.jobs_per_row = jobs_per_row;
    f.slab_jobs = slab_jobs;
    f.rows_per_slab = rows_per_slab;
    f.fused = fused;
    f.replay = replay;
    return 0;
}

// Scene pointers, camera, dimensions and the division constants
void bind_scene(DeviceState *d, const CameraModel &cam, size_t width, size_t height, const RtRenderOptions &o,
                const SerialPass *sp, const uint32_t *d_replay, const FrameValues &f, TraceParams &p) {
    bind_scene_arrays(d, cam, width, height, p);
    p.samples = d->samples.get();
    p.job_counter = d->counter.get();
    p.job_counter_next = nullptr;
    // (set 0 is also the SERIAL passes' scratch: the double-buffered frame sets
    // start over from a fill after them)
    if (sp) d->cset_clean[0] = d->cset_clean[1] = false;
    p.replay = d_replay ? d_replay : d->replay.get();
    p.spp = f.spp;
    p.depth = o.max_ray_bounces;
    p.mode = f.replay ? (uint32_t)RT_RNG_REPLAY : (uint32_t)RT_RNG_COUNTER;
    p.seed = o.seed;
    p.ablate = (uint32_t)env_u64("RT_AMD_ABLATE", 0);
    p.div_spp = make_fastdiv(f.spp ? f.spp : 1);
    p.div_rowblock = make_fastdiv(f.B);
    // node visits per lane per loop iteration of a sliced walk (A/B on C5, 8
    // waves per SIMD: 32 -> 277 ms, 64 -> 259, 96 -> 252, 128 -> 248, 192 ->
    // 251, 256 -> 263, 512 -> 353; 6 waves: 64 -> 243, 96 -> 240, 128 -> 242)
    p.steps = (uint32_t)std::max<uint64_t>(1, env_u64("RT_AMD_STEPS", 128));
    p.row_block = f.B; p.rank = o.rank; p.nranks = f.nranks;
}

// The sphere tree, its LDS layout (f.corner_img, f.want) and the
// primary sphere lists, built on the device or adopted from the host build
int bind_sphere_search(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                       const RtRenderOptions &o, const SerialPass *sp, hipStream_t s, FrameValues &f,
                       TraceParams &p) {
    f.use_bvh = d->nnodes > 0 && o.accel != RT_ACCEL_BRUTE;
    if (f.use_bvh) {
        bind_sphere_tree(w, d, p);
        // The LDS layout: corner records for the sphere-only frame kernels when
        // they fit (RT_AMD_CORNER=0: box records, for A/B runs and tests), box
        // records for the SERIAL passes and everything else; RT_AMD_LDS=0 or
        // neither fitting: the walk from global memory
        const bool lds_on = env_u64("RT_AMD_LDS", 1) != 0;
        if (lds_on && sp == nullptr && d->corner_bytes > 0 && env_u64("RT_AMD_CORNER", 1) != 0)
            f.corner_img = d->bvh_corner.get();
        f.want.corner = f.corner_img != nullptr;
        // (RT_AMD_LEAF_DEFER=0: the lean corner kernel tests leaves where it
        // enters them, for A/B runs and tests)
        f.want.defer = f.want.corner && env_u64("RT_AMD_LEAF_DEFER", 1) != 0;
        // (RT_AMD_PLAIN=0: every launch runs the generic instance, for A/B runs and tests;
        // so does a frame of depth <= 0: the plain instance ends a path after a hit)
        f.want.plain = f.want.defer && d->plain_fits() && p.depth >= 1 && env_u64("RT_AMD_PLAIN", 1) != 0;
        p.use_lds = lds_on && (d->lds_bytes > 0 || f.corner_img != nullptr);
        // sphere-only scenes: primary rays test their pixel's candidates
        if (d->ntri == 0 && env_u64("RT_AMD_SPHERE_LISTS", 1) != 0 && gpu_lists()) {
            bool ok = false;
            const int rc = device_sphere_lists(w, d, cam, width, height, s, f.capturing, ok);
            if (rc) return rc;
            p.spl = ok ? d->gspl.lists.get() : nullptr;
            f.primary_lists = ok;
            if (ok) f.dev_sky = d->gspl.sky;
        } else if (d->ntri == 0 && env_u64("RT_AMD_SPHERE_LISTS", 1) != 0) {
            bool current = false;
            if (int rc = prepare_primary_sphere_lists(w, cam, width, height, f.capturing, current)) return rc;
            if (current && d->spl_version != w.spl_version) {
                if (int rc = replace_contents(d, d->spl, w.spl.rec, f.capturing)) return rc;
                d->spl_version = w.spl_version;
            }
            if (current) p.spl = d->spl.get();
            f.primary_lists = p.spl != nullptr;
        }
    }
    return 0;
}

// The triangle trees, the camera-origin records (uploaded when the origin
// changed) and the primary strip lists: the device's, or the host's uploaded
// (f.ptl_where says which).  A capturing frame finds all of them current, or is cold.
int bind_triangle_search(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                         const RtRenderOptions &o, hipStream_t s, FrameValues &f, TraceParams &p) {
    f.use_tbvh = d->tnodes > 0 && o.accel != RT_ACCEL_BRUTE;
    const bool use_tbvh = f.use_tbvh;
    const bool want_ptl = width >= 2 && height >= 2 && env_u64("RT_AMD_PRIMARY_LISTS", 1) != 0;
    // the lists on the device (the records alone on the host)
    bool gpu_ptl = use_tbvh && want_ptl && gpu_tri_lists();
    const bool capturing = f.capturing;
    // (the host's per-camera builds: milliseconds of work that a capture would not repeat)
    if (use_tbvh && capturing &&
        !(camera_current(w, cam, !gpu_ptl && !want_ptl) &&
          (gpu_ptl || !want_ptl || !w.ctree_version || camera_lists_current(w, cam, width, height))))
        return cold_request("the camera's triangle records are not built for this camera and size");
    if (use_tbvh && gpu_ptl) {
        prepare_camera(w, cam, false);
    } else if (use_tbvh) {
        prepare_camera_lists(w, cam, width, height, want_ptl);
    }
    if (use_tbvh && w.ctree_version && d->cam_version != w.ctree_version) {
        const CameraTriangleBVH &ct = w.ctree;
        if (int rc = replace_contents(d, d->cam_tris, ct.tris, capturing)) return rc;
        d->cam_nnodes = 0;
        if (ct.nodes.empty()) {  // (records only)
            d->retire(d->cam_nodes);
            HIP_TRY(wait_for_readers((bool)d->cam_nodes));
            d->cam_nodes.reset();
        } else {
            if (int rc = replace_contents(d, d->cam_nodes, ct.qnodes, capturing)) return rc;
            d->cam_nnodes = (uint32_t)(ct.qnodes.size() / 8);
        }
        d->cam_version = w.ctree_version;
    }
    if (use_tbvh) {
        if (d->cam_tris && std::memcmp(w.ctree.origin, &cam.origin, 12) == 0) {
            p.cam_tris = d->cam_tris.get();
            if (d->cam_nnodes) {
                p.cam_nodes = d->cam_nodes.get();
                p.cam_nnodes = d->cam_nnodes;
            }
            bool dev_lists = false;
            if (gpu_ptl) {
                const int rc = device_tri_lists(w, d, cam, width, height, s, capturing, dev_lists);
                if (rc) return rc;
                if (d->gptl.host) {  // (beyond the kernels' range)
                    gpu_ptl = false;
                    if (capturing && !camera_lists_current(w, cam, width, height))
                        return cold_request("the primary triangle lists are not built for this camera and size");
                    prepare_camera_lists(w, cam, width, height, true);
                }
            }
            if (dev_lists) {
                f.primary_lists = true;
                f.ptl_where = 2;
                p.ptl_off = d->gptl.off.get();
                p.ptl_items = d->gptl.items.get();
                p.ptl_spr = d->gptl.spr;
                p.ptl_always = d->gptl.total;
                p.ptl_end = d->gptl.total + d->gptl.nalways;
            } else if (!gpu_ptl && want_ptl && camera_lists_current(w, cam, width, height)) {
                if (d->ptl_version != w.ptl_version) {
                    const PrimaryTriLists &pl = w.ptl;
                    if (int rc = replace_contents(d, d->ptl_off, pl.offsets, capturing)) return rc;
                    // (the items' pointer goes to the kernel even when there are none)
                    if (d->ptl_off) {
                        if (int rc = replace_contents(d, d->ptl_items, pl.items, capturing, 1)) return rc;
                    } else {
                        d->retire(d->ptl_items);
                        d->ptl_items.reset();
                    }
                    d->ptl_version = w.ptl_version;
                }
                if (d->ptl_off) {
                    f.primary_lists = true;
                    f.ptl_where = 1;
                    p.ptl_off = d->ptl_off.get();
                    p.ptl_items = d->ptl_items.get();
                    p.ptl_spr = w.ptl.strips_per_row;
                    p.ptl_always = w.ptl.offsets.back();
                    p.ptl_end = (uint32_t)w.ptl.items.size();
                }
            }
            for (int k = 0; k < 3; ++k) { p.cq_base[k] = w.ctree.qbox.base[k]; p.cq_step[k] = w.ctree.qbox.step[k]; }
        }
        bind_triangle_tree(w, d, p);
        if (d->tw_nodes) {
            p.tw_nodes = d->tw_nodes.get();
            p.tw_depth = d->tw_depth;
            p.tw_tris = (const float4 *)d->tbvh_tris.get();
            if (d->tw_tris) {
                const TriangleCells &tc = w.tcells;
                p.tw_tris = (const float4 *)d->tw_tris.get();
                p.tw_stride = tc.stride_w;
                p.tc_ncells = tc.ncells;
                for (int k = 0; k < 3; ++k) { p.tc_n[k] = tc.n[k]; p.tc_lo[k] = tc.lo[k]; }
                p.tc_size = tc.size;
                p.tc_inv_size = 1.0f / tc.size;
            }
            // wide-node fetches per lane per loop iteration of a sliced walk (A/B
            // on C5: 16 -> 166.1 ms, 20 -> 163.9, 24 -> 163.5, 28 -> 164.4, 32 -> 166.4)
            p.wsteps = (uint32_t)std::max<uint64_t>(1, env_u64("RT_AMD_WSTEPS", 24));
        }
    }
    return 0;
}

// every sample's alpha is exactly 1.0, so each pixel's
// alpha byte is this one fold, done once (resolve_kernel does it per pixel)
uint32_t alpha_byte(uint32_t nheld, float inv_spp) {
    float a = 1.0f;  // Color::new(0,0,0) has alpha 1 (color.rs:21-23)
    for (uint32_t k = 0; k < nheld && a + 1.0f != a; ++k) a = a + 1.0f;
    const float x = a * inv_spp * 255.999f;
    return !(x > 0.0f) ? 0u : x >= 255.0f ? 255u : (uint32_t)x;  // saturating `as u8`
}

// The instance a frame's launches of kernel kind `kind` run, the plain one
// apart (that takes the launch's chunk: enqueue_launches resolves it)
TraceVariant frame_variant(const TraceParams &p, TraceRequest want, int kind) {
    want.kind = kind, want.plain = false;
    return resolve_trace_variant(p, want);
}

// The walk's refill and gate thresholds, the kernel kind and instance the frame runs
// (f.want.kind, f.tv) with its occupancy, and the counters' buffer of a counted frame
int choose_kernel_instance(DeviceState *d, const SerialPass *sp, const AccumPass *ap, hipStream_t s,
                           FrameValues &f, TraceParams &p) {
    // sliced walks pay off when walk lengths vary a lot: scenes with a triangle tree
    p.step = (uint32_t)env_u64("RT_AMD_STEP", f.use_tbvh ? 1 : 0) != 0;
    // whole walks (sphere scenes): refill once half the wave is idle, so lanes
    // refilled together start samples of the same pixel and their primary
    // walks stay coherent (A/B on C2: 1 -> 6.16 ms, 8 -> 6.14, 16 -> 6.12,
    // 32 -> 6.10); sliced walks refill every iteration (C5: 32 costs +5 %)
    // The wide triangle walk (frames only; SERIAL passes walk the binary tree):
    // refill at 16 idle lanes and walk only when no lane can advance without
    // it (A/B on C5, refill / walk gate: 1 / 32 -> 163.5 ms, 8 / 32 -> 159.7,
    // 8 / 64 -> 156.8, 12 / 64 -> 153.1, 16 / 64 -> 151.8, 20 / 64 -> 152.2,
    // 24 / 64 -> 154.6, 32 / 64 -> 164.7)
    const bool wide_frame = p.tw_nodes != nullptr && sp == nullptr;
    p.refill_min = (uint32_t)std::max<uint64_t>(
        1, env_u64("RT_AMD_REFILL", wide_frame ? 16 : p.step ? 1 : 24));
    p.walk_min = (uint32_t)env_u64("RT_AMD_WALK_MIN", 65);  // sphere-only: walk when nothing else can advance
    p.tri_walk_min = (uint32_t)env_u64("RT_AMD_TRI_WALK_MIN", wide_frame ? 64 : 32);
    // (f.timed: HIP-event timing + counters need a host wait)
    // the counting kind iff p.stats (set below), the SERIAL instances for sp: launch_trace checks both
    // (an accumulation pass: its own kind, which has no counting twin -- a timed
    // pass gets its HIP-event times and schedule, the work counters stay 0)
    // (an adaptive pass: the accumulation kernels' twins that take their pixels from a list)
    f.want.kind = sp ? kKindSerial : ap && ap->list ? kKindAdapt : ap ? kKindAccum : f.timed ? kKindCounting : kKindLean;
    f.tv = frame_variant(p, f.want, f.want.kind);
    const TraceVariant tv = f.tv;
    if (ap && d->occupancy(tv) == 0) {
        int blocks = 0;
        HIP_TRY(trace_occupancy(&blocks, tv, trace_dyn_lds(p, tv)));
        if (const uint64_t bpc = env_u64("RT_AMD_BLOCKS_PER_CU", 0))
            if (tv.search != kSearchLdsCorner) blocks = (int)bpc;
        if (blocks < 1 && tv.lds()) { set_error("accumulation kernel does not fit its LDS tree"); return -1; }
        d->occupancy(tv) = std::max(blocks, 1);
    }
    f.waves_per_block = trace_block_threads(tv) / 64;
    f.full_blocks = (uint64_t)d->occupancy(tv) * (uint64_t)d->num_cus;
    // counters only when asked for: one 16-slot record per wave, summed here
    f.max_waves = ap ? 0 : f.full_blocks * f.waves_per_block;
    p.stats = nullptr;
    if (f.timed && !ap) {
        HIP_TRY(d->stats.grow(f.max_waves * kStatSlots));
        HIP_TRY(hipMemsetAsync(d->stats.get(), 0, f.max_waves * kStatSlots * 8, s));
        p.stats = d->stats.get();
    }
    return 0;
}

// The rows the frame renders with the sky kernel: those the
// lists' build classified, for a frame whose every traced sample of such a row
// would be the background and nothing else -- COUNTER, one rank, a sphere-only
// scene searched by the tree with primary lists, fused resolve, no counters,
// no pass, depth >= 1 (a frame of depth <= 0 is black).  RT_AMD_SKY_ROWS=0:
// every row is traced (A/B runs and tests).  RT_AMD_SKY_FORK=0: the sky kernel
// stays on the frame's stream, in front of the trace launches.
void choose_sky_rows(const DeviceState *d, const SerialPass *sp, const AccumPass *ap, FrameValues &f,
                     const TraceParams &p) {
    f.sky = SkyRows{};
    f.sky_fork = false;
    if (sp || ap || f.timed || !f.fused || f.replay || f.nranks != 1 || d->ntri != 0 || !f.use_bvh ||
        !f.primary_lists || p.depth < 1 || p.ablate != 0 || env_u64("RT_AMD_SKY_ROWS", 1) == 0)
        return;
    f.sky = f.dev_sky;
    f.sky_fork = env_u64("RT_AMD_SKY_FORK", 1) != 0;
}

// The join of a frame that forked: the frame's stream waits for the end of what
// the side stream holds.  Armed once that stream may hold work; a path that
// leaves enqueue_launches early (a failed launch) then still joins, and records
// the device's fence behind the join, so no work stays on the side stream that
// the caller's stream and `done` do not follow.
class SkyJoin {
public:
    SkyJoin(DeviceState *d, hipStream_t s) : d_(d), s_(s) {}
    SkyJoin(const SkyJoin &) = delete;
    SkyJoin &operator=(const SkyJoin &) = delete;
    ~SkyJoin() {
        if (armed_ && join() == hipSuccess) (void)d_->done.record(s_);
    }
    void arm() { armed_ = true; }
    hipError_t join() {
        armed_ = false;
        const hipError_t e = d_->sky_join.record(d_->sky_stream.get());
        return e != hipSuccess ? e : d_->sky_join.wait(s_);
    }

private:
    DeviceState *d_;
    hipStream_t s_;
    bool armed_ = false;
};

// launch_trace, with the instance it ran noted in the device's set (rt_trace_launched)
hipError_t launch_recorded(DeviceState *d, TraceVariant v, const TraceParams &p, const TraceTail &tail,
                           uint32_t blocks, hipStream_t s) {
    const hipError_t e = launch_trace(v, p, tail, blocks, s);
    if (e == hipSuccess) d->trace_launched[trace_key(v)] = 1;
    return e;
}

// One SERIAL pass instead of a frame (serial_states.cpp's inner launches).
// Its chunk and partition formula is its own, tuned apart from plan_launch's.
int launch_serial_pass(DeviceState *d, size_t width, size_t height, const RtRenderOptions &o,
                       const SerialPass *sp, hipStream_t s, const FrameValues &f, TraceParams &p) {
    const uint32_t spp = f.spp;
    // one SERIAL pass: nsamples x variants jobs (job = launch sample *
    // variants + variant); each stores its scatter count to slab plane 0
    const uint64_t njobs = (uint64_t)sp->nsamples * sp->variants;
    if (njobs == 0) return 0;
    if (njobs > 0x7FFFFFFFull) { set_error("serial pass too large"); return -1; }
    if (sp->mode != kRngSerialCoalesce && sp->mode != kRngSerialPixel)
        if (int rc = grow_scratch(d, d->samples, 3 * njobs, false, "")) return rc;
    p.samples = sp->mode == kRngSerialPixel ? sp->ptab : d->samples.get();
    p.sL = sp->L;
    p.sK = sp->Kmax;
    p.ring = nullptr;
    p.ring_shift = 0;
    p.mode = sp->mode;
    p.spp = sp->variants;
    p.div_spp = make_fastdiv(sp->variants);
    p.sspp = spp;
    p.div_sspp = make_fastdiv(spp ? spp : 1);
    p.cbase = sp->cbase;
    p.nserial = (uint32_t)((uint64_t)width * height * spp);
    p.win = sp->win;
    p.sM = sp->M;
    p.slo = sp->lo;
    p.spix = sp->spix;
    p.ctrl = sp->ctrl;
    p.max_draws = 2u + 3u * (uint32_t)std::max(o.max_ray_bounces, 0);
    p.njobs = (uint32_t)njobs;
    p.npix = sp->nsamples;
    p.slab_row0 = 0;
    const uint64_t waves_per_block = f.waves_per_block, full_blocks = f.full_blocks;
    const uint64_t jobs_per_block = waves_per_block * 256;
    const uint64_t blocks = std::max<uint64_t>(
        1, std::min<uint64_t>(full_blocks, (njobs + jobs_per_block - 1) / jobs_per_block));
    const uint64_t nwaves = blocks * waves_per_block;
    // the count pass: chunks of 128 jobs, not whole samples of K candidates
    // (the end of the launch drains sooner: c_raytracer 960x540x16 SERIAL
    // 671 -> 608 ms; 64: 610 ms; more partitions cost, 64: +8 %, 256: +30 %)
    uint64_t chunk = std::min<uint64_t>(256, std::max<uint64_t>(64, njobs / (nwaves * 16) / 64 * 64));
    chunk = chunk >= sp->variants ? chunk / sp->variants * sp->variants : sp->variants;
    if (sp->mode == kRngSerialCount) chunk = env_u64("RT_AMD_SERIAL_CCHUNK", 128);
    // the pixel table pass: chunks of consecutive positions of one pixel, not
    // whole pixels (a pixel's span is 10^3 positions: whole-pixel chunks
    // left most waves without work); 128 since round 5
    // (profiles/round5_serial/sweep_pchunk.jsonl: 64 / 128 / 192 / 256 / 512
    // -> world.txt 960x540x16 89.1 / 84.6 / 83.9 / 85.0 / 88.9 ms, 1920x1080x16
    // 365 / 337 / 334 / 337 / 355 ms, RTOW at C2 settings 699 / 665 / 670 /
    // 693 / 790 ms)
    if (sp->mode == kRngSerialPixel) chunk = env_u64("RT_AMD_SERIAL_PCHUNK", 128);
    p.chunk = (uint32_t)std::max<uint64_t>(1, chunk);
    uint64_t parts = std::max<uint64_t>(
        1, std::min<uint64_t>({(uint64_t)(p.step ? 64 : 16), kMaxParts, njobs / (16 * chunk) + 1}));
    if (const uint64_t np = env_u64("RT_AMD_SERIAL_PARTS", 0)) parts = std::min<uint64_t>(np, kMaxParts);
    p.nparts = (uint32_t)parts;
    if (sp->mode == kRngSerialPixel) {
        // (job counters zeroed by serial_window_kernel, kPixtabParts of them)
        p.nparts = (uint32_t)std::min<uint64_t>(parts, kPixtabParts);
        HIP_TRY(launch_recorded(d, resolve_trace_variant(p, f.want), p, TraceTail{}, (uint32_t)blocks, s));
    } else if (sp->mode == kRngSerialCoalesce) {
        // one workgroup per block of sp->R samples; the tree in LDS when it
        // fits beside the search's own arrays (64 KB per workgroup)
        const bool tree_lds = p.use_lds && serial_coalesce_lds(p, sp->variants, true) <= 64 * 1024;
        HIP_TRY(launch_serial_coalesce(p, sp->path, sp->bend, sp->nsamples, sp->variants, sp->R, tree_lds,
                                       sp->dbg, s));
    } else {
        HIP_TRY(hipMemsetAsync(d->counter.get(), 0, parts * 128, s));
        HIP_TRY(launch_recorded(d, resolve_trace_variant(p, f.want), p, TraceTail{}, (uint32_t)blocks, s));
    }
    HIP_TRY(d->done.record(s));
    d->last_jobs = 0;  // the slab holds counts now, not samples
    return 0;
}

// The schedule of one frame launch of njobs jobs with instance v
LaunchPlan plan_launch(DeviceState *d, const TraceParams &p, const FrameValues &f, TraceVariant v, uint64_t njobs) {
    const uint32_t spp = f.spp;
    const uint64_t wpb = trace_block_threads(v) / 64;
    const uint64_t jobs_per_block = wpb * 256;
    uint64_t blocks = std::min<uint64_t>((uint64_t)d->occupancy(v) * d->num_cus,
                                         (njobs + jobs_per_block - 1) / jobs_per_block);
    blocks = std::max<uint64_t>(blocks, 1);
    const uint64_t nwaves = blocks * wpb;
    uint64_t chunk = env_u64("RT_AMD_CHUNK", 0);
    if (!chunk) chunk = std::min<uint64_t>(256, std::max<uint64_t>(64, njobs / (nwaves * 16) / 64 * 64));
    // whole pixels per chunk (partitions are pixel-aligned too), so a
    // chunk's pixels are complete once its samples are
    chunk = chunk >= spp ? chunk / spp * spp : spp;
    if (f.fused) {
        // a resolve sums one pixel per lane, so whole-walk kernels take
        // chunks of >= 8 pixels (<= 4096 jobs unless spp is larger;
        // A/B, C2: 4 px 7.10 ms, 8 px 6.79, 16 px 6.83, 32 px 7.36,
        // slab + resolve_kernel 6.94).  Sliced walks keep their chunk
        // (C5: 16 px +1.5 %, 4 px = slab)
        uint64_t px = std::max<uint64_t>(1, std::min<uint64_t>(
            env_u64("RT_AMD_RESOLVE_PIX", p.step ? 1 : 8), 4096 / spp));
        // small launches (multi-GPU tiles) keep >= 16 chunks per wave
        // where 4-pixel chunks allow it (C2 tile of 8 ranks: 8 px 1.12 ms,
        // 4 px 1.04, 2 px 1.22; C3 tile of 8 ranks, 21 chunks of 8 px per
        // wave: 8 px 9.80 ms, 4 px 9.17, 2 px 9.32; of 4 ranks, 42: 8 and
        // 4 px 18.0 ms; of 2 ranks: 8 px 35.0, 4 px 35.5).  Round 5: 32
        // until then, which put the full C2 frame (31.6 chunks of 8 px per
        // wave at 8,192 waves) on 4-pixel chunks: lean frame 3.900 ms
        // against 3.745 ms with 8, 3.811 with 12 and 3.912 with 16 pixels
        // (profiles/round5_walk/ab_c2_chunk.jsonl); the 8-rank tile keeps
        // 4 px (0.678 ms, 8 px 0.849 ms).  The C2 launch without its 535 sky
        // rows has 15.97 chunks of 8 px per wave and takes
        // 4 px by this rule: 2.929 ms against 2.917 with 8 px, inside either
        // variant's spread of 0.03 (profiles/sky_rows/ab_c2.jsonl, new against
        // new8px, RT_AMD_CHUNKS_PER_WAVE=15; C3 has 250 chunks per wave either
        // way), so the rule stays at 16 for that launch too
        const uint64_t min_chunks = env_u64("RT_AMD_CHUNKS_PER_WAVE", 16);
        while (px > 4 && njobs / (nwaves * px * spp) < min_chunks) px /= 2;
        chunk = std::max<uint64_t>(chunk, px * spp);
    }
    // job-queue partitions: each keeps >= 16 chunks.  Whole-walk
    // kernels take 8: a wave whose partition is drained probes the
    // others one atomic at a time, so at the end of a launch fewer
    // partitions drain faster (A/B, round 2, C2: 64 -> 5.42 ms, 32 ->
    // 5.38, 16 -> 5.35, 8 -> 5.36; round 4, 8192 waves of 1024-thread
    // workgroups, lean frames: 16 -> 4.453 ms, 12 -> 4.335, 10 -> 4.331,
    // 8 -> 4.346, 4 -> +6 % on the tiles; 8-rank tile 16 -> 0.78, 8 ->
    // 0.76 ms; C3 62.44 -> 62.37 ms).  Sliced walks keep 64 (C5: 16
    // costs +1.6 %).
    uint64_t parts = env_u64("RT_AMD_PARTS", p.step ? 64 : 8);
    parts = std::max<uint64_t>(1, std::min<uint64_t>({parts, kMaxParts, njobs / (16 * chunk) + 1}));
    return LaunchPlan{blocks, nwaves, chunk, parts, wpb * 64};
}

// The sample rings of a fused launch with plan lp: log2 of a slot's samples, and the floats
uint32_t ring_shift_for(const LaunchPlan &lp) {
    uint32_t shift = 0;
    while ((1ull << shift) < lp.chunk) ++shift;
    return shift;
}
size_t ring_floats(const LaunchPlan &lp) { return lp.nwaves * 3 * ((size_t)kTraceRing << ring_shift_for(lp)); }

// The frame's launches: slabs of rows (an adaptive pass: of list entries),
// each on one of the two job-counter sets, then the end-of-frame events.
// A capturing frame ("Capture"): every launch on the third set
// behind a fill, the host's parity untouched, no fork and no fence recorded.
int enqueue_launches(DeviceState *d, size_t width, size_t height, uint32_t *d_out, const uint32_t *replay_table,
                     const AccumPass *ap, hipStream_t s, const FrameValues &f, TraceParams &p, LaunchesDone &done) {
    const uint32_t spp = f.spp;
    const bool fused = f.fused, timed = f.timed, adapt = f.want.kind == kKindAdapt;
    TraceTail tail;
    tail.corner = f.corner_img;
    done.variant = f.tv;  // (a frame without a launch reports its own)
    if (ap) {
        AccumState &acc = *ap->acc;
        // the sums are the accumulator's own, not the device's scratch: a pass on
        // another stream than the last one waits for it here
        HIP_TRY(acc.done.wait(s));
        // the first pass (after creation or a reset) starts every fold from 0.0f
        if (ap->n0 == 0) HIP_TRY(hipMemsetAsync(acc.sums.get(), 0, 3 * width * height * sizeof(float), s));
        tail.sums = acc.sums.get(), tail.n0 = ap->n0, tail.stride = acc.stride;
        if (adapt) tail.sumsq = acc.sumsq.get();
        if (adapt && ap->n0 == 0) {
            // ... and an adaptive one with zero counts and every pixel listed
            HIP_TRY(hipMemsetAsync(acc.sumsq.get(), 0, width * height * sizeof(float), s));
            HIP_TRY(hipMemsetAsync(acc.count.get(), 0, width * height * sizeof(uint32_t), s));
            HIP_TRY(launch_adapt_iota(const_cast<uint32_t *>(ap->list), (uint32_t)(width * height), s));
        }
    }
    // An adaptive pass enumerates its jobs from the list: the launches are
    // ranges of list entries (units of one pixel = spp jobs) instead of ranges
    // of rows (units of jobs_per_row jobs).
    const size_t units = adapt ? ap->nactive : f.T;
    const uint64_t jobs_per_unit = adapt ? spp : f.jobs_per_row;
    done.samples = (uint64_t)units * jobs_per_unit;
    const size_t units_per_slab =
        adapt ? (size_t)std::min<uint64_t>(std::max<uint64_t>(1, f.slab_jobs / spp), std::max<size_t>(units, 1))
              : f.rows_per_slab;
    // the sky rows in their own kernel: the trace launches take the rows between
    // the two blocks (none: no trace launch, and rt_trace_plain, rt_leaf_defer and
    // rt_trace_launched keep saying what the last trace launch ran)
    const size_t row_lo = f.sky.top, row_hi = units - f.sky.bottom;
    // (a capturing frame's rings are checked before its first node, not launch by launch)
    if (f.capturing && fused)
        for (size_t r0 = row_lo; r0 < row_hi; r0 += units_per_slab) {
            const uint64_t njobs = std::min(units_per_slab, row_hi - r0) * jobs_per_unit;
            if (njobs && ring_floats(plan_launch(d, p, f, f.tv, njobs)) > d->ring.cap())
                return cold_request("the sample rings are too small");
        }
    if (f.replay_upload)
        HIP_TRY(hipMemcpyAsync(d->replay.get(), replay_table, f.replay_upload * 4, hipMemcpyHostToDevice, s));
    d->last_sky_rows = f.sky.top + f.sky.bottom;
    // With trace launches to run beside, the sky kernel goes to the device's side
    // stream, behind this point of s (what s holds may still use d_out): it is
    // enqueued after the trace launches and at the lowest priority, so their
    // workgroups are placed first, and its waves take the slots that the trace
    // launch's last waves leave idle.  A capturing stream keeps
    // the one-stream order, so a captured frame has no parallel branches.
    const bool fork = d->last_sky_rows && row_lo < row_hi && f.sky_fork && !f.capturing;
    d->last_sky_forked = fork;
    SkyJoin sky(d, s);
    if (fork) {
        HIP_TRY(d->sky_fork.record(s));
    } else if (d->last_sky_rows) {
        HIP_TRY(launch_sky_rows(p, f.sky.top, f.sky.bottom, s));
    }
    uint32_t &nslab = done.nslab;  // (counted frames: event triple per launch)
    for (size_t r0 = row_lo; r0 < row_hi; r0 += units_per_slab, ++nslab) {
        const size_t rows = std::min(units_per_slab, row_hi - r0);
        DevEvent *ev3 = nullptr;
        if (timed) {
            if (d->tev.size() < 3 * (size_t)(nslab + 1)) d->tev.resize(3 * (size_t)(nslab + 1));
            ev3 = &d->tev[3 * (size_t)nslab];
            for (int k = 0; k < 3; ++k) HIP_TRY(ev3[k].create(true));
        }
        const uint64_t njobs = rows * jobs_per_unit;
        p.slab_row0 = adapt ? 0u : (uint32_t)r0;
        p.gj32 = f.nranks == 1 && (uint64_t)width * height * spp < (1ull << 32) ? 1u : 0u;
        p.gj_c0 = (uint32_t)(((uint64_t)height - 1 - r0) * width * spp);
        p.gj_2p = (uint32_t)(2ull * width * spp);
        // (accumulation: jobs at the accumulator's stride, render.h TraceTail)
        if (ap) p.gj32 = (uint64_t)width * height * ap->acc->stride < (1ull << 32) ? 1u : 0u;
        p.njobs = (uint32_t)njobs;
        p.npix = adapt ? (uint32_t)rows : (uint32_t)(rows * width);
        if (timed) HIP_TRY(hipEventRecord(ev3[0].get(), s));
        if (njobs) {
            const LaunchPlan lp = plan_launch(d, p, f, f.tv, njobs);
            const uint64_t blocks = lp.blocks, nwaves = lp.nwaves, chunk = lp.chunk, parts = lp.parts;
            p.chunk = (uint32_t)chunk;
            p.ring = nullptr;
            p.ring_shift = 0;
            if (fused) {
                p.ring_shift = ring_shift_for(lp);
                if (int rc = grow_scratch(d, d->ring, ring_floats(lp), f.capturing, "the sample rings are too small"))
                    return rc;
                p.ring = d->ring.get();
            }
            p.nparts = (uint32_t)parts;
            // two counter sets: this launch takes set cset (zeroed by the launch
            // before it, or filled here) and zeroes the other for the next one,
            // so back-to-back frames need no fill launch (a fill plus its gap
            // before the trace kernel was ~20 us of every C2 frame)
            // (a captured launch runs any number of times, unseen: set 2 behind a fill node)
            const uint32_t set = f.capturing ? 2u : d->cset;
            uint32_t *const cur = d->counter.get() + (size_t)set * kMaxParts * 32;
            if (f.capturing || !d->cset_clean[set]) HIP_TRY(hipMemsetAsync(cur, 0, parts * 128, s));
            p.job_counter = cur;
            p.job_counter_next = f.capturing ? nullptr : d->counter.get() + (size_t)(set ^ 1u) * kMaxParts * 32;
            // the launch's instance, resolved once (chunk, ring and gj32 are set per launch)
            const TraceVariant v = resolve_trace_variant(p, f.want);
            if (adapt) tail.list = ap->list + r0;
            HIP_TRY(launch_recorded(d, v, p, tail, (uint32_t)blocks, s));
            done.variant = v;
            d->last_leaf_defer = trace_leaf_defer(v);
            d->last_plain = v.leaf == TraceLeaf::Plain;
            d->last_ptl = f.ptl_where;
            if (!f.capturing) {
                d->cset_clean[d->cset] = false;
                d->cset ^= 1u;
                d->cset_clean[d->cset] = true;
            }
            p.job_counter = d->counter.get();
            p.job_counter_next = nullptr;
            done.lean_plan =
                f.want.kind != kKindCounting ? lp : plan_launch(d, p, f, frame_variant(p, f.want, kKindLean), njobs);
            d->last_jobs = fused ? 0 : njobs;
            d->last_spp = spp;
            d->last_fused = fused;  // rt_read_samples needs the slab
            ++done.launches;
            done.waves = (uint32_t)nwaves;
        }
        if (timed) HIP_TRY(hipEventRecord(ev3[1].get(), s));
        if (!fused)  // (spp 0: no samples, the resolve still writes every pixel)
            HIP_TRY(launch_resolve_ex(d->samples.get(), d_out, (uint32_t)(rows * width), spp, f.inv_spp,
                                      (uint32_t)width, (uint32_t)r0, s));
        if (timed) HIP_TRY(hipEventRecord(ev3[2].get(), s));
    }
    if (fork) {
        HIP_TRY(d->sky_fork.wait(d->sky_stream.get()));
        sky.arm();
        HIP_TRY(launch_sky_rows(p, f.sky.top, f.sky.bottom, d->sky_stream.get()));
        HIP_TRY(sky.join());
    }
    // (an event recorded on a capturing stream belongs to the graph: a later wait on
    // it would draw the waiting stream into the capture; replays are the caller's to order)
    if (!f.capturing) HIP_TRY(d->done.record(s));
    if (ap) HIP_TRY(ap->acc->done.record(s));
    return 0;
}

// What a captured frame's nodes name of the device state beyond the scene's
// own arrays -- the scratch and the per-camera arrays it bound -- is held from
// here on: a later camera, size or request that would rewrite, grow or free one
// of them gets a fresh buffer (DeviceState::retire), and the graph stays valid.
void hold_bound_buffers(DeviceState *d, const FrameValues &f, const TraceParams &p) {
    if (f.fused) d->ring.hold();
    else d->samples.hold();
    if (f.replay_upload) d->replay.hold();
    if (p.spl == d->gspl.lists.get()) d->gspl.lists.hold();
    if (p.spl == d->spl.get()) d->spl.hold();
    if (p.cam_tris) d->cam_tris.hold();
    if (p.cam_nodes) d->cam_nodes.hold();
    if (p.ptl_off == d->gptl.off.get()) d->gptl.off.hold(), d->gptl.items.hold();
    if (p.ptl_off == d->ptl_off.get()) d->ptl_off.hold(), d->ptl_items.hold();
}

// A counted frame's pending record on its device (collect_frame_stats reads it)
int queue_frame_stats(DeviceState *d, hipStream_t s, const FrameValues &f, const TraceParams &p,
                      const LaunchesDone &done) {
    const bool use_bvh = f.use_bvh, use_tbvh = f.use_tbvh;
    // the wave records into pinned host memory (an asynchronous copy, so a
    // deferred frame does not wait here)
    const size_t nrec = f.max_waves * kStatSlots;
    HIP_TRY(d->hrec.grow(nrec));
    if (nrec) HIP_TRY(hipMemcpyAsync(d->hrec.get(), d->stats.get(), nrec * 8, hipMemcpyDeviceToHost, s));
    auto &pd = d->pend;
    pd.active = true;
    pd.nrec = nrec;
    pd.nslab = done.nslab;
    pd.launches = done.launches;
    pd.samples = done.samples;
    pd.use_bvh = use_bvh;
    pd.use_tbvh = use_tbvh;
    pd.stream = s;
    RtRenderStatsFixed &fx = pd.fixed;
    fx = RtRenderStatsFixed{};
    fx.waves = done.waves;
    fx.accel = (use_bvh || use_tbvh) ? RT_ACCEL_BVH : RT_ACCEL_BRUTE;
    fx.tri_bvh = use_tbvh ? 1u : 0u;
    fx.fused_resolve = f.fused ? 1u : 0u;
    fx.primary_lists = f.primary_lists ? 1u : 0u;
    fx.camera_tree = p.cam_tris != nullptr ? 1u : 0u;  // camera-origin records (tree or lists)
    // (the schedule of the frame's uncounted kernel: what a timed frame runs)
    fx.launch_parts = (uint32_t)done.lean_plan.parts;
    fx.launch_chunk = (uint32_t)done.lean_plan.chunk;
    fx.launch_refill_min = p.refill_min;
    fx.launch_walk_min = p.walk_min;
    fx.launch_tri_walk_min = p.tri_walk_min;
    fx.launch_wsteps = p.wsteps;
    fx.launch_block_threads = (uint32_t)done.lean_plan.block_threads;
    fx.launch_blocks = (uint32_t)done.lean_plan.blocks;
    const TraceVariant v = done.variant;
    fx.sphere_tree = (uint32_t)v.search;
    fx.sphere_tree_lds_bytes = v.lds() ? (uint32_t)trace_lds_bytes(p, v.search == kSearchLdsCorner) : 0u;
    fx.nsph = d->nsph;
    fx.ntri = d->ntri;
    fx.nbig = d->nbig;
    return 0;
}

}  // namespace

// bind_triangle_search for a caller outside this unit (first_hit.cpp): the
// static tree and, where they apply, the camera-origin records and primary
// strip lists, made current for (cam, width, height) as for a frame.
int bind_primary_triangle_search(WorldState &w, DeviceState *d, const CameraModel &cam, size_t width, size_t height,
                                 int32_t accel, hipStream_t s, TraceParams &p) {
    RtRenderOptions o{};
    o.accel = accel;
    FrameValues f;
    return bind_triangle_search(w, d, cam, width, height, o, s, f, p);
}

int render_frame(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                 const RtRenderOptions &o, uint32_t *d_out, hipStream_t stream,
                 RtRenderStats *stats, const SerialPass *sp, const uint32_t *d_replay, bool defer_stats,
                 const AccumPass *ap) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    FrameValues f;
    // A caller's stream that is capturing into a graph (raytracer_amd.h, rt_render_device):
    // the one query of the frame.  Such a frame is warm -- nothing below allocates,
    // uploads, builds lists or waits on the host for it -- or refused as cold.
    f.capturing = stream_capturing(stream);
    if (f.capturing && stats) return refuse_capture("rt_render_device", "a frame with stats");
    int rc = check_frame_request(o, width, height, sp, d_replay, ap, d_out, f);
    if (f.capturing && rc == kFrameSerial) return refuse_capture("rt_render_device", "a SERIAL frame");
    if (rc == kFrameSerial) return render_frame_serial(w, cam, width, height, o, d_out, stream, stats);
    if (rc) return rc < 0 ? rc : 0;

    std::lock_guard<std::recursive_mutex> lock(w.mu);
    DeviceState *d = nullptr;
    rc = device_for(w, o.device, d, f.capturing);
    if (rc) return rc;
    hipStream_t s = stream ? stream : d->stream.get();
    // the device's scratch (job counters, rings, slab, stats) is shared by every
    // frame on it: a frame enqueued on another stream waits for the last one
    // (a capturing frame enqueues nothing that runs now, and its replays are the
    // caller's to order: no wait node, and no wait on an event outside the capture)
    if (!f.capturing) HIP_TRY(d->done.wait(s));

    rc = plan_sample_storage(d, o, width, height, sp, d_replay, ap, f);
    if (rc) return rc;
    TraceParams p{};
    bind_scene(d, cam, width, height, o, sp, d_replay, f, p);
    rc = bind_sphere_search(w, d, cam, width, height, o, sp, s, f, p);
    if (rc) return rc;
    rc = bind_triangle_search(w, d, cam, width, height, o, s, f, p);
    if (rc) return rc;
    // (an accumulation pass writes the frame of all N = n0 + n samples held after it)
    const uint32_t nheld = ap ? ap->n0 + f.spp : f.spp;
    f.inv_spp = ap ? 1.0f / (float)nheld
                   : 1.0f / (float)o.samples_per_pixel;  // 1.0 / spp as f32 (common.rs:345)
    p.inv_spp = f.inv_spp;
    p.alpha_u8 = alpha_byte(nheld, f.inv_spp);
    p.out = d_out;
    f.timed = stats != nullptr;
    rc = choose_kernel_instance(d, sp, ap, s, f, p);
    if (rc) return rc;
    if (sp) return launch_serial_pass(d, width, height, o, sp, s, f, p);
    choose_sky_rows(d, sp, ap, f, p);

    LaunchesDone done;
    rc = enqueue_launches(d, width, height, d_out, o.replay_states, ap, s, f, p, done);
    if (rc) return rc;
    if (f.capturing) hold_bound_buffers(d, f, p);
    classify_pending_sky_rows(w, d);  // (for the next frame, while the device runs this one)
    // without stats the frame stays asynchronous on the stream (no host wait)
    if (!f.timed) return 0;
    rc = queue_frame_stats(d, s, f, p, done);
    if (rc || defer_stats) return rc;
    return collect_frame_stats(d, stats);
}

int collect_frame_stats(DeviceState *d, RtRenderStats *stats) {
    auto &pd = d->pend;
    if (!pd.active) {
        set_error("no counted frame pending on this device");
        return -1;
    }
    pd.active = false;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(pd.stream));
    double trace_ms = 0.0, resolve_ms = 0.0;
    for (uint32_t k = 0; k < pd.nslab; ++k) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, d->tev[3 * k].get(), d->tev[3 * k + 1].get()));
        HIP_TRY(hipEventElapsedTime(&b, d->tev[3 * k + 1].get(), d->tev[3 * k + 2].get()));
        trace_ms += a;
        resolve_ms += b;
    }
    const unsigned long long *rec = d->hrec.get();
    if (const char *dump = std::getenv("RT_AMD_WAVE_DUMP")) {  // diagnostic: raw per-wave records
        if (FILE *f = std::fopen(dump, "wb")) {
            std::fwrite(rec, 8, pd.nrec, f);
            std::fclose(f);
        }
    }
    unsigned long long st[kStatSlots] = {};
    for (size_t i = 0; i < pd.nrec; ++i) st[i % kStatSlots] += rec[i];
    if (stats) {
        const RtRenderStatsFixed &fx = pd.fixed;
        const bool use_bvh = pd.use_bvh, use_tbvh = pd.use_tbvh;
        stats->samples = pd.samples;
        stats->rays = st[0];
        stats->sphere_tests = st[0] * (uint64_t)fx.nsph;
        stats->tri_tests = st[0] * (uint64_t)fx.ntri;  // the reference's brute-force count
        stats->tri_in_range = st[1];
        stats->trace_ms = trace_ms;
        stats->resolve_ms = resolve_ms;
        stats->trace_launches = pd.launches;
        stats->waves = fx.waves;
        stats->launch_parts = fx.launch_parts;
        stats->launch_chunk = fx.launch_chunk;
        stats->launch_refill_min = fx.launch_refill_min;
        stats->launch_walk_min = fx.launch_walk_min;
        stats->launch_tri_walk_min = fx.launch_tri_walk_min;
        stats->launch_wsteps = fx.launch_wsteps;
        stats->launch_block_threads = fx.launch_block_threads;
        stats->launch_blocks = fx.launch_blocks;
        stats->sphere_tree = fx.sphere_tree;
        stats->sphere_tree_lds_bytes = fx.sphere_tree_lds_bytes;
        stats->accel = fx.accel;
        stats->bvh_sphere_tests = st[2];
        stats->bvh_node_tests = st[3];
        stats->big_sphere_tests = use_bvh ? st[0] * (uint64_t)fx.nbig : st[0] * (uint64_t)fx.nsph;
        for (int k = 0; k < 4; ++k) stats->stamp_cycles[k] = st[4 + k];
#ifdef RT_STAMPS
        {   // fine segments (tools/stamps.py parses this line)
            double tot = 0;
            for (uint32_t k = 0; k < kStampSegs; ++k) tot += (double)st[16 + k];
            std::fprintf(stderr, "stamp segments:");
            for (uint32_t k = 0; k < kStampSegs; ++k) std::fprintf(stderr, " %.4f", st[16 + k] / std::max(1.0, tot));
            std::fprintf(stderr, " cycles %.6e\n", tot);
        }
#endif
        stats->tri_node_tests = st[8];
#ifdef RT_WALK_MIX
        std::fprintf(stderr, "walk mix: %llu walks, %.2f iterations per walk, %.2f with a leaf, %.2f leaf trips\n",
                     st[7], st[4] / std::max(1.0, (double)st[7]), st[5] / std::max(1.0, (double)st[7]),
                     st[6] / std::max(1.0, (double)st[7]));
#endif
        if (env_u64("RT_AMD_ITER_DEBUG", 0))
            std::fprintf(stderr, "iteration mix: %llu iterations (%.1f active lanes), %llu walking (%.1f lanes), "
                         "%llu other (%.1f lanes)\n", st[10], st[12] / std::max(1.0, (double)st[10]), st[11],
                         st[13] / std::max(1.0, (double)st[11]), st[10] - st[11],
                         (st[12] - st[13]) / std::max(1.0, (double)(st[10] - st[11])));
        stats->tri_bvh = fx.tri_bvh;
        stats->fused_resolve = fx.fused_resolve;
        stats->primary_lists = fx.primary_lists;
        stats->camera_tree = fx.camera_tree;
        stats->bvh_tri_tests = use_tbvh ? st[9] : stats->tri_tests;
    }
    return 0;
}

int leaf_defer(WorldState &w, int device) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    return d->last_leaf_defer;
}

int trace_plain(WorldState &w, int device) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    return d->last_plain ? 1 : 0;
}

int sky_rows(WorldState &w, int device) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    return (int)d->last_sky_rows;
}

int sky_forked(WorldState &w, int device) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    return d->last_sky_forked ? 1 : 0;
}

int trace_launched(WorldState &w, int device, uint8_t *out, size_t n, bool clear) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    if (out) std::memcpy(out, d->trace_launched, std::min<size_t>(n, kTraceKeys));
    if (clear) std::memset(d->trace_launched, 0, sizeof(d->trace_launched));
    return kTraceKeys;
}

int trace_instances(uint8_t *out, size_t n) {
    for (int key = 0; key < kTraceKeys && (size_t)key < n && out; ++key)
        out[key] = trace_instance_exists(key) ? 1 : 0;
    return kTraceKeys;
}

int primary_tri_lists(WorldState &w, int device) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    return d->last_ptl;
}

long read_samples(WorldState &w, int device, float *out, size_t n) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);  // (device_for may add a device)
    DeviceState *d = nullptr;
    int rc = device_for(w, device, d);
    if (rc) return rc;
    if (d->last_fused) {
        set_error("rt_read_samples: the last launch resolved in the trace kernel "
                  "(render with RT_FLAG_KEEP_SAMPLES to keep the samples)");
        return -1;
    }
    const size_t count = std::min(n / 4, d->last_jobs);
    if (!count) return 0;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float> planes(3 * d->last_jobs);
    for (int c = 0; c < 3; ++c)
        HIP_TRY(hipMemcpy(planes.data() + c * d->last_jobs, d->samples.get() + c * d->last_jobs,
                          d->last_jobs * sizeof(float), hipMemcpyDeviceToHost));
    // (r, g, b, 0) per sample, as documented: sample-major order (s * npix +
    // pixel) from the pixel-major slab (pixel * spp + s)
    const size_t spp = std::max<size_t>(1, d->last_spp), npix = d->last_jobs / spp;
    for (size_t i = 0; i < count; ++i) {
        const size_t src = (i % npix) * spp + i / npix;
        out[4 * i] = planes[src];
        out[4 * i + 1] = planes[d->last_jobs + src];
        out[4 * i + 2] = planes[2 * d->last_jobs + src];
        out[4 * i + 3] = 0.0f;
    }
    return (long)(count * 4);
}

int render_frame_host(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                      const RtRenderOptions &o, void *host_out, RtRenderStats *stats) {
    std::lock_guard<std::recursive_mutex> lock(w.mu);
    if (o.ndevices >= 1) {
        if (width == 0 || height == 0) {
            if (stats) std::memset(stats, 0, sizeof(*stats));
            return 0;
        }
        if (!host_out) { set_error("null framebuffer pixels"); return -1; }
        std::vector<int> devs;
        int rc = device_list(o.device, o.ndevices, devs);
        if (rc) return rc;
        DeviceState *root = nullptr;
        rc = device_for(w, devs[0], root);
        if (rc) return rc;
        HIP_TRY(root->out.grow(width * height));
        hipStream_t s = root->stream.get();
        rc = render_frame_multi(w, cam, width, height, o, root->out.get(), s, stats);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(devs[0]));
        HIP_TRY(hipMemcpyAsync(host_out, root->out.get(), width * height * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    }
    const uint32_t nranks = o.nranks ? o.nranks : 1;
    const uint32_t B = nranks > 1 ? (o.row_block ? o.row_block : 1) : (uint32_t)std::max<size_t>(height, 1);
    const size_t T = o.rank < nranks ? tile_rows(height, B, o.rank, nranks) : 0;
    if (width == 0 || T == 0) {
        if (stats) std::memset(stats, 0, sizeof(*stats));
        return o.rank < nranks ? 0 : -1;
    }
    if (!host_out) { set_error("null framebuffer pixels"); return -1; }
    DeviceState *d = nullptr;
    int rc = device_for(w, o.device, d);
    if (rc) return rc;
    HIP_TRY(d->out.grow(T * width));
    hipStream_t s = d->stream.get();
    rc = render_frame(w, cam, width, height, o, d->out.get(), s, stats);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(host_out, d->out.get(), T * width * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}
}  // namespace rtamd
