// runtime.h -- device-side state of a loaded world and the frame driver.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <cstring>
#include <future>
#include <map>
#include <mutex>
#include <memory>
#include <string>
#include <vector>

#include "bvh.h"
#include "device_buffer.h"
#include "device_fence.h"
#include "render.h"
#include "scene.h"

struct RtRenderOptions;
struct RtRenderStats;
struct RtFirstHitOptions;
struct RtFilterOptions;

namespace rtamd {

// The RtRenderStats fields of a counted frame that the host knows when it
// enqueues the frame (the rest come from the device's wave records).
struct RtRenderStatsFixed {
    uint32_t waves = 0, accel = 0, tri_bvh = 0, fused_resolve = 0, primary_lists = 0, camera_tree = 0;
    uint32_t launch_parts = 0, launch_chunk = 0, launch_refill_min = 0, launch_walk_min = 0;
    uint32_t launch_tri_walk_min = 0, launch_wsteps = 0, launch_block_threads = 0, launch_blocks = 0;
    uint32_t nsph = 0, ntri = 0, nbig = 0;
    uint32_t sphere_tree = 0, sphere_tree_lds_bytes = 0;
};

void set_error(const std::string &msg);
const std::string &last_error();

// One device's copy of a scene plus the scratch a frame needs.  Buffers grow
// on demand and persist across frames (the interactive flow re-renders the
// same scene with a moved camera, GameView.swift:198-219 / lib.rs:60-63).
// Every member owns what it holds (device_buffer.h, device_fence.h): the
// destructor selects the device, the members follow.
struct DeviceState {
    int device = -1;
    // WorldState::edit_version the scene arrays were uploaded under: device_for
    // refreshes the state in place when the world's has moved on (device_state.cpp)
    uint64_t edit_version = 0;
    size_t lds_hw_cap = 0;  // LDS a workgroup may take here (the kernels' opt-in, asked once at set-up)
    DevStream stream;
    DevEvent sev[3];  // SERIAL mode: start, tables done, states found
    DevBuf<float4> sph_hot, sph_cold, tri_hot, tri_geo;
    DevBuf<float> mats;
    DevBuf<float4> sph_shade;
    DevBuf<uint32_t> sph_kind;
    uint32_t nsph = 0, nsph_padded = 0, ntri = 0;
    DevBuf<float4> bvh_nodes, bvh_prims, big_hot;
    DevBuf<uint32_t> bvh_miss, bvh_prim_id, big_id;
    DevBuf<uint16_t> bvh_miss16;                                // (null: no LDS box tree)
    uint32_t nnodes = 0, nbig = 0, nprims = 0;
    DevBuf<uint4> tbvh_nodes;                                   // triangle BVH (bvh.h qnodes)
    DevBuf<float4> tbvh_tris;
    DevBuf<uint32_t> tbvh_loose;
    uint32_t tnodes = 0, ttris = 0, tloose = 0;
    DevBuf<uint4> tw_nodes;                                     // its 4-wide image (bvh.h wnodes); null: binary walk
    uint32_t tw_depth = 0;                                      // stack entries per lane
    DevBuf<float> tw_tris;                                      // per-cell trees' records (tcells); null: none
    DevBuf<uint4> cam_nodes;                                    // camera-origin triangle BVH (null: records only)
    DevBuf<float4> cam_tris;                                    // (null: no camera records)
    uint32_t cam_nnodes = 0;
    uint64_t cam_version = 0;                                  // WorldState::ctree_version uploaded
    DevBuf<uint32_t> ptl_off, ptl_items;                        // primary-ray triangle lists (ptl_off null: none)
    uint64_t ptl_version = 0;
    DevBuf<uint2> spl;                                          // primary sphere lists (null: every ray walks)
    uint64_t spl_version = 0;
    // primary sphere lists built on the device (serial.hip launch_sphere_lists)
    // for (cam, w, h); ok = false: no lists (every primary ray walks)
    struct DeviceSphereLists {
        DevBuf<uint2> lists;
        DevBuf<int4> rects;
        DevBuf<uint32_t> flag;
        CameraModel cam{};
        size_t w = 0, h = 0;
        bool built = false, ok = false;
        SkyRows sky;                                           // the lists' sky rows (none without lists) ...
        bool sky_pending = false;                              // ... still to be classified (classify_pending_sky_rows)
        bool current(const CameraModel &c, size_t width, size_t height) const {
            return built && w == width && h == height && std::memcmp(&cam, &c, sizeof(c)) == 0;
        }
        void remember(const CameraModel &c, size_t width, size_t height) {
            cam = c;
            w = width;
            h = height;
            built = true;
        }
    } gspl;
    // primary triangle strip lists built on the device (tri_lists.hip) for
    // (cam, w, h, ctree): the records' boxes (uploaded once per
    // ctree_version), the lists, scratch
    struct DeviceTriLists {
        DevBuf<float> box;
        uint64_t box_version = 0;                              // WorldState::ctree_version uploaded
        DevBuf<uint32_t> off, items;
        DevBuf<int4> rects;
        DevBuf<uint32_t> count, alw, meta;
        PinnedBuf<uint32_t> hmeta;                             // (the lengths read back)
        CameraModel cam{};
        size_t w = 0, h = 0;
        uint64_t ctree = 0;
        uint32_t spr = 0, total = 0, nalways = 0;
        bool built = false, ok = false, host = false;          // host: out of range, the host builds
        bool current(const CameraModel &c, size_t width, size_t height, uint64_t ctree_version) const {
            return built && w == width && h == height && ctree == ctree_version &&
                   std::memcmp(&cam, &c, sizeof(c)) == 0;
        }
        void remember(const CameraModel &c, size_t width, size_t height, uint64_t ctree_version) {
            cam = c;
            w = width;
            h = height;
            ctree = ctree_version;
            built = true;
        }
    } gptl;
    int last_ptl = 0;                                          // rt_primary_tri_lists of the last launch
    size_t lds_bytes = 0;                                      // 0: tree not LDS-stageable
    // corner records (bvh.h SphereBVH::corner), uploaded when the sphere-only
    // frame kernels can stage them without losing a workgroup per CU
    DevBuf<uint4> bvh_corner;                                   // (null: none uploaded)
    size_t corner_bytes = 0;                                   // 0: box records (or no LDS tree)
    DevBuf<float> samples;                                      // sample slab (3 planes)
    DevBuf<float> ring;                                         // per-wave sample rings (fused resolve)
    DevBuf<uint32_t> out;                                       // RGBA8 tile (host path)
    DevBuf<uint32_t> tile;                                      // multi-device: this rank's tile
    DevBuf<uint32_t> gath;                                      // multi-device root: gathered tiles
    DevBuf<uint32_t> first_hit;                                 // first-hit records / views (host path)
    Fence done;                      // the last work enqueued on the scratch and the scene arrays
    // A frame's sky kernel beside its trace launches (frame.cpp enqueue_launches):
    // the side stream (lowest priority; created with the library's stream at device
    // set-up), the point of the frame's stream it starts behind and its end, which
    // the frame's stream waits for before it records `done`
    DevStream sky_stream;
    Fence sky_fork, sky_join;
    DevBuf<uint32_t> replay;
    // SERIAL mode (render_frame_serial): start states, candidate offsets, the
    // stream window of a chunk, xorshift jump matrices, control block
    DevBuf<uint32_t> sstates;
    DevBuf<double> stab;                                        // prediction tables (render.h serial_tab_doubles)
    DevBuf<double> sscan;                                       // their scan's scratch
    DevBuf<uint32_t> slo;                                       // an iteration's window bases (launch_serial_window)
    DevBuf<uint32_t> ssbend;                                    // superblock ends and block starts (launch_serial_walk)
    DevBuf<uint32_t> ssb;
    DevBuf<uint32_t> swin;
    DevBuf<uint32_t> sbend;
    DevBuf<uint32_t> spath;                                     // block walks' paths (L x K)
    DevBuf<float> sptab;                                        // pixel table pass: b per (pixel, position)
    DevBuf<uint4> sspix;                                        // pixel table pass: spans per pixel, 2 buffers
    DevBuf<float> sptab2;                                       // (the previous iteration's table: reuse)
    DevBuf<uint32_t> sfin;                                      // chain result (4 + kMaxWalkBlocks)
    DevBuf<uint32_t> sjump;
    DevBuf<uint32_t> sctrl;
    DevBuf<unsigned long long> scheck;                          // chain-check count
    DevBuf<uint32_t> counter;                                   // job counters: 3 sets of kMaxParts
    uint32_t cset = 0;              // the set (0 or 1) the next frame launch uses ...
    bool cset_clean[2] = {false, false};  // ... and whether each set is known to be zero
    // (set 2: the launches captured into a graph, which run when the host does not
    // see them; each fills it first and leaves cset and cset_clean alone)
    DevBuf<unsigned long long> stats;                           // per-wave counter records
    // resident workgroups per CU of the scene's kernel instances, by render.h
    // trace_key less the mesh: a device holds one scene, whose frames all plan
    // with its family's figures (a RT_ACCEL_BRUTE frame too).  The frame kinds
    // and the two deferred-leaf instances are queried once at device set-up (the
    // corner search: lean and counting only), the accumulation kinds by the
    // first pass that runs an instance, 0 until then (same workgroup size, LDS
    // request and waves per SIMD as the lean twin the set-up decided with).
    // A variant without an instance: kTraceNoKey's slot, which stays 0.
    int blocks_per_cu[kTraceKeys] = {};
    int &occupancy(TraceVariant v) {
        v.mesh = 0;
        return blocks_per_cu[trace_key(v)];
    }
    // the plain instance may run: it keeps the deferred-leaf instance's workgroups, which the launch plans use
    bool plain_fits() const {
        return blocks_per_cu[kTraceKeyPlain] != 0 && blocks_per_cu[kTraceKeyPlain] == blocks_per_cu[kTraceKeyDeferred];
    }
    int num_cus = 0;
    // a counted frame's timing events (3 per launch: start, trace end, resolve
    // end) and its wave records copied to pinned host memory; with
    // render_frame(..., defer_stats) the host collects them later
    // (collect_frame_stats), so several devices' counted frames run at once
    std::vector<DevEvent> tev;
    PinnedBuf<unsigned long long> hrec;
    struct PendingStats {
        bool active = false;
        size_t nrec = 0;          // records (waves x kStatSlots) in hrec
        uint32_t nslab = 0;       // event triples in tev (one per slab)
        uint32_t launches = 0;    // trace launches
        uint64_t samples = 0;
        bool use_bvh = false, use_tbvh = false;
        RtRenderStatsFixed fixed; // the fields known before the frame ran
        hipStream_t stream = nullptr;
    } pend;
    size_t last_jobs = 0;                                       // jobs of the last launch
    size_t last_spp = 0;                                        // and its spp
    bool last_fused = false;                                    // it resolved in-kernel (no slab)
    int last_leaf_defer = 0;                                    // its walk's pending leaves per lane (rt_leaf_defer)
    bool last_plain = false;                                    // it ran the plain instance (rt_trace_plain)
    uint32_t last_sky_rows = 0;                                 // rows the last frame launch gave the sky kernel (rt_sky_rows)
    bool last_sky_forked = false;                               // ... and that kernel ran on sky_stream (rt_sky_forked)
    // the instances launched on this device since the last clear, one byte per
    // render.h trace_key (rt_trace_launched): frames, passes and SERIAL passes
    uint8_t trace_launched[kTraceKeys] = {};
    // Buffers that captured frames bound (DevBuf::hold) and that a later camera,
    // size or request would have rewritten, grown or freed: moved here instead,
    // with their memory, and freed with the device state.  A graph's nodes so
    // stay valid until the scene is edited or the world freed ("Capture").
    std::vector<std::shared_ptr<void>> retired;
    template <typename T>
    void retire(DevBuf<T> &buf) {
        if (buf.held()) retired.push_back(std::make_shared<DevBuf<T>>(std::move(buf)));
    }
    ~DeviceState();
};

struct AccumState;

struct WorldState {
    SceneModel scene;
    PackedScene packed;
    SphereBVH bvh;
    uint32_t sphere_leaf = 2;  // spheres per leaf bvh was built with (a geometry edit rebuilds at it)
    TriangleBVH tbvh;
    TriangleCells tcells;  // per-origin-cell trees (RT_AMD_TRI_CELLS), usually empty
    CameraTriangleBVH ctree;      // for the camera origin of ctree_version
    uint64_t ctree_version = 0;   // 0: none built
    bool ctree_full = false;      // ctree has its nodes (else records only)
    PrimaryTriLists ptl;          // for ptl_cam at ptl_w x ptl_h (and ctree_version)
    CameraModel ptl_cam{};
    size_t ptl_w = 0, ptl_h = 0;
    uint64_t ptl_ctree = 0, ptl_version = 0;
    PrimarySphereLists spl;       // for spl_cam at spl_w x spl_h
    CameraModel spl_cam{};
    size_t spl_w = 0, spl_h = 0;
    uint64_t spl_version = 0;
    // Primary sphere lists for a new camera or size are built on a host thread
    // while frames render without them (same pixels); adopted by the first
    // frame after the build is done.  (Declared after the structures the
    // build reads: a pending future's destructor waits for its build.)
    struct SplJob { std::future<PrimarySphereLists> f; CameraModel cam{}; size_t w = 0, h = 0; };
    SplJob spl_job;
    std::map<int, std::unique_ptr<DeviceState>> devices;
    uint64_t device_setups = 0;  // device states set up from nothing (rt_device_setups)
    // bumped by every scene edit (rt_world_set_*_material, rt_world_set_sphere_geometry):
    // an accumulator whose samples were traced under another value starts over
    uint64_t edit_version = 0;
    // the accumulators created on this world (accum_create / accum_free);
    // the world's destructor detaches them, after which their calls fail
    std::vector<AccumState *> accums;
    // calls on those accumulators that are under way (accum_enter / accum_leave):
    // world_retire, before the world is freed, waits until there are none
    uint32_t accum_calls = 0;
    // one frame at a time per handle: calls from several host threads are
    // serialised here (render_frame_multi re-enters render_frame)
    std::recursive_mutex mu;
    ~WorldState();
};

// An edge-aware filter's scratch for one image size on one device (DESIGN.md
// 5.9, rt_filter_*): the ping-pong colours and the packed guides a level
// gathers, and staging for the host entries.  Everything is allocated by the
// first run (a filter can be created without a GPU; running it fails there).
struct FilterState {
    size_t width = 0, height = 0;
    int device = -1;              // < 0: the current device at the first run
    DevBuf<float4> col[2];        // {r, g, b, L}: a level reads one, writes the other
    DevBuf<float4> g0, g1;        // {normal, prim bits}, {position, sigma_z * t}
    DevBuf<float> in_rgb, out_rgb;        // host entries: staging
    DevBuf<uint32_t> in_rec, out_rgba;
    DevStream stream;             // its own (rt_filter_run; rt_filter_run_device with a null stream)
    Fence done;                   // the last run enqueued on the scratch and the staging
    std::mutex mu;                // one run at a time per filter
    ~FilterState();
};

// A progressive accumulation: per-pixel f32 sums of sample
// colours for one world, frame size and camera, on one device, filled in
// passes.  Owns the sum planes and, in REPLAY mode, the device copy of its
// start-state table; the device's scratch stays shared with the frames.
struct AccumState {
    WorldState *world = nullptr;  // nullptr: the world was freed first
    size_t width = 0, height = 0;
    uint32_t stride = 0;          // S: samples per pixel at most, the job stride
    int32_t depth = 0, device = -1, accel = 0;
    uint32_t mode = 0, seed = 0;
    uint32_t held = 0;            // N: samples per pixel in the sums
    float cam[12] = {};           // the camera they were traced with ...
    uint64_t edit_version = 0;    // ... and the scene version
    DevBuf<float> sums;           // 3 planes of width * height (R, G, B), top row first
    DevBuf<uint32_t> replay;      // REPLAY: width * height * stride start states
    Fence done;                   // the last pass or read enqueued on the sums, adaptive planes and snapshots
    // Adaptive accumulation (rt_adapt_enable): the pixels still
    // sampled are those of list[cur] (frame indices, ascending), nactive of
    // them, all holding `held` samples; the others stopped at count[pixel].
    // Everything below is allocated by adapt_enable and freed with the sums
    // (frame last: its presence means all are).
    bool adaptive = false;
    float tolerance = 0.0f, bias = 0.0f;
    uint32_t min_samples = 0;
    DevBuf<float> sumsq;          // width * height: the fold of y y, y = (r + g) + b
    DevBuf<uint32_t> count;       // width * height: samples each pixel holds
    DevBuf<uint32_t> frame;       // width * height RGBA8: frozen pixels keep their last pass's bytes
    DevBuf<uint32_t> list[2];     // two lists alternate (the compaction's input and output)
    uint32_t cur = 0;
    uint32_t nactive = 0;         // entries of list[cur] (meaningful while held != 0)
    DevBuf<uint32_t> keep;        // width * height flags of the last decision
    DevBuf<uint32_t> totals;      // the compaction's block totals
    DevBuf<uint32_t> d_len;       // the new list length on the device ...
    PinnedBuf<uint32_t> h_len;    // ... and in pinned host memory
    // The filter of the held samples (rt_filter_accum): created
    // by the first call; the first-hit records of the frame (su = sv = 0.5,
    // this accel) for rec_cam and rec_edit, rebuilt when those differ from cam
    // and edit_version and dropped with the sums (rec_valid).
    std::unique_ptr<FilterState> filter;
    DevBuf<uint32_t> records;     // width * height RtFirstHit
    float rec_cam[12] = {};
    uint64_t rec_edit = 0;
    bool rec_valid = false;
    // The history of resolved views (rt_history_*): two
    // snapshots, hist[hist_cur] the last resolve's and the other one prev, each
    // valid for the camera and scene version it was made under.  Allocated by
    // the first resolve; hist_rgb is the blended image a filtered resolve hands
    // to the filter.
    struct HistorySnap {
        DevBuf<float4> col;       // {r, g, b, len}
        DevBuf<float4> guide;     // {position, prim bits}
        float cam[12] = {};
        uint64_t edit = 0;
        bool valid = false;
        // The spheres whose {centre, radius} when the snapshot was made differ from
        // the world's now: index -> the geometry then.  Kept by
        // rt_world_set_sphere_geometry (accums_sphere_moved); a new snapshot starts
        // empty, and a world without geometry edits never fills it.
        std::map<uint32_t, std::array<float, 4>> moved;
    };
    bool hist_enabled = false;
    float hist_max = 0.0f, hist_sigma_z = 0.0f;
    HistorySnap hist[2];
    uint32_t hist_cur = 0;
    DevBuf<float> hist_rgb;
    // The neighbourhood clamp of a resolve (rt_clamp_*): a
    // setting only, which outlives the history's enable, disable and reset.
    bool clamp_enabled = false;
    float clamp_gamma = 0.0f;
    uint32_t clamp_radius = 0, clamp_flags = 0;
    // A resolve that follows moved spheres: prev's sphere table,
    // dense, staged in pinned memory and uploaded on the resolve's stream.  The
    // host waits for `done` before it rewrites the staging: an earlier resolve,
    // still enqueued, may be reading it.  Allocated by the first such resolve.
    PinnedBuf<float4> move_stage;
    DevBuf<float4> move_table;
};

// One pass of an accumulation, for render_frame: n0 samples held, the frame's
// o.samples_per_pixel more are traced (1..4096).  list (adaptive accumulators):
// the pass traces only the nactive pixels listed, with the adaptive instances;
// d_out is then the accumulator's own frame.
struct AccumPass {
    AccumState *acc;
    uint32_t n0;
    const uint32_t *list = nullptr;
    uint32_t nactive = 0;
};

// One launch of a SERIAL-mode pass (render_frame_serial): the frame's jobs are
// replaced by nsamples x variants jobs starting at frame sample cbase, each
// storing its sample's diffuse/metal scatter count to plane 0 of the slab
// (DeviceState::samples) instead of a colour (render.h kRngSerial*).
struct SerialPass {
    uint32_t mode;            // kRngSerialCount or kRngSerialEstimate
    uint32_t cbase, nsamples, variants;
    const uint32_t *win;
    SerialPred M;
    const uint32_t *ctrl;
    const uint32_t *lo;       // kRngSerialCount (optional): tabulated window bases
    // kRngSerialCoalesce: the block walks' outputs (launch_serial_coalesce),
    // iteration length (nsamples), candidates (variants) and block length R
    uint32_t *path = nullptr, *bend = nullptr;
    uint32_t R = 0;
    unsigned long long *dbg = nullptr;  // (RT_AMD_SERIAL_DEBUG: launch_serial_coalesce's counters)
    // kRngSerialPixel: the table it writes (nsamples pixels x variants
    // positions, the launch's bounds), the iteration length and its K
    float *ptab = nullptr;
    uint32_t L = 0, Kmax = 0;
    const uint4 *spix = nullptr;  // its pixels' position spans (serial_window_kernel)
};

// Renders rank's tile of a width x height frame into device memory d_out
// (RGBA8 words, tile row-major).  stream may be null (library stream).
// sp: launch that SERIAL pass instead (d_out unused).  d_replay: REPLAY from
// this device-resident start-state table (frame sample order).
// defer_stats (with stats): the counted frame is only enqueued, and its
// counters and times are left pending on its device until
// collect_frame_stats(device state) fills stats.
int render_frame(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                 const RtRenderOptions &opts, uint32_t *d_out, hipStream_t stream,
                 RtRenderStats *stats, const SerialPass *sp = nullptr,
                 const uint32_t *d_replay = nullptr, bool defer_stats = false,
                 const AccumPass *ap = nullptr);
// (ap: the frame is that accumulation pass -- o.samples_per_pixel more samples
// per pixel folded into ap->acc's sums, d_out the frame of all samples held)

// Progressive accumulation (rt_accum_*, include/raytracer_amd.h).  create
// allocates on o.device (or the current device), uploads the REPLAY table and
// registers the accumulator with the world.  add: n more samples per pixel
// (passes of <= 4096), the frame of all held samples to d_out (device, or
// nullptr) and host_out (or nullptr); with host_out or stats it waits for the
// pass.  Camera moves and scene edits since the held samples were traced
// reset it first (accum_samples and accum_read see the same rule).
AccumState *accum_create(WorldState &w, size_t width, size_t height, uint32_t stride, int32_t depth,
                         uint32_t mode, uint32_t seed, const uint32_t *replay_states, int32_t device,
                         int32_t accel);
int accum_add(AccumState &a, const CameraModel &cam, int64_t nsamples, uint32_t *d_out, hipStream_t stream,
              void *host_out, RtRenderStats *stats);
long accum_samples(AccumState &a, const CameraModel &cam);
int accum_read(AccumState &a, const CameraModel &cam, float *sums);
int accum_reset(AccumState &a);
void accum_free(AccumState *a);
// A call on an accumulator from the C ABI: accum_enter returns the accumulator's
// world (nullptr: it was freed) and keeps it from being freed until accum_leave.
// world_retire detaches the world's accumulators, so that their later calls fail,
// and waits for the calls under way on other threads; rt_free_world calls it
// before it deletes the world and the handle those calls read.
WorldState *accum_enter(AccumState &a);
void accum_leave(WorldState *w);
void world_retire(WorldState &w);
// Adaptive accumulation (rt_adapt_*, include/raytracer_amd.h).  enable and
// disable need an accumulator that holds no samples; the reads wait for the
// last pass.  read_active returns the list's length (list may be nullptr).
int adapt_enable(AccumState &a, const CameraModel &cam, float tolerance, float bias, uint32_t min_samples);
int adapt_disable(AccumState &a, const CameraModel &cam);
long adapt_active(AccumState &a, const CameraModel &cam);
int adapt_read_counts(AccumState &a, const CameraModel &cam, uint32_t *counts);
int adapt_read_sumsq(AccumState &a, const CameraModel &cam, float *sumsq);
long adapt_read_active(AccumState &a, const CameraModel &cam, uint32_t *list, size_t cap);
// First-hit records (rt_first_hit_*, include/raytracer_amd.h) of
// the rectangle in opts (nullptr: the defaults) for the camera given, on the
// device's resident scene.  views: RT_VIEW_* `view` as RGBA8, else 32-byte
// records.  d_out (device memory, on stream; only enqueued) or host_out (waits).
// pick: the rectangle is that one pixel (row from the top).  who: the entry
// point, for the messages.  Checks every argument with a message before it
// looks for a device.
struct FirstHitPick { size_t col, row; };
int first_hit(WorldState &w, const CameraModel &cam, size_t width, size_t height, const RtFirstHitOptions *opts,
              bool views, int view, void *d_out, hipStream_t stream, void *host_out, const char *who,
              const FirstHitPick *pick = nullptr);
// The edge-aware filter (rt_filter_*, include/raytracer_amd.h).
// Every call checks its arguments with a message (who: the entry point) before
// it looks for a device.  create: the size only (nullptr with the error set).
// run: width x height interleaved colours and RtFirstHit records in, the
// filtered colours (f32) and / or their RGBA8 out; on_device: all four are
// device memory and the run is only enqueued on stream (null: the filter's
// own), else host memory and the call waits.  accum: the same on the
// accumulator's held samples (means of the sums, the accumulator's cached
// first-hit records), stream null: the device's library stream.
FilterState *filter_create(size_t width, size_t height, int device);
int filter_run(FilterState *f, const RtFilterOptions *opts, const float *rgb, const void *records, float *out_rgb,
               void *out_rgba, bool on_device, hipStream_t stream, const char *who);
int filter_accum(AccumState *a, const CameraModel *cam, const RtFilterOptions *opts, float *out_rgb, void *out_rgba,
                 bool on_device, hipStream_t stream, const char *who);
// Temporal reprojection (rt_history_*, include/raytracer_amd.h).
// check: a resolve's arguments that need no accumulator (outputs, the filter's
// options when given), with a message.  enable (on false: disable, which also
// frees the buffers) and reset drop both snapshots.  resolve: as filter_accum, with the history's
// step in front; filter null: no filter.  run: step 5 on host arrays.
int history_check(const RtFilterOptions *filter, const void *out_rgb, const void *out_rgba, const char *who);
int history_enable(AccumState &a, const CameraModel &cam, bool on, float max_history, float sigma_z);
int history_reset(AccumState &a, const CameraModel &cam);
int history_resolve(AccumState *a, const CameraModel *cam, const RtFilterOptions *filter, float *out_rgb,
                    void *out_rgba, bool on_device, hipStream_t stream, const char *who);
int history_read_length(AccumState &a, const CameraModel &cam, float *len);
// (run with clamp: rt_clamp_run, the clamped step 5 and, with out_box, every pixel's box;
// with move as well: rt_move_run, the same through the kernel that follows moved spheres)
struct HistoryRunMove {
    const float *prev_spheres, *spheres;  // nspheres x {centre, r}, dense host arrays
    size_t nspheres;
};
int history_run(size_t width, size_t height, float max_history, float sigma_z, const float *prev_cam,
                const float *prev_rgbl, const void *prev_records, const float *rgb, const uint32_t *n,
                const void *records, float *out_rgbl, int device, const RtClampOptions *clamp = nullptr,
                float *out_box = nullptr, const HistoryRunMove *move = nullptr);
// The resolve's neighbourhood clamp (rt_clamp_*): the setting
// (on false: off); it drops no snapshot.  The options were checked by the caller.
int clamp_enable(AccumState &a, const CameraModel &cam, bool on, const RtClampOptions &o);
// Sphere i of w was {old.center, old.radius} and is w.scene.spheres[i] now: every
// valid snapshot of every accumulator of w remembers the old value if it has none
// for i, and forgets i where the new value is the remembered one on bits.  The
// caller holds w.mu (rt_world_set_sphere_geometry).
void accums_sphere_moved(WorldState &w, size_t i, const Sphere &old);
// Waits for device d's pending counted frame and fills stats from it.
int collect_frame_stats(DeviceState *d, RtRenderStats *stats);

// RT_RNG_SERIAL: the reference's single frame-wide xorshift32 stream
// (common.rs:321).  Finds every sample's start state on the device (chunked
// candidate tables + walks), then renders in REPLAY mode.
int render_frame_serial(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                        const RtRenderOptions &opts, uint32_t *d_out, hipStream_t stream,
                        RtRenderStats *stats);

// A frame row-tiled over opts.ndevices devices (first = opts.device, or the
// current device) in this one process: each device renders its row blocks
// (blocks of opts.row_block rows, round-robin) into its own tile, an RCCL
// ncclGather (communicators from ncclCommInitAll, cached per device list)
// collects the tiles on the first device, and assemble_kernel writes the
// frame to d_out there (width x height RGBA8, top row first).  stream (may be
// null) is a stream of the first device; the others use their library streams.
int render_frame_multi(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                       const RtRenderOptions &opts, uint32_t *d_out, hipStream_t stream,
                       RtRenderStats *stats);

// assemble_kernel on its own (rt_assemble_tiles): checks the arguments
// against the tile layout of tile_rows / tile_row, then launches.
int assemble_tiles(const uint32_t *gathered, uint32_t *out, size_t width, size_t height, uint32_t row_block,
                   uint32_t nranks, size_t max_rows, hipStream_t stream);

// Ranks of the cached RCCL communicator of devices [first, first + n)
// (created on first use), or a negative error.
int comm_count(int first, int n);

// Same, into host memory (the reference's synchronous render(), lib.rs:49-57).
int render_frame_host(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                      const RtRenderOptions &opts, void *host_out, RtRenderStats *stats);

// (Re)builds the camera-origin triangle tree when the origin changed
// (load_world, move_camera_position, or a render with another camera).
void prepare_camera(WorldState &w, const CameraModel &cam, bool tree = false);

long read_samples(WorldState &w, int device, float *out, size_t n);
int leaf_defer(WorldState &w, int device);
int trace_plain(WorldState &w, int device);
int sky_rows(WorldState &w, int device);
int sky_forked(WorldState &w, int device);
// the device's set of launched instances into out (n bytes at most, one per
// render.h trace_key; out may be null), cleared afterwards when asked -> kTraceKeys
// (rt_trace_launched)
int trace_launched(WorldState &w, int device, uint8_t *out, size_t n, bool clear);
// one byte per trace_key, 1 where the library has an instance; no device needed
// (rt_trace_instances)
int trace_instances(uint8_t *out, size_t n);
// where the last frame launch's primary triangle lists were built (rt_primary_tri_lists)
int primary_tri_lists(WorldState &w, int device);

size_t tile_rows(size_t height, uint32_t row_block, uint32_t rank, uint32_t nranks);
size_t tile_row(size_t k, uint32_t row_block, uint32_t rank, uint32_t nranks);

}  // namespace rtamd
