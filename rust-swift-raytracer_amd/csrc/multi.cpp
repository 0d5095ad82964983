// multi.cpp -- one frame over several devices in one process: RCCL
// communicators, the row-tiled frame (render_frame_multi) and the assembly of
// gathered tiles.
#include <algorithm>
#include <map>
#include <mutex>

#include "runtime_internal.h"

namespace rtamd {

namespace {
// RCCL communicators, one set per device list (ncclCommInitAll is expensive:
// created once per process and kept; map nodes are stable)
std::mutex g_comm_mu;
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comms;

int device_comms(const std::vector<int> &devs, std::vector<ncclComm_t> *&out) {
    std::lock_guard<std::mutex> lock(g_comm_mu);
    auto it = g_comms.find(devs);
    if (it == g_comms.end()) {
        std::vector<ncclComm_t> c(devs.size(), nullptr);
        NCCL_TRY(ncclCommInitAll(c.data(), (int)devs.size(), devs.data()));
        it = g_comms.emplace(devs, std::move(c)).first;
    }
    out = &it->second;
    return 0;
}
}  // namespace

int device_list(int first, int n, std::vector<int> &devs) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device available: the MI355X render path requires a GPU");
        return -3;
    }
    if (first < 0) HIP_TRY(hipGetDevice(&first));
    if (n < 1 || first + n > count) {
        set_error("ndevices: devices [" + std::to_string(first) + ", " + std::to_string(first + n) +
                  ") are not all visible (" + std::to_string(count) + " devices)");
        return -1;
    }
    devs.resize(n);
    for (int g = 0; g < n; ++g) devs[g] = first + g;
    return 0;
}

int comm_count(int first, int n) {
    std::vector<int> devs;
    int rc = device_list(first, n, devs);
    if (rc) return rc;
    std::vector<ncclComm_t> *comms = nullptr;
    rc = device_comms(devs, comms);
    if (rc) return rc;
    int ranks = 0;
    NCCL_TRY(ncclCommCount((*comms)[0], &ranks));
    return ranks;
}

int render_frame_multi(WorldState &w, const CameraModel &cam, size_t width, size_t height,
                       const RtRenderOptions &o, uint32_t *d_out, hipStream_t stream,
                       RtRenderStats *stats) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if ((o.nranks > 1) || o.rank) {
        set_error("ndevices renders the whole frame: rank/nranks must be 0/1");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lock(w.mu);
    std::vector<int> devs;
    int rc = device_list(o.device, o.ndevices, devs);
    if (rc) return rc;
    const uint32_t n = (uint32_t)devs.size();
    const uint32_t B = o.row_block ? o.row_block : 8;
    if (width == 0 || height == 0) return 0;
    if (!d_out) { set_error("null output"); return -1; }
    if (width > 0xFFFFFFu || height > 0xFFFFFFu) { set_error("frame too large"); return -1; }
    size_t max_rows = 0;
    for (uint32_t g = 0; g < n; ++g) max_rows = std::max(max_rows, tile_rows(height, B, g, n));
    std::vector<ncclComm_t> *comms = nullptr;
    rc = device_comms(devs, comms);
    if (rc) return rc;
    std::vector<DeviceState *> ds(n, nullptr);
    std::vector<hipStream_t> ss(n, nullptr);
    for (uint32_t g = 0; g < n; ++g) {
        rc = device_for(w, devs[g], ds[g]);
        if (rc) return rc;
        ss[g] = (g == 0 && stream) ? stream : ds[g]->stream.get();
        if (n > 1) HIP_TRY(ds[g]->tile.grow(max_rows * width));
    }
    if (n > 1) {
        HIP_TRY(hipSetDevice(devs[0]));
        HIP_TRY(ds[0]->gath.grow(n * max_rows * width));
    }
    // SERIAL: the reference's one stream is a sequential dependency, so the
    // start states are found once, on the first device, and broadcast over
    // RCCL; every device then renders its row blocks from them (REPLAY)
    const bool serial = o.rng_mode == RT_RNG_SERIAL;
    RtRenderStats sst{};
    if (serial) {
        rc = serial_check_args(width, height, o);
        if (rc) return rc;
        HIP_TRY(hipSetDevice(devs[0]));
        rc = serial_find_states(w, cam, width, height, o, ds[0], ss[0], stats ? &sst : nullptr);
        if (rc) return rc;
        const uint64_t N = (uint64_t)width * height * (uint64_t)std::max(o.samples_per_pixel, 0);
        if (n > 1 && N > 0) {
            for (uint32_t g = 1; g < n; ++g) {
                HIP_TRY(hipSetDevice(devs[g]));
                HIP_TRY(ds[g]->sstates.grow(N));
            }
            NCCL_TRY(ncclGroupStart());
            for (uint32_t g = 0; g < n; ++g) {
                const ncclResult_t r = ncclBroadcast(ds[0]->sstates.get(), ds[g]->sstates.get(), N, ncclUint32, 0,
                                                     (*comms)[g], ss[g]);
                if (r != ncclSuccess) {
                    (void)ncclGroupEnd();
                    set_error(std::string("ncclBroadcast failed: ") + ncclGetErrorString(r));
                    return -4;
                }
            }
            NCCL_TRY(ncclGroupEnd());
        }
    }
    // every device renders its row blocks, all enqueued before any host wait:
    // a counted frame leaves its counters pending on its device
    // (render_frame defer_stats) and they are collected once every device's
    // tile is in flight, so counted frames keep the timed frames' schedule
    for (uint32_t g = 0; g < n; ++g) {
        RtRenderOptions og = o;
        og.ndevices = 0;
        og.rank = g;
        og.nranks = n;
        og.row_block = B;
        og.device = devs[g];
        if (serial) {
            og.rng_mode = RT_RNG_REPLAY;
            og.replay_states = nullptr;
        }
        RtRenderStats sg;
        HIP_TRY(hipSetDevice(devs[g]));
        // (one device: its tile is the frame, rendered in place -- no gather)
        rc = render_frame(w, cam, width, height, og, n == 1 ? d_out : ds[g]->tile.get(), ss[g], stats ? &sg : nullptr,
                          nullptr, serial ? ds[g]->sstates.get() : nullptr, /*defer_stats=*/true);
        if (rc) return rc;
    }
    // RCCL gather of equal-size tiles to the first device (over xGMI); with one
    // device the tile was rendered into d_out (until round 5 a one-rank gather
    // copied it there: one RCCL kernel and ~17 us per frame)
    const size_t bytes = max_rows * width * 4;
    if (n > 1) NCCL_TRY(ncclGroupStart());
    for (uint32_t g = 0; g < n && n > 1; ++g) {
        const ncclResult_t r = ncclGather(ds[g]->tile.get(), n > 1 ? (void *)ds[0]->gath.get() : (void *)d_out, bytes,
                                          ncclUint8, 0, (*comms)[g], ss[g]);
        if (r != ncclSuccess) {
            (void)ncclGroupEnd();  // (never leave this thread's group open)
            set_error(std::string("ncclGather failed: ") + ncclGetErrorString(r));
            return -4;
        }
    }
    if (n > 1) NCCL_TRY(ncclGroupEnd());
    HIP_TRY(hipSetDevice(devs[0]));
    if (n > 1)
        HIP_TRY(launch_assemble(ds[0]->gath.get(), d_out, (uint32_t)width, (uint32_t)height, B, n,
                                (uint32_t)max_rows, ss[0]));
    // the tiles and the gather buffer are reused by the next frame on these streams
    for (uint32_t g = 0; g < n; ++g) {
        HIP_TRY(hipSetDevice(devs[g]));
        HIP_TRY(ds[g]->done.record(ss[g]));
    }
    // the counted tiles' counters, collected only now: every device's tile, the
    // gather and the assembly are enqueued before the host waits on any of them
    for (uint32_t g = 0; g < n && stats; ++g) {
        HIP_TRY(hipSetDevice(devs[g]));
        RtRenderStats sg;
        std::memset(&sg, 0, sizeof(sg));
        rc = collect_frame_stats(ds[g], &sg);
        if (rc) return rc;
        {
            stats->samples += sg.samples; stats->rays += sg.rays;
            stats->sphere_tests += sg.sphere_tests; stats->tri_tests += sg.tri_tests;
            stats->tri_in_range += sg.tri_in_range;
            stats->trace_ms = std::max(stats->trace_ms, sg.trace_ms);
            stats->resolve_ms = std::max(stats->resolve_ms, sg.resolve_ms);
            stats->trace_launches = std::max(stats->trace_launches, sg.trace_launches);
            stats->waves += sg.waves; stats->accel = sg.accel;
            stats->bvh_sphere_tests += sg.bvh_sphere_tests; stats->bvh_node_tests += sg.bvh_node_tests;
            stats->big_sphere_tests += sg.big_sphere_tests;
            for (int k = 0; k < 4; ++k) stats->stamp_cycles[k] += sg.stamp_cycles[k];
            stats->tri_node_tests += sg.tri_node_tests; stats->bvh_tri_tests += sg.bvh_tri_tests;
            stats->tri_bvh = sg.tri_bvh; stats->fused_resolve = sg.fused_resolve;
            stats->primary_lists = sg.primary_lists; stats->camera_tree = sg.camera_tree;
            stats->launch_parts = sg.launch_parts; stats->launch_chunk = sg.launch_chunk;
            stats->launch_refill_min = sg.launch_refill_min; stats->launch_walk_min = sg.launch_walk_min;
            stats->launch_tri_walk_min = sg.launch_tri_walk_min; stats->launch_wsteps = sg.launch_wsteps;
            stats->launch_block_threads = sg.launch_block_threads; stats->launch_blocks = sg.launch_blocks;
            stats->sphere_tree = sg.sphere_tree; stats->sphere_tree_lds_bytes = sg.sphere_tree_lds_bytes;
        }
    }
    HIP_TRY(hipSetDevice(devs[0]));
    if (stats) {
        HIP_TRY(hipStreamSynchronize(ss[0]));
        if (serial) {
            stats->serial_retries = sst.serial_retries;
            stats->serial_iterations = sst.serial_iterations;
            stats->serial_checked = sst.serial_checked;
            stats->serial_chain_breaks = sst.serial_chain_breaks;
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, ds[0]->sev[0].get(), ds[0]->sev[1].get()));
            stats->serial_ms = ms;
            if (width * height * (size_t)std::max(o.samples_per_pixel, 0) > 0) {
                HIP_TRY(hipEventElapsedTime(&ms, ds[0]->sev[0].get(), ds[0]->sev[2].get()));
                stats->serial_setup_ms = ms;
            }
        }
    }
    return 0;
}

int assemble_tiles(const uint32_t *gathered, uint32_t *out, size_t width, size_t height, uint32_t row_block,
                   uint32_t nranks, size_t max_rows, hipStream_t stream) {
    if (width == 0 || height == 0) return 0;
    if (!gathered || !out) { set_error("rt_assemble_tiles: null buffer"); return -1; }
    if (nranks == 0 || row_block == 0) { set_error("rt_assemble_tiles: nranks and row_block must be >= 1"); return -1; }
    if (width > 0xFFFFFFu || height > 0xFFFFFFu) { set_error("frame too large"); return -1; }
    for (uint32_t g = 0; g < nranks; ++g)
        if (tile_rows(height, row_block, g, nranks) > max_rows) {
            set_error("rt_assemble_tiles: max_rows is smaller than a rank's tile");
            return -1;
        }
    HIP_TRY(launch_assemble(gathered, out, (uint32_t)width, (uint32_t)height, row_block, nranks,
                            (uint32_t)max_rows, stream));
    return 0;
}

}  // namespace rtamd
