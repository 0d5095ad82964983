// capi.cpp -- the C-ABI of the library: the reference's three entry points
// (Naxaes/Rust-Swift-Raytracer raytracer/src/lib.rs:37-63, header
// MacOSPlatform/MacOSPlatform/Engine/includes/raytracer.h:42-47) plus the
// extensions declared in include/raytracer_amd.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/raytracer.h"
#include "../../include/raytracer_amd.h"
#include "runtime_internal.h"  // (the shared argument checks)
#include "scene.h"
#include "sphere_edit.h"

// The opaque types of raytracer.h.  Rust_WorldHandle stays two pointers;
// the camera is heap-allocated on its own because callers replace it
// (GameView.swift:200-216 writes handle->camera = move_camera_position(...)).
struct Rust_World {
    rtamd::WorldState state;
};
struct Rust_Camera {
    rtamd::CameraModel cam;
};
// The handle is read at every call (callers replace handle->camera), never
// after its world was freed (state->world is nullptr then).
struct RtAccum {
    const Rust_WorldHandle *handle;
    rtamd::AccumState *state;
};
struct RtFilter {
    rtamd::FilterState *state;
};

namespace {
thread_local int g_parse_status = rtamd::kParseOk;

RtRenderOptions reference_options() {
    RtRenderOptions o;
    rt_default_options(&o);
    return o;
}

// A leaf-size knob (RT_AMD_LEAF / RT_AMD_TRI_LEAF): a whole decimal number in
// [1, 8], else the default (the BVH builders clamp it as well)
uint32_t env_leaf(const char *name, uint32_t dflt) {
    const char *e = std::getenv(name);
    if (!e || !*e) return dflt;
    char *end = nullptr;
    const long n = std::strtol(e, &end, 10);
    return (end && *end == '\0' && n >= 1 && n <= 8) ? (uint32_t)n : dflt;
}

// render()'s device count: RT_AMD_DEVICES=N (N >= 1) row-tiles its frames over
// N devices; unset, invalid or 0 keeps one device
int32_t env_devices() {
    const char *e = std::getenv("RT_AMD_DEVICES");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const long n = std::strtol(e, &end, 10);
    return (end && *end == '\0' && n >= 1 && n <= 64) ? (int32_t)n : 0;
}
}  // namespace

extern "C" {

// lib.rs:37-46
Rust_WorldHandle *load_world(const char *source) {
    if (!source) {
        rtamd::set_error("load_world: null source");
        return nullptr;
    }
    auto *world = new Rust_World();
    g_parse_status = rtamd::parse_scene(std::string(source), world->state.scene);
    if (g_parse_status != rtamd::kParseOk) {
        rtamd::set_error("load_world: parse error " + std::to_string(g_parse_status));
        delete world;
        return nullptr;
    }
    // spheres padded to the kernel's scalar-load batch of 8 with NaN centres
    world->state.packed = rtamd::pack_scene(world->state.scene, 8, 1);
    // spheres per BVH leaf (A/B with walk gating, C2 / C3: 3 -> 4.72 / 70.6 ms,
    // 2 -> 4.65 / 69.6, 1 -> 6.33 / 95.3 -- its tree no longer fits 64 KB of LDS)
    world->state.sphere_leaf = env_leaf("RT_AMD_LEAF", 2u);
    world->state.bvh = rtamd::build_sphere_bvh(world->state.scene.spheres, world->state.sphere_leaf);
    // triangles per BVH leaf (A/B on C5 at 96-node walk slices: 1 -> 222 ms,
    // 2 -> 240, 3 -> 293)
    world->state.tbvh = rtamd::build_triangle_bvh(world->state.scene.triangles,
                                                  world->state.packed.tri_hot,
                                                  env_leaf("RT_AMD_TRI_LEAF", 1u));
    // per-origin-cell trees: for meshes of >= 64 k triangles
    // by default, over the box of the mesh and the spheres around it, starting
    // from the edge that cuts the mesh's box into <= 1024 cells and grown to the
    // trees' budget (bvh.h TriangleCells; C5: 396 trees of 2-unit cells, static
    // tree 143.6 ms -> 88.7 ms); RT_AMD_TRI_CELLS=<edge> sets the starting
    // edge, 0 switches them off.  The static tree is re-quantised on their
    // common grid.
    {
        float size = 0.0f;
        if (const char *cs = std::getenv("RT_AMD_TRI_CELLS")) {
            size = std::strtof(cs, nullptr);
        } else if (world->state.scene.triangles.size() >= 65536 && !world->state.tbvh.nodes.empty()) {
            size = rtamd::triangle_cell_edge(world->state.scene.triangles, 1024);
        }
        if (size > 0.0f)
            world->state.tcells = rtamd::build_triangle_cells(world->state.scene.triangles,
                                                              world->state.packed.tri_hot,
                                                              world->state.scene.spheres,
                                                              env_leaf("RT_AMD_TRI_LEAF", 1u), size,
                                                              world->state.tbvh);
        const auto &tc = world->state.tcells;
        if (std::getenv("RT_AMD_TRI_CELLS_DEBUG")) std::fprintf(stderr, "tri cells: %u x %u x %u = %u cells of %.3g, %u wide nodes per tree, "
                     "%zu records, %.1f MB\n", tc.n[0], tc.n[1], tc.n[2], tc.ncells, tc.size, tc.stride_w,
                     tc.tris.size() / 16,
                     (tc.wnodes.size() * 4.0 + tc.tris.size() * 4.0) / 1e6);
    }
    // bounce-0 triangle tree for the scene camera (rebuilt by the first render
    // after move_camera_position, which does not see the world)
    rtamd::prepare_camera(world->state, world->state.scene.camera);
    auto *cam = new Rust_Camera{world->state.scene.camera};
    return new Rust_WorldHandle{world, cam};
}

// lib.rs:60-63: consumes the old camera, returns Camera::new_at(pos + d, aspect).
Rust_Camera *move_camera_position(Rust_Camera *camera, float x, float y, float z) {
    if (!camera) return nullptr;
    auto *moved = new Rust_Camera{rtamd::camera_moved(camera->cam, x, y, z)};
    delete camera;
    return moved;
}

// lib.rs:49-57: Options::new(16, 8, None, true); synchronous.  Writes into the
// caller's pixels (the reference returned a pointer into a freed Vec).
Rust_CFramebuffer render(Rust_CFramebuffer framebuffer, const Rust_WorldHandle *handle) {
    RtRenderOptions o = reference_options();
    o.ndevices = env_devices();
    // the reference's own frame (one xorshift32 stream, common.rs:321) unless
    // RT_AMD_RNG=counter asks for the fast per-sample-seeded mode
    const char *rng = std::getenv("RT_AMD_RNG");
    if (rng && std::strcmp(rng, "counter") == 0) o.rng_mode = RT_RNG_COUNTER;
    int rc = rt_render_ex(framebuffer, handle, &o, nullptr);
    if (rc != 0) {
        std::fprintf(stderr, "raytracer render() failed (%d): %s\n", rc, rtamd::last_error().c_str());
        return Rust_CFramebuffer{0, 0, nullptr};
    }
    return framebuffer;
}

void rt_default_options(RtRenderOptions *o) {
    std::memset(o, 0, sizeof(*o));
    o->samples_per_pixel = 16;  // lib.rs:51
    o->max_ray_bounces = 8;     // lib.rs:51
    o->rng_mode = RT_RNG_SERIAL;  // the reference's stream (common.rs:321)
    o->seed = 2547549u;         // random.rs:9
    o->row_block = 8;  // multi-GPU tiles: blocks of 8 rows
    o->rank = 0;
    o->nranks = 1;
    o->device = -1;
    o->accel = RT_ACCEL_AUTO;
}

size_t rt_tile_rows(size_t height, uint32_t row_block, uint32_t rank, uint32_t nranks) {
    if (rank >= (nranks ? nranks : 1)) return 0;
    return rtamd::tile_rows(height, row_block, rank, nranks);
}

size_t rt_tile_row(size_t k, uint32_t row_block, uint32_t rank, uint32_t nranks) {
    return rtamd::tile_row(k, row_block, rank, nranks);
}

uint32_t rt_sample_seed(uint32_t seed, uint64_t job) {
    uint64_t z = job + (uint64_t)seed * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    uint32_t r = (uint32_t)(z ^ (z >> 32));
    return r ? r : 2547549u;
}

int rt_render_ex(Rust_CFramebuffer fb, const Rust_WorldHandle *h, const RtRenderOptions *opts,
                 RtRenderStats *stats) {
    if (!h || !h->world || !h->camera) {
        rtamd::set_error("render: null world handle");
        return -1;
    }
    RtRenderOptions o = opts ? *opts : reference_options();
    return rtamd::render_frame_host(h->world->state, h->camera->cam, fb.width, fb.height, o,
                                    fb.pixels, stats);
}

int rt_render_device(const Rust_WorldHandle *h, size_t width, size_t height,
                     const RtRenderOptions *opts, void *d_rgba, void *hip_stream,
                     RtRenderStats *stats) {
    if (!h || !h->world || !h->camera) {
        rtamd::set_error("render: null world handle");
        return -1;
    }
    RtRenderOptions o = opts ? *opts : reference_options();
    if (o.ndevices >= 1 && rtamd::stream_capturing(static_cast<hipStream_t>(hip_stream)))
        return rtamd::refuse_capture("rt_render_device", "a frame tiled over devices (ndevices >= 1)");
    if (o.ndevices >= 1)
        return rtamd::render_frame_multi(h->world->state, h->camera->cam, width, height, o,
                                         static_cast<uint32_t *>(d_rgba),
                                         static_cast<hipStream_t>(hip_stream), stats);
    return rtamd::render_frame(h->world->state, h->camera->cam, width, height, o,
                               static_cast<uint32_t *>(d_rgba),
                               static_cast<hipStream_t>(hip_stream), stats);
}

int rt_trace_plain(const Rust_WorldHandle *h, int device) {
    if (!h || !h->world) {
        rtamd::set_error("rt_trace_plain: null argument");
        return -1;
    }
    return rtamd::trace_plain(h->world->state, device);
}

int rt_sky_rows(const Rust_WorldHandle *h, int device) {
    if (!h || !h->world) {
        rtamd::set_error("rt_sky_rows: null argument");
        return -1;
    }
    return rtamd::sky_rows(h->world->state, device);
}

int rt_sky_forked(const Rust_WorldHandle *h, int device) {
    if (!h || !h->world) {
        rtamd::set_error("rt_sky_forked: null argument");
        return -1;
    }
    return rtamd::sky_forked(h->world->state, device);
}

int rt_leaf_defer(const Rust_WorldHandle *h, int device) {
    if (!h || !h->world) {
        rtamd::set_error("rt_leaf_defer: null argument");
        return -1;
    }
    return rtamd::leaf_defer(h->world->state, device);
}

int rt_trace_launched(const Rust_WorldHandle *h, int device, unsigned char *out, size_t n, int clear) {
    if (!h || !h->world) {
        rtamd::set_error("rt_trace_launched: null argument");
        return -1;
    }
    return rtamd::trace_launched(h->world->state, device, out, n, clear != 0);
}

int rt_trace_instances(unsigned char *out, size_t n) { return rtamd::trace_instances(out, n); }

long rt_read_samples(const Rust_WorldHandle *h, int device, float *out, size_t n) {
    if (!h || !h->world || !out) {
        rtamd::set_error("rt_read_samples: null argument");
        return -1;
    }
    return rtamd::read_samples(h->world->state, device, out, n);
}

void rt_free_world(Rust_WorldHandle *h) {
    if (!h) return;
    // (calls on the world's accumulators that other threads are in return first;
    // later ones fail: they read the handle's camera and take the world's lock)
    if (h->world) rtamd::world_retire(h->world->state);
    delete h->world;
    delete h->camera;
    delete h;
}

const char *rt_last_error(void) { return rtamd::last_error().c_str(); }

int rt_last_parse_error(void) { return g_parse_status; }

size_t rt_world_num_spheres(const Rust_WorldHandle *h) {
    return h && h->world ? h->world->state.scene.spheres.size() : 0;
}
size_t rt_world_num_triangles(const Rust_WorldHandle *h) {
    return h && h->world ? h->world->state.scene.triangles.size() : 0;
}

// The one way a scene edit reaches the devices and the accumulators (the caller
// holds the world's lock and has put the new scene into w.scene, w.packed and,
// for a geometry edit, w.bvh): the host waits for every frame, pass and read
// still enqueued on the scene arrays; the device states stay, and the next call
// on each finds its edit_version behind the world's and refreshes it in place
// (device_state.cpp refresh_after_edit).  geometry: what was derived from the
// old spheres on the host is stale too.
static void edit_begin(rtamd::WorldState &w) {
    for (auto &kv : w.devices) {
        if (!kv.second) continue;
        (void)hipSetDevice(kv.first);
        (void)kv.second->done.sync();
    }
}
static void edit_commit(rtamd::WorldState &w, bool geometry) {
    if (geometry) {
        // the host's primary sphere lists were built from the old tree (the device's
        // lists and their sky rows are marked stale by its refresh)
        w.spl = rtamd::PrimarySphereLists{};
        w.spl_w = w.spl_h = 0;
        ++w.spl_version;
    }
    ++w.edit_version;  // (accumulators start over; every device state is behind now)
}

// Replaces primitive i's material.  Each primitive owns its material copy
// (parser.rs:237-310 clone the named material), so this changes one primitive.
static int set_material(Rust_WorldHandle *h, bool tri, size_t i, const float *m) {
    if (!h || !h->world || !m) return -1;
    rtamd::WorldState &w = h->world->state;
    std::lock_guard<std::recursive_mutex> lock(w.mu);
    rtamd::SceneModel &sc = w.scene;
    if (tri ? i >= sc.triangles.size() : i >= sc.spheres.size()) {
        rtamd::set_error("set material: primitive index out of range");
        return -1;
    }
    // kinds of materials.rs:7-12; every Color the reference builds has alpha 1.0
    // (color.rs:21-23), which the resolve relies on
    const float k = m[0];
    if (!(k == 0.0f || k == 1.0f || k == 2.0f || k == 3.0f) || m[4] != 1.0f) {
        rtamd::set_error("set material: kind must be 0-3 and alpha 1.0");
        return -1;
    }
    const uint32_t idx = tri ? sc.triangles[i].material : sc.spheres[i].material;
    edit_begin(w);
    sc.materials[idx] = rtamd::Material{(uint32_t)k, m[1], m[2], m[3], m[4], m[5]};
    w.packed = rtamd::pack_scene(sc, 8, 1);
    edit_commit(w, false);
    return 0;
}

int rt_world_set_sphere_material(Rust_WorldHandle *h, size_t i, const float material[6]) {
    return set_material(h, false, i, material);
}

int rt_world_set_triangle_material(Rust_WorldHandle *h, size_t i, const float material[6]) {
    return set_material(h, true, i, material);
}

int rt_world_set_sphere_geometry(Rust_WorldHandle *h, size_t i, const float geometry[4]) {
    const char *who = "rt_world_set_sphere_geometry";
    if (!h || !h->world) return rtamd::fail(who, "null world handle");
    if (!geometry) return rtamd::fail(who, "null input: geometry");
    rtamd::WorldState &w = h->world->state;
    std::lock_guard<std::recursive_mutex> lock(w.mu);
    if (i >= w.scene.spheres.size()) return rtamd::fail(who, "sphere index out of range");
    for (int k = 0; k < 4; ++k)
        if (geometry[k] != geometry[k]) return rtamd::fail(who, "geometry must not be NaN");
    // A background build of the host's primary sphere lists reads w.bvh and the
    // spheres (primary_lists.cpp): it ends before they are replaced, and what it
    // built is of the old scene
    if (w.spl_job.f.valid()) (void)w.spl_job.f.get();
    edit_begin(w);
    const rtamd::Sphere old = w.scene.spheres[i];
    if (!rtamd::set_sphere_geometry(w.scene, w.packed, w.bvh, i, geometry, w.sphere_leaf))
        return rtamd::fail(who, "sphere index out of range");
    rtamd::accums_sphere_moved(w, i, old);
    edit_commit(w, true);
    return 0;
}

long rt_device_setups(const Rust_WorldHandle *h) {
    if (!h || !h->world) return rtamd::fail("rt_device_setups", "null argument");
    std::lock_guard<std::recursive_mutex> lock(h->world->state.mu);
    return (long)h->world->state.device_setups;
}

static void material_out(const rtamd::Material &m, float *o) {
    o[0] = (float)m.kind; o[1] = m.r; o[2] = m.g; o[3] = m.b; o[4] = m.a; o[5] = m.param;
}

int rt_world_sphere(const Rust_WorldHandle *h, size_t i, float out[10]) {
    if (!h || !h->world || i >= h->world->state.scene.spheres.size()) return -1;
    const auto &sc = h->world->state.scene;
    const auto &s = sc.spheres[i];
    out[0] = s.center.x; out[1] = s.center.y; out[2] = s.center.z; out[3] = s.radius;
    material_out(sc.materials[s.material], out + 4);
    return 0;
}

int rt_world_triangle(const Rust_WorldHandle *h, size_t i, float out[18]) {
    if (!h || !h->world || i >= h->world->state.scene.triangles.size()) return -1;
    const auto &sc = h->world->state.scene;
    const auto &t = sc.triangles[i];
    const rtamd::Vec3 v[4] = {t.v0, t.v1, t.v2, t.normal};
    for (int k = 0; k < 4; ++k) { out[3 * k] = v[k].x; out[3 * k + 1] = v[k].y; out[3 * k + 2] = v[k].z; }
    material_out(sc.materials[t.material], out + 12);
    return 0;
}

void rt_camera_get(const Rust_Camera *c, float out[12]) {
    const rtamd::Vec3 v[4] = {c->cam.origin, c->cam.lower_left, c->cam.horizontal, c->cam.vertical};
    for (int k = 0; k < 4; ++k) { out[3 * k] = v[k].x; out[3 * k + 1] = v[k].y; out[3 * k + 2] = v[k].z; }
}

// ---- cameras no handle owns yet (camera.rs:34-69); the caller swaps one in:
// rt_camera_free(h->camera); h->camera = c;
Rust_Camera *rt_camera_new_with_vertical_fov(const float origin[3], float vertical_fov, float aspect_ratio) {
    if (!origin) {
        rtamd::set_error("rt_camera_new_with_vertical_fov: null origin");
        return nullptr;
    }
    return new Rust_Camera{rtamd::camera_with_vertical_fov({origin[0], origin[1], origin[2]}, vertical_fov,
                                                           aspect_ratio)};
}

Rust_Camera *rt_camera_new_look_at(const float origin[3], const float look_at[3], const float up[3],
                                   float vertical_fov, float aspect_ratio) {
    if (!origin || !look_at || !up) {
        rtamd::set_error("rt_camera_new_look_at: null argument");
        return nullptr;
    }
    rtamd::CameraModel cam;
    const int rc = rtamd::camera_look_at({origin[0], origin[1], origin[2]}, {look_at[0], look_at[1], look_at[2]},
                                         {up[0], up[1], up[2]}, vertical_fov, aspect_ratio, cam);
    if (rc != 0) {  // (the reference asserts, camera.rs:50 and :61)
        rtamd::set_error(rc == 1 ? "rt_camera_new_look_at: origin and look_at must differ"
                                 : "rt_camera_new_look_at: the view's vertical has no y component "
                                   "(up along the view direction, or a NaN)");
        return nullptr;
    }
    return new Rust_Camera{cam};
}

Rust_Camera *rt_camera_from_floats(const float camera[12]) {
    if (!camera) {
        rtamd::set_error("rt_camera_from_floats: null camera");
        return nullptr;
    }
    static_assert(sizeof(rtamd::CameraModel) == 12 * sizeof(float), "CameraModel is rt_camera_get's 12 floats");
    auto *c = new Rust_Camera{};
    std::memcpy(&c->cam, camera, 12 * sizeof(float));  // (bits as given, NaN payloads included)
    return c;
}

Rust_Camera *rt_camera_translate(Rust_Camera *camera, float x, float y, float z) {
    if (!camera) return nullptr;
    camera->cam = rtamd::camera_translated(camera->cam, x, y, z);
    return camera;
}

void rt_camera_free(Rust_Camera *camera) { delete camera; }

int rt_primary_tri_lists(const Rust_WorldHandle *h, int device) {
    if (!h || !h->world) {
        rtamd::set_error("rt_primary_tri_lists: null argument");
        return -1;
    }
    return rtamd::primary_tri_lists(h->world->state, device);
}

long rt_camera_record_builds(const Rust_WorldHandle *h) {
    if (!h || !h->world) {
        rtamd::set_error("rt_camera_record_builds: null argument");
        return -1;
    }
    std::lock_guard<std::recursive_mutex> lock(h->world->state.mu);
    return (long)h->world->state.ctree_version;
}

// image.rs:59-81: "P3\n{w} {h}\n255\n" then "r g b\n" per pixel, top row first.
int rt_write_ppm(const Rust_CFramebuffer *fb, const char *path) {
    if (!fb || !path || (!fb->pixels && fb->width * fb->height)) return -1;
    FILE *f = std::fopen(path, "wb");
    if (!f) return -1;
    std::fprintf(f, "P3\n%zu %zu\n255\n", fb->width, fb->height);
    for (size_t i = 0; i < fb->width * fb->height; ++i) {
        const Rust_ColorU8 &c = fb->pixels[i];
        std::fprintf(f, "%u %u %u\n", (unsigned)c.r, (unsigned)c.g, (unsigned)c.b);
    }
    return std::fclose(f) == 0 ? 0 : -1;
}

int rt_comm_count(int first, int n) { return rtamd::comm_count(first, n); }

int rt_assemble_tiles(const void *d_gathered, void *d_out, size_t width, size_t height, uint32_t row_block,
                      uint32_t nranks, size_t max_rows, void *hip_stream) {
    return rtamd::assemble_tiles(static_cast<const uint32_t *>(d_gathered), static_cast<uint32_t *>(d_out), width,
                                 height, row_block, nranks, max_rows, static_cast<hipStream_t>(hip_stream));
}

// ---- progressive accumulation
void rt_accum_default_options(RtAccumOptions *o) {
    std::memset(o, 0, sizeof(*o));
    o->max_ray_bounces = 8;       // lib.rs:51
    o->rng_mode = RT_RNG_COUNTER;
    o->seed = 2547549u;           // random.rs:9
    o->sample_stride = 64;
    o->device = -1;
    o->accel = RT_ACCEL_AUTO;
}

RtAccum *rt_accum_create(const Rust_WorldHandle *h, size_t width, size_t height, const RtAccumOptions *opts) {
    if (!h || !h->world || !h->camera) {
        rtamd::set_error("rt_accum_create: null world handle");
        return nullptr;
    }
    RtAccumOptions o;
    if (opts) o = *opts;
    else rt_accum_default_options(&o);
    rtamd::AccumState *st = rtamd::accum_create(h->world->state, width, height, o.sample_stride, o.max_ray_bounces,
                                                o.rng_mode, o.seed, o.replay_states, o.device, o.accel);
    return st ? new RtAccum{h, st} : nullptr;
}

// One call on an accumulator: keeps the accumulator's world alive until it
// returns (rt_free_world on another thread waits for it, runtime.h accum_enter)
// and gives the handle's current camera.  False, with the error set, for a null
// accumulator and after the world was freed: the freed handle is not touched.
namespace {
class AccumCall {
public:
    AccumCall(const RtAccum *acc, const char *who) {
        if (!acc || !acc->state) { rtamd::fail(who, "null accumulator"); return; }
        world_ = rtamd::accum_enter(*acc->state);
        if (!world_) { rtamd::fail(who, "the accumulator's world was freed"); return; }
        if (!acc->handle->camera) { rtamd::fail(who, "null camera"); return; }
        cam_ = &acc->handle->camera->cam;
    }
    ~AccumCall() {
        if (world_) rtamd::accum_leave(world_);
    }
    AccumCall(const AccumCall &) = delete;
    AccumCall &operator=(const AccumCall &) = delete;
    explicit operator bool() const { return cam_ != nullptr; }
    const rtamd::CameraModel &cam() const { return *cam_; }

private:
    rtamd::WorldState *world_ = nullptr;
    const rtamd::CameraModel *cam_ = nullptr;
};
}  // namespace

int rt_accum_add(RtAccum *acc, int64_t nsamples, Rust_ColorU8 *pixels, RtRenderStats *stats) {
    const AccumCall call(acc, "rt_accum_add");
    if (!call) return -1;
    return rtamd::accum_add(*acc->state, call.cam(), nsamples, nullptr, nullptr, pixels, stats);
}

int rt_accum_add_device(RtAccum *acc, int64_t nsamples, void *d_rgba, void *hip_stream, RtRenderStats *stats) {
    const AccumCall call(acc, "rt_accum_add_device");
    if (!call) return -1;
    return rtamd::accum_add(*acc->state, call.cam(), nsamples, static_cast<uint32_t *>(d_rgba),
                            static_cast<hipStream_t>(hip_stream), nullptr, stats);
}

long rt_accum_samples(RtAccum *acc) {
    const AccumCall call(acc, "rt_accum_samples");
    return call ? rtamd::accum_samples(*acc->state, call.cam()) : -1;
}

int rt_accum_read(RtAccum *acc, float *sums) {
    const AccumCall call(acc, "rt_accum_read");
    return call ? rtamd::accum_read(*acc->state, call.cam(), sums) : -1;
}

int rt_accum_reset(RtAccum *acc) {
    const AccumCall call(acc, "rt_accum_reset");
    if (!call) return -1;
    return rtamd::accum_reset(*acc->state);
}

void rt_accum_free(RtAccum *acc) {
    if (!acc) return;
    rtamd::accum_free(acc->state);
    delete acc;
}

// ---- adaptive accumulation
void rt_adapt_default_options(RtAdaptOptions *o) {
    o->tolerance = 0.05f;
    o->bias = 0.05f;
    o->min_samples = 8;
}

int rt_adapt_enable(RtAccum *acc, const RtAdaptOptions *opts) {
    RtAdaptOptions o;
    if (opts) o = *opts;
    else rt_adapt_default_options(&o);
    // (the options first: a caller's mistake shows whatever the accumulator's state)
    if (!rtamd::finite_from(o.tolerance, 0.0f) || !rtamd::finite_from(o.bias, 0.0f))
        return rtamd::fail("rt_adapt_enable", "tolerance and bias must be finite and >= 0");
    if (o.min_samples < 2) return rtamd::fail("rt_adapt_enable", "min_samples must be at least 2");
    const AccumCall call(acc, "rt_adapt_enable");
    if (!call) return -1;
    return rtamd::adapt_enable(*acc->state, call.cam(), o.tolerance, o.bias, o.min_samples);
}

int rt_adapt_disable(RtAccum *acc) {
    const AccumCall call(acc, "rt_adapt_disable");
    return call ? rtamd::adapt_disable(*acc->state, call.cam()) : -1;
}

long rt_adapt_active(RtAccum *acc) {
    const AccumCall call(acc, "rt_adapt_active");
    return call ? rtamd::adapt_active(*acc->state, call.cam()) : -1;
}

int rt_adapt_read_counts(RtAccum *acc, uint32_t *counts) {
    const AccumCall call(acc, "rt_adapt_read_counts");
    return call ? rtamd::adapt_read_counts(*acc->state, call.cam(), counts) : -1;
}

int rt_adapt_read_sumsq(RtAccum *acc, float *sumsq) {
    const AccumCall call(acc, "rt_adapt_read_sumsq");
    return call ? rtamd::adapt_read_sumsq(*acc->state, call.cam(), sumsq) : -1;
}

long rt_adapt_read_active(RtAccum *acc, uint32_t *list, size_t cap) {
    const AccumCall call(acc, "rt_adapt_read_active");
    return call ? rtamd::adapt_read_active(*acc->state, call.cam(), list, cap) : -1;
}

// ---- first-hit records
void rt_first_hit_default_options(RtFirstHitOptions *o) {
    std::memset(o, 0, sizeof(*o));
    o->su = 0.5f;
    o->sv = 0.5f;
    o->device = -1;
    o->accel = RT_ACCEL_AUTO;
}

// the handle's world and camera as they are now, or an error
static int first_hit_call(const Rust_WorldHandle *h, size_t width, size_t height, const RtFirstHitOptions *opts,
                          bool views, int view, void *d_out, void *hip_stream, void *host_out, const char *who,
                          const rtamd::FirstHitPick *pick = nullptr) {
    if (!h || !h->world || !h->camera) return rtamd::fail(who, "null world handle");
    return rtamd::first_hit(h->world->state, h->camera->cam, width, height, opts, views, view, d_out,
                            static_cast<hipStream_t>(hip_stream), host_out, who, pick);
}

int rt_first_hit(const Rust_WorldHandle *h, size_t width, size_t height, const RtFirstHitOptions *opts,
                 RtFirstHit *records) {
    return first_hit_call(h, width, height, opts, false, 0, nullptr, nullptr, records, "rt_first_hit");
}

int rt_first_hit_device(const Rust_WorldHandle *h, size_t width, size_t height, const RtFirstHitOptions *opts,
                        void *d_records, void *hip_stream) {
    return first_hit_call(h, width, height, opts, false, 0, d_records, hip_stream, nullptr, "rt_first_hit_device");
}

int rt_first_hit_pick(const Rust_WorldHandle *h, size_t width, size_t height, size_t col, size_t row,
                      const RtFirstHitOptions *opts, RtFirstHit *out) {
    const rtamd::FirstHitPick pick{col, row};
    return first_hit_call(h, width, height, opts, false, 0, nullptr, nullptr, out, "rt_first_hit_pick", &pick);
}

int rt_first_hit_view(const Rust_WorldHandle *h, size_t width, size_t height, const RtFirstHitOptions *opts,
                      int view, Rust_ColorU8 *pixels) {
    return first_hit_call(h, width, height, opts, true, view, nullptr, nullptr, pixels, "rt_first_hit_view");
}

int rt_first_hit_view_device(const Rust_WorldHandle *h, size_t width, size_t height, const RtFirstHitOptions *opts,
                             int view, void *d_rgba, void *hip_stream) {
    return first_hit_call(h, width, height, opts, true, view, d_rgba, hip_stream, nullptr,
                          "rt_first_hit_view_device");
}

// ---- edge-aware filter
void rt_filter_default_options(RtFilterOptions *o) {
    std::memset(o, 0, sizeof(*o));
    o->levels = 3;
    o->sigma_l = 0.5f;
    o->sigma_z = 0.02f;
    o->normal_squarings = 5;
}

RtFilter *rt_filter_create(size_t width, size_t height, int device) {
    rtamd::FilterState *st = rtamd::filter_create(width, height, device);
    return st ? new RtFilter{st} : nullptr;
}

void rt_filter_free(RtFilter *f) {
    if (!f) return;
    delete f->state;
    delete f;
}

int rt_filter_run_device(RtFilter *f, const RtFilterOptions *opts, const float *d_rgb, const void *d_records,
                         float *d_out_rgb, void *d_out_rgba, void *hip_stream) {
    return rtamd::filter_run(f ? f->state : nullptr, opts, d_rgb, d_records, d_out_rgb, d_out_rgba, true,
                             static_cast<hipStream_t>(hip_stream), "rt_filter_run_device");
}

int rt_filter_run(RtFilter *f, const RtFilterOptions *opts, const float *rgb, const RtFirstHit *records,
                  float *out_rgb, Rust_ColorU8 *out_pixels) {
    return rtamd::filter_run(f ? f->state : nullptr, opts, rgb, records, out_rgb, out_pixels, false, nullptr,
                             "rt_filter_run");
}

int rt_filter_accum(RtAccum *acc, const RtFilterOptions *opts, float *out_rgb, Rust_ColorU8 *pixels) {
    const AccumCall call(acc, "rt_filter_accum");
    if (!call) return -1;
    return rtamd::filter_accum(acc->state, &call.cam(), opts, out_rgb, pixels, false, nullptr, "rt_filter_accum");
}

int rt_filter_accum_device(RtAccum *acc, const RtFilterOptions *opts, float *d_out_rgb, void *d_rgba,
                           void *hip_stream) {
    const AccumCall call(acc, "rt_filter_accum_device");
    if (!call) return -1;
    return rtamd::filter_accum(acc->state, &call.cam(), opts, d_out_rgb, d_rgba, true, static_cast<hipStream_t>(hip_stream),
                               "rt_filter_accum_device");
}

// ---- temporal reprojection
void rt_history_default_options(RtHistoryOptions *o) {
    o->max_history = 32.0f;
    o->sigma_z = 0.02f;
}

namespace {
// the options (null: the defaults), checked; -1 with the error set
int history_options(const RtHistoryOptions *opts, const char *who, RtHistoryOptions &o) {
    if (opts) o = *opts;
    else rt_history_default_options(&o);
    if (!rtamd::finite_from(o.max_history, 1.0f)) return rtamd::fail(who, "max_history must be finite and >= 1");
    if (!rtamd::finite_from(o.sigma_z, 0.0f, true)) return rtamd::fail(who, "sigma_z must be finite and > 0");
    return 0;
}
int clamp_options(const RtClampOptions *opts, const char *who, RtClampOptions &o);

// rt_history_run's, rt_clamp_run's and rt_move_run's arguments: the size, the
// history's options -> o, the clamp's -> *c (c null: rt_history_run, none), the arrays
int history_run_check(const char *who, size_t width, size_t height, const RtHistoryOptions *opts, RtHistoryOptions &o,
                      const RtClampOptions *clamp, RtClampOptions *c, const float *prev_cam, const float *prev_rgbl,
                      const RtFirstHit *prev_records, const float *rgb, const uint32_t *n, const RtFirstHit *records,
                      const float *out_rgbl) {
    if (rtamd::check_image_size(width, height, "image size", who)) return -1;
    if (history_options(opts, who, o)) return -1;
    if (c && clamp_options(clamp, who, *c)) return -1;
    if (prev_rgbl && !prev_cam) return rtamd::fail(who, "null input: prev_cam (with prev_rgbl given)");
    if (prev_rgbl && !prev_records) return rtamd::fail(who, "null input: prev_records (with prev_rgbl given)");
    if (!rgb) return rtamd::fail(who, "null input: rgb");
    if (!n) return rtamd::fail(who, "null input: n");
    if (!records) return rtamd::fail(who, "null input: records");
    if (!out_rgbl) return rtamd::fail(who, "null output: out_rgbl");
    return 0;
}
}  // namespace

int rt_history_enable(RtAccum *acc, const RtHistoryOptions *opts) {
    // (the options first: a caller's mistake shows whatever the accumulator's state)
    RtHistoryOptions o;
    if (history_options(opts, "rt_history_enable", o)) return -1;
    const AccumCall call(acc, "rt_history_enable");
    if (!call) return -1;
    return rtamd::history_enable(*acc->state, call.cam(), true, o.max_history, o.sigma_z);
}

int rt_history_disable(RtAccum *acc) {
    const AccumCall call(acc, "rt_history_disable");
    return call ? rtamd::history_enable(*acc->state, call.cam(), false, 0.0f, 0.0f) : -1;
}

int rt_history_reset(RtAccum *acc) {
    const AccumCall call(acc, "rt_history_reset");
    return call ? rtamd::history_reset(*acc->state, call.cam()) : -1;
}

int rt_history_resolve(RtAccum *acc, const RtFilterOptions *filter, float *out_rgb, Rust_ColorU8 *pixels) {
    if (rtamd::history_check(filter, out_rgb, pixels, "rt_history_resolve")) return -1;
    const AccumCall call(acc, "rt_history_resolve");
    if (!call) return -1;
    return rtamd::history_resolve(acc->state, &call.cam(), filter, out_rgb, pixels, false, nullptr,
                                  "rt_history_resolve");
}

int rt_history_resolve_device(RtAccum *acc, const RtFilterOptions *filter, float *d_out_rgb, void *d_rgba,
                              void *hip_stream) {
    if (rtamd::history_check(filter, d_out_rgb, d_rgba, "rt_history_resolve_device")) return -1;
    const AccumCall call(acc, "rt_history_resolve_device");
    if (!call) return -1;
    return rtamd::history_resolve(acc->state, &call.cam(), filter, d_out_rgb, d_rgba, true,
                                  static_cast<hipStream_t>(hip_stream), "rt_history_resolve_device");
}

int rt_history_read_length(RtAccum *acc, float *len) {
    const AccumCall call(acc, "rt_history_read_length");
    return call ? rtamd::history_read_length(*acc->state, call.cam(), len) : -1;
}

int rt_history_run(size_t width, size_t height, const RtHistoryOptions *opts, const float *prev_cam,
                   const float *prev_rgbl, const RtFirstHit *prev_records, const float *rgb, const uint32_t *n,
                   const RtFirstHit *records, float *out_rgbl, int device) {
    RtHistoryOptions o;
    if (history_run_check("rt_history_run", width, height, opts, o, nullptr, nullptr, prev_cam, prev_rgbl, prev_records,
                          rgb, n, records, out_rgbl))
        return -1;
    return rtamd::history_run(width, height, o.max_history, o.sigma_z, prev_cam, prev_rgbl, prev_records, rgb, n,
                              records, out_rgbl, device);
}

// ---- the resolve's neighbourhood clamp
void rt_clamp_default_options(RtClampOptions *o) {
    o->gamma = 1.5f;
    o->radius = 1;
    o->flags = 0;
}

namespace {
// the options (null: the defaults), checked; -1 with the error set
int clamp_options(const RtClampOptions *opts, const char *who, RtClampOptions &o) {
    if (opts) o = *opts;
    else rt_clamp_default_options(&o);
    if (!rtamd::finite_from(o.gamma, 0.0f)) return rtamd::fail(who, "gamma must be finite and >= 0");
    if (o.radius < 1 || o.radius > 3) return rtamd::fail(who, "radius must be 1 .. 3");
    if (o.flags & ~(uint32_t)RT_CLAMP_KEEP_ON_EDIT) return rtamd::fail(who, "flags: unknown bits");
    return 0;
}
}  // namespace

int rt_clamp_enable(RtAccum *acc, const RtClampOptions *opts) {
    // (the options first, as rt_history_enable)
    RtClampOptions o;
    if (clamp_options(opts, "rt_clamp_enable", o)) return -1;
    const AccumCall call(acc, "rt_clamp_enable");
    if (!call) return -1;
    return rtamd::clamp_enable(*acc->state, call.cam(), true, o);
}

int rt_clamp_disable(RtAccum *acc) {
    const AccumCall call(acc, "rt_clamp_disable");
    return call ? rtamd::clamp_enable(*acc->state, call.cam(), false, RtClampOptions{}) : -1;
}

int rt_clamp_run(size_t width, size_t height, const RtHistoryOptions *opts, const RtClampOptions *clamp,
                 const float *prev_cam, const float *prev_rgbl, const RtFirstHit *prev_records, const float *rgb,
                 const uint32_t *n, const RtFirstHit *records, float *out_rgbl, float *out_box, int device) {
    RtHistoryOptions o;
    RtClampOptions c;
    if (history_run_check("rt_clamp_run", width, height, opts, o, clamp, &c, prev_cam, prev_rgbl, prev_records, rgb, n,
                          records, out_rgbl))
        return -1;
    return rtamd::history_run(width, height, o.max_history, o.sigma_z, prev_cam, prev_rgbl, prev_records, rgb, n,
                              records, out_rgbl, device, &c, out_box);
}

int rt_move_run(size_t width, size_t height, const RtHistoryOptions *opts, const RtClampOptions *clamp,
                const float *prev_cam, const float *prev_rgbl, const RtFirstHit *prev_records, const float *rgb,
                const uint32_t *n, const RtFirstHit *records, float *out_rgbl, float *out_box, const float *prev_spheres,
                const float *spheres, size_t nspheres, int device) {
    const char *who = "rt_move_run";
    RtHistoryOptions o;
    RtClampOptions c;
    if (history_run_check(who, width, height, opts, o, clamp, &c, prev_cam, prev_rgbl, prev_records, rgb, n, records,
                          out_rgbl))
        return -1;
    // (any bits are legal in the tables: the contract says what the kernel does with them)
    if ((uint64_t)nspheres >= (1ull << 32)) return rtamd::fail(who, "nspheres must be below 2^32");
    if (nspheres && !prev_spheres) return rtamd::fail(who, "null input: prev_spheres (with nspheres > 0)");
    if (nspheres && !spheres) return rtamd::fail(who, "null input: spheres (with nspheres > 0)");
    const rtamd::HistoryRunMove move{prev_spheres, spheres, nspheres};
    return rtamd::history_run(width, height, o.max_history, o.sigma_z, prev_cam, prev_rgbl, prev_records, rgb, n,
                              records, out_rgbl, device, &c, out_box, &move);
}

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
