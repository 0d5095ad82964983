/*
 * raytracer_amd.h -- extensions of the MI355X raytracer library beyond the
 * reference C-ABI (raytracer.h).  Nothing here changes the reference entry
 * points; it exposes what the reference hard-codes (Options, common.rs:288-317,
 * fixed to 16 spp / 8 bounces at lib.rs:51), device-resident rendering for
 * benchmarks, row tiles for multi-GPU, scene introspection and PPM output.
 */
#ifndef RAYTRACER_AMD_H
#define RAYTRACER_AMD_H

#include "raytracer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RNG modes.  The reference draws every sample from ONE xorshift32 stream
 * seeded 2547549 for the whole frame (common.rs:321, random.rs:8-10), which
 * is a sequential dependency.  The GPU offers:
 *   RT_RNG_SERIAL: that stream, seeded `seed`: the reference's own frame, bit
 *     for bit.  The library finds every sample's start state on the GPU
 *     (chunked candidate tables and walks), then renders as
 *     REPLAY; width*height*spp must be below 2^32.  The default of render().
 *   RT_RNG_COUNTER: sample (pixel p, index s) starts xorshift32 from
 *     rt_sample_seed(seed, p*spp + s); draws inside a sample follow the
 *     reference order exactly.  The fast mode (no sequential dependency);
 *     statistically, not bitwise, equal to the reference.
 *   RT_RNG_REPLAY: sample start states are read from a table (e.g. recorded
 *     from a serial CPU run), which reproduces the serial frame bit-for-bit. */
enum { RT_RNG_COUNTER = 1, RT_RNG_REPLAY = 2, RT_RNG_SERIAL = 3 };

typedef struct RtRenderOptions {
  int32_t samples_per_pixel;      /* Options.samples_per_pixel (common.rs:290) */
  int32_t max_ray_bounces;        /* Options.max_ray_bounces   (common.rs:291) */
  uint32_t rng_mode;              /* RT_RNG_*                                   */
  uint32_t seed;                  /* COUNTER base seed (default 2547549)        */
  const uint32_t *replay_states;  /* REPLAY: host table, width*height*spp u32,
                                     index (row*width + col)*spp + s, row 0 =
                                     bottom (common.rs:327-336 loop order)      */
  uint32_t row_block;             /* multi-GPU tile: image rows are dealt in    */
  uint32_t rank;                  /* blocks of row_block rows, round-robin over */
  uint32_t nranks;                /* nranks; this call renders rank's rows      */
  int32_t device;                 /* HIP device ordinal, -1 = current device    */
  int32_t accel;                  /* RT_ACCEL_*: how World::hit finds spheres   */
  uint32_t flags;                 /* RT_FLAG_* (0 = default)                    */
  int32_t ndevices;               /* 0: one device (`device`), this call renders
                                     rank's tile.  >= 1: the WHOLE frame, row-
                                     tiled (blocks of row_block rows) over
                                     devices [first, first + ndevices), first =
                                     `device` or the current device, in this one
                                     process; an RCCL ncclGather (communicators
                                     from ncclCommInitAll) collects the tiles on
                                     the first device.  rank/nranks must be 0/1. */
} RtRenderOptions;

/* Frame resolve.  By default the trace kernel resolves each pixel itself: a
 * wave keeps its chunks' samples in a small per-wave ring (cache-resident)
 * and sums a pixel's samples in order once its last sample is done, so only
 * the RGBA8 frame reaches HBM.  RT_FLAG_KEEP_SAMPLES writes every sample to a
 * full slab in HBM instead and resolves with a second kernel, which
 * rt_read_samples can then read.  Both give bit-identical frames. */
enum { RT_FLAG_KEEP_SAMPLES = 1 };

/* RT_RNG_SERIAL self-check.  RT_FLAG_SERIAL_CHECK traces every sample once
 * more from the start state found for it and checks the chain the reference's
 * one stream forms (common.rs:321-341): sample 0 starts at the seed, and each
 * sample's end state is the next sample's start state (the last one's: the
 * stream state the search ended on).  Mismatches are counted in
 * RtRenderStats.serial_chain_breaks (0 = the start states are the
 * reference's). */
enum { RT_FLAG_SERIAL_CHECK = 2 };

/* Sphere search.  Both give bit-identical frames:
 *   RT_ACCEL_BRUTE: every sphere in file order (common.rs:241-247).
 *   RT_ACCEL_BVH:   exact-pruning BVHs: spheres (BRUTE below 16 spheres) and
 *                   the phantom-aware triangle tree (BRUTE below 16 triangles).
 *   RT_ACCEL_AUTO:  BVH when the scene has one, else BRUTE.  Default. */
enum { RT_ACCEL_AUTO = 0, RT_ACCEL_BRUTE = 1, RT_ACCEL_BVH = 2 };

typedef struct RtRenderStats {
  uint64_t samples;        /* pixel samples traced                           */
  uint64_t rays;           /* World::hit calls (primary + bounces)           */
  uint64_t sphere_tests;   /* rays * spheres (brute force, common.rs:241)     */
  uint64_t tri_tests;      /* rays * triangles (common.rs:182)               */
  uint64_t tri_in_range;   /* triangle tests that passed the t-range check   */
  double trace_ms;         /* HIP-event time of the trace kernel(s)          */
  double resolve_ms;       /* HIP-event time of the resolve kernel(s)        */
  uint32_t trace_launches; /* number of trace launches (slabs)               */
  uint32_t waves;          /* persistent waves per trace launch              */
  uint32_t accel;          /* RT_ACCEL_BRUTE or RT_ACCEL_BVH (what ran)      */
  uint64_t bvh_sphere_tests; /* sphere tests executed inside the BVH         */
  uint64_t bvh_node_tests;   /* BVH node (box) tests executed                */
  uint64_t big_sphere_tests; /* rays * spheres kept out of the BVH           */
  uint64_t stamp_cycles[4];  /* diagnostic builds (-DRT_STAMPS) only: wave
                                cycles in refill+store / ray setup / BVH
                                walks / shading; zero in the product build             */
  uint64_t tri_node_tests;   /* triangle-BVH node tests executed              */
  uint64_t bvh_tri_tests;    /* triangle tests executed (== tri_tests brute)  */
  uint32_t tri_bvh;          /* 1 when the triangle BVH ran                   */
  uint32_t fused_resolve;    /* 1 when the trace kernel resolved the pixels
                                (no slab, resolve_ms ~ 0)                    */
  double serial_ms;          /* RT_RNG_SERIAL: HIP-event time spent finding the
                                start states (before the REPLAY render)       */
  uint32_t serial_retries;   /* RT_RNG_SERIAL: iterations whose walk stopped
                                short of their samples (the next one resumed) */
  uint32_t primary_lists;    /* 1: primary rays used per-pixel / per-strip
                                candidate lists (0 right after a camera move or
                                resize while they are built on a host thread) */
  uint32_t camera_tree;      /* 1: bounce-0 triangle rays used the camera-origin records (tree or strip lists) */
  uint32_t serial_iterations;   /* RT_RNG_SERIAL: candidate-table iterations run   */
  uint64_t serial_checked;      /* RT_FLAG_SERIAL_CHECK: samples whose chain link
                                   was checked (0 without the flag)             */
  uint64_t serial_chain_breaks; /* RT_FLAG_SERIAL_CHECK: broken links (0 = the
                                   reference's stream)                          */
  double serial_setup_ms;       /* RT_RNG_SERIAL: HIP-event time of the estimate
                                   pass and its tables (part of serial_ms)      */
  /* The frame trace launch's scheduling settings (the last launch of the
   * frame; they decide the schedule, so profiles record them with their
   * counters): job-queue partitions, jobs per queue pull, refill threshold
   * (idle lanes), walk gates (sphere / triangle walks), wide-walk fetches per
   * slice, threads per workgroup and workgroups per launch. */
  uint32_t launch_parts;
  uint32_t launch_chunk;
  uint32_t launch_refill_min;
  uint32_t launch_walk_min;
  uint32_t launch_tri_walk_min;
  uint32_t launch_wsteps;
  uint32_t launch_block_threads;
  uint32_t launch_blocks;
  /* Where that launch's sphere walk read the tree from: 0 no tree (brute
   * force), 1 global memory, 2 the workgroup's LDS copy as 64-B box records,
   * 3 the LDS copy as 128-B octant corner records (sphere-only scenes whose
   * image fits; RT_AMD_CORNER=0 keeps the box records) -- and the LDS bytes
   * that copy takes per workgroup (0 without one). */
  uint32_t sphere_tree;
  uint32_t sphere_tree_lds_bytes;
} RtRenderStats;

/* spp 16, depth 8 (lib.rs:51), SERIAL, seed 2547549, one rank, device -1,
 * row_block 8, ndevices 0: render()'s settings.  render() also reads two
 * environment variables: RT_AMD_RNG=counter selects RT_RNG_COUNTER (fast,
 * statistically equal frames) instead of the reference's stream, and
 * RT_AMD_DEVICES=N (N >= 1) row-tiles its frames over N GPUs (in SERIAL mode
 * the first device finds the whole frame's start states -- the stream is one
 * sequential dependency -- and broadcasts them over RCCL; the REPLAY render is
 * split). */
void rt_default_options(RtRenderOptions *opts);

/* Rows of a `height`-row image that belong to `rank` (see RtRenderOptions). */
size_t rt_tile_rows(size_t height, uint32_t row_block, uint32_t rank, uint32_t nranks);
/* Image row (0 = top) of the k-th row of rank's tile. */
size_t rt_tile_row(size_t k, uint32_t row_block, uint32_t rank, uint32_t nranks);

/* Counter-mode seed of global sample `job` (splitmix64 finaliser, nonzero). */
uint32_t rt_sample_seed(uint32_t seed, uint64_t job);

/* Renders `framebuffer` (full image size) with explicit options.  pixels
 * receives rank's tile: rt_tile_rows() rows of `width` pixels, tile row k =
 * image row rt_tile_row(k).  Synchronous.  Returns 0 or a negative error. */
int rt_render_ex(Rust_CFramebuffer framebuffer, const Rust_WorldHandle *handle,
                 const RtRenderOptions *opts, RtRenderStats *stats);

/* Threading: one frame at a time per handle.  Calls from several host threads
 * on one handle are serialised by a lock; frames enqueued on different streams
 * of one device are ordered (the later waits for the earlier: they share the
 * device's scratch).  Inside a frame the library may run part of it on a
 * stream of its own, which starts behind what the frame's stream holds and
 * which that stream waits for before the call returns. */

/* Same, but the tile is written to DEVICE memory `d_rgba` (rt_tile_rows*width
 * RGBA8; with ndevices >= 1 the whole width*height frame on the first device)
 * on HIP stream `hip_stream` (NULL = the library's stream; with ndevices it is
 * the first device's stream).  The scene
 * stays resident on the device between calls.  With `stats`, returns after the
 * frame is complete (HIP-event timings and counters filled in); with
 * stats == NULL the frame is only enqueued on the stream (no host wait), so
 * consecutive frames and the caller's collectives pipeline -- except in
 * RT_RNG_SERIAL mode, whose start-state search reads its progress back and
 * waits on the host between batches of iterations (the REPLAY render that
 * follows is only enqueued).  Returns 0 or a negative error.
 *
 * Capture.  A call whose `hip_stream` is capturing into a HIP graph
 * (hipStreamBeginCapture) records the frame instead of running it:
 *  - What may be captured: rt_render_device with stats == NULL, ndevices == 0,
 *    RT_RNG_COUNTER or RT_RNG_REPLAY, on a stream of the caller's.  Nothing
 *    else is promised.  With stats, in RT_RNG_SERIAL mode or with ndevices >= 1
 *    the call returns a negative error on a capturing stream, and so does
 *    rt_accum_add_device (a pass's first sample index would be baked into the
 *    graph: every replay would add the same samples again).  The first-hit,
 *    filter and history device entries are not promised inside a capture.
 *  - Warm rule: the same request must have been rendered outside a capture on
 *    that device since the world's last camera change, resize or scene edit.
 *    The same request: frame size, camera, accel, flags, samples per pixel and
 *    bounces (with the environment knobs unchanged), and in REPLAY mode the
 *    table's size; the seed may differ.  Warm means that the primary lists are
 *    current, every buffer is large enough and the kernels are loaded -- render
 *    the frame twice before capturing it and the capture also has the sky rows
 *    of the frames that follow the first.
 *  - A capturing call that is not warm returns a negative error whose message
 *    says "render this frame once outside the capture first".  It enqueues
 *    nothing (the capture stays valid and gets no node from it), allocates
 *    nothing and changes none of the library's bookkeeping.
 *  - REPLAY: the graph holds a copy node that reads the caller's replay_states
 *    table at every launch.  Keep the table alive and unchanged for the graph's
 *    lifetime.
 *  - Lifetime: the graph's nodes name the world's device buffers and the
 *    per-camera lists of the frame it recorded.  The library keeps those for
 *    the graph across later camera changes, resizes and other requests (it
 *    moves them aside instead of rewriting or freeing them, so every captured
 *    camera and size holds its lists' memory until the next edit or free):
 *    graphs of several cameras or sizes of one world can be launched in turn.
 *    A scene edit (rt_world_set_*_material) and rt_free_world release
 *    everything: destroy the graph before the edit or the free, and do not
 *    launch it afterwards.
 *  - Ordering: the ordering between streams described above covers calls, not
 *    replays.  Order every graph launch against the other work on that world's
 *    device yourself, by launching on the same stream or with events. */
int rt_render_device(const Rust_WorldHandle *handle, size_t width, size_t height,
                     const RtRenderOptions *opts, void *d_rgba, void *hip_stream,
                     RtRenderStats *stats);

/* Progressive accumulation: refine a frame pass by pass.
 *
 * An accumulator is a device-resident per-pixel f32 sum of sample colours for
 * one world, one frame size and the handle's camera, on one device (whole
 * frames: no row tiles, no ndevices).  It is created with a sample stride S,
 * the most samples per pixel it will ever hold.  Sample s (0 <= s < S) of the
 * pixel at reference (row, col), row 0 = bottom, is global job
 * g = (row*width + col)*S + s: in COUNTER mode it starts xorshift32 from
 * rt_sample_seed(seed, g), in REPLAY mode from replay_states[g]; inside a
 * sample everything is the frame's trace.  With N0 samples held, a pass of n
 * traces samples N0 .. N0+n-1 of every pixel, continues each pixel's three
 * sums in sample order (the reference's fold, common.rs:333-341, stopped and
 * continued from the stored f32 sum: the same bits as a fold that never
 * stopped) and writes the RGBA8 frame of N = N0 + n samples,
 * sqrt(sum * (1/(N as f32))) * 255.999 as u8 per channel.  So after passes
 * totalling S the frame is bit-identical to rt_render_ex at
 * samples_per_pixel = S in the same mode, whatever the split.
 *
 * The accumulator resets itself to N = 0 when the handle's camera (its 12
 * floats) differs from the one the held samples were traced with, and when the
 * scene was edited (rt_world_set_*_material): a viewer's loop is "move, add,
 * show".  RT_RNG_SERIAL is rejected (one stream over the whole frame has no
 * per-pass meaning).  A pass that would exceed S, or nsamples <= 0, is an
 * error and traces nothing.  Requests above 4096 samples run as consecutive
 * passes inside the call.
 *
 * Ownership: free the accumulator before its world.  After rt_free_world
 * every call on the accumulator but rt_accum_free fails with an error (it
 * does not touch the freed handle); rt_free_world waits for the calls on the
 * world's accumulators that other threads are in, so such a call either
 * completes or fails with that error.  Calls on one handle's accumulators and
 * frames are serialised by the handle's lock. */
typedef struct RtAccum RtAccum;

typedef struct RtAccumOptions {
  int32_t max_ray_bounces;        /* as RtRenderOptions                          */
  uint32_t rng_mode;              /* RT_RNG_COUNTER or RT_RNG_REPLAY             */
  uint32_t seed;                  /* COUNTER base seed                           */
  const uint32_t *replay_states;  /* REPLAY: host table of width*height*S u32,
                                     index (row*width + col)*S + s, row 0 =
                                     bottom; uploaded once by rt_accum_create   */
  uint32_t sample_stride;         /* S >= 1                                      */
  int32_t device;                 /* HIP device ordinal, -1 = current device     */
  int32_t accel;                  /* RT_ACCEL_*                                  */
} RtAccumOptions;

/* depth 8, COUNTER, seed 2547549, sample_stride 64, device -1, RT_ACCEL_AUTO. */
void rt_accum_default_options(RtAccumOptions *opts);
/* NULL on error (rt_last_error); opts NULL = the defaults. */
RtAccum *rt_accum_create(const Rust_WorldHandle *handle, size_t width, size_t height,
                         const RtAccumOptions *opts);
/* Adds nsamples per pixel and writes the frame of all held samples to host
 * `pixels` (width*height RGBA8, top row first; NULL: accumulate only).
 * Synchronous when pixels or stats is given.  Stats of a pass fill samples,
 * trace_ms, trace_launches (summed over the call's passes), waves,
 * fused_resolve, accel, sphere_tree* and launch_*; the work counters (rays,
 * sphere_tests, tri_*, bvh_*, big_sphere_tests) stay 0: accumulation has no
 * counting kernel.  Returns 0 or a negative error. */
int rt_accum_add(RtAccum *acc, int64_t nsamples, Rust_ColorU8 *pixels, RtRenderStats *stats);
/* Same, the frame to DEVICE memory d_rgba (NULL: accumulate only) on
 * hip_stream (NULL = the library's stream).  With stats == NULL the pass is
 * only enqueued (no host wait), like rt_render_device -- except on an adaptive
 * accumulator (rt_adapt_enable below), whose deciding passes read the new list
 * length back and wait on the host, as RT_RNG_SERIAL does in rt_render_device.
 * On a capturing stream every pass is refused with a negative error
 * (rt_render_device, "Capture"). */
int rt_accum_add_device(RtAccum *acc, int64_t nsamples, void *d_rgba, void *hip_stream,
                        RtRenderStats *stats);
/* Samples per pixel held (0 after a reset, also one that the next add would
 * make: a moved camera or an edited scene), or a negative error. */
long rt_accum_samples(RtAccum *acc);
/* The raw sums: width*height*3 f32, top row first, RGB interleaved (all 0.0
 * with no samples held).  Waits for the last pass.  0 or a negative error. */
int rt_accum_read(RtAccum *acc, float *sums);
/* Forgets the held samples (the next pass starts from zero sums). */
int rt_accum_reset(RtAccum *acc);
void rt_accum_free(RtAccum *acc);

/* Adaptive accumulation: stop sampling pixels that have converged (DESIGN.md
 * 5.7).
 *
 * An accumulator that holds no samples can be switched to adaptive.  Besides
 * its three sums it then owns, per pixel, sumsq (f32: the in-order fold
 * q <- q + y*y over the pixel's samples, y = (r + g) + b of the sample's
 * colour, every operation one rounded f32 operation, the product rounded
 * before the add) and count (u32: samples the pixel holds); the RGBA8 frame (a
 * pixel that stopped keeps the bytes of its last pass); and the active list,
 * the frame indices (top row first, ascending) of the pixels still sampled.
 * All active pixels hold the same N, which rt_accum_samples returns.
 *
 * With N0 samples held by the active pixels, rt_accum_add(n) traces samples
 * N0 .. N0+n-1 of the listed pixels only (same jobs g as above), continues
 * their four folds and writes their RGBA8 at N = N0 + n.  If N >= min_samples
 * it then decides per listed pixel, in f32, one rounded operation each:
 *   inv = 1.0f / (float)N
 *   m   = ((R + G) + B) * inv
 *   v   = q * inv - m * m;  v = v < 0 ? 0 : v        (NaN stays NaN)
 *   e   = v * inv
 *   lim = tolerance * (m + bias)
 *   converged iff e <= lim * lim                      (false for NaN)
 * Converged pixels leave the list (order kept) and never return until a reset;
 * count becomes N for every pixel the pass traced.  So each pixel always
 * carries exactly the in-order fold of its own first count samples.
 *
 * Camera moves, scene edits and rt_accum_reset make every pixel active again
 * with zero counts; the adaptive setting stays.  A pass with an empty list
 * traces nothing, leaves N alone, still delivers the frame and returns 0; a
 * pass beyond S stays an error.  Requests above 4096 samples run as
 * consecutive passes, each with its decision.  A viewer's loop becomes "move,
 * add while rt_adapt_active > 0, show".
 *
 * A deciding pass reads the new list length back (4 bytes) and therefore
 * waits on the host for the pass, also with stats == NULL in
 * rt_accum_add_device -- like RT_RNG_SERIAL in rt_render_device. */
typedef struct RtAdaptOptions {
  float tolerance;       /* relative standard error of the mean to stop at      */
  float bias;            /* added to the mean: dark pixels stop on an absolute  */
  uint32_t min_samples;  /* no decision before a pixel holds this many (>= 2)   */
} RtAdaptOptions;

/* tolerance 0.05, bias 0.05, min_samples 8. */
void rt_adapt_default_options(RtAdaptOptions *opts);
/* Switches to adaptive (opts NULL = the defaults).  An error unless the
 * accumulator holds 0 samples; tolerance and bias must be finite and >= 0,
 * min_samples >= 2.  0 or a negative error. */
int rt_adapt_enable(RtAccum *acc, const RtAdaptOptions *opts);
/* Back to every pixel every pass; an error unless 0 samples are held. */
int rt_adapt_disable(RtAccum *acc);
/* Pixels on the active list (width*height with no samples held or when the
 * accumulator is not adaptive), or a negative error. */
long rt_adapt_active(RtAccum *acc);
/* count and sumsq: width*height values, top row first (all 0 with no samples
 * held).  Adaptive accumulators only.  Wait for the last pass. */
int rt_adapt_read_counts(RtAccum *acc, uint32_t *counts);
int rt_adapt_read_sumsq(RtAccum *acc, float *sumsq);
/* Copies at most cap entries of the active list and returns its length (list
 * may be NULL with cap 0), or a negative error. */
long rt_adapt_read_active(RtAccum *acc, uint32_t *list, size_t cap);

/* First-hit records: what the primary ray of each pixel hits.
 *
 * Maps pixels back to primitives, so that a viewer can pick ("this click is
 * sphere 137", then rt_world_set_sphere_material), show debug views, and feed
 * image-space steps with per-pixel primitive, depth and normal.
 *
 * For a width x height frame, the handle's camera (its 12 floats, as it is at
 * the call) and sub-pixel offsets su, sv in [0, 1), the ray of the pixel at
 * reference (row, col), row 0 = bottom, is the frame's primary ray with its
 * two random draws replaced by the constants (common.rs:335-337):
 *   u = (col as f32 + su) / (width  - 1) as f32     one rounded add, one
 *   v = (row as f32 + sv) / (height - 1) as f32     correctly rounded divide
 *   ray = camera.cast_ray(u, v)                      camera.rs:84-89
 *   hit = world.hit(&ray)                            common.rs:237-258, t_min 0.001
 * No RNG is involved.  width - 1 == 0 or height - 1 == 0 divides by zero as a
 * frame does: the infinite or NaN ray hits nothing.  The hit is World::hit's
 * winner, ties included: the lowest sphere index at equal t, the first
 * triangle at equal t, and a triangle at the spheres' closest t beats the
 * sphere.  RT_ACCEL_BRUTE and RT_ACCEL_BVH give identical bits.
 *
 * Records are stored top row first like every frame: index
 * (height - 1 - row) * width + col.  A rectangle x0, y0, w, h in frame
 * coordinates (y0 counted from the top row) restricts a call to those pixels;
 * the output then holds w * h records (or pixels), the rectangle's top row
 * first.  0, 0, 0, 0 is the whole frame.
 *
 * Calls take the handle's lock like frames, use the device's resident scene
 * (uploaded on first use and again after rt_world_set_*_material) and are
 * ordered against frames and passes on other streams as frames are.  They
 * never read anything that was built for an earlier camera. */
typedef struct RtFirstHit {
  uint32_t prim;      /* 0: no hit.  1 + i: sphere i (file order, rt_world_sphere's i).
                         1 + rt_world_num_spheres + j: triangle j (rt_world_triangle's j) */
  float t;            /* hit.t; +inf for no hit */
  float normal[3];    /* hit.normal as World::hit returns it (sphere: ((p - c) / r).normalize(),
                         so a negative radius flips it; triangle: its stored normal); 0 0 0 for no hit */
  float position[3];  /* hit.position = ray.at(t); 0 0 0 for no hit */
} RtFirstHit;

/* Views of a record as RGBA8.  Every step is one rounded f32 operation,
 * unfused; `as u8` is Rust's saturating cast, as in the frame resolve.  Alpha
 * is 255; a no-hit pixel is 0, 0, 0 in every view.
 *   RT_VIEW_NORMAL: channel k = ((n_k * 0.5f) + 0.5f) * 255.999f as u8
 *   RT_VIEW_DEPTH:  r = g = b = (1.0f / (1.0f + t)) * 255.999f as u8
 *   RT_VIEW_ALBEDO: channel = c_k * 255.999f as u8, c the hit primitive's
 *                   current material colour (Dielectric: 1, 1, 1, the colour
 *                   its scatter returns, materials.rs:96)
 *   RT_VIEW_PRIM:   h = prim * 2654435761u (mod 2^32); r, g, b = h >> 24,
 *                   (h >> 16) & 255, (h >> 8) & 255 */
enum { RT_VIEW_NORMAL = 0, RT_VIEW_DEPTH = 1, RT_VIEW_ALBEDO = 2, RT_VIEW_PRIM = 3 };

typedef struct RtFirstHitOptions {
  float su, sv;              /* [0, 1); default 0.5, 0.5 */
  uint32_t x0, y0, w, h;     /* rectangle, y0 from the top; all 0 = whole frame */
  int32_t device;            /* -1 = current */
  int32_t accel;             /* RT_ACCEL_*: BRUTE and BVH give identical bits */
} RtFirstHitOptions;

/* su = sv = 0.5, the whole frame, device -1, RT_ACCEL_AUTO. */
void rt_first_hit_default_options(RtFirstHitOptions *opts);
/* Every call below: opts NULL = the defaults; returns 0 or a negative error
 * with rt_last_error set.  Arguments are checked before a device is looked
 * for: a null handle or output; a zero frame size or width * height >= 2^31; a
 * rectangle that leaves the frame or has exactly one of w, h zero; su or sv
 * outside [0, 1) (NaN included); an unknown view or accel; a pick outside the
 * frame.  Without a GPU every call fails. */
/* Records to host memory (synchronous) ... */
int rt_first_hit(const Rust_WorldHandle *handle, size_t width, size_t height,
                 const RtFirstHitOptions *opts, RtFirstHit *records);
/* ... or to DEVICE memory on hip_stream (NULL = the library's stream): only
 * enqueued, no host wait. */
int rt_first_hit_device(const Rust_WorldHandle *handle, size_t width, size_t height,
                        const RtFirstHitOptions *opts, void *d_records, void *hip_stream);
/* One pixel, col from the left and row from the top: the record of that pixel
 * (a 1 x 1 rectangle; the rectangle in opts is ignored).  Synchronous. */
int rt_first_hit_pick(const Rust_WorldHandle *handle, size_t width, size_t height, size_t col,
                      size_t row, const RtFirstHitOptions *opts, RtFirstHit *out);
/* A view (RT_VIEW_*) of the same pixels as RGBA8, to host memory / to device
 * memory; no record buffer is needed. */
int rt_first_hit_view(const Rust_WorldHandle *handle, size_t width, size_t height,
                      const RtFirstHitOptions *opts, int view, Rust_ColorU8 *pixels);
int rt_first_hit_view_device(const Rust_WorldHandle *handle, size_t width, size_t height,
                             const RtFirstHitOptions *opts, int view, void *d_rgba,
                             void *hip_stream);

/* ---- Edge-aware filter of a noisy frame, guided by first-hit records
 * (DESIGN.md 5.9).
 *
 * An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over per-pixel
 * mean colours, stopped at geometric edges by the records above: a viewer that
 * has just moved the camera filters its 1 to 4 samples and shows the result,
 * all on the device.  It is a preview filter, not a replacement for samples:
 * on primitives a few pixels wide it blurs detail away.
 *
 * Inputs, for a width x height image, top row first: colours c (RGB f32),
 * records g (RtFirstHit, as rt_first_hit_device writes them) and options.
 * Every step below is one rounded f32 operation, unfused; divisions are
 * correctly rounded; comparisons are false for NaN.
 *
 * Level l = 0 .. levels - 1 reads the previous level's colours (level 0 the
 * input) and writes new ones; the records never change.  step = 1 << l,
 * sl = sigma_l * 2^-l (exact), taps H = (1/16, 1/4, 3/8, 1/4, 1/16).
 * Per centre pixel p: L_p = (r + g) + b of its input colour at this level,
 * zs = sigma_z * t_p.  The taps q = p + ((i - 2) step, (j - 2) step), y growing
 * downwards, are visited with j = 0..4 outer and i = 0..4 inner; sums are
 * accumulated in that order.  Per tap:
 *   1. q outside the image: skip.
 *   2. hp = prim_p != 0, hq = prim_q != 0; hp != hq: skip.  With
 *      RT_FILTER_SAME_PRIM, prim_p != prim_q: skip.
 *   3. w = H[j] * H[i]
 *   4. if hp: d = ((n_p.x*n_q.x) + (n_p.y*n_q.y)) + (n_p.z*n_q.z)
 *             d = d > 0 ? d : 0;  normal_squarings times: d = d*d
 *             v = pos_q - pos_p
 *             e = fabs(((v.x*n_p.x) + (v.y*n_p.y)) + (v.z*n_p.z)) / zs
 *             wz = 1 / (1 + e*e);  w = (w*d) * wz
 *   5. el = fabs(L_q - L_p) / sl;  wl = 1 / (1 + el*el);  w = w * wl
 *   6. if not w > 0: skip (NaN and zero weights)
 *   7. num_k = num_k + w*c_q,k for k = r, g, b;  den = den + w
 * Output channel k of p: den > 0 ? num_k / den : c_p,k.
 * After the last level the f32 output is the colour and the RGBA8 output is
 * sqrt(c_k) * 255.999 as u8 (Rust's saturating cast, as the frame resolve),
 * alpha 255.  With levels = 0 the output is the input.
 *
 * On an accumulator the input colour of pixel p is sum_k * inv with
 * inv = 1.0f / (float)n_p, n_p the samples held (rt_accum_samples) or, for an
 * adaptive accumulator, count[p]: what the frame's resolve takes the square
 * root of, so levels = 0 returns the last pass's frame byte for byte.  The
 * records are the first-hit records at the accumulator's size with
 * su = sv = 0.5, its accel and the camera its samples were traced with; they
 * are kept until the camera moves or the scene is edited. */
enum { RT_FILTER_SAME_PRIM = 1 };  /* flags: only taps on the centre's primitive count */

typedef struct RtFilterOptions {
  int32_t levels;             /* 0 .. 8; default 3 */
  float sigma_l;              /* finite, > 0; default 0.5 */
  float sigma_z;              /* finite, > 0; default 0.02 */
  int32_t normal_squarings;   /* 0 .. 8; default 5 (the normals' dot to the power 32) */
  uint32_t flags;             /* RT_FILTER_*; default 0 */
} RtFilterOptions;

typedef struct RtFilter RtFilter;   /* owns the per-size device scratch, one device */

void rt_filter_default_options(RtFilterOptions *opts);
/* A filter for width x height images on `device` (-1: the current device at
 * its first run).  NULL + rt_last_error for a zero size or
 * width * height >= 2^31.  Needs no GPU; running it does. */
RtFilter *rt_filter_create(size_t width, size_t height, int device);
void rt_filter_free(RtFilter *f);
/* Every call below: opts NULL = the defaults; returns 0 or a negative error
 * with rt_last_error naming the call and the argument.  Checked before a
 * device is looked for: a null filter or accumulator, a null input, both
 * outputs null (either one may be), levels, sigma_l, sigma_z or
 * normal_squarings out of range, unknown flag bits.  rgb buffers are
 * width * height * 3 f32, interleaved, top row first (rt_accum_read's layout).
 *
 * Any image, any records: DEVICE buffers, only enqueued on hip_stream.  NULL =
 * the library's stream for this filter: a filter belongs to no world, so it
 * is a non-blocking stream of the filter's own, which is NOT ordered against
 * the null stream -- a caller whose inputs are produced on another stream
 * (the null stream included) passes that stream, or synchronises first, and
 * waits for the device before reading the outputs.  d_records must be
 * 16-byte aligned (the records are read as 16-byte halves; hipMalloc'd
 * memory is); d_rgb and the outputs need only their elements' alignment.
 * d_out_rgb == d_rgb is allowed (the input is repacked before the first
 * level). */
int rt_filter_run_device(RtFilter *f, const RtFilterOptions *opts, const float *d_rgb,
                         const void *d_records, float *d_out_rgb, void *d_out_rgba,
                         void *hip_stream);
/* The same from and to host memory, synchronous. */
int rt_filter_run(RtFilter *f, const RtFilterOptions *opts, const float *rgb,
                  const RtFirstHit *records, float *out_rgb, Rust_ColorU8 *out_pixels);
/* The accumulator's held samples, filtered: to host memory (synchronous), or
 * to device memory on hip_stream (NULL = the library's stream; only
 * enqueued).  Takes the handle's lock and is ordered after the accumulator's
 * last pass like its other calls.  Fails with "no samples held" when the
 * accumulator holds none -- also when its next add would reset it because the
 * camera moved or the scene was edited -- and when its world was freed.  The
 * filter's size limit is lower than the accumulator's: an accumulator of
 * 2^31 pixels or more (rt_accum_create takes up to 2^32 - 1) cannot be
 * filtered, and the call says so. */
int rt_filter_accum(RtAccum *acc, const RtFilterOptions *opts, float *out_rgb,
                    Rust_ColorU8 *pixels);
int rt_filter_accum_device(RtAccum *acc, const RtFilterOptions *opts, float *d_out_rgb,
                           void *d_rgba, void *hip_stream);

/* ---- Temporal reprojection: an accumulator's result carried across camera
 * moves.
 *
 * An accumulator starts over on every camera move; its history does not.  A
 * history belongs to one accumulator and holds two snapshots, cur and prev, of
 * resolved views.  A snapshot is, per pixel of the accumulator's frame, top row
 * first, a colour with a length {r, g, b, len} (f32: len is the number of
 * samples the colour stands for) and a guide {position.xyz, prim} from the
 * first-hit records it was made with; plus the 12 camera floats and the scene
 * edit version it was made under.  A snapshot is valid or not.
 *
 * Every step below is one rounded f32 operation, unfused; divisions are
 * correctly rounded; comparisons are false for NaN; only + - * /, fabs, floor,
 * sqrt and compares appear.
 *
 * rt_history_resolve on an accumulator that holds n_p samples per pixel (the
 * samples held, or count[p] on an adaptive accumulator):
 *   1. The accumulator's reset rule is applied first, as by rt_filter_accum:
 *      "no samples held" and "the accumulator's world was freed" are errors.
 *   2. A snapshot made under another scene edit version: both become invalid.
 *   3. cur valid and its camera differs on bits from the accumulator's camera
 *      C: cur and prev swap (the old cur is the new prev).  Else prev stays.
 *   4. The accumulator's first-hit records g are made current (rt_filter_accum's
 *      cache: su = sv = 0.5, the accumulator's accel, camera C).
 *   5. Per pixel p:  inv = 1.0f / (float)n_p;  m_k = sum_k * inv;  nf = (float)n_p.
 *      No history if prev is invalid or prim_p == 0 (sky takes none).  Else, with
 *      prev's camera O, L, H, V (origin, lower-left corner, horizontal, vertical)
 *      and P = position_p:
 *        A = L - O;  d = P - O;  n0 = H x V;  n1 = V x A;  n2 = A x H
 *          (a x b = (a.y*b.z - a.z*b.y, -(a.x*b.z - a.z*b.x), a.x*b.y - a.y*b.x),
 *           maths.rs:88-94, each product rounded before the subtraction)
 *        dot3(a, b) = ((a.x*b.x) + (a.y*b.y)) + (a.z*b.z)
 *        det = dot3(A, n0);  s = dot3(d, n0);  a = dot3(d, n1);  b = dot3(d, n2)
 *        unless (s > 0 && det > 0) || (s < 0 && det < 0): no history (behind)
 *        u = a / s;  v = b / s
 *        fx = u * (float)(width - 1) - 0.5f;  fy = v * (float)(height - 1) - 0.5f
 *          (fy counts rows from the bottom, as v does in cast_ray)
 *        unless fx > -1 && fx < (float)width && fy > -1 && fy < (float)height:
 *          no history
 *        x0 = floor(fx), tx = fx - x0;  y0 = floor(fy), ty = fy - y0
 *        taps j = 0, 1 outer, i = 0, 1 inner: q = prev's pixel at column x0 + i,
 *        bottom row y0 + j (frame index (height - 1 - row) * width + column).
 *        A tap is skipped when q is outside the image; when len_q > 0 is false;
 *        when prim_q != prim_p; when
 *          fabs(dot3(pos_q - P, normal_p)) <= sigma_z * t_p
 *        is false; and when, with wx = i ? tx : 1 - tx, wy = j ? ty : 1 - ty,
 *        w = wx * wy, w > 0 is false.  Else
 *          cs_k = cs_k + w * c_q,k;  ls = ls + w * len_q;  ws = ws + w
 *        ws > 0 false: no history.  Else hc_k = cs_k / ws, hl = ls / ws.
 *      Blend.  No history: out_k = m_k, len = nf.  With history:
 *        cap = max_history > nf ? max_history : nf
 *        tl = hl + nf;  tl = tl > cap ? cap : tl;  alpha = nf / tl
 *        out_k = hc_k + (m_k - hc_k) * alpha;  len = tl
 *   6. cur becomes {out, len} with the guide of g, camera C, valid.  Resolving
 *      again under the same camera recomputes cur from the same prev and the
 *      accumulator's newer mean: the result is a function of (prev, accumulator
 *      state), whatever the call pattern.
 *   7. Outputs: the f32 out, its RGBA8 (sqrt(out_k) * 255.999 as u8, alpha 255,
 *      as the frame resolve) or both.  With filter options the outputs are the
 *      edge-aware filter above of out with the records g; the history always
 *      stores the unfiltered out.  With prev invalid and no filter the RGBA8
 *      output is the accumulator's last frame byte for byte.
 *
 * Known limits: reflections and refractions are reprojected with the surface
 * that shows them, so they lag and ghost unless the neighbourhood clamp below
 * (rt_clamp_*) is enabled; sky takes no history. */
typedef struct RtHistoryOptions {
  float max_history;   /* finite, >= 1; default 32: the length a pixel's history is capped at */
  float sigma_z;       /* finite, > 0; default 0.02: the filter's plane-distance scale          */
} RtHistoryOptions;

/* max_history 32, sigma_z 0.02. */
void rt_history_default_options(RtHistoryOptions *opts);
/* Every call below returns 0 or a negative error with rt_last_error naming the
 * call and the argument.  Checked before a device is looked for: a null
 * accumulator, both outputs null, options out of range (the history's and the
 * filter's), a history that is not enabled, an accumulator of 2^31 pixels or
 * more.  Without a GPU every call that runs a kernel fails.
 *
 * Gives the accumulator a history with these options (NULL = the defaults), at
 * any time; both snapshots are dropped.  Buffers are allocated by the first
 * resolve and freed by rt_history_disable and rt_accum_free. */
int rt_history_enable(RtAccum *acc, const RtHistoryOptions *opts);
int rt_history_disable(RtAccum *acc);
/* Drops both snapshots and keeps the setting. */
int rt_history_reset(RtAccum *acc);
/* Resolves (above) to host memory, synchronous: out_rgb width*height*3 f32 and
 * / or pixels, top row first.  filter NULL: no filter. */
int rt_history_resolve(RtAccum *acc, const RtFilterOptions *filter, float *out_rgb,
                       Rust_ColorU8 *pixels);
/* The same to DEVICE memory on hip_stream (NULL = the library's stream), only
 * enqueued; ordered against passes, frames and filters as rt_filter_accum_device. */
int rt_history_resolve_device(RtAccum *acc, const RtFilterOptions *filter, float *d_out_rgb,
                              void *d_rgba, void *hip_stream);
/* cur's length plane: width*height f32, top row first, all 0 when cur is
 * invalid.  Waits for the last resolve. */
int rt_history_read_length(RtAccum *acc, float *len);
/* Step 5 alone on host arrays, synchronous, on `device` (-1 = current):
 * prev_cam the 12 floats of prev's camera, prev_rgbl {r, g, b, len} and
 * prev_records of prev (prev_rgbl NULL: prev is invalid; prev_cam and
 * prev_records are then not read), rgb the means m (3 f32 per pixel), n the
 * samples per pixel, records the current view's; out_rgbl {out, len}.  All
 * arrays width*height entries, top row first. */
int rt_history_run(size_t width, size_t height, const RtHistoryOptions *opts,
                   const float *prev_cam, const float *prev_rgbl, const RtFirstHit *prev_records,
                   const float *rgb, const uint32_t *n, const RtFirstHit *records, float *out_rgbl,
                   int device);

/* ---- Neighbourhood clamp of the reprojected history.
 *
 * A setting of the accumulator that rt_history_resolve and
 * rt_history_resolve_device honour.  Disabled (the default), every call
 * returns exactly what it returned without it.  Enabled, the history colour
 * of a pixel is clamped, before the blend, to a box around the mean of the
 * new samples of the pixel's neighbourhood, gamma standard deviations wide: a
 * history that no longer agrees with what the new samples show (a reflection
 * that moved, a material that was edited) is pulled to them instead of
 * ghosting for max_history samples.
 *
 * The rules of the resolve hold: every step is one rounded f32 operation,
 * unfused; / and sqrt are correctly rounded; comparisons are false for NaN;
 * only + - * /, fabs, floor, sqrt and compares appear.
 *
 * The clamp is a step inside step 5 above, between hc_k = cs_k / ws and the
 * blend, for pixels with history (ws > 0) only.  With r = radius, visit the
 * taps q = p + (i - r, j - r) in frame coordinates (columns, rows from the
 * top), j = 0 .. 2r outer, i = 0 .. 2r inner.  A q outside the image is
 * skipped.  With c = 0 (an integer) and s1_k = s2_k = 0 before the first tap,
 * each remaining tap:
 *     m_q,k = sum_q,k * inv_q,  inv_q = 1.0f / (float)n_q
 *       (the means of step 5: n_q the samples held, or count[q] on an adaptive
 *        accumulator; rt_clamp_run's rgb are these means)
 *     c = c + 1
 *     s1_k = s1_k + m_q,k
 *     s2_k = s2_k + (m_q,k * m_q,k)        (the product rounded, then the add)
 * then
 *     ic = 1.0f / (float)c
 *     mu_k  = s1_k * ic
 *     var_k = s2_k * ic - mu_k * mu_k      (both products rounded, then the subtraction)
 *     var_k = var_k < 0 ? 0 : var_k        (NaN stays NaN)
 *     wd_k  = gamma * sqrt(var_k);  lo_k = mu_k - wd_k;  hi_k = mu_k + wd_k
 *     hc_k  = hc_k < lo_k ? lo_k : hc_k;  then  hc_k = hc_k > hi_k ? hi_k : hc_k
 * A NaN bound leaves hc alone and a NaN hc stays NaN.  hl, tl, alpha, len and
 * the blend are those of step 5, applied to the clamped hc; the history stores
 * the blended out; a filter behind the resolve filters that out.  Pixels
 * without history and sky pixels are untouched.  At 1 x 1 the box collapses
 * onto the pixel's own mean: a pixel with history returns its mean on bits,
 * with len = tl.
 *
 * RT_CLAMP_KEEP_ON_EDIT (only while the clamp is enabled with it): step 2 no
 * longer invalidates snapshots made under another scene edit version, and
 * step 3 swaps cur and prev when cur is valid and its camera or its edit
 * version differs from the accumulator's.  A material edit leaves the guides
 * true; the stale colours are what the clamp is for.  A geometry edit
 * (rt_world_set_sphere_geometry) is kept too: the resolve follows the moved
 * sphere, as stated next.  Triangles cannot move.  Without the flag, or with
 * the clamp disabled, any edit drops both snapshots as before.
 *
 * A moved sphere.  A snapshot remembers {c, r} of every sphere as it was when
 * the snapshot was made.  In step 5, take a pixel p with 1 <= prim_p <=
 * nspheres, so that prim_p - 1 is its sphere; let (c1, r1) be that sphere now
 * and (c0, r0) that sphere in prev's memory.  If the four floats are equal on
 * bits, P' = P and nothing is computed.  Otherwise
 *     k  = r0 / r1
 *     e  = P - c1                 (per component)
 *     P' = c0 + e * k             (per component: the product rounded, then the add)
 * and P' replaces P in two places: in d = P' - O, and in every tap's plane test
 * fabs(dot3(pos_q - P', normal_p)) <= sigma_z * t_p.  Everything else is
 * unchanged: prim_p, normal_p, t_p, the clamp's box, the blend and len; the
 * guide stored in cur is the unmapped P.  Triangle pixels and sky are
 * untouched.  A non-finite k or P' fails the range test, and the pixel takes
 * no history; the prim-id test already denies history to pixels that the moved
 * sphere uncovered; the clamp is what pulls in the moved sphere's shadow and
 * reflections on other surfaces, which is why the flag belongs to the clamp.
 * A world that never gets a geometry edit runs exactly the kernels it ran. */
enum { RT_CLAMP_KEEP_ON_EDIT = 1 };  /* flags: a material or geometry edit keeps the history */

typedef struct RtClampOptions {
  float gamma;      /* finite, >= 0; default 1.5: half-width of the box in standard deviations */
  int32_t radius;   /* 1 .. 3; default 1: the neighbourhood is (2*radius+1)^2 pixels           */
  uint32_t flags;   /* RT_CLAMP_*; default 0; unknown bits are an error                         */
} RtClampOptions;

/* gamma 1.5, radius 1, flags 0. */
void rt_clamp_default_options(RtClampOptions *opts);
/* Every call below returns 0 or a negative error with rt_last_error naming the
 * call and the argument; the options are checked first, then the accumulator,
 * all before a device is looked for.
 *
 * Turns the clamp on with these options (NULL = the defaults), at any time,
 * with or without an enabled history.  No snapshot is dropped: a resolve is a
 * function of prev, the accumulator's state and the options.  The setting
 * survives rt_history_enable, rt_history_disable and rt_history_reset and goes
 * with rt_accum_free. */
int rt_clamp_enable(RtAccum *acc, const RtClampOptions *opts);
int rt_clamp_disable(RtAccum *acc);
/* rt_history_run with the clamp (clamp NULL = the defaults): step 5 with the
 * step above on host arrays.  out_box may be NULL; otherwise it receives
 * {lo_r, lo_g, lo_b, hi_r, hi_g, hi_b} (6 f32) for EVERY pixel, with history
 * or not, top row first: a mistake in the moments shows there, one in the
 * blend in out_rgbl. */
int rt_clamp_run(size_t width, size_t height, const RtHistoryOptions *opts,
                 const RtClampOptions *clamp, const float *prev_cam, const float *prev_rgbl,
                 const RtFirstHit *prev_records, const float *rgb, const uint32_t *n,
                 const RtFirstHit *records, float *out_rgbl, float *out_box, int device);
/* rt_clamp_run with two sphere tables: step 5 with the clamp and the "A moved
 * sphere" step on host arrays, through the kernel that a resolve after a
 * geometry edit runs.  prev_spheres is the table prev remembers and spheres
 * the table now: nspheres x {cx, cy, cz, r} each, dense; both may be NULL when
 * nspheres is 0 (every pixel is then rt_clamp_run's), a NULL table with
 * nspheres > 0 and nspheres >= 2^32 are errors.  Any bits are legal in the
 * tables, NaN included: the step above says what becomes of them.  Equal
 * tables give rt_clamp_run's out_rgbl and out_box on bits.  The device reads
 * `spheres` as an accumulator's resolve does, two float4 per sphere of which
 * the first is {c, r}; the call fills every second one with NaN and puts one
 * guard entry behind each table (NaN in prev's, zeros in the present one). */
int rt_move_run(size_t width, size_t height, const RtHistoryOptions *opts,
                const RtClampOptions *clamp, const float *prev_cam, const float *prev_rgbl,
                const RtFirstHit *prev_records, const float *rgb, const uint32_t *n,
                const RtFirstHit *records, float *out_rgbl, float *out_box,
                const float *prev_spheres, const float *spheres, size_t nspheres, int device);

/* Diagnostics: copies the per-sample colours (r, g, b, 0 as 4 f32) of the
 * LAST trace launch on `device` (-1 = current) to host `out` (n floats max).
 * That launch must have been rendered with RT_FLAG_KEEP_SAMPLES.  Output
 * order is sample-major: slot = s*(rows*width) + k*width + col for sample s
 * of tile row k (rows = tile rows of that launch).  Returns the number of
 * floats copied or a negative error. */
long rt_read_samples(const Rust_WorldHandle *handle, int device, float *out, size_t n);

/* Diagnostics: how the LAST frame trace launch on `device` (-1 = current)
 * tested the sphere tree's leaves.  0: each lane tested a leaf where its walk
 * entered it.  C >= 2: the walk recorded entered leaves, at most C per lane,
 * and the wave tested them in shared passes (the lean
 * corner-record kernel, RT_AMD_LEAF_DEFER=0 turns it off).  Both give
 * bit-identical frames.  Negative: an error. */
int rt_leaf_defer(const Rust_WorldHandle *handle, int device);

/* Diagnostics: 1 when the LAST frame trace launch on `device` (-1 = current)
 * ran the plain instance of the lean deferred-leaf kernel, in which the
 * launch's constants are compiled in (COUNTER frames of one
 * rank with primary sphere lists whose chunks resolve with plane lanes,
 * RT_AMD_PLAIN=0 turns it off), 0 when it ran another instance.  Both give
 * bit-identical frames.  Negative: an error. */
int rt_trace_plain(const Rust_WorldHandle *handle, int device);

/* Diagnostics: the number of image rows the last frame launch on `device`
 * (-1 = current) rendered with the sky kernel instead of the trace kernel:
 * rows at the top and the bottom of the image none of whose primary rays can
 * hit a sphere (one rank, COUNTER, a sphere-only scene with primary sphere
 * lists, fused resolve, no stats, depth >= 1; RT_AMD_SKY_ROWS=0 turns it
 * off).  The rows are classified on the host once the first frame of a camera
 * and frame size is enqueued, so that frame still traces every row.  0 when
 * every row was traced.  Both give bit-identical frames.
 * Negative: an error. */
int rt_sky_rows(const Rust_WorldHandle *handle, int device);

/* Diagnostics: 1 when the last frame launch on `device` (-1 = current) ran its
 * sky kernel on the library's side stream, beside the trace launches, 0 when
 * it ran on the frame's stream in front of them or the frame had no sky kernel
 * (no sky rows, nothing but sky rows, a capturing stream, RT_AMD_SKY_FORK=0).
 * Both give bit-identical frames.  Negative: an error. */
int rt_sky_forked(const Rust_WorldHandle *handle, int device);

/* Diagnostics: which trace-kernel instances were launched on `device` (-1 =
 * current) since the set was last cleared -- by frames, accumulation and
 * adaptive passes and the passes of a SERIAL frame.  The library compiles one
 * instance per combination of sphere search (0 brute force, 1 tree in global
 * memory, 2 LDS box records, 3 LDS corner records), sliced walk (0 / 1),
 * triangle search (0 none, 1 brute force, 2 binary tree, 3 its 4-wide image)
 * and kind (0 lean, 1 counted, 2 SERIAL pass, 3 accumulation pass, 4 adaptive
 * pass), at key ((search * 2 + step) * 4 + mesh) * 5 + kind, then the lean
 * corner kernel's deferred-leaf instance (key 160) and its plain twin (161).
 * Copies min(n, keys) bytes to `out` (may be NULL), 1 for each key launched,
 * clears the set when `clear` is nonzero, and returns the number of keys.
 * Negative: an error. */
int rt_trace_launched(const Rust_WorldHandle *handle, int device, unsigned char *out, size_t n,
                      int clear);
/* ... and which keys the library holds an instance for at all (some
 * combinations are served by another: DESIGN.md 5.1), 1 per such key.  Needs
 * no device.  Returns the number of keys. */
int rt_trace_instances(unsigned char *out, size_t n);

/* Frees a handle from load_world (the reference never frees, lib.rs:42-45). */
void rt_free_world(Rust_WorldHandle *handle);

/* Last error message of this thread ("" if none). */
const char *rt_last_error(void);

/* Host-side scene introspection (no GPU needed). */
size_t rt_world_num_spheres(const Rust_WorldHandle *handle);
size_t rt_world_num_triangles(const Rust_WorldHandle *handle);
/* center(3) radius material(type, r, g, b, a, param) */
int rt_world_sphere(const Rust_WorldHandle *handle, size_t i, float out[10]);
/* v0 v1 v2 normal material(type, r, g, b, a, param) */
int rt_world_triangle(const Rust_WorldHandle *handle, size_t i, float out[18]);
/* Scene editing: replaces sphere / triangle i's material with (type, r, g,
 * b, a, param), type 0 Diffuse, 1 Metal (param = fuzz), 2 Dielectric (param =
 * ir), 3 Emission (materials.rs:7-12, 100-102; the scene grammar cannot
 * produce Emission, parser.rs:175-234).  a must be 1.0 (every reference Color
 * has alpha 1).  The next frame re-uploads the scene into the device state it
 * has (streams, scratch and job counters stay; rt_device_setups does not
 * move).  0 or -1. */
int rt_world_set_sphere_material(Rust_WorldHandle *handle, size_t i, const float material[6]);
int rt_world_set_triangle_material(Rust_WorldHandle *handle, size_t i, const float material[6]);
/* Replaces sphere i's centre and radius: {cx, cy, cz, r}.  Any value a scene
 * file can spell is legal and renders as that scene file would: negative and
 * zero radius, +-inf (a 60-digit literal parses to inf).  NaN is rejected (the
 * grammar cannot produce one).  The material, the sphere's index and the
 * order of the spheres stay.  After the call the world is, for every entry of
 * this header, the world load_world returns for the scene text with that one
 * sphere statement changed (and the handle's camera, and earlier edits).
 * Accumulators start over, like after rt_world_set_sphere_material; captured
 * graphs must be destroyed before the call, as before a material edit.
 * Frames that were only enqueued (stats == NULL) may still be reading the
 * scene: the call waits on the host for every frame, pass and read enqueued on
 * the world's devices before it changes anything, and so does a material edit.
 * The sphere tree is rebuilt in full on the host (0.4 ms for 486 spheres,
 * DESIGN.md 5.10b) and the device state is kept; triangles cannot be moved.
 * Needs no GPU.  0 or -1 (rt_last_error: null handle or array, index out of
 * range, NaN). */
int rt_world_set_sphere_geometry(Rust_WorldHandle *handle, size_t i, const float geometry[4]);
/* Diagnostics: how many times a device state was set up from nothing for this world. */
long rt_device_setups(const Rust_WorldHandle *handle);
/* origin, lower_left_corner, horizontal, vertical (camera.rs:8-15) */
void rt_camera_get(const Rust_Camera *camera, float out[12]);

/* Cameras beyond the scene file's `camera origin ... aspect ...;` (always
 * looking down -z): the reference crate's other two constructors, which its
 * C-ABI never exported.  Each returns a camera that no handle owns; the caller
 * swaps it in:
 *
 *   Rust_Camera *c = rt_camera_new_look_at(from, to, up, fov, aspect);
 *   if (c) { rt_camera_free(handle->camera); handle->camera = c; }
 *
 * The field of view is in radians (camera.rs:5 Radians).  Every step is one
 * f32 operation in the reference's order (camera.rs:34-69, maths.rs:88-137,
 * 204-214): `up` is normalised first (NVec3::new), u = up x w and v = w x u
 * are NOT renormalised, and tan is the host libm's tanf, as Rust's f32::tan
 * is the platform's.  So the 12 floats are the reference's on the same host.
 *
 * Deviation: where the reference asserts (origin - look_at near zero, i.e.
 * every |component| < 1e-8; |v.y| > 1e-8 false, NaN included) rt_camera_new_
 * look_at returns NULL with rt_last_error set, like load_world on a parse
 * error.  rt_camera_from_floats rejects nothing: it is the inverse of
 * rt_camera_get on bits (a mirrored or singular camera renders; it only loses
 * the primary candidate lists where they do not apply).
 *
 * Every frame, accumulator pass and multi-device frame takes the handle's
 * camera as its 12 floats; accumulators reset when any of them changes, so a
 * mouse-look loop is "rt_camera_new_look_at, swap, add, show". */
Rust_Camera *rt_camera_new_with_vertical_fov(const float origin[3], float vertical_fov,
                                             float aspect_ratio);
Rust_Camera *rt_camera_new_look_at(const float origin[3], const float look_at[3],
                                   const float up[3], float vertical_fov, float aspect_ratio);
Rust_Camera *rt_camera_from_floats(const float camera[12]);
/* Consumes `camera` like move_camera_position and returns it moved: origin
 * and lower_left_corner + (x, y, z), one f32 add per component; horizontal
 * and vertical (the orientation and the field of view) stay.
 * move_camera_position itself remains the reference's
 * Camera::new_at(position + d, horizontal.x / vertical.y) (lib.rs:60-63),
 * which drops an oriented camera's orientation. */
Rust_Camera *rt_camera_translate(Rust_Camera *camera, float x, float y, float z);
/* Frees a camera that no handle owns (NULL is fine). */
void rt_camera_free(Rust_Camera *camera);

/* Diagnostics: where the primary triangle strip lists of the LAST frame trace
 * launch on `device` (-1 = current) were built.  0: the launch used none,
 * 1: on the host (bvh.h build_primary_tri_lists, then uploaded), 2: on the
 * device, on the frame's stream (RT_AMD_GPU_TRI_LISTS=0 keeps
 * the host build).  Both hold the same bytes.  Negative: an error. */
int rt_primary_tri_lists(const Rust_WorldHandle *handle, int device);
/* Diagnostics: how often the camera-origin triangle records of this world
 * were built (load_world builds them once for the scene's camera; 0 for a
 * scene without a triangle tree).  They are keyed on the camera origin alone:
 * a camera that turns or zooms in place leaves the count alone, and only the
 * primary lists are rebuilt.  Negative: an error. */
long rt_camera_record_builds(const Rust_WorldHandle *handle);

/* ParseError discriminant of the last failed load_world (parser.rs:11-18),
 * 100 = input on which the reference panics, -1 = none. */
int rt_last_parse_error(void);

/* image.rs:59-81: writes an ASCII PPM (P3).  Returns 0 on success. */
int rt_write_ppm(const Rust_CFramebuffer *framebuffer, const char *path);

/* The last step of a multi-device frame (ndevices > 1), on its own: reads
 * `nranks` tiles of `max_rows` rows each from DEVICE memory d_gathered (rank
 * g's tile at row g*max_rows, tile row k = image row rt_tile_row(k), the
 * layout the RCCL gather leaves on the first device) and writes the
 * width x height frame to DEVICE memory d_out, on hip_stream (NULL: the null
 * stream), without waiting.  Lets one GPU check the assembly for any rank
 * count.  Returns 0 or a negative error. */
int rt_assemble_tiles(const void *d_gathered, void *d_out, size_t width, size_t height, uint32_t row_block,
                      uint32_t nranks, size_t max_rows, void *hip_stream);

/* Number of HIP devices visible (0 if the runtime is unavailable). */
int rt_device_count(void);

/* Rank count of the RCCL communicator that multi-device frames (ndevices =
 * n, first device `first`, -1 = current) use; creates it on first use.
 * Returns n, or a negative error (e.g. fewer than first + n devices). */
int rt_comm_count(int first, int n);

#ifdef __cplusplus
}
#endif

#endif /* RAYTRACER_AMD_H */
