"""Python binding of libraytracer.so (the MI355X render path) over its C-ABI.

Mirrors the reference crate's FFI surface (Naxaes/Rust-Swift-Raytracer
raytracer/src/lib.rs:37-63: load_world / render / move_camera_position) plus
the extensions of include/raytracer_amd.h.  This module only marshals
arguments: every frame is rendered by the HIP kernels inside the library.
There is no CPU fallback -- without a GPU, rendering raises RenderError.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RT_AMD_LIB: another build of the library (A/B timing of build variants)
LIB_PATH = os.environ.get("RT_AMD_LIB") or os.path.join(HERE, "lib", "libraytracer.so")

RNG_COUNTER, RNG_REPLAY, RNG_SERIAL = 1, 2, 3
ACCEL_AUTO, ACCEL_BRUTE, ACCEL_BVH = 0, 1, 2
FLAG_KEEP_SAMPLES = 1
FLAG_SERIAL_CHECK = 2
DEFAULT_SEED = 2547549
VIEW_NORMAL, VIEW_DEPTH, VIEW_ALBEDO, VIEW_PRIM = 0, 1, 2, 3
FILTER_SAME_PRIM = 1
CLAMP_KEEP_ON_EDIT = 1

# Every symbol declared in include/raytracer.h and include/raytracer_amd.h.
EXPORTS = (
    "load_world", "render", "move_camera_position",
    "rt_default_options", "rt_tile_rows", "rt_tile_row", "rt_sample_seed", "rt_render_ex",
    "rt_render_device", "rt_read_samples", "rt_free_world", "rt_last_error", "rt_world_num_spheres",
    "rt_world_num_triangles", "rt_world_sphere", "rt_world_triangle", "rt_camera_get",
    "rt_last_parse_error", "rt_write_ppm", "rt_device_count", "rt_comm_count",
    "rt_world_set_sphere_material", "rt_world_set_triangle_material", "rt_assemble_tiles",
    "rt_accum_default_options", "rt_accum_create", "rt_accum_add", "rt_accum_add_device",
    "rt_accum_samples", "rt_accum_read", "rt_accum_reset", "rt_accum_free",
    "rt_adapt_default_options", "rt_adapt_enable", "rt_adapt_disable", "rt_adapt_active",
    "rt_adapt_read_counts", "rt_adapt_read_sumsq", "rt_adapt_read_active", "rt_leaf_defer",
    "rt_trace_plain", "rt_trace_launched", "rt_trace_instances", "rt_sky_rows",
    "rt_sky_forked",
    "rt_camera_new_with_vertical_fov", "rt_camera_new_look_at", "rt_camera_from_floats",
    "rt_camera_translate", "rt_camera_free", "rt_primary_tri_lists", "rt_camera_record_builds",
    "rt_first_hit_default_options", "rt_first_hit", "rt_first_hit_device", "rt_first_hit_pick",
    "rt_first_hit_view", "rt_first_hit_view_device",
    "rt_filter_default_options", "rt_filter_create", "rt_filter_free", "rt_filter_run_device",
    "rt_filter_run", "rt_filter_accum", "rt_filter_accum_device",
    "rt_history_default_options", "rt_history_enable", "rt_history_disable", "rt_history_reset",
    "rt_history_resolve", "rt_history_resolve_device", "rt_history_read_length", "rt_history_run",
    "rt_clamp_default_options", "rt_clamp_enable", "rt_clamp_disable", "rt_clamp_run",
    "rt_world_set_sphere_geometry", "rt_device_setups", "rt_move_run",
)


class RenderError(RuntimeError):
    pass


class ColorU8(C.Structure):
    _fields_ = [("r", C.c_uint8), ("g", C.c_uint8), ("b", C.c_uint8), ("a", C.c_uint8)]


class CFramebuffer(C.Structure):  # lib.rs:22-27
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("pixels", C.POINTER(ColorU8))]


class WorldHandle(C.Structure):  # lib.rs:29-33
    _fields_ = [("world", C.c_void_p), ("camera", C.c_void_p)]


class RenderOptions(C.Structure):
    _fields_ = [("samples_per_pixel", C.c_int32), ("max_ray_bounces", C.c_int32),
                ("rng_mode", C.c_uint32), ("seed", C.c_uint32),
                ("replay_states", C.POINTER(C.c_uint32)), ("row_block", C.c_uint32),
                ("rank", C.c_uint32), ("nranks", C.c_uint32), ("device", C.c_int32),
                ("accel", C.c_int32), ("flags", C.c_uint32), ("ndevices", C.c_int32)]


class AccumOptions(C.Structure):
    _fields_ = [("max_ray_bounces", C.c_int32), ("rng_mode", C.c_uint32), ("seed", C.c_uint32),
                ("replay_states", C.POINTER(C.c_uint32)), ("sample_stride", C.c_uint32),
                ("device", C.c_int32), ("accel", C.c_int32)]


class AdaptOptions(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("bias", C.c_float), ("min_samples", C.c_uint32)]


class RtFirstHit(C.Structure):
    """One pixel's first hit (raytracer_amd.h RtFirstHit): prim 0 = no hit, 1 + i =
    sphere i, 1 + num_spheres + j = triangle j."""
    _fields_ = [("prim", C.c_uint32), ("t", C.c_float), ("normal", C.c_float * 3),
                ("position", C.c_float * 3)]


# the same 32 bytes as a numpy structured dtype (World.first_hit's arrays)
FIRST_HIT_DTYPE = np.dtype([("prim", "<u4"), ("t", "<f4"), ("normal", "<f4", (3,)), ("position", "<f4", (3,))])


class FirstHitOptions(C.Structure):
    _fields_ = [("su", C.c_float), ("sv", C.c_float), ("x0", C.c_uint32), ("y0", C.c_uint32),
                ("w", C.c_uint32), ("h", C.c_uint32), ("device", C.c_int32), ("accel", C.c_int32)]


class FilterOptions(C.Structure):
    """raytracer_amd.h RtFilterOptions (defaults: 3, 0.5, 0.02, 5, 0)."""
    _fields_ = [("levels", C.c_int32), ("sigma_l", C.c_float), ("sigma_z", C.c_float),
                ("normal_squarings", C.c_int32), ("flags", C.c_uint32)]


class HistoryOptions(C.Structure):
    """raytracer_amd.h RtHistoryOptions (defaults: 32, 0.02)."""
    _fields_ = [("max_history", C.c_float), ("sigma_z", C.c_float)]


class ClampOptions(C.Structure):
    """raytracer_amd.h RtClampOptions (defaults: 1.5, 1, 0)."""
    _fields_ = [("gamma", C.c_float), ("radius", C.c_int32), ("flags", C.c_uint32)]


class RenderStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("sphere_tests", C.c_uint64),
                ("tri_tests", C.c_uint64), ("tri_in_range", C.c_uint64),
                ("trace_ms", C.c_double), ("resolve_ms", C.c_double),
                ("trace_launches", C.c_uint32), ("waves", C.c_uint32), ("accel", C.c_uint32),
                ("bvh_sphere_tests", C.c_uint64), ("bvh_node_tests", C.c_uint64),
                ("big_sphere_tests", C.c_uint64), ("stamp_cycles", C.c_uint64 * 4),
                ("tri_node_tests", C.c_uint64), ("bvh_tri_tests", C.c_uint64),
                ("tri_bvh", C.c_uint32), ("fused_resolve", C.c_uint32), ("serial_ms", C.c_double),
                ("serial_retries", C.c_uint32), ("primary_lists", C.c_uint32),
                ("camera_tree", C.c_uint32), ("serial_iterations", C.c_uint32),
                ("serial_checked", C.c_uint64), ("serial_chain_breaks", C.c_uint64),
                ("serial_setup_ms", C.c_double),
                ("launch_parts", C.c_uint32), ("launch_chunk", C.c_uint32),
                ("launch_refill_min", C.c_uint32), ("launch_walk_min", C.c_uint32),
                ("launch_tri_walk_min", C.c_uint32), ("launch_wsteps", C.c_uint32),
                ("launch_block_threads", C.c_uint32), ("launch_blocks", C.c_uint32),
                ("sphere_tree", C.c_uint32), ("sphere_tree_lds_bytes", C.c_uint32)]

    def as_dict(self):
        out = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            out[k] = float(v) if t is C.c_double else list(v) if k == "stamp_cycles" else int(v)
        return out


_libs = {}


def build():
    subprocess.run(["make", "-s", "-C", HERE], check=True)


def lib(path=None):
    """The loaded library (another build can be loaded side by side for A/B runs)."""
    path = path or LIB_PATH
    if path not in _libs:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 /
        # librccl.so.1 (same sonames as /opt/rocm's).  Whichever loads first
        # serves both, and torch cannot initialise on /opt/rocm's runtime
        # ("No HIP GPUs are available"), so torch is loaded first when present.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise RenderError(f"{path} is missing: run `make -C {HERE}` (build())")
        L = C.CDLL(path)
        fp = C.POINTER(C.c_float)
        H = C.POINTER(WorldHandle)
        L.load_world.restype = H
        L.load_world.argtypes = [C.c_char_p]
        L.render.restype = CFramebuffer
        L.render.argtypes = [CFramebuffer, H]
        L.move_camera_position.restype = C.c_void_p
        L.move_camera_position.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.rt_default_options.argtypes = [C.POINTER(RenderOptions)]
        L.rt_tile_rows.restype = C.c_size_t
        L.rt_tile_rows.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rt_tile_row.restype = C.c_size_t
        L.rt_tile_row.argtypes = [C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32]
        L.rt_sample_seed.restype = C.c_uint32
        L.rt_sample_seed.argtypes = [C.c_uint32, C.c_uint64]
        L.rt_render_ex.restype = C.c_int
        L.rt_render_ex.argtypes = [CFramebuffer, H, C.POINTER(RenderOptions),
                                   C.POINTER(RenderStats)]
        L.rt_render_device.restype = C.c_int
        L.rt_render_device.argtypes = [H, C.c_size_t, C.c_size_t, C.POINTER(RenderOptions),
                                       C.c_void_p, C.c_void_p, C.POINTER(RenderStats)]
        L.rt_read_samples.restype = C.c_long
        L.rt_read_samples.argtypes = [H, C.c_int, C.POINTER(C.c_float), C.c_size_t]
        L.rt_free_world.argtypes = [H]
        L.rt_last_error.restype = C.c_char_p
        L.rt_world_num_spheres.restype = C.c_size_t
        L.rt_world_num_spheres.argtypes = [H]
        L.rt_world_num_triangles.restype = C.c_size_t
        L.rt_world_num_triangles.argtypes = [H]
        L.rt_world_sphere.restype = C.c_int
        L.rt_world_sphere.argtypes = [H, C.c_size_t, fp]
        L.rt_world_triangle.restype = C.c_int
        L.rt_world_triangle.argtypes = [H, C.c_size_t, fp]
        L.rt_camera_get.argtypes = [C.c_void_p, fp]
        for f in (L.rt_world_set_sphere_material, L.rt_world_set_triangle_material):
            f.restype = C.c_int
            f.argtypes = [H, C.c_size_t, fp]
        L.rt_last_parse_error.restype = C.c_int
        L.rt_write_ppm.restype = C.c_int
        L.rt_write_ppm.argtypes = [C.POINTER(CFramebuffer), C.c_char_p]
        L.rt_device_count.restype = C.c_int
        L.rt_comm_count.restype = C.c_int
        L.rt_comm_count.argtypes = [C.c_int, C.c_int]
        L.rt_assemble_tiles.restype = C.c_int
        L.rt_assemble_tiles.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32,
                                        C.c_uint32, C.c_size_t, C.c_void_p]
        if hasattr(L, "rt_leaf_defer"):  # (an older build loaded for an A/B run has none)
            L.rt_leaf_defer.restype = C.c_int
            L.rt_leaf_defer.argtypes = [H, C.c_int]
        if hasattr(L, "rt_trace_plain"):  # (likewise)
            L.rt_trace_plain.restype = C.c_int
            L.rt_trace_plain.argtypes = [H, C.c_int]
        if hasattr(L, "rt_sky_rows"):  # (likewise)
            L.rt_sky_rows.restype = C.c_int
            L.rt_sky_rows.argtypes = [H, C.c_int]
        if hasattr(L, "rt_sky_forked"):  # (likewise)
            L.rt_sky_forked.restype = C.c_int
            L.rt_sky_forked.argtypes = [H, C.c_int]
        if hasattr(L, "rt_trace_launched"):  # (likewise)
            L.rt_trace_launched.restype = C.c_int
            L.rt_trace_launched.argtypes = [H, C.c_int, C.POINTER(C.c_uint8), C.c_size_t, C.c_int]
            L.rt_trace_instances.restype = C.c_int
            L.rt_trace_instances.argtypes = [C.POINTER(C.c_uint8), C.c_size_t]
        if hasattr(L, "rt_camera_new_look_at"):  # (likewise)
            L.rt_camera_new_with_vertical_fov.restype = C.c_void_p
            L.rt_camera_new_with_vertical_fov.argtypes = [fp, C.c_float, C.c_float]
            L.rt_camera_new_look_at.restype = C.c_void_p
            L.rt_camera_new_look_at.argtypes = [fp, fp, fp, C.c_float, C.c_float]
            L.rt_camera_from_floats.restype = C.c_void_p
            L.rt_camera_from_floats.argtypes = [fp]
            L.rt_camera_translate.restype = C.c_void_p
            L.rt_camera_translate.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
            L.rt_camera_free.restype = None
            L.rt_camera_free.argtypes = [C.c_void_p]
            L.rt_primary_tri_lists.restype = C.c_int
            L.rt_primary_tri_lists.argtypes = [H, C.c_int]
            L.rt_camera_record_builds.restype = C.c_long
            L.rt_camera_record_builds.argtypes = [H]
        if hasattr(L, "rt_accum_create"):  # (an older build loaded for an A/B run has none)
            L.rt_accum_default_options.argtypes = [C.POINTER(AccumOptions)]
            L.rt_accum_create.restype = C.c_void_p
            L.rt_accum_create.argtypes = [H, C.c_size_t, C.c_size_t, C.POINTER(AccumOptions)]
            L.rt_accum_add.restype = C.c_int
            L.rt_accum_add.argtypes = [C.c_void_p, C.c_int64, C.POINTER(ColorU8), C.POINTER(RenderStats)]
            L.rt_accum_add_device.restype = C.c_int
            L.rt_accum_add_device.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                              C.POINTER(RenderStats)]
            L.rt_accum_samples.restype = C.c_long
            L.rt_accum_samples.argtypes = [C.c_void_p]
            L.rt_accum_read.restype = C.c_int
            L.rt_accum_read.argtypes = [C.c_void_p, fp]
            L.rt_accum_reset.restype = C.c_int
            L.rt_accum_reset.argtypes = [C.c_void_p]
            L.rt_accum_free.argtypes = [C.c_void_p]
        if hasattr(L, "rt_adapt_enable"):  # (likewise)
            L.rt_adapt_default_options.argtypes = [C.POINTER(AdaptOptions)]
            L.rt_adapt_enable.restype = C.c_int
            L.rt_adapt_enable.argtypes = [C.c_void_p, C.POINTER(AdaptOptions)]
            L.rt_adapt_disable.restype = C.c_int
            L.rt_adapt_disable.argtypes = [C.c_void_p]
            L.rt_adapt_active.restype = C.c_long
            L.rt_adapt_active.argtypes = [C.c_void_p]
            L.rt_adapt_read_counts.restype = C.c_int
            L.rt_adapt_read_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            L.rt_adapt_read_sumsq.restype = C.c_int
            L.rt_adapt_read_sumsq.argtypes = [C.c_void_p, fp]
            L.rt_adapt_read_active.restype = C.c_long
            L.rt_adapt_read_active.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t]
        if hasattr(L, "rt_first_hit"):  # (likewise)
            FO = C.POINTER(FirstHitOptions)
            L.rt_first_hit_default_options.restype = None
            L.rt_first_hit_default_options.argtypes = [FO]
            L.rt_first_hit.restype = C.c_int
            L.rt_first_hit.argtypes = [H, C.c_size_t, C.c_size_t, FO, C.c_void_p]
            L.rt_first_hit_device.restype = C.c_int
            L.rt_first_hit_device.argtypes = [H, C.c_size_t, C.c_size_t, FO, C.c_void_p, C.c_void_p]
            L.rt_first_hit_pick.restype = C.c_int
            L.rt_first_hit_pick.argtypes = [H, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, FO,
                                            C.POINTER(RtFirstHit)]
            L.rt_first_hit_view.restype = C.c_int
            L.rt_first_hit_view.argtypes = [H, C.c_size_t, C.c_size_t, FO, C.c_int, C.POINTER(ColorU8)]
            L.rt_first_hit_view_device.restype = C.c_int
            L.rt_first_hit_view_device.argtypes = [H, C.c_size_t, C.c_size_t, FO, C.c_int, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_filter_create"):  # (likewise)
            LO = C.POINTER(FilterOptions)
            L.rt_filter_default_options.restype = None
            L.rt_filter_default_options.argtypes = [LO]
            L.rt_filter_create.restype = C.c_void_p
            L.rt_filter_create.argtypes = [C.c_size_t, C.c_size_t, C.c_int]
            L.rt_filter_free.restype = None
            L.rt_filter_free.argtypes = [C.c_void_p]
            L.rt_filter_run_device.restype = C.c_int
            L.rt_filter_run_device.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
            L.rt_filter_run.restype = C.c_int
            L.rt_filter_run.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.rt_filter_accum.restype = C.c_int
            L.rt_filter_accum.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p]
            L.rt_filter_accum_device.restype = C.c_int
            L.rt_filter_accum_device.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(L, "rt_history_enable"):  # (likewise)
            LO = C.POINTER(FilterOptions)
            HO = C.POINTER(HistoryOptions)
            L.rt_history_default_options.restype = None
            L.rt_history_default_options.argtypes = [HO]
            L.rt_history_enable.restype = C.c_int
            L.rt_history_enable.argtypes = [C.c_void_p, HO]
            L.rt_history_disable.restype = C.c_int
            L.rt_history_disable.argtypes = [C.c_void_p]
            L.rt_history_reset.restype = C.c_int
            L.rt_history_reset.argtypes = [C.c_void_p]
            L.rt_history_resolve.restype = C.c_int
            L.rt_history_resolve.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p]
            L.rt_history_resolve_device.restype = C.c_int
            L.rt_history_resolve_device.argtypes = [C.c_void_p, LO, C.c_void_p, C.c_void_p, C.c_void_p]
            L.rt_history_read_length.restype = C.c_int
            L.rt_history_read_length.argtypes = [C.c_void_p, C.c_void_p]
            L.rt_history_run.restype = C.c_int
            L.rt_history_run.argtypes = [C.c_size_t, C.c_size_t, HO] + [C.c_void_p] * 7 + [C.c_int]
        if hasattr(L, "rt_clamp_enable"):  # (likewise)
            HO = C.POINTER(HistoryOptions)
            CO = C.POINTER(ClampOptions)
            L.rt_clamp_default_options.restype = None
            L.rt_clamp_default_options.argtypes = [CO]
            L.rt_clamp_enable.restype = C.c_int
            L.rt_clamp_enable.argtypes = [C.c_void_p, CO]
            L.rt_clamp_disable.restype = C.c_int
            L.rt_clamp_disable.argtypes = [C.c_void_p]
            L.rt_clamp_run.restype = C.c_int
            L.rt_clamp_run.argtypes = [C.c_size_t, C.c_size_t, HO, CO] + [C.c_void_p] * 8 + [C.c_int]
        if hasattr(L, "rt_world_set_sphere_geometry"):  # (likewise)
            L.rt_world_set_sphere_geometry.restype = C.c_int
            L.rt_world_set_sphere_geometry.argtypes = [H, C.c_size_t, fp]
            L.rt_device_setups.restype = C.c_long
            L.rt_device_setups.argtypes = [H]
        if hasattr(L, "rt_move_run"):  # (likewise)
            L.rt_move_run.restype = C.c_int
            L.rt_move_run.argtypes = ([C.c_size_t, C.c_size_t, C.POINTER(HistoryOptions), C.POINTER(ClampOptions)] +
                                      [C.c_void_p] * 10 + [C.c_size_t, C.c_int])
        _libs[path] = L
    return _libs[path]


def trace_instances(L=None) -> np.ndarray:
    """rt_trace_instances: uint8 per trace-kernel key, 1 where the library holds an
    instance (raytracer_amd.h rt_trace_launched spells the key).  Needs no device."""
    L = L or lib()
    out = np.zeros(L.rt_trace_instances(None, 0), np.uint8)
    L.rt_trace_instances(out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size)
    return out


def last_error() -> str:
    return lib().rt_last_error().decode("utf-8", "replace")


def device_count() -> int:
    return int(lib().rt_device_count())


def comm_count(first: int, n: int) -> int:
    """Ranks of the RCCL communicator a multi-device frame over devices
    [first, first + n) uses (created on first use); raises on error."""
    r = int(lib().rt_comm_count(first, n))
    if r < 0:
        raise RenderError(f"rt_comm_count failed ({r}): {last_error()}")
    return r


def assemble_tiles(gathered_ptr: int, out_ptr: int, width, height, row_block, nranks, max_rows,
                   stream_ptr: int = 0):
    """rt_assemble_tiles: the multi-device frame assembly on device buffers."""
    rc = lib().rt_assemble_tiles(C.c_void_p(gathered_ptr), C.c_void_p(out_ptr), width, height, row_block,
                                 nranks, max_rows, C.c_void_p(stream_ptr or None))
    if rc != 0:
        raise RenderError(f"rt_assemble_tiles failed ({rc}): {last_error()}")


def tile_rows(height, row_block, rank, nranks) -> int:
    return int(lib().rt_tile_rows(height, row_block, rank, nranks))


def tile_row(k, row_block, rank, nranks) -> int:
    return int(lib().rt_tile_row(k, row_block, rank, nranks))


def sample_seed(seed: int, job: int) -> int:
    return int(lib().rt_sample_seed(seed, job))


def options(spp=16, depth=8, mode=RNG_COUNTER, seed=DEFAULT_SEED, replay=None, row_block=8,
            rank=0, nranks=1, device=-1, accel=ACCEL_AUTO, keep_samples=False, L=None,
            ndevices=0, serial_check=False):
    o = RenderOptions()
    (L or lib()).rt_default_options(C.byref(o))
    o.samples_per_pixel, o.max_ray_bounces, o.rng_mode, o.seed = spp, depth, mode, seed
    o.row_block, o.rank, o.nranks, o.device = row_block, rank, nranks, device
    o.accel = accel
    o.ndevices = ndevices
    o.flags = (FLAG_KEEP_SAMPLES if keep_samples else 0) | (FLAG_SERIAL_CHECK if serial_check else 0)
    keep = None
    if replay is not None:
        keep = np.ascontiguousarray(replay, dtype=np.uint32)
        o.replay_states = keep.ctypes.data_as(C.POINTER(C.c_uint32))
    return o, keep


def _vec3(v):
    a = np.ascontiguousarray(v, dtype=np.float32)
    if a.size != 3:
        raise ValueError("a point or vector is 3 floats")
    return a


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class World:
    """A loaded world: load_world (lib.rs:37-46) + camera moves + rendering."""

    def __init__(self, source: str | bytes, lib_path=None):
        self._L = lib(lib_path)
        if isinstance(source, str):
            source = source.encode("utf-8")
        self._h = self._L.load_world(source)
        if not self._h:
            raise ValueError(f"load_world failed: parse error {self._L.rt_last_parse_error()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.rt_free_world(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def num_spheres(self):
        return int(self._L.rt_world_num_spheres(self._h))

    @property
    def num_triangles(self):
        return int(self._L.rt_world_num_triangles(self._h))

    def spheres(self):
        out = np.zeros((self.num_spheres, 10), np.float32)
        for i in range(self.num_spheres):
            self._L.rt_world_sphere(self._h, i, out[i].ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def triangles(self):
        out = np.zeros((self.num_triangles, 18), np.float32)
        for i in range(self.num_triangles):
            self._L.rt_world_triangle(self._h, i, out[i].ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def set_material(self, i, kind, rgb, param=0.0, triangle=False):
        """rt_world_set_{sphere,triangle}_material: kind 0 Diffuse, 1 Metal,
        2 Dielectric, 3 Emission (materials.rs:7-12)."""
        m = np.array([kind, rgb[0], rgb[1], rgb[2], 1.0, param], np.float32)
        f = self._L.rt_world_set_triangle_material if triangle else self._L.rt_world_set_sphere_material
        if f(self._h, i, m.ctypes.data_as(C.POINTER(C.c_float))) != 0:
            raise ValueError(f"set_material failed: {last_error()}")

    def set_sphere(self, i, center, radius):
        """rt_world_set_sphere_geometry: sphere i's centre and radius replaced (any
        float but NaN); its material and index stay.  Needs no GPU."""
        g = np.array([center[0], center[1], center[2], radius], np.float32)
        if self._L.rt_world_set_sphere_geometry(self._h, i, _fp(g)) != 0:
            raise ValueError(f"set_sphere failed: {self._L.rt_last_error().decode()}")

    def device_setups(self):
        """rt_device_setups: device states set up from nothing for this world so far."""
        return int(self._L.rt_device_setups(self._h))

    def camera(self):
        c = np.zeros(12, np.float32)
        self._L.rt_camera_get(self._h.contents.camera, c.ctypes.data_as(C.POINTER(C.c_float)))
        return c

    def move_camera(self, x, y, z):
        """GameView.swift:200-216: handle.camera = move_camera_position(camera, ...)."""
        self._h.contents.camera = self._L.move_camera_position(self._h.contents.camera, x, y, z)

    def _swap_camera(self, cam, what):
        """The header's pattern: if (c) { rt_camera_free(h->camera); h->camera = c; }"""
        if not cam:
            raise ValueError(f"{what} failed: {self._L.rt_last_error().decode()}")
        self._L.rt_camera_free(self._h.contents.camera)
        self._h.contents.camera = cam

    def look_at(self, origin, target, up=(0.0, 1.0, 0.0), vfov=np.pi / 2, aspect=1.5):
        """rt_camera_new_look_at (camera.rs:49-69): the camera at `origin` facing
        `target`; vfov in radians.  ValueError where the reference asserts."""
        o, t, u = (_vec3(v) for v in (origin, target, up))
        self._swap_camera(self._L.rt_camera_new_look_at(_fp(o), _fp(t), _fp(u), vfov, aspect), "look_at")

    def vertical_fov(self, origin, vfov, aspect=1.5):
        """rt_camera_new_with_vertical_fov (camera.rs:34-48): looking down -z."""
        o = _vec3(origin)
        self._swap_camera(self._L.rt_camera_new_with_vertical_fov(_fp(o), vfov, aspect), "vertical_fov")

    def set_camera(self, cam12):
        """rt_camera_from_floats: the 12 floats of camera(), bits as given (what a
        tiles.py rank or a second World needs to share this one's view)."""
        c = np.ascontiguousarray(cam12, dtype=np.float32)
        if c.size != 12:
            raise ValueError("a camera is 12 floats")
        self._swap_camera(self._L.rt_camera_from_floats(_fp(c)), "set_camera")

    def translate_camera(self, x, y, z):
        """rt_camera_translate: moves the camera and keeps its orientation
        (move_camera rebuilds a -z camera, as the reference does)."""
        self._h.contents.camera = self._L.rt_camera_translate(self._h.contents.camera, x, y, z)

    def primary_tri_lists(self, device=-1):
        """rt_primary_tri_lists: where the last frame launch's primary triangle
        lists were built (0 none, 1 host, 2 device)."""
        n = self._L.rt_primary_tri_lists(self._h, device)
        if n < 0:
            raise RenderError(f"rt_primary_tri_lists failed ({n}): {self._L.rt_last_error().decode()}")
        return n

    def camera_record_builds(self):
        """rt_camera_record_builds: builds of the camera-origin triangle records so far."""
        return int(self._L.rt_camera_record_builds(self._h))

    def render_reference(self, width, height):
        """The reference ABI call render(fb, handle): 16 spp, depth 8 (lib.rs:49-57)."""
        px = np.zeros((height, width, 4), np.uint8)
        fb = CFramebuffer(width, height, px.ctypes.data_as(C.POINTER(ColorU8)))
        res = self._L.render(fb, self._h)
        if not res.pixels and width * height:
            raise RenderError(self._L.rt_last_error().decode())
        return px

    def render(self, width, height, spp=16, depth=8, mode=RNG_COUNTER, seed=DEFAULT_SEED,
               replay=None, row_block=8, rank=0, nranks=1, device=-1, accel=ACCEL_AUTO,
               keep_samples=False, stats=True, ndevices=0, serial_check=False):
        """rt_render_ex -> (rgba uint8[tile_rows, width, 4], stats dict).
        keep_samples: write every sample to the slab (for read_samples) and
        resolve with the second kernel; the frame is bit-identical.
        stats=False: no counters (the kernel variant without them; stats None).
        ndevices >= 1: the whole frame, row-tiled over that many devices of this
        process and gathered with RCCL (RtRenderOptions.ndevices).
        serial_check: RT_FLAG_SERIAL_CHECK (SERIAL: verify the start-state chain)."""
        o, keep = options(spp, depth, mode, seed, replay, row_block, rank, nranks, device, accel,
                          keep_samples, self._L, ndevices, serial_check)
        rows = int(self._L.rt_tile_rows(height, row_block, rank, nranks)) if nranks > 1 else height
        px = np.zeros((rows, width, 4), np.uint8)
        fb = CFramebuffer(width, height, px.ctypes.data_as(C.POINTER(ColorU8)))
        st = RenderStats()
        rc = self._L.rt_render_ex(fb, self._h, C.byref(o), C.byref(st) if stats else None)
        del keep
        if rc != 0:
            raise RenderError(f"rt_render_ex failed ({rc}): {self._L.rt_last_error().decode()}")
        return px, (st.as_dict() if stats else None)

    def accumulator(self, width, height, stride, depth=8, mode=RNG_COUNTER, seed=DEFAULT_SEED,
                    replay=None, accel=ACCEL_AUTO, device=-1):
        """rt_accum_create: a progressive accumulation of this world's frame at
        its current camera, `stride` samples per pixel at most (Accumulator)."""
        return Accumulator(self, width, height, stride, depth, mode, seed, replay, accel, device)

    def read_samples(self, njobs, device=-1):
        """Per-sample colours of the last trace launch: float32[njobs, 4]."""
        out = np.zeros((njobs, 4), np.float32)
        n = self._L.rt_read_samples(self._h, device, out.ctypes.data_as(C.POINTER(C.c_float)),
                                  out.size)
        if n < 0:
            raise RenderError(f"rt_read_samples failed ({n}): {self._L.rt_last_error().decode()}")
        return out[: n // 4]

    def leaf_defer(self, device=-1):
        """rt_leaf_defer: pending leaves per lane of the deferred-leaf walk the
        last frame trace launch ran (0: it tested leaves where it entered them)."""
        n = self._L.rt_leaf_defer(self._h, device)
        if n < 0:
            raise RenderError(f"rt_leaf_defer failed ({n}): {self._L.rt_last_error().decode()}")
        return n

    def trace_plain(self, device=-1):
        """rt_trace_plain: 1 when the last frame trace launch ran the plain instance
        of the lean deferred-leaf kernel, 0 when it ran another instance."""
        n = self._L.rt_trace_plain(self._h, device)
        if n < 0:
            raise RenderError(f"rt_trace_plain failed ({n}): {self._L.rt_last_error().decode()}")
        return n

    def sky_rows(self, device=-1):
        """rt_sky_rows: image rows the last frame launch rendered with the sky kernel
        (rows whose primary rays can hit nothing), 0 when every row was traced."""
        n = self._L.rt_sky_rows(self._h, device)
        if n < 0:
            raise RenderError(f"rt_sky_rows failed ({n}): {self._L.rt_last_error().decode()}")
        return n

    def sky_forked(self, device=-1):
        """rt_sky_forked: 1 when the last frame launch ran its sky kernel on the
        library's side stream, beside the trace launches, else 0."""
        n = self._L.rt_sky_forked(self._h, device)
        if n < 0:
            raise RenderError(f"rt_sky_forked failed ({n}): {self._L.rt_last_error().decode()}")
        return n

    def trace_launched(self, clear=False, device=-1):
        """rt_trace_launched: uint8 per trace-kernel key, 1 for each instance launched
        on the device since the set was last cleared (clear=True: cleared after the read)."""
        out = np.zeros(self._L.rt_trace_instances(None, 0), np.uint8)
        n = self._L.rt_trace_launched(self._h, device, out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size,
                                      1 if clear else 0)
        if n < 0:
            raise RenderError(f"rt_trace_launched failed ({n}): {self._L.rt_last_error().decode()}")
        return out

    def render_device(self, width, height, out_ptr: int, stream_ptr: int = 0, spp=16, depth=8,
                      mode=RNG_COUNTER, seed=DEFAULT_SEED, row_block=8, rank=0, nranks=1,
                      device=-1, accel=ACCEL_AUTO, stats=True, keep_samples=False, ndevices=0,
                      serial_check=False):
        """rt_render_device into a device buffer (e.g. a torch uint8 tensor).
        stats=False: no counters and no host wait -- the frame is only enqueued
        on the stream (returns None)."""
        o, _ = options(spp, depth, mode, seed, None, row_block, rank, nranks, device, accel,
                       keep_samples, self._L, ndevices, serial_check)
        st = RenderStats()
        rc = self._L.rt_render_device(self._h, width, height, C.byref(o), C.c_void_p(out_ptr),
                                    C.c_void_p(stream_ptr or None), C.byref(st) if stats else None)
        if rc != 0:
            raise RenderError(f"rt_render_device failed ({rc}): {self._L.rt_last_error().decode()}")
        return st.as_dict() if stats else None


    # ---- first-hit records (rt_first_hit_*)
    def _first_hit_options(self, su, sv, rect, accel, device):
        o = FirstHitOptions()
        self._L.rt_first_hit_default_options(C.byref(o))
        o.su, o.sv, o.accel, o.device = su, sv, accel, device
        if rect is not None:
            o.x0, o.y0, o.w, o.h = rect
        return o

    @staticmethod
    def _first_hit_shape(width, height, rect):
        return (height, width) if rect is None or tuple(rect) == (0, 0, 0, 0) else (rect[3], rect[2])

    def _first_hit_check(self, rc, what):
        if rc != 0:
            raise RenderError(f"{what} failed ({rc}): {self._L.rt_last_error().decode()}")

    def first_hit(self, width, height, su=0.5, sv=0.5, rect=None, accel=ACCEL_AUTO, device=-1):
        """rt_first_hit: what each pixel's primary ray (sub-pixel offsets su, sv, no
        RNG) hits first -> FIRST_HIT_DTYPE[h, w], top row first.  rect = (x0, y0, w,
        h), y0 from the top row: only those pixels."""
        o = self._first_hit_options(su, sv, rect, accel, device)
        out = np.zeros(self._first_hit_shape(width, height, rect), FIRST_HIT_DTYPE)
        self._first_hit_check(self._L.rt_first_hit(self._h, width, height, C.byref(o), out.ctypes.data), "rt_first_hit")
        return out

    def first_hit_device(self, width, height, out_ptr: int, stream_ptr: int = 0, su=0.5, sv=0.5, rect=None,
                         accel=ACCEL_AUTO, device=-1):
        """rt_first_hit_device: the records into device memory (32 bytes per pixel),
        only enqueued on the stream."""
        o = self._first_hit_options(su, sv, rect, accel, device)
        self._first_hit_check(self._L.rt_first_hit_device(self._h, width, height, C.byref(o), C.c_void_p(out_ptr),
                                                          C.c_void_p(stream_ptr or None)), "rt_first_hit_device")

    def pick(self, width, height, col, row, su=0.5, sv=0.5, accel=ACCEL_AUTO, device=-1):
        """rt_first_hit_pick: the record of the pixel at col (from the left), row (from
        the top) -> a FIRST_HIT_DTYPE scalar (rec["prim"]: 0 none, 1 + i sphere i,
        1 + num_spheres + j triangle j)."""
        o = self._first_hit_options(su, sv, None, accel, device)
        rec = RtFirstHit()
        self._first_hit_check(self._L.rt_first_hit_pick(self._h, width, height, col, row, C.byref(o), C.byref(rec)),
                              "rt_first_hit_pick")
        return np.frombuffer(bytes(rec), FIRST_HIT_DTYPE)[0]

    def first_hit_view(self, width, height, view, su=0.5, sv=0.5, rect=None, accel=ACCEL_AUTO, device=-1):
        """rt_first_hit_view: VIEW_NORMAL / VIEW_DEPTH / VIEW_ALBEDO / VIEW_PRIM of the
        same pixels -> uint8[h, w, 4]."""
        o = self._first_hit_options(su, sv, rect, accel, device)
        px = np.zeros(self._first_hit_shape(width, height, rect) + (4,), np.uint8)
        self._first_hit_check(self._L.rt_first_hit_view(self._h, width, height, C.byref(o), view,
                                                        px.ctypes.data_as(C.POINTER(ColorU8))), "rt_first_hit_view")
        return px

    def first_hit_view_device(self, width, height, view, out_ptr: int, stream_ptr: int = 0, su=0.5, sv=0.5,
                              rect=None, accel=ACCEL_AUTO, device=-1):
        """rt_first_hit_view_device: the view into device memory (RGBA8), only enqueued."""
        o = self._first_hit_options(su, sv, rect, accel, device)
        self._first_hit_check(self._L.rt_first_hit_view_device(self._h, width, height, C.byref(o), view,
                                                               C.c_void_p(out_ptr), C.c_void_p(stream_ptr or None)),
                              "rt_first_hit_view_device")


class Accumulator:
    """rt_accum_*: a progressive accumulation of one world's frame (World.accumulator).
    Holds its World, so the world outlives it."""

    def __init__(self, world, width, height, stride, depth=8, mode=RNG_COUNTER, seed=DEFAULT_SEED,
                 replay=None, accel=ACCEL_AUTO, device=-1):
        self._world, self._L = world, world._L
        self.width, self.height, self.stride = width, height, stride
        o = AccumOptions()
        self._L.rt_accum_default_options(C.byref(o))
        o.max_ray_bounces, o.rng_mode, o.seed, o.sample_stride = depth, mode, seed, stride
        o.device, o.accel = device, accel
        keep = None
        if replay is not None:
            keep = np.ascontiguousarray(replay, dtype=np.uint32)
            if keep.size != width * height * stride:
                raise ValueError("replay table must hold width * height * stride states")
            o.replay_states = keep.ctypes.data_as(C.POINTER(C.c_uint32))
        self._a = self._L.rt_accum_create(world.handle, width, height, C.byref(o))
        del keep  # (uploaded at creation)
        if not self._a:
            raise RenderError(f"rt_accum_create failed: {self._L.rt_last_error().decode()}")

    def close(self):
        if getattr(self, "_a", None):
            self._L.rt_accum_free(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise RenderError(f"{what} failed ({rc}): {self._L.rt_last_error().decode()}")
        return rc

    def add(self, n, stats=True):
        """n more samples per pixel -> (rgba uint8[height, width, 4] of all held samples, stats dict)."""
        px = np.zeros((self.height, self.width, 4), np.uint8)
        st = RenderStats()
        self._check(self._L.rt_accum_add(self._a, n, px.ctypes.data_as(C.POINTER(ColorU8)),
                                         C.byref(st) if stats else None), "rt_accum_add")
        return px, (st.as_dict() if stats else None)

    def add_device(self, n, out_ptr, stream_ptr=0, stats=False):
        """rt_accum_add_device: the frame into device memory (out_ptr 0: accumulate only);
        without stats the pass is only enqueued on the stream."""
        st = RenderStats()
        self._check(self._L.rt_accum_add_device(self._a, n, C.c_void_p(out_ptr or None),
                                                C.c_void_p(stream_ptr or None),
                                                C.byref(st) if stats else None), "rt_accum_add_device")
        return st.as_dict() if stats else None

    @property
    def samples(self):
        return int(self._check(self._L.rt_accum_samples(self._a), "rt_accum_samples"))

    def sums(self):
        """The raw f32 sums: float32[height, width, 3], top row first."""
        out = np.zeros((self.height, self.width, 3), np.float32)
        self._check(self._L.rt_accum_read(self._a, out.ctypes.data_as(C.POINTER(C.c_float))), "rt_accum_read")
        return out

    def reset(self):
        self._check(self._L.rt_accum_reset(self._a), "rt_accum_reset")

    # ---- adaptive accumulation (rt_adapt_*)
    def set_adaptive(self, tolerance=None, bias=None, min_samples=None, enable=True):
        """rt_adapt_enable with the defaults overridden (enable=False: rt_adapt_disable);
        the accumulator must hold no samples."""
        if not enable:
            self._check(self._L.rt_adapt_disable(self._a), "rt_adapt_disable")
            return
        o = AdaptOptions()
        self._L.rt_adapt_default_options(C.byref(o))
        if tolerance is not None:
            o.tolerance = tolerance
        if bias is not None:
            o.bias = bias
        if min_samples is not None:
            o.min_samples = min_samples
        self._check(self._L.rt_adapt_enable(self._a, C.byref(o)), "rt_adapt_enable")

    @property
    def active(self):
        """Pixels still sampled (width * height with no samples held or when not adaptive)."""
        return int(self._check(self._L.rt_adapt_active(self._a), "rt_adapt_active"))

    def counts(self):
        """Samples each pixel holds: uint32[height, width], top row first."""
        out = np.zeros((self.height, self.width), np.uint32)
        self._check(self._L.rt_adapt_read_counts(self._a, out.ctypes.data_as(C.POINTER(C.c_uint32))),
                    "rt_adapt_read_counts")
        return out

    def sumsq(self):
        """The fold of y * y, y = (r + g) + b: float32[height, width], top row first."""
        out = np.zeros((self.height, self.width), np.float32)
        self._check(self._L.rt_adapt_read_sumsq(self._a, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "rt_adapt_read_sumsq")
        return out

    # ---- the held samples, filtered (rt_filter_accum*)
    def filtered(self, **opts):
        """rt_filter_accum -> (rgb float32[height, width, 3], rgba uint8[height, width, 4]);
        options as filter_options (levels, sigma_l, sigma_z, normal_squarings, flags)."""
        o = filter_options(self._L, **opts)
        out = np.zeros((self.height, self.width, 3), np.float32)
        px = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(self._L.rt_filter_accum(self._a, C.byref(o), out.ctypes.data, px.ctypes.data), "rt_filter_accum")
        return out, px

    def filtered_device(self, out_rgb_ptr: int = 0, out_rgba_ptr: int = 0, stream_ptr: int = 0, **opts):
        """rt_filter_accum_device: into device memory, only enqueued on the stream."""
        o = filter_options(self._L, **opts)
        self._check(self._L.rt_filter_accum_device(self._a, C.byref(o), C.c_void_p(out_rgb_ptr or None),
                                                   C.c_void_p(out_rgba_ptr or None),
                                                   C.c_void_p(stream_ptr or None)), "rt_filter_accum_device")

    # ---- the resolved view carried across camera moves (rt_history_*)
    def history_enable(self, **opts):
        """rt_history_enable with the defaults overridden (max_history, sigma_z); drops both snapshots."""
        o = history_options(self._L, **opts)
        self._check(self._L.rt_history_enable(self._a, C.byref(o)), "rt_history_enable")

    def history_disable(self):
        self._check(self._L.rt_history_disable(self._a), "rt_history_disable")

    def history_reset(self):
        """Drops both snapshots and keeps the setting."""
        self._check(self._L.rt_history_reset(self._a), "rt_history_reset")

    def resolved(self, filter=None):
        """rt_history_resolve -> (rgb float32[height, width, 3], rgba uint8[height, width, 4]): the
        held samples blended with the history reprojected from the last camera.  filter: None,
        or a dict of filter_options fields ({} = the default filter) applied to the result."""
        o = None if filter is None else filter_options(self._L, **filter)
        out = np.zeros((self.height, self.width, 3), np.float32)
        px = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(self._L.rt_history_resolve(self._a, C.byref(o) if o is not None else None, out.ctypes.data,
                                               px.ctypes.data), "rt_history_resolve")
        return out, px

    def resolved_device(self, out_rgb_ptr: int = 0, out_rgba_ptr: int = 0, stream_ptr: int = 0, filter=None):
        """rt_history_resolve_device: into device memory, only enqueued on the stream."""
        o = None if filter is None else filter_options(self._L, **filter)
        self._check(self._L.rt_history_resolve_device(self._a, C.byref(o) if o is not None else None,
                                                      C.c_void_p(out_rgb_ptr or None),
                                                      C.c_void_p(out_rgba_ptr or None),
                                                      C.c_void_p(stream_ptr or None)), "rt_history_resolve_device")

    def history_length(self):
        """The samples each pixel of the last resolve stands for: float32[height, width], top row
        first (all 0 before the first resolve)."""
        out = np.zeros((self.height, self.width), np.float32)
        self._check(self._L.rt_history_read_length(self._a, out.ctypes.data), "rt_history_read_length")
        return out

    # ---- the resolve's neighbourhood clamp (rt_clamp_*)
    def clamp_enable(self, **opts):
        """rt_clamp_enable with the defaults overridden (gamma, radius, flags;
        keep_on_edit=True sets CLAMP_KEEP_ON_EDIT); drops no snapshot."""
        o = clamp_options(self._L, **opts)
        self._check(self._L.rt_clamp_enable(self._a, C.byref(o)), "rt_clamp_enable")

    def clamp_disable(self):
        self._check(self._L.rt_clamp_disable(self._a), "rt_clamp_disable")

    def active_list(self):
        """The active list: uint32 frame indices (row * width + col, top row first), ascending."""
        out = np.zeros(self.width * self.height, np.uint32)
        n = self._check(self._L.rt_adapt_read_active(self._a, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size),
                        "rt_adapt_read_active")
        return out[:n].copy()


def filter_options(L=None, **opts):
    """rt_filter_default_options with the fields given overridden (levels, sigma_l,
    sigma_z, normal_squarings, flags; same_prim=True sets FILTER_SAME_PRIM)."""
    o = FilterOptions()
    (L or lib()).rt_filter_default_options(C.byref(o))
    if opts.pop("same_prim", False):
        o.flags |= FILTER_SAME_PRIM
    for k, v in opts.items():
        if k not in ("levels", "sigma_l", "sigma_z", "normal_squarings", "flags"):
            raise TypeError(f"unknown filter option {k!r}")
        setattr(o, k, (o.flags | v) if k == "flags" else v)
    return o


def history_options(L=None, **opts):
    """rt_history_default_options with the fields given overridden (max_history, sigma_z)."""
    o = HistoryOptions()
    (L or lib()).rt_history_default_options(C.byref(o))
    for k, v in opts.items():
        if k not in ("max_history", "sigma_z"):
            raise TypeError(f"unknown history option {k!r}")
        setattr(o, k, v)
    return o


def history_run(rgb, n, records, prev_cam=None, prev_rgbl=None, prev_records=None, device=-1, L=None, **opts):
    """rt_history_run: the reprojection and blend of one resolve on host arrays.  rgb
    float32[height, width, 3] (the means), n uint32[height, width], records
    FIRST_HIT_DTYPE[height, width]; prev_cam (12 floats), prev_rgbl float32[height, width, 4]
    and prev_records of the last view, or all None for none -> float32[height, width, 4]
    {r, g, b, len}."""
    L = L or lib()
    o = history_options(L, **opts)
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("rgb is height x width x 3 floats")
    h, w = c.shape[:2]
    cnt = np.ascontiguousarray(n, dtype=np.uint32)
    g = np.ascontiguousarray(records, dtype=FIRST_HIT_DTYPE)
    if cnt.size != w * h or g.size != w * h:
        raise ValueError("n and records are height x width")
    pc = pl = pg = None
    if prev_rgbl is not None:
        pc = np.ascontiguousarray(prev_cam, dtype=np.float32)
        pl = np.ascontiguousarray(prev_rgbl, dtype=np.float32)
        pg = np.ascontiguousarray(prev_records, dtype=FIRST_HIT_DTYPE)
        if pc.size != 12 or pl.size != 4 * w * h or pg.size != w * h:
            raise ValueError("prev_cam is 12 floats, prev_rgbl height x width x 4, prev_records height x width")
    out = np.zeros((h, w, 4), np.float32)
    rc = L.rt_history_run(w, h, C.byref(o), *(a.ctypes.data if a is not None else None for a in (pc, pl, pg)),
                          c.ctypes.data, cnt.ctypes.data, g.ctypes.data, out.ctypes.data, device)
    if rc != 0:
        raise RenderError(f"rt_history_run failed ({rc}): {L.rt_last_error().decode()}")
    return out


def clamp_options(L=None, **opts):
    """rt_clamp_default_options with the fields given overridden (gamma, radius,
    flags; keep_on_edit=True sets CLAMP_KEEP_ON_EDIT)."""
    o = ClampOptions()
    (L or lib()).rt_clamp_default_options(C.byref(o))
    if opts.pop("keep_on_edit", False):
        o.flags |= CLAMP_KEEP_ON_EDIT
    for k, v in opts.items():
        if k not in ("gamma", "radius", "flags"):
            raise TypeError(f"unknown clamp option {k!r}")
        setattr(o, k, (o.flags | v) if k == "flags" else v)
    return o


def clamp_run(rgb, n, records, prev_cam=None, prev_rgbl=None, prev_records=None, clamp=None, box=True, device=-1,
              L=None, **opts):
    """rt_clamp_run: rt_history_run with the neighbourhood clamp.  The arrays as
    history_run's; clamp: a dict of clamp_options fields (None: the defaults); opts:
    history_options fields -> (rgbl float32[height, width, 4], box float32[height,
    width, 6] {lo.rgb, hi.rgb} of every pixel, or None with box=False)."""
    L = L or lib()
    o = history_options(L, **opts)
    co = clamp_options(L, **(clamp or {}))
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("rgb is height x width x 3 floats")
    h, w = c.shape[:2]
    cnt = np.ascontiguousarray(n, dtype=np.uint32)
    g = np.ascontiguousarray(records, dtype=FIRST_HIT_DTYPE)
    if cnt.size != w * h or g.size != w * h:
        raise ValueError("n and records are height x width")
    pc = pl = pg = None
    if prev_rgbl is not None:
        pc = np.ascontiguousarray(prev_cam, dtype=np.float32)
        pl = np.ascontiguousarray(prev_rgbl, dtype=np.float32)
        pg = np.ascontiguousarray(prev_records, dtype=FIRST_HIT_DTYPE)
        if pc.size != 12 or pl.size != 4 * w * h or pg.size != w * h:
            raise ValueError("prev_cam is 12 floats, prev_rgbl height x width x 4, prev_records height x width")
    out = np.zeros((h, w, 4), np.float32)
    out_box = np.zeros((h, w, 6), np.float32) if box else None
    rc = L.rt_clamp_run(w, h, C.byref(o), C.byref(co),
                        *(a.ctypes.data if a is not None else None for a in (pc, pl, pg)),
                        c.ctypes.data, cnt.ctypes.data, g.ctypes.data, out.ctypes.data,
                        out_box.ctypes.data if box else None, device)
    if rc != 0:
        raise RenderError(f"rt_clamp_run failed ({rc}): {L.rt_last_error().decode()}")
    return out, out_box


def move_run(rgb, n, records, prev_spheres, spheres, prev_cam=None, prev_rgbl=None, prev_records=None, clamp=None,
             box=True, device=-1, L=None, **opts):
    """rt_move_run: rt_clamp_run through the kernel that follows moved spheres.  The
    arrays, clamp, box and opts as clamp_run's; prev_spheres and spheres: float32[nspheres,
    4] {cx, cy, cz, r} as prev remembers them and as they are now (None or empty: no
    spheres) -> (rgbl, box) as clamp_run's."""
    L = L or lib()
    o = history_options(L, **opts)
    co = clamp_options(L, **(clamp or {}))
    c = np.ascontiguousarray(rgb, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3:
        raise ValueError("rgb is height x width x 3 floats")
    h, w = c.shape[:2]
    cnt = np.ascontiguousarray(n, dtype=np.uint32)
    g = np.ascontiguousarray(records, dtype=FIRST_HIT_DTYPE)
    if cnt.size != w * h or g.size != w * h:
        raise ValueError("n and records are height x width")
    pc = pl = pg = None
    if prev_rgbl is not None:
        pc = np.ascontiguousarray(prev_cam, dtype=np.float32)
        pl = np.ascontiguousarray(prev_rgbl, dtype=np.float32)
        pg = np.ascontiguousarray(prev_records, dtype=FIRST_HIT_DTYPE)
        if pc.size != 12 or pl.size != 4 * w * h or pg.size != w * h:
            raise ValueError("prev_cam is 12 floats, prev_rgbl height x width x 4, prev_records height x width")
    s0 = s1 = None
    nsph = 0
    if prev_spheres is not None and np.size(prev_spheres) or spheres is not None and np.size(spheres):
        if prev_spheres is None or spheres is None:
            raise ValueError("prev_spheres and spheres are nspheres x 4 floats each")
        s0 = np.ascontiguousarray(prev_spheres, dtype=np.float32)
        s1 = np.ascontiguousarray(spheres, dtype=np.float32)
        if s0.size != s1.size or s0.size % 4:
            raise ValueError("prev_spheres and spheres are nspheres x 4 floats each")
        nsph = s0.size // 4
    out = np.zeros((h, w, 4), np.float32)
    out_box = np.zeros((h, w, 6), np.float32) if box else None
    rc = L.rt_move_run(w, h, C.byref(o), C.byref(co),
                       *(a.ctypes.data if a is not None else None for a in (pc, pl, pg)),
                       c.ctypes.data, cnt.ctypes.data, g.ctypes.data, out.ctypes.data,
                       out_box.ctypes.data if box else None,
                       *(a.ctypes.data if a is not None else None for a in (s0, s1)), nsph, device)
    if rc != 0:
        raise RenderError(f"rt_move_run failed ({rc}): {L.rt_last_error().decode()}")
    return out, out_box


class Filter:
    """rt_filter_*: the edge-aware filter for width x height images."""

    def __init__(self, width, height, device=-1, lib_path=None):
        self._L = lib(lib_path)
        self.width, self.height = width, height
        self._f = self._L.rt_filter_create(width, height, device)
        if not self._f:
            raise RenderError(f"rt_filter_create failed: {self._L.rt_last_error().decode()}")

    def close(self):
        if getattr(self, "_f", None):
            self._L.rt_filter_free(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, rgb, records, want_rgb=True, want_rgba=True, **opts):
        """rt_filter_run: rgb float32[height, width, 3] and records FIRST_HIT_DTYPE[height,
        width] -> (rgb float32[height, width, 3], rgba uint8[height, width, 4]); an output
        not wanted is None."""
        o = filter_options(self._L, **opts)
        c = np.ascontiguousarray(rgb, dtype=np.float32)
        g = np.ascontiguousarray(records, dtype=FIRST_HIT_DTYPE)
        if c.size != 3 * self.width * self.height or g.size != self.width * self.height:
            raise ValueError("rgb is height x width x 3 floats, records height x width")
        out = np.zeros((self.height, self.width, 3), np.float32) if want_rgb else None
        px = np.zeros((self.height, self.width, 4), np.uint8) if want_rgba else None
        rc = self._L.rt_filter_run(self._f, C.byref(o), c.ctypes.data, g.ctypes.data,
                                   out.ctypes.data if want_rgb else None, px.ctypes.data if want_rgba else None)
        if rc != 0:
            raise RenderError(f"rt_filter_run failed ({rc}): {self._L.rt_last_error().decode()}")
        return out, px

    def run_device(self, rgb_ptr: int, records_ptr: int, out_rgb_ptr: int = 0, out_rgba_ptr: int = 0,
                   stream_ptr: int = 0, **opts):
        """rt_filter_run_device: device buffers, only enqueued on the stream (0: the
        filter's own); an output pointer of 0 is not written."""
        o = filter_options(self._L, **opts)
        rc = self._L.rt_filter_run_device(self._f, C.byref(o), C.c_void_p(rgb_ptr or None),
                                          C.c_void_p(records_ptr or None), C.c_void_p(out_rgb_ptr or None),
                                          C.c_void_p(out_rgba_ptr or None), C.c_void_p(stream_ptr or None))
        if rc != 0:
            raise RenderError(f"rt_filter_run_device failed ({rc}): {self._L.rt_last_error().decode()}")


def write_ppm(rgba: np.ndarray, path: str):
    h, w = rgba.shape[:2]
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    fb = CFramebuffer(w, h, a.ctypes.data_as(C.POINTER(ColorU8)))
    if lib().rt_write_ppm(C.byref(fb), path.encode()) != 0:
        raise OSError(f"cannot write {path}")
