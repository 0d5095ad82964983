"""Which trace-kernel instance a frame runs and the launch sized for it
(render.h TraceVariant: launch_trace and the runtime's occupancy table both
go through trace_variant).  Per case one counted frame: its sphere search,
LDS bytes, workgroup size and workgroup count equal the constants below,
taken from a run of the same calls on the library of the commit before the
instance table, on the same MI355X (256 CUs); the frame equals the brute-force
frame of the same world bit for bit.

launch_blocks = min(workgroups per CU x CUs, ceil(jobs / (waves per workgroup
x 256))): every frame here has more jobs than the occupancy term covers
(asserted), so a figure looked up for another instance shows."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from conftest import scene_text
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 640, 360, 16, 8  # 3.7 M jobs

SCENES = {
    "rtow": S.rtow,
    "soup": lambda: S.triangle_soup(7, 300, spheres=40, grid=6),
    # 12 triangles: below the 16 a triangle tree is built for (bvh.cpp build_triangle_bvh)
    "small soup": lambda: S.triangle_soup(7, 12, spheres=40),
}

# case: (scene, environment, accel)
CASES = {
    "rtow": ("rtow", {}, R.ACCEL_AUTO),
    "rtow box records": ("rtow", {"RT_AMD_CORNER": "0"}, R.ACCEL_AUTO),
    "rtow global tree": ("rtow", {"RT_AMD_LDS": "0"}, R.ACCEL_AUTO),
    "rtow brute": ("rtow", {}, R.ACCEL_BRUTE),
    "rtow sliced": ("rtow", {"RT_AMD_STEP": "1"}, R.ACCEL_AUTO),
    "soup": ("soup", {}, R.ACCEL_AUTO),
    "soup binary walk": ("soup", {"RT_AMD_TRI_WIDE": "0"}, R.ACCEL_AUTO),
    "soup brute": ("soup", {}, R.ACCEL_BRUTE),
    "small soup": ("small soup", {}, R.ACCEL_AUTO),
}

# (sphere_tree, sphere_tree_lds_bytes, launch_block_threads, launch_blocks, accel, tri_bvh)
PARENT = {
    "rtow": (3, 80756, 1024, 512, 2, 0),
    "rtow box records": (2, 62788, 1024, 512, 2, 0),
    "rtow global tree": (1, 0, 256, 1792, 2, 0),
    "rtow brute": (0, 0, 256, 1792, 1, 0),
    "rtow sliced": (3, 80756, 1024, 512, 2, 0),
    "soup": (2, 5376, 512, 768, 2, 1),
    "soup binary walk": (2, 5376, 512, 768, 2, 1),
    "soup brute": (0, 0, 256, 1536, 1, 0),
    "small soup": (2, 5120, 512, 768, 2, 0),
}

_brute_frames = {}


def _brute_frame(scene):
    if scene not in _brute_frames:
        out, st = R.World(SCENES[scene]()).render(W, H, SPP, DEPTH, accel=R.ACCEL_BRUTE)
        assert st["accel"] == R.ACCEL_BRUTE and st["sphere_tree"] == 0 and st["tri_bvh"] == 0
        out.setflags(write=False)
        _brute_frames[scene] = out
    return _brute_frames[scene]


@pytest.mark.parametrize("case", list(CASES))
def test_instance_and_launch_geometry(monkeypatch, case):
    scene, env, accel = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read at device setup: a fresh World per case)
    world = R.World(SCENES[scene]())
    out, st = world.render(W, H, SPP, DEPTH, accel=accel)
    got = tuple(st[k] for k in ("sphere_tree", "sphere_tree_lds_bytes", "launch_block_threads", "launch_blocks",
                                "accel", "tri_bvh"))
    print(f"GEOMETRY {case!r}: {got},")
    jobs_per_block = st["launch_block_threads"] // 64 * 256
    assert st["launch_blocks"] < -(-W * H * SPP // jobs_per_block), "clamped by the jobs, not the occupancy"
    assert got == PARENT.get(case), (case, got, PARENT.get(case))
    lean, _ = world.render(W, H, SPP, DEPTH, accel=accel, stats=False)
    assert_bits_equal(lean, out, f"{case}: lean vs counting frame")
    assert_bits_equal(out, _brute_frame(scene), f"{case}: frame vs brute force")


def test_serial_frame_against_the_oracle():
    """The SERIAL kind's instances and occupancy figures (its launch geometry is
    not in the stats: the frame and the ray count are the check)."""
    src = scene_text("c_raytracer_world.txt")
    w, h, spp, depth = 64, 48, 4, 8
    img, ost, _ = O.Scene(src).render(w, h, spp, depth, mode=O.RNG_SERIAL)
    out, st = R.World(src).render(w, h, spp, depth, mode=R.RNG_SERIAL)
    assert np.array_equal(out, img) and st["rays"] == ost["rays"]
