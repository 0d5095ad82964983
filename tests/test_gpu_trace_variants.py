"""Which trace-kernel instance a frame runs and the launch sized for it
(render.h TraceVariant: every launch resolves its instance once, through
resolve_trace_variant, and launch_trace and the runtime's occupancy store
look it up by that).  Per case one counted frame: its sphere search, LDS
bytes, workgroup size and workgroup count equal the constants below, taken
from a run of the same calls on the library of the commit before the instance
table, on the same MI355X (256 CUs); the frame equals the brute-force frame of
the same world bit for bit.  The cases with a pass add one accumulation or
adaptive pass of the frame's samples (stride 16, 16 samples, stats) and assert
the same figures of it; every case also asserts which walk the lean frame, the
counted frame and the pass ran (World.leaf_defer(), World.trace_plain()).  These
constants are from the library of the commit before the one launcher.

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

# case: (scene, environment, accel, pass: None, "accum" or "adapt")
CASES = {
    "rtow": ("rtow", {}, R.ACCEL_AUTO, None),
    "rtow box records": ("rtow", {"RT_AMD_CORNER": "0"}, R.ACCEL_AUTO, None),
    "rtow global tree": ("rtow", {"RT_AMD_LDS": "0"}, R.ACCEL_AUTO, None),
    "rtow brute": ("rtow", {}, R.ACCEL_BRUTE, None),
    "rtow sliced": ("rtow", {"RT_AMD_STEP": "1"}, R.ACCEL_AUTO, None),
    "soup": ("soup", {}, R.ACCEL_AUTO, None),
    "soup binary walk": ("soup", {"RT_AMD_TRI_WIDE": "0"}, R.ACCEL_AUTO, None),
    "soup brute": ("soup", {}, R.ACCEL_BRUTE, None),
    "small soup": ("small soup", {}, R.ACCEL_AUTO, None),
    "rtow immediate leaves": ("rtow", {"RT_AMD_LEAF_DEFER": "0"}, R.ACCEL_AUTO, None),
    "rtow generic instance": ("rtow", {"RT_AMD_PLAIN": "0"}, R.ACCEL_AUTO, None),
    "rtow accumulation pass": ("rtow", {}, R.ACCEL_AUTO, "accum"),
    "soup accumulation pass": ("soup", {}, R.ACCEL_AUTO, "accum"),
    "rtow adaptive pass": ("rtow", {}, R.ACCEL_AUTO, "adapt"),
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
    "rtow immediate leaves": (3, 80756, 1024, 512, 2, 0),
    "rtow generic instance": (3, 80756, 1024, 512, 2, 0),
    "rtow accumulation pass": (3, 80756, 1024, 512, 2, 0),
    "soup accumulation pass": (2, 5376, 512, 768, 2, 1),
    "rtow adaptive pass": (3, 80756, 1024, 512, 2, 0),
}
# the pass's own figures (the same keys)
PARENT_PASS = {
    "rtow accumulation pass": (3, 80756, 1024, 512, 2, 0),
    "soup accumulation pass": (2, 5376, 512, 768, 2, 1),
    "rtow adaptive pass": (3, 80756, 1024, 512, 2, 0),
}
# (leaf_defer, trace_plain) after the lean frame, after the counted frame, after the pass
PARENT_WALKS = {
    "rtow": ((2, 1), (0, 0), None),
    "rtow box records": ((0, 0), (0, 0), None),
    "rtow global tree": ((0, 0), (0, 0), None),
    "rtow brute": ((0, 0), (0, 0), None),
    "rtow sliced": ((0, 0), (0, 0), None),
    "soup": ((0, 0), (0, 0), None),
    "soup binary walk": ((0, 0), (0, 0), None),
    "soup brute": ((0, 0), (0, 0), None),
    "small soup": ((0, 0), (0, 0), None),
    "rtow immediate leaves": ((0, 0), (0, 0), None),
    "rtow generic instance": ((2, 0), (0, 0), None),
    "rtow accumulation pass": ((2, 1), (0, 0), (0, 0)),
    "soup accumulation pass": ((0, 0), (0, 0), (0, 0)),
    "rtow adaptive pass": ((2, 1), (0, 0), (0, 0)),
}

_brute_frames = {}


def _brute_frame(scene):
    if scene not in _brute_frames:
        out, st = R.World(SCENES[scene]()).render(W, H, SPP, DEPTH, accel=R.ACCEL_BRUTE)
        assert st["accel"] == R.ACCEL_BRUTE and st["sphere_tree"] == 0 and st["tri_bvh"] == 0
        out.setflags(write=False)
        _brute_frames[scene] = out
    return _brute_frames[scene]


GEOMETRY_KEYS = ("sphere_tree", "sphere_tree_lds_bytes", "launch_block_threads", "launch_blocks", "accel", "tri_bvh")


def _walk(world):
    return (world.leaf_defer(), world.trace_plain())


@pytest.mark.parametrize("case", list(CASES))
def test_instance_and_launch_geometry(monkeypatch, case):
    scene, env, accel, pass_kind = CASES[case]
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # (read at device setup: a fresh World per case)
    world = R.World(SCENES[scene]())
    out, st = world.render(W, H, SPP, DEPTH, accel=accel)
    counted_walk = _walk(world)
    lean, _ = world.render(W, H, SPP, DEPTH, accel=accel, stats=False)
    lean_walk = _walk(world)
    got = tuple(st[k] for k in GEOMETRY_KEYS)
    pass_out, pass_got, pass_walk = None, None, None
    if pass_kind:
        acc = world.accumulator(W, H, SPP, depth=DEPTH, accel=accel)
        if pass_kind == "adapt":
            acc.set_adaptive()
        pass_out, pst = acc.add(SPP, stats=True)
        pass_walk = _walk(world)
        pass_got = tuple(pst[k] for k in GEOMETRY_KEYS)
        acc.close()
    walks = (lean_walk, counted_walk, pass_walk)
    print(f"GEOMETRY {case!r}: {got},")
    print(f"PASS {case!r}: {pass_got},")
    print(f"WALKS {case!r}: {walks},")
    jobs_per_block = st["launch_block_threads"] // 64 * 256
    assert st["launch_blocks"] < -(-W * H * SPP // jobs_per_block), "clamped by the jobs, not the occupancy"
    assert got == PARENT.get(case), (case, got, PARENT.get(case))
    assert pass_got == PARENT_PASS.get(case), (case, pass_got, PARENT_PASS.get(case))
    assert walks == PARENT_WALKS.get(case), (case, walks, PARENT_WALKS.get(case))
    assert_bits_equal(lean, out, f"{case}: lean vs counting frame")
    assert_bits_equal(out, _brute_frame(scene), f"{case}: frame vs brute force")
    if pass_kind:
        # (the pass's samples are the frame's: stride = samples = SPP)
        assert_bits_equal(pass_out, out, f"{case}: the pass's frame vs the frame")


def test_serial_frame_against_the_oracle():
    """The SERIAL kind's instances and occupancy figures (its launch geometry is
    not in the stats: the frame and the ray count are the check)."""
    src = scene_text("c_raytracer_world.txt")
    w, h, spp, depth = 64, 48, 4, 8
    img, ost, _ = O.Scene(src).render(w, h, spp, depth, mode=O.RNG_SERIAL)
    out, st = R.World(src).render(w, h, spp, depth, mode=R.RNG_SERIAL)
    assert np.array_equal(out, img) and st["rays"] == ost["rays"]
