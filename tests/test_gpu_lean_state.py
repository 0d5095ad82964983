"""Where the frame kernels derive and keep their per-lane state (trace_body.h
trace_body): the sphere walk's reciprocals, octant and entry node are derived
at the walk (sphere-only, unsliced kernels), a leaf's second sphere is read
with its first (LDS trees), the scattered and the new primary directions share
the loop's one normalisation, and the plane-lane resolve converts each plane's
sum on its own lane.  None of it changes a sample: every comparison is on raw
bits against the brute-force kernel (accel=R.ACCEL_BRUTE), and the BVH counters
equal the constants below, taken from a run of the same calls on the library
of the commit before the change (so the same nodes and spheres are still
tested)."""
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from conftest import scene_text
from test_gpu_corner_tree import TREE_BOX, TREE_CORNER, TREE_GLOBAL, _brute, _random_scene
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order, render_kept

pytestmark = pytest.mark.gpu

# (rays, bvh_node_tests, bvh_sphere_tests) of the counting frame, per call
PARENT = {
    "rtow 64x36x4 d8": (15383, 141578, 17252),
    "rtow 64x36x4 d1": (9216, 44838, 7759),
    "rtow 64x36x4 d0": (0, 0, 0),
    "rtow moved 80x60x4 d8": (39172, 584832, 73653),
    "axis cluster 1x5x2": (10, 100, 0),
    "axis cluster 5x1x2": (10, 100, 0),
    "axis cluster 1x1x4": (4, 40, 0),
    "axis cluster 33x33x2": (4298, 75612, 12472),
    "500 spheres 96x64x8": (71974, 493428, 54640),
    "500 spheres 96x64x8 global": (71974, 509058, 54640),
    "random seed 1 96x64x8": (87203, 1141712, 129875),
    "random seed 2 96x64x8": (163987, 3280312, 494890),
    "random seed 5 96x64x8": (303719, 11631524, 1676387),
    "random seed 1 emissive 96x64x8": (82017, 1028750, 118510),
    "soup 48x27x2": (3245, 26878, 3553),
    "bright 24x10x4": (2355, 44758, 6606),
    "bright 24x10x8": (4462, 84834, 12331),
    "bright 24x10x64": (36393, 687846, 100190),
    "bright 12x5x256": (34542, 647006, 90091),
    "bright 24x10x3": (1754, 33850, 5050),
    "bright 24x10x5": (2916, 55764, 8363),
    "bright 11x3x8": (530, 9688, 1305),
    "bright 6x3x8": (297, 5014, 666),
    "bright 9x3x8": (464, 8492, 1126),
    "bright 4x3x8": (175, 2732, 329),
    "bright 7x3x8": (368, 6592, 850),
    "bright 10x3x8": (488, 8648, 1045),
    "bright 5x3x8": (218, 3564, 472),
    "bright 24x10x4 d0": (0, 0, 0),
}


def _counters(key, st):
    got = (st["rays"], st["bvh_node_tests"], st["bvh_sphere_tests"])
    print(f"COUNTERS {key!r}: {got},")
    assert got == PARENT.get(key), (key, got, PARENT.get(key))


def _check(world, key, w, h, spp, depth, tree=None, ref=None):
    """Lean, counting and kept-sample frames against brute force, bit for bit,
    every sample included; the counters against the parent's."""
    ref = ref or _brute(world, w, h, spp, depth)
    out, st = render_kept(world, w, h, spp, depth)
    if tree is not None:
        assert st["sphere_tree"] in tree, st["sphere_tree"]
    assert_bits_equal(out, ref[0], f"{key}: frames vs brute force")
    assert_bits_equal(world.read_samples(w * h * spp), ref[2], f"{key}: samples vs brute force")
    assert st["rays"] == ref[1]["rays"]
    _counters(key, st)
    return ref


# ---- walk-start state ------------------------------------------------------

def test_rtow_walk_gate_settings(monkeypatch):
    """RT_AMD_WALK_MIN 1: a lane walks in the iteration that set it up; 32 and
    the default: after waiting for other lanes, its ray unchanged meanwhile."""
    world = R.World(S.rtow())
    w, h, spp, depth = 64, 36, 4, 8
    ref = _check(world, "rtow 64x36x4 d8", w, h, spp, depth, tree=(TREE_CORNER,))
    for wm in ("1", "32"):
        monkeypatch.setenv("RT_AMD_WALK_MIN", wm)
        _check(world, "rtow 64x36x4 d8", w, h, spp, depth, tree=(TREE_CORNER,), ref=ref)
    monkeypatch.delenv("RT_AMD_WALK_MIN")
    monkeypatch.setenv("RT_AMD_CORNER", "0")
    box = R.World(S.rtow())
    for wm in (None, "1", "32"):
        if wm:
            monkeypatch.setenv("RT_AMD_WALK_MIN", wm)
        _check(box, "rtow 64x36x4 d8", w, h, spp, depth, tree=(TREE_BOX,), ref=ref)


@pytest.mark.parametrize("corner", ["1", "0"])
def test_rtow_lists_and_walks_share_bounce_0(monkeypatch, corner):
    monkeypatch.setenv("RT_AMD_CORNER", corner)
    world = R.World(S.rtow())
    world.move_camera(0.5, -1.5, -9.0)
    _check(world, "rtow moved 80x60x4 d8", 80, 60, 4, 8, tree=(TREE_CORNER if corner == "1" else TREE_BOX,))


@pytest.mark.parametrize("corner", ["1", "0"])
@pytest.mark.parametrize("depth", [1, 0])
def test_rtow_shallow_depths(monkeypatch, corner, depth):
    monkeypatch.setenv("RT_AMD_CORNER", corner)
    world = R.World(S.rtow())
    ref = _check(world, f"rtow 64x36x4 d{depth}", 64, 36, 4, depth)
    if depth == 0:
        assert not ref[0][..., :3].any()  # every sample (0, 0, 0)


@pytest.mark.parametrize("corner", ["1", "0"])
@pytest.mark.parametrize("w,h,spp", [(1, 5, 2), (5, 1, 2), (1, 1, 4), (33, 33, 2)])
def test_axis_aligned_camera_zero_and_tiny_direction_components(monkeypatch, corner, w, h, spp):
    """The camera looks straight down -z at the cluster: the central rays of
    the odd-sized frame have tiny x and y components, the frames of width or
    height 1 divide by zero (infinite and NaN directions): the reciprocal
    clamp and the octant's sign rule at their new place."""
    monkeypatch.setenv("RT_AMD_CORNER", corner)
    world = R.World(_random_scene(seed=7, n=300, spread=2.0, radius=0.4, big=False))
    _check(world, f"axis cluster {w}x{h}x{spp}", w, h, spp, 8,
           tree=(TREE_CORNER if corner == "1" else TREE_BOX,))


def test_tree_in_global_memory(monkeypatch):
    src = _random_scene(seed=3, n=500, spread=20.0, radius=0.05)
    w, h, spp = 96, 64, 8
    world = R.World(src)
    ref = _check(world, "500 spheres 96x64x8", w, h, spp, 8, tree=(TREE_GLOBAL, TREE_BOX))
    # (the walk over global memory tests the root too: one node test more per walk)
    monkeypatch.setenv("RT_AMD_LDS", "0")
    _check(world, "500 spheres 96x64x8 global", w, h, spp, 8, tree=(TREE_GLOBAL,), ref=ref)


# ---- scatter directions and the shared normalisation -----------------------

@pytest.mark.parametrize("case", [
    dict(seed=1, n=400, spread=6.0, radius=0.3),
    dict(seed=2, n=300, spread=3.0, radius=0.6, dup=40),
    dict(seed=5, n=250, spread=2.0, radius=0.5, big=False, cam=(0.0, 0.0, -4.0)),
])
def test_four_material_scenes(case):
    """Diffuse, fuzzy and mirror metal and dielectric scatters all hand their
    direction to the loop's shared normalisation."""
    world = R.World(_random_scene(**case))
    _check(world, f"random seed {case['seed']} 96x64x8", 96, 64, 8, 8, tree=(TREE_CORNER,))


def test_emissive_spheres_end_paths():
    world = R.World(_random_scene(seed=1, n=400, spread=6.0, radius=0.3))
    for i in range(1, world.num_spheres, 3):
        world.set_material(i, 3, (0.9, 0.7, 0.4))
    _check(world, "random seed 1 emissive 96x64x8", 96, 64, 8, 8)


def test_replay_serial_frame_against_the_oracle():
    src = scene_text("world.txt")
    w, h, spp, depth = 33, 17, 3, 8
    img, st, states, smp = O.Scene(src).render(w, h, spp, depth, mode=O.RNG_SERIAL, record_states=True,
                                               record_samples=True)
    world = R.World(src)
    out, gst = render_kept(world, w, h, spp, depth, mode=R.RNG_REPLAY, replay=states)
    assert_bits_equal(out, img, "REPLAY frame vs the oracle's SERIAL frame")
    assert_bits_equal(world.read_samples(w * h * spp)[:, :3],
                      oracle_samples_to_gpu_order(smp, w, h, spp)[:, :3], "samples")
    assert gst["rays"] == st["rays"]
    out, gst = world.render(w, h, spp, depth, mode=R.RNG_SERIAL)
    assert_bits_equal(out, img, "SERIAL frame vs the oracle's")
    assert gst["rays"] == st["rays"]


def test_mesh_scene():
    world = R.World(S.triangle_soup(41, 400, spheres=40))
    w, h, spp = 48, 27, 2
    ref, rst, ref_s = _brute(world, w, h, spp)
    out, st = render_kept(world, w, h, spp, 8)
    assert st["tri_bvh"] == 1
    assert_bits_equal(out, ref, "mesh frames vs brute force")
    assert_bits_equal(world.read_samples(w * h * spp), ref_s, "mesh samples vs brute force")
    assert st["rays"] == rst["rays"]
    _counters("soup 48x27x2", st)


# ---- resolve epilogue ------------------------------------------------------

def _bright_world():
    """Every third sphere an emitter far above 1: channels saturate at 255."""
    world = R.World(_random_scene(seed=2, n=300, spread=3.0, radius=0.6))
    for i in range(1, world.num_spheres, 3):
        world.set_material(i, 3, (40.0, 3.0, 0.6))
    return world


@pytest.mark.parametrize("spp", [4, 8, 64, 256, 3, 5])
def test_resolve_paths_by_spp(spp):
    """spp % 4 == 0: one lane per (pixel, plane), each converting its own sum;
    3 and 5: one lane per pixel.  Lean, counting and kept-sample frames."""
    world = _bright_world()
    w, h = (24, 10) if spp <= 64 else (12, 5)
    ref = _check(world, f"bright {w}x{h}x{spp}", w, h, spp, 8)
    assert (ref[0][..., 0] == 255).any() and (ref[0][..., :3] < 255).any()


@pytest.mark.parametrize("w", [11, 6, 9, 4, 7, 10, 5])
def test_resolve_last_chunk_of_1_to_7_pixels(monkeypatch, w):
    """One partition of 8-pixel chunks over 3 * w pixels: the last chunk holds
    (3 * w) % 8 = 1 .. 7 pixels (fewer pixel lanes than the others)."""
    spp = 8
    assert (3 * w) % 8 == [11, 6, 9, 4, 7, 10, 5].index(w) + 1
    monkeypatch.setenv("RT_AMD_PARTS", "1")
    monkeypatch.setenv("RT_AMD_CHUNK", str(8 * spp))
    _check(_bright_world(), f"bright {w}x3x8", w, 3, spp, 8)


@pytest.mark.parametrize("pix", ["1", "3", "64"])
def test_resolve_chunk_knob(monkeypatch, pix):
    monkeypatch.setenv("RT_AMD_RESOLVE_PIX", pix)
    _check(_bright_world(), "bright 24x10x4", 24, 10, 4, 8)


def test_resolve_all_zero_frame():
    world = _bright_world()
    ref = _check(world, "bright 24x10x4 d0", 24, 10, 4, 0)
    assert not ref[0][..., :3].any() and (ref[0][..., 3] == 255).all()
