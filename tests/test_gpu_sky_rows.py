"""Sky rows: the rows at the top and the bottom of the image
none of whose primary rays can hit a sphere are rendered by sky.hip's
sky_rows_kernel, the trace kernel gets the rows between.  Nothing a sample
computes changes, so every comparison here is on the raw RGBA8 bytes of the
lean frame (stats=False) against three references -- the brute-force kernel,
the counting frame (neither takes the path) and the lean frame of a fresh World
under RT_AMD_SKY_ROWS=0.  World.sky_rows() (rt_sky_rows) says how many rows the
last frame launch gave the sky kernel: a frame meant for the path renders once,
renders again and asserts the count on the second frame, a frame that must not
take it asserts 0, so no case can test the other path unnoticed.  A build
without the kernel fails here, it does not skip."""
import numpy as np
import pytest

import camera_cases as CC
import raytracer_amd as R
import scene_values as V
import scenes as S
from test_gpu_corner_tree import _brute, _random_scene
from test_gpu_parity import assert_bits_equal
from test_sky_rows_host import ground_scene, horizon_rows

pytestmark = pytest.mark.gpu


def _expect(n, h, rows, what):
    print(f"{what}: sky_rows = {n} of {h}")
    if rows == "some":
        assert 1 <= n < h, (what, n)
    elif rows == "all":
        assert n == h, (what, n)
    elif rows == "none":
        assert n == 0, (what, n)
    elif isinstance(rows, int):
        assert n == rows, (what, n, rows)


def _check(monkeypatch, make_world, w, h, spp, depth, rows, what=""):
    """The lean frames of make_world() against brute force, the counting frame
    and the RT_AMD_SKY_ROWS=0 lean frame of a fresh world; rows: what
    sky_rows() must say after the second lean frame ("some", "all", "none",
    "any" or the count).  Returns that count."""
    world = make_world()
    ref = _brute(world, w, h, spp, depth)
    first, st = world.render(w, h, spp, depth, stats=False)
    assert st is None
    lean, _ = world.render(w, h, spp, depth, stats=False)  # (the device was synchronised in between)
    n = world.sky_rows()
    _expect(n, h, rows, what)
    assert_bits_equal(first, ref[0], f"{what}: first lean frame vs brute force")
    assert_bits_equal(lean, ref[0], f"{what}: lean frame vs brute force")
    out, st = world.render(w, h, spp, depth)
    assert world.sky_rows() == 0  # (a counted frame traces every row)
    assert_bits_equal(lean, out, f"{what}: lean frame vs counting frame")
    assert st["rays"] == ref[1]["rays"]
    monkeypatch.setenv("RT_AMD_SKY_ROWS", "0")
    off_world = make_world()
    off, _ = off_world.render(w, h, spp, depth, stats=False)
    assert off_world.sky_rows() == 0
    monkeypatch.delenv("RT_AMD_SKY_ROWS")
    assert_bits_equal(lean, off, f"{what}: sky rows vs every row traced")
    return n


@pytest.mark.parametrize("depth", [8, 1])
@pytest.mark.parametrize("spp", [1, 4, 6, 64])
@pytest.mark.parametrize("w,h", [(64, 36), (93, 41)])
def test_rtow_sky_rows_are_found(monkeypatch, w, h, spp, depth):
    _check(monkeypatch, lambda: R.World(S.rtow()), w, h, spp, depth, "some", f"rtow {w}x{h}x{spp} d{depth}")


@pytest.mark.parametrize("radius,height", [(1000.0, 0.01), (1000.0, 1.0), (1000.0, 100.0),
                                           (100000.0, 0.01), (100000.0, 1.0), (100000.0, 100.0)])
def test_horizon_grazing(monkeypatch, radius, height):
    """The last sky row and the first traced row lie at the ground's horizon
    (the camera 0.01 above the 1e5 ground is within the f32 error bound of it:
    no rows there, tests/test_sky_rows_host.py)."""
    w, h = 96, 54
    src = ground_scene(radius, height)
    near = 2 * radius * height + height ** 2 <= 2.0 ** -18 * (radius + height) ** 2
    n = _check(monkeypatch, lambda: R.World(src), w, h, 4, 8, "none" if near else "some",
               f"ground {radius:g} camera +{height:g}")
    if not near:
        exact = horizon_rows(radius, height, h)
        assert exact - 3 <= n <= exact, (n, exact)


def _rtow_with(camera):
    def make():
        world = R.World(S.rtow())
        camera(world)
        return world
    return make


@pytest.mark.parametrize("name,rows", [("up", "all"), ("down", "none"), ("roll", "any"), ("fov", "some"),
                                       ("far", "none")])
def test_cameras(monkeypatch, name, rows):
    cams = {
        # up and away from the field (which lies behind the camera plane): no trace launch at all
        "up": lambda wd: wd.look_at((0, 2, 13), (0, 3, 14), CC.Y, float(CC.radians(50)), 1.5),
        "down": lambda wd: wd.look_at((0, 6, 0.5), (0, 0, 0), CC.Y, float(CC.radians(50)), 1.5),
        "roll": lambda wd: wd.look_at((0, 2, 13), (0, 2, 0), (1, 1, 0), float(CC.radians(60)), 1.5),
        "fov": lambda wd: wd.vertical_fov((0, 2, 13), float(CC.radians(50)), 1.5),
        # a camera coordinate of 1000: no primary lists (bvh.cpp sphere_list_params), so no sky rows
        "far": lambda wd: wd.set_camera(CC.new_at((0, 2, 1000), 1.5)),
    }
    _check(monkeypatch, _rtow_with(cams[name]), 64, 36, 4, 8, rows, f"camera {name}")


def test_whole_frame_of_sky_launches_no_trace_kernel():
    world = R.World(S.rtow())
    world.look_at((0, 2, 13), (0, 3, 14), CC.Y, float(CC.radians(50)), 1.5)
    world.render(64, 36, 4, 8, stats=False)  # (the rows are known once this frame is enqueued)
    world.trace_launched(clear=True)
    world.render(64, 36, 4, 8, stats=False)
    assert world.sky_rows() == 36
    assert not world.trace_launched().any()


# ---- frames that must not take the path: every row traced, the same bits
def test_depth_zero_is_black_not_sky():
    world = R.World(S.rtow())
    lean, _ = world.render(64, 36, 4, 0, stats=False)
    assert world.sky_rows() == 0
    assert not lean[..., :3].any()
    assert_bits_equal(lean, _brute(world, 64, 36, 4, 0)[0], "depth 0")


def test_replay_frames_trace_every_row():
    w, h, spp = 64, 36, 4
    states = np.random.default_rng(11).integers(1, 2**32, w * h * spp, dtype=np.uint64).astype(np.uint32)
    world = R.World(S.rtow())
    ref, _ = world.render(w, h, spp, 8, mode=R.RNG_REPLAY, replay=states, accel=R.ACCEL_BRUTE)
    world.render(w, h, spp, 8, stats=False)
    world.render(w, h, spp, 8, stats=False)
    assert world.sky_rows() > 0
    lean, _ = world.render(w, h, spp, 8, mode=R.RNG_REPLAY, replay=states, stats=False)
    assert world.sky_rows() == 0
    assert_bits_equal(lean, ref, "REPLAY lean frame vs brute force")


def test_rank_tiles_trace_every_row():
    w, h, spp = 64, 36, 4
    world = R.World(S.rtow())
    for rank in range(2):
        ref, _ = world.render(w, h, spp, 8, rank=rank, nranks=2, row_block=4, accel=R.ACCEL_BRUTE)
        tile, _ = world.render(w, h, spp, 8, rank=rank, nranks=2, row_block=4, stats=False)
        assert world.sky_rows() == 0
        assert_bits_equal(tile, ref, f"tile of rank {rank}")


def test_triangle_scenes_trace_every_row():
    world = R.World(S.triangle_soup(7, 300, spheres=40, grid=6))
    ref, _ = world.render(48, 32, 4, 8, accel=R.ACCEL_BRUTE)
    lean, _ = world.render(48, 32, 4, 8, stats=False)
    lean, _ = world.render(48, 32, 4, 8, stats=False)
    assert world.sky_rows() == 0
    assert_bits_equal(lean, ref, "triangle soup")


def test_non_finite_sphere_traces_every_row(monkeypatch):
    w, h, spp, depth = V.FRAME
    case = V.case("nonfinite")
    _check(monkeypatch, lambda: R.World(case.src), w, h, spp, depth, "none", "nonfinite")


def test_camera_move_rows_follow_the_camera():
    """Frame, move, frame, frame: each equals brute force of its camera, and the
    rows are those of the camera the frame was rendered with."""
    w, h, spp = 64, 36, 4
    world = R.World(S.rtow())
    world.render(w, h, spp, 8, stats=False)
    a, _ = world.render(w, h, spp, 8, stats=False)
    rows_a = world.sky_rows()
    world.move_camera(0.0, 4.0, 0.0)  # higher: the horizon and the field sink in the image
    b, _ = world.render(w, h, spp, 8, stats=False)
    rows_b1 = world.sky_rows()
    b2, _ = world.render(w, h, spp, 8, stats=False)
    rows_b = world.sky_rows()
    print(f"rows {rows_a} -> {rows_b1}, {rows_b}")
    assert rows_a >= 1 and rows_b > rows_a and rows_b1 in (0, rows_b)  # (not known yet, or the new camera's)
    assert_bits_equal(b, _brute(world, w, h, spp)[0], "first frame after the move")
    assert_bits_equal(b2, b, "second frame after the move")
    world.move_camera(0.0, -4.0, 0.0)
    a2, _ = world.render(w, h, spp, 8, stats=False)
    assert world.sky_rows() in (0, rows_a)
    assert_bits_equal(a2, a, "back at the first camera")
    assert_bits_equal(a, _brute(world, w, h, spp)[0], "first camera vs brute force")


def test_big_sphere_above_the_camera_vetoes_rows(monkeypatch):
    """A big sphere over the field covers the top rows: in no list, so the
    lists alone would call them sky."""
    src = S.rtow() + "sphere center 0.0 60.0 -20.0 radius 40.0 material S0;\n"
    _check(monkeypatch, lambda: R.World(src), 64, 36, 4, 8, "none", "big sphere above")


def test_ground_field_of_the_other_tests(monkeypatch):
    """The random field with its r = 999 ground sphere one unit under the camera."""
    src = _random_scene(seed=1, n=60, spread=3.0, radius=0.4)
    _check(monkeypatch, lambda: R.World(src), 48, 32, 4, 8, "any", "random field")
