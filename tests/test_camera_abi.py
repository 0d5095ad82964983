"""CPU tests of the camera C-ABI (rt_camera_*, include/raytracer_amd.h): the
reference crate's new_with_vertical_fov and new_look_at (camera.rs:34-69)
restated in numpy f32 (tests/camera_cases.py) give the library's 12 floats bit
for bit, the reference's two asserts come back as NULL with a message,
rt_camera_from_floats is rt_camera_get's inverse on bits, and
rt_camera_translate / move_camera_position match their restatements on an
oriented camera."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as CC
import raytracer_amd as R
from conftest import scene_text
from test_abi import declared_functions

CAMERA = ["rt_camera_free", "rt_camera_from_floats", "rt_camera_get", "rt_camera_new_look_at",
          "rt_camera_new_with_vertical_fov", "rt_camera_record_builds", "rt_camera_translate"]
ALL = [(tab, name) for tab in ("RTOW", "FIELD") for name in getattr(CC, tab)]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _floats(cam):
    out = np.zeros(12, np.float32)
    R.lib().rt_camera_get(cam, _fp(out))
    return out


def _look_at(o, t, up, vfov, aspect=CC.ASPECT):
    a = [np.array(v, np.float32) for v in (o, t, up)]
    return R.lib().rt_camera_new_look_at(_fp(a[0]), _fp(a[1]), _fp(a[2]), float(vfov), aspect)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_camera_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert sorted(n for n in names if n.startswith("rt_camera_")) == CAMERA
    assert "rt_primary_tri_lists" in names
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in CAMERA + ["rt_primary_tri_lists"] if not hasattr(lib, n)]
    assert set(CAMERA) <= set(R.EXPORTS)


@pytest.mark.parametrize("tab,name", ALL)
def test_look_at_matches_the_restatement(tab, name):
    o, t, up, deg = getattr(CC, tab)[name]
    want = CC.look_at(o, t, up, CC.radians(deg))
    assert want is not None
    cam = _look_at(o, t, up, CC.radians(deg))
    assert cam, R.last_error()
    got = _floats(cam)
    R.lib().rt_camera_free(cam)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    # far from the reference's assert (the smallest |v.y| is `down`'s 1 - w.y^2 =
    # 0.25 / 36.25 = 0.0069), and a regular camera map
    vh = np.float32(2) * CC.tanf(CC.radians(deg) / np.float32(2))
    assert abs(want[10]) / vh > 0.00689
    assert CC.det(want) != 0.0


@pytest.mark.parametrize("deg", [40, 100])
def test_vertical_fov_matches_the_restatement(deg):
    o = np.array([0.25, -0.5, 1.0], np.float32)
    cam = R.lib().rt_camera_new_with_vertical_fov(_fp(o), float(CC.radians(deg)), CC.ASPECT)
    assert cam
    got = _floats(cam)
    R.lib().rt_camera_free(cam)
    want = CC.with_vertical_fov(o, CC.radians(deg))
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    assert got[8] == 0 and got[9] == 0 and got[5] == o[2] - 1  # still looking down -z


def test_the_reference_asserts_return_null_with_a_message():
    assert CC.look_at((1, 2, 3), (1, 2, 3), CC.Y, CC.radians(60)) is None
    assert not _look_at((1, 2, 3), (1, 2, 3), CC.Y, CC.radians(60))
    assert "must differ" in R.last_error()
    # straight down with up = -z: v = w x (up x w) has no y component
    assert CC.look_at((0, 5, 0), (0, 0, 0), (0, 0, -1), CC.radians(60)) is None
    assert not _look_at((0, 5, 0), (0, 0, 0), (0, 0, -1), CC.radians(60))
    assert "y component" in R.last_error()
    # |v.y| > 1e-8 is false for NaN as well
    assert not _look_at((0, 5, 0), (0, 0, 0), (0, 0, 0), CC.radians(60))
    assert not _look_at((np.nan, 5, 0), (0, 0, 0), CC.Y, CC.radians(60))
    assert not R.lib().rt_camera_new_look_at(None, None, None, 1.0, 1.5)


def test_from_floats_inverts_get_on_bits():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2**32, size=12, dtype=np.uint64).astype(np.uint32)
    bits[0] = 0x7FC00001  # a quiet NaN with a payload
    bits[4] = 0xFFC12345  # a negative one
    bits[7] = 0x7F800000  # +inf
    bits[9] = 0x80000000  # -0.0
    bits[11] = 0x00000001  # a subnormal
    cam = R.lib().rt_camera_from_floats(_fp(bits.view(np.float32)))
    assert cam
    got = _floats(cam)
    R.lib().rt_camera_free(cam)
    assert np.array_equal(_bits(got), bits)
    assert not R.lib().rt_camera_from_floats(None)


def test_translate_and_move_on_an_oriented_camera():
    o, t, up, deg = CC.RTOW["roll"]
    want = CC.look_at(o, t, up, CC.radians(deg))
    d = (0.3, -1.25, 2.0)
    cam = R.lib().rt_camera_translate(_look_at(o, t, up, CC.radians(deg)), *d)
    got = _floats(cam)
    assert np.array_equal(_bits(got), _bits(CC.translated(want, *d)))
    assert np.array_equal(_bits(got[6:]), _bits(want[6:]))  # the orientation stays
    # move_camera_position is the reference's new_at(position + d, horizontal.x / vertical.y):
    # the orientation is gone, and the "aspect" is whatever those two components give
    cam = R.lib().move_camera_position(cam, *d)
    moved = _floats(cam)
    R.lib().rt_camera_free(cam)
    assert np.array_equal(_bits(moved), _bits(CC.moved(got, *d)))
    assert moved[7] == 0 and moved[8] == 0 and moved[9] == 0 and moved[10] == 2.0
    assert np.array_equal(moved[0:3], got[0:3] + np.array(d, np.float32))
    assert R.lib().rt_camera_translate(None, 1.0, 2.0, 3.0) is None


def test_free_null_is_harmless():
    R.lib().rt_camera_free(None)


def test_record_builds_and_tri_lists_diagnostics_without_a_frame():
    import scene_values as V
    assert R.World(scene_text("world.txt")).camera_record_builds() == 0  # no triangle tree
    soup = R.World(V.soup())
    assert soup.camera_record_builds() == 1  # load_world, for the scene's camera
    soup.look_at((1, 2, 3), (0, 0, -5))  # (a swap alone builds nothing: the next frame does)
    assert soup.camera_record_builds() == 1
    assert R.lib().rt_camera_record_builds(None) == -1 and "null" in R.last_error()
    assert R.lib().rt_primary_tri_lists(None, -1) == -1


def test_world_methods_swap_the_handles_camera():
    world = R.World(scene_text("world.txt"))
    o, t, up, deg = CC.FIELD["roll"]
    world.look_at(o, t, up, float(CC.radians(deg)), CC.ASPECT)
    want = CC.look_at(o, t, up, CC.radians(deg))
    assert np.array_equal(_bits(world.camera()), _bits(want))
    world.translate_camera(1.0, 0.5, -2.0)
    assert np.array_equal(_bits(world.camera()), _bits(CC.translated(want, 1.0, 0.5, -2.0)))
    # a second world (a tiles.py rank holds its own) is given the same camera
    other = R.World(scene_text("world.txt"))
    other.set_camera(world.camera())
    assert np.array_equal(_bits(other.camera()), _bits(world.camera()))
    world.vertical_fov((0, 0, 1), float(CC.radians(40)), 2.0)
    assert np.array_equal(_bits(world.camera()), _bits(CC.with_vertical_fov((0, 0, 1), CC.radians(40), 2.0)))
    with pytest.raises(ValueError, match="must differ"):
        world.look_at((1, 1, 1), (1, 1, 1))
    assert np.array_equal(_bits(world.camera()), _bits(CC.with_vertical_fov((0, 0, 1), CC.radians(40), 2.0)))
    with pytest.raises(ValueError):
        world.set_camera(np.zeros(11, np.float32))
