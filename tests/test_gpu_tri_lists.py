"""The primary triangle strip lists built on the device (tri_lists.hip,
DESIGN.md 5.3a) against the host build and the oracle.

RT_AMD_PTL_CHECK=1 is set throughout: a frame fails unless the device build's
offsets, items and trailing `always` records equal bvh.cpp
build_primary_tri_lists byte for byte (that build is checked ray by ray by
tests/test_camera_lists_host.py, which also asserts what the spliced scene and
the camera behind the soup put on the lists).  Per case the frame and every
sample equal the oracle's, rt_primary_tri_lists reports 2, and the same frame
with RT_AMD_GPU_TRI_LISTS=0 reports 1 and holds the same bits."""
import numpy as np
import pytest

import camera_cases as CC
import oracle as O
import raytracer_amd as R
import scene_values as V
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order, render_kept
from test_gpu_scene_values import assert_samples_equal

pytestmark = pytest.mark.gpu

SPP, DEPTH = V.FRAME[2:]
CAMERAS = ["default"] + list(CC.SOUP)
# 50 x 30: the last strip of a row is partial; 9 x 2 and 8 x 2: one strip and a
# one-pixel second strip; 2 x 2: the smallest frame with lists
SIZES = [(48, 32), (50, 30), (9, 2), (8, 2), (2, 2)]
HOST, DEVICE = 1, 2


@pytest.fixture(autouse=True)
def _checked_lists(monkeypatch):
    monkeypatch.setenv("RT_AMD_PTL_CHECK", "1")
    monkeypatch.delenv("RT_AMD_GPU_TRI_LISTS", raising=False)


_MEMO = {}


def _pair(src_name):
    if src_name not in _MEMO:
        src = V.soup() if src_name == "soup" else CC.spliced_soup()
        world, ref = R.World(src), O.Scene(src)
        assert world.num_triangles == ref.num_triangles >= 300  # (>= 16: the tree and the lists run)
        _MEMO[src_name] = (world, ref, ref.camera().copy())
    return _MEMO[src_name]


def _set(world, default, name):
    if name == "default":
        world.set_camera(default)
    else:
        CC.apply(world, CC.SOUP, name)


def _check_frame(world, ref, w, h, what, where=DEVICE):
    """A frame at world's camera: equal to the oracle, its lists built `where`."""
    out, st = render_kept(world, w, h, SPP, DEPTH)
    assert world.primary_tri_lists() == where, (what, world.primary_tri_lists())
    assert st["tri_bvh"] == 1 and st["camera_tree"] == 1, (what, st["tri_bvh"], st["camera_tree"])
    assert st["primary_lists"] == (1 if where else 0), what
    ref.set_camera(world.camera())
    img, ost, _, smp = ref.render(w, h, SPP, DEPTH, mode=O.RNG_COUNTER, nthreads=8, record_samples=True)
    assert_bits_equal(out, img, f"{what}: frame vs the oracle")
    assert_samples_equal(world.read_samples(w * h * SPP), oracle_samples_to_gpu_order(smp, w, h, SPP),
                         f"{what}: samples vs the oracle")
    assert st["rays"] == ost["rays"], what
    return out, st


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", CAMERAS)
def test_device_lists_equal_the_host_build_and_the_oracle(monkeypatch, name, w, h):
    world, ref, default = _pair("soup")
    _set(world, default, name)
    what = f"soup/{name} {w}x{h}"
    out, st = _check_frame(world, ref, w, h, what)
    monkeypatch.setenv("RT_AMD_GPU_TRI_LISTS", "0")
    host, hst = world.render(w, h, SPP, DEPTH)
    assert world.primary_tri_lists() == HOST, what
    assert_bits_equal(host, out, f"{what}: host-built lists vs device-built lists")
    assert hst["rays"] == st["rays"] and hst["primary_lists"] == 1


def test_a_frame_too_narrow_for_lists_reports_none_and_renders():
    world, ref, default = _pair("soup")
    world.set_camera(default)
    w, h = 1, 5
    out, st = world.render(w, h, SPP, DEPTH)
    assert world.primary_tri_lists() == 0 and st["primary_lists"] == 0 and st["tri_bvh"] == 1
    ref.set_camera(default)
    img, ost, _ = ref.render(w, h, SPP, DEPTH, mode=O.RNG_COUNTER)
    assert_bits_equal(out, img, "soup 1x5: frame vs the oracle")
    assert st["rays"] == ost["rays"]


@pytest.mark.parametrize("name", ["default", "inside", "roll"])
def test_spanning_and_straddling_triangles(name):
    """A triangle on every strip's list and one across the camera plane (`always`)."""
    world, ref, default = _pair("spliced")
    _set(world, default, name)
    for (w, h) in [(48, 32), (50, 30)]:
        _check_frame(world, ref, w, h, f"spliced soup/{name} {w}x{h}")


def test_every_triangle_behind_the_camera():
    """All offsets are 0 and there is no `always` record: the lists exist and are empty."""
    world, ref, _ = _pair("soup")
    o, t, up, deg = CC.ALL_BEHIND
    world.look_at(o, t, up, float(CC.radians(deg)), CC.ASPECT)
    _check_frame(world, ref, 48, 32, "soup, every triangle behind the camera")


def test_a_turn_in_place_rebuilds_the_lists_not_the_records():
    world, ref, _ = _pair("soup")
    CC.apply(world, CC.SOUP, "side")
    before, _ = _check_frame(world, ref, 48, 32, "soup/side")
    builds = world.camera_record_builds()
    assert builds >= 1
    o, _, up, deg = CC.SOUP["side"]
    world.look_at(o, (0.5, -0.4, -4.0), up, float(CC.radians(deg)), CC.ASPECT)  # same origin
    after, _ = _check_frame(world, ref, 48, 32, "soup/side, turned in place")
    assert world.camera_record_builds() == builds
    assert not np.array_equal(before, after)
    world.translate_camera(0.0, 0.25, 0.0)  # (a move does rebuild them)
    _check_frame(world, ref, 48, 32, "soup/side, turned and moved")
    assert world.camera_record_builds() == builds + 1


def test_a_resize_rebuilds_the_lists():
    world, ref, _ = _pair("soup")
    CC.apply(world, CC.SOUP, "high")
    for (w, h) in [(48, 32), (50, 30), (48, 32), (24, 32)]:
        _check_frame(world, ref, w, h, f"soup/high resized to {w}x{h}")
