"""Every render path under oriented cameras (rt_camera_new_look_at, DESIGN.md
2), bit for bit.  Until these cameras every primary ray the library had traced
pointed down -z; here the RTOW field, the 60-sphere field and the triangle
soup are seen from the side, from behind, from above, rolled, through a 10
degree and a 120 degree lens and from inside the scene (tests/camera_cases.py).

The expectation is the oracle with the same 12 floats
(ref.set_camera(world.camera())): frame, every sample and ray counts on raw
bits.  RT_AMD_SPL_CHECK=1 and RT_AMD_PTL_CHECK=1 are set throughout, so every
device-built list is also compared with the host build (which
tests/test_camera_lists_host.py checks ray by ray).

PATHS records what each case ran with on an MI355X."""
import numpy as np
import pytest

import camera_cases as CC
import oracle as O
import raytracer_amd as R
import scene_values as V
import scenes as S
from test_gpu_accum import Expect, _run
from test_gpu_adapt import check, restate
from test_gpu_corner_tree import TREE_BOX, TREE_CORNER, TREE_GLOBAL
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order, render_kept
from test_gpu_scene_values import assert_samples_equal

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = V.FRAME
NJOBS = W * H * SPP
SCENES = {"rtow": (S.rtow, CC.RTOW), "field": (V.field, CC.FIELD), "soup": (V.soup, CC.SOUP)}
CASES = [(s, c) for s, (_, tab) in SCENES.items() for c in tab]

# (sphere_tree, primary_lists, tri_bvh, camera_tree) of each case's default frame.
# sphere_tree 3: LDS corner records, 2: LDS box records.  primary_lists is 1 in
# the sphere scenes also where a ball lies across the camera plane (rtow back,
# roll, wide, inside; field inside): the device build still delivers records,
# and every one of them says "walk" (the host build then has no lists).
PATHS = {
    ("rtow", "book"): (3, 1, 0, 0),
    ("rtow", "back"): (3, 1, 0, 0),
    ("rtow", "down"): (3, 1, 0, 0),
    ("rtow", "roll"): (3, 1, 0, 0),
    ("rtow", "wide"): (3, 1, 0, 0),
    ("rtow", "inside"): (3, 1, 0, 0),
    ("field", "side"): (3, 1, 0, 0),
    ("field", "behind"): (3, 1, 0, 0),
    ("field", "high"): (3, 1, 0, 0),
    ("field", "inside"): (3, 1, 0, 0),
    ("field", "roll"): (3, 1, 0, 0),
    ("field", "tele"): (3, 1, 0, 0),
    ("field", "wide"): (3, 1, 0, 0),
    ("soup", "side"): (2, 1, 1, 1),
    ("soup", "behind"): (2, 1, 1, 1),
    ("soup", "high"): (2, 1, 1, 1),
    ("soup", "inside"): (2, 1, 1, 1),
    ("soup", "roll"): (2, 1, 1, 1),
    ("soup", "tele"): (2, 1, 1, 1),
    ("soup", "wide"): (2, 1, 1, 1),
}


@pytest.fixture(autouse=True)
def _checked_lists(monkeypatch):
    monkeypatch.setenv("RT_AMD_SPL_CHECK", "1")
    monkeypatch.setenv("RT_AMD_PTL_CHECK", "1")


_MEMO = {}


def _src(scene):
    if ("src", scene) not in _MEMO:
        _MEMO["src", scene] = SCENES[scene][0]()
    return _MEMO["src", scene]


def _world(scene):
    """One library world per scene (the cases swap its camera)."""
    if ("world", scene) not in _MEMO:
        _MEMO["world", scene] = R.World(_src(scene))
    return _MEMO["world", scene]


def _oracle(scene, cam, w=W, h=H, spp=SPP, mode=O.RNG_COUNTER):
    """The oracle's frame, samples (GPU order) and rays at the 12 floats `cam`; computed once."""
    key = ("oracle", scene, np.asarray(cam, np.float32).tobytes(), w, h, spp, mode)
    if key not in _MEMO:
        if ("ref", scene) not in _MEMO:
            _MEMO["ref", scene] = O.Scene(_src(scene))
        ref = _MEMO["ref", scene]
        ref.set_camera(cam)
        assert np.array_equal(ref.camera().view(np.uint32), np.asarray(cam, np.float32).view(np.uint32))
        img, st, _, smp = ref.render(w, h, spp, DEPTH, mode=mode, nthreads=8 if mode == O.RNG_COUNTER else 1,
                                     record_samples=True)
        _MEMO[key] = (img, oracle_samples_to_gpu_order(smp, w, h, spp), st["rays"])
    return _MEMO[key]


def _assert_equals_oracle(scene, world, out, st, what):
    img, smp, rays = _oracle(scene, world.camera())
    assert_bits_equal(out, img, f"{what}: frame vs the oracle")
    assert_samples_equal(world.read_samples(NJOBS), smp, f"{what}: samples vs the oracle")
    assert st["rays"] == rays, (what, st["rays"], rays)


def _paths(st):
    return (st["sphere_tree"], st["primary_lists"], st["tri_bvh"], st["camera_tree"])


# ---- a. oracle parity at every camera --------------------------------------------------

@pytest.mark.parametrize("scene,name", CASES)
def test_oracle_parity(scene, name):
    world = _world(scene)
    CC.apply(world, SCENES[scene][1], name)
    assert np.array_equal(world.camera().view(np.uint32), CC.camera(SCENES[scene][1], name).view(np.uint32))
    out, st = render_kept(world, W, H, SPP, DEPTH)
    print(f"PATH {scene}/{name}: sphere_tree {st['sphere_tree']} primary_lists {st['primary_lists']} "
          f"tri_bvh {st['tri_bvh']} camera_tree {st['camera_tree']} tri_lists {world.primary_tri_lists()} "
          f"rays {st['rays']}")
    _assert_equals_oracle(scene, world, out, st, f"{scene}/{name}")
    assert st["accel"] == R.ACCEL_BVH
    assert _paths(st) == PATHS[scene, name]
    # not a plain sky frame: floors of rays per sample, from the oracle alone (the
    # smallest are rtow book 2.566, field wide 1.151, soup inside 1.195), and the
    # pixels that differ from the scene camera's frame (the fewest: rtow back, 1386)
    floor = {"rtow": 2.5, "field": 1.15, "soup": 1.19}[scene]
    assert st["rays"] >= floor * NJOBS, (st["rays"] / NJOBS, floor)
    default, _, _ = _oracle(scene, O.Scene(_src(scene)).camera())
    assert np.count_nonzero((out != default).any(axis=2)) >= 1386


def test_paths_cover_lists_and_walks():
    """An oriented RTOW case runs corner records with lists, and a case looks
    from inside the scene (a ball across the camera plane: every pixel walks,
    test_camera_lists_host asserts it on the host build)."""
    assert PATHS["rtow", "book"][:2] == (TREE_CORNER, 1)
    assert ("field", "inside") in PATHS and ("rtow", "inside") in PATHS


# ---- b. other layouts ---------------------------------------------------------------------

LAYOUT_CASES = [("rtow", "book"), ("field", "roll"), ("soup", "side")]
LAYOUTS = [dict(RT_AMD_CORNER="0"), dict(RT_AMD_LDS="0"), dict(RT_AMD_PRIMARY_LISTS="0")]
SOUP_LAYOUTS = [dict(RT_AMD_TRI_WIDE="0"), dict(RT_AMD_TRI_CELLS="2.5")]


def _layouts():
    for scene, name in LAYOUT_CASES:
        for env in LAYOUTS + (SOUP_LAYOUTS if scene == "soup" else []):
            yield pytest.param(scene, name, env, id=f"{scene}-{name}-" + "-".join(f"{k[7:]}={v}" for k, v in env.items()))


@pytest.mark.parametrize("scene,name,env", list(_layouts()))
def test_every_layout(monkeypatch, scene, name, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    world = R.World(_src(scene))  # (the cell trees are a load-time knob)
    CC.apply(world, SCENES[scene][1], name)
    out, st = render_kept(world, W, H, SPP, DEPTH)
    what = f"{scene}/{name} {env}"
    _assert_equals_oracle(scene, world, out, st, what)
    assert st["accel"] == R.ACCEL_BVH and st["sphere_tree"] != 0
    if "RT_AMD_CORNER" in env:
        assert st["sphere_tree"] in (TREE_BOX, TREE_GLOBAL)
    if "RT_AMD_LDS" in env:
        assert st["sphere_tree"] == TREE_GLOBAL
    if "RT_AMD_PRIMARY_LISTS" in env and scene == "soup":
        assert st["primary_lists"] == 0 and world.primary_tri_lists() == 0
    if scene == "soup":
        assert st["tri_bvh"] == 1


# ---- c. SERIAL ----------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,name", [("field", "roll"), ("soup", "side")])
def test_serial_stream(scene, name):
    w, h, spp = 33, 17, 3
    world = _world(scene)
    CC.apply(world, SCENES[scene][1], name)
    img, _, rays = _oracle(scene, world.camera(), w, h, spp, mode=O.RNG_SERIAL)
    out, st = world.render(w, h, spp, DEPTH, mode=R.RNG_SERIAL)
    assert_bits_equal(out, img, f"{scene}/{name}: SERIAL frame vs the oracle")
    assert st["rays"] == rays


# ---- d. mirrored and singular cameras -------------------------------------------------------------

@pytest.mark.parametrize("kind", ["mirrored", "singular"])
def test_cameras_the_constructors_cannot_make(kind):
    """rt_camera_from_floats takes any 12 floats: a mirrored camera (det > 0) and
    one whose vertical is parallel to its horizontal (det = 0) render, without lists."""
    world = _world("field")
    cam = getattr(CC, kind)(CC.camera(CC.FIELD, "roll"))
    assert CC.det(cam) > 0 if kind == "mirrored" else CC.det(cam) == 0
    world.set_camera(cam)
    out, st = render_kept(world, W, H, SPP, DEPTH)
    _assert_equals_oracle("field", world, out, st, f"field, {kind} camera")
    assert st["primary_lists"] == 0 and st["sphere_tree"] == TREE_CORNER


def test_soup_under_cameras_without_lists():
    world = _world("soup")
    for kind in ("mirrored", "singular"):
        world.set_camera(getattr(CC, kind)(CC.camera(CC.SOUP, "side")))
        out, st = render_kept(world, W, H, SPP, DEPTH)
        _assert_equals_oracle("soup", world, out, st, f"soup, {kind} camera")
        assert st["primary_lists"] == 0 and world.primary_tri_lists() == 0 and st["tri_bvh"] == 1


# ---- e. accumulators: a turn in place resets them ---------------------------------------------------

ACC_W, ACC_H, ACC_STRIDE = 40, 24, 8
TOL, BIAS, MIN_SAMPLES = 0.08, 0.05, 4
TURNED = ((7, 1, -5), (0.5, -0.4, -4.0), CC.Y, 50)  # FIELD["side"], turned in place


def _expect(scene, cam):
    key = ("expect", scene, np.asarray(cam, np.float32).tobytes())
    if key not in _MEMO:
        ref = O.Scene(_src(scene))
        ref.set_camera(cam)
        _MEMO[key] = Expect(ref, ACC_W, ACC_H, ACC_STRIDE, DEPTH)
    return _MEMO[key]


@pytest.mark.parametrize("scene", ["field", "soup"])
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_a_turn_in_place_resets_the_accumulator(scene, adaptive):
    world = R.World(_src(scene))
    CC.apply(world, SCENES[scene][1], "side")
    acc = world.accumulator(ACC_W, ACC_H, ACC_STRIDE, depth=DEPTH)
    if adaptive:
        acc.set_adaptive(TOL, BIAS, MIN_SAMPLES)
    acc.add(2)
    assert acc.samples == 2
    builds = world.camera_record_builds()
    o, t, up, deg = TURNED
    world.look_at(o, t, up, float(CC.radians(deg)), CC.ASPECT)
    before, after = CC.camera(SCENES[scene][1], "side"), world.camera()
    assert np.array_equal(before[:3], after[:3]) and not np.array_equal(before[3:], after[3:])
    assert acc.samples == 0
    exp = _expect(scene, after)
    if adaptive:
        assert acc.active == ACC_W * ACC_H
        states = restate(exp, (4,), TOL, BIAS, MIN_SAMPLES)
        assert 0 < len(states[0]["active"]) < ACC_W * ACC_H  # (the pass decides, and not trivially)
        out, st = acc.add(4)
        assert st["samples"] == states[0]["traced"]
        check(acc, exp, states[0], out, f"{scene}: adaptive pass after the turn")
    else:
        out, _ = _run(acc, (4,), exp, f"{scene} after the turn ")
        assert acc.samples == 4
    # the camera-origin records are keyed on the origin, which did not move
    assert world.camera_record_builds() == builds


# ---- f. the multi-device driver ---------------------------------------------------------------------

def test_one_oriented_frame_through_ndevices_1():
    world = _world("soup")
    CC.apply(world, CC.SOUP, "roll")
    img, _, rays = _oracle("soup", world.camera())
    out, st = world.render(W, H, SPP, DEPTH, ndevices=1)
    assert_bits_equal(out, img, "soup/roll, ndevices = 1: frame vs the oracle")
    assert st["rays"] == rays
