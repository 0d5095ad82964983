"""Deferred leaf tests in the lean corner walk (trace_body.h trace_body kDefer,
DESIGN.md 5.2): a lane that enters a leaf records it and walks on, and the wave
tests the recorded leaves in shared passes.  Deferral only delays the decrease
of best_t, so the tested leaves are a superset of the immediate walk's and the
(t, index) argmin is the same: every comparison here is on the raw bits of the
lean frame (stats=False) against three references -- the brute-force kernel,
the lean frame of a fresh World under RT_AMD_LEAF_DEFER=0 (the immediate walk)
and the counting frame (which keeps the immediate walk).  World.leaf_defer()
(rt_leaf_defer) says which walk the last frame launch ran; a build without the
deferred instance fails here, it does not skip."""
import pytest

import raytracer_amd as R
import scenes as S
from test_gpu_corner_tree import TREE_CORNER, _brute, _random_scene
from test_gpu_parity import assert_bits_equal, render_kept

pytestmark = pytest.mark.gpu


def _lean_deferred(world, w, h, spp, depth):
    lean, st = world.render(w, h, spp, depth, stats=False)
    assert st is None
    c = world.leaf_defer()
    assert c in (2, 3), f"the lean frame ran the immediate walk (rt_leaf_defer = {c})"
    return lean


def _check(monkeypatch, make_world, w, h, spp, depth, ref=None, what=""):
    """The deferred lean frame of make_world() against brute force, the
    immediate-walk lean frame of a fresh world and the counting frame.
    Returns (brute-force reference, counting frame's stats)."""
    world = make_world()
    ref = ref or _brute(world, w, h, spp, depth)
    lean = _lean_deferred(world, w, h, spp, depth)
    assert_bits_equal(lean, ref[0], f"{what}: deferred lean frame vs brute force")
    out, st = render_kept(world, w, h, spp, depth)  # counting == lean == kept samples
    assert st["sphere_tree"] == TREE_CORNER, st["sphere_tree"]
    assert world.leaf_defer() == 0  # (the last launch: the counting kernel, immediate walk)
    assert_bits_equal(lean, out, f"{what}: deferred lean frame vs counting frame")
    assert_bits_equal(world.read_samples(w * h * spp), ref[2], f"{what}: samples vs brute force")
    assert st["rays"] == ref[1]["rays"]
    monkeypatch.setenv("RT_AMD_LEAF_DEFER", "0")
    off_world = make_world()
    off, _ = off_world.render(w, h, spp, depth, stats=False)
    assert off_world.leaf_defer() == 0
    monkeypatch.delenv("RT_AMD_LEAF_DEFER")
    assert_bits_equal(lean, off, f"{what}: deferred vs immediate lean frame")
    return ref, st


@pytest.mark.parametrize("depth", [8, 1])
def test_rtow_walk_gate_settings(monkeypatch, depth):
    """Default gate (walk when nothing else can advance), 1 (a lane walks in
    the iteration that set it up: few lanes per walk) and 32."""
    w, h, spp = 64, 36, 4
    ref, _ = _check(monkeypatch, lambda: R.World(S.rtow()), w, h, spp, depth, what=f"rtow d{depth}")
    for wm in ("1", "32"):
        monkeypatch.setenv("RT_AMD_WALK_MIN", wm)
        _check(monkeypatch, lambda: R.World(S.rtow()), w, h, spp, depth, ref=ref,
               what=f"rtow d{depth} walk_min {wm}")


@pytest.mark.parametrize("case", [
    # ties: duplicates land in different pending entries, the lower index must win
    dict(seed=2, n=300, spread=3.0, radius=0.6, dup=40),
    # camera inside the cluster, no ground sphere: long walks through many leaves
    dict(seed=5, n=250, spread=2.0, radius=0.5, big=False, cam=(0.0, 0.0, -4.0)),
    # large magnitudes in the stored t_near
    dict(seed=4, n=200, spread=5.0, radius=0.4, offset=(3000.0, -2000.0, 1500.0),
         cam=(3000.0, -2000.0, 1500.0)),
])
def test_dense_scenes_fill_and_overflow_the_pending_lists(monkeypatch, case):
    src = _random_scene(**case)
    _, st = _check(monkeypatch, lambda: R.World(src), 48, 32, 4, 8, what=f"seed {case['seed']}")
    if case["seed"] == 5:
        # A ray that enters at most 2 leaves tests at most 4 spheres (leaf size
        # 2; a primary list holds at most 3), so a mean above 4 per ray means
        # rays entered 3 leaves and more: lists filled to 2 and to 3, overflowed
        # at C = 2, and lanes with short walks ended with entries pending.
        assert st["bvh_sphere_tests"] > 4 * st["rays"], (st["bvh_sphere_tests"], st["rays"])


@pytest.mark.parametrize("w,h,spp", [(1, 5, 2), (5, 1, 2), (1, 1, 4), (33, 33, 2)])
def test_axis_aligned_camera_nan_infinite_and_zero_directions(monkeypatch, w, h, spp):
    """Frames of width or height 1 divide by zero (infinite and NaN directions,
    NaN t_near in the recorded entries); the odd-sized frame's central rays
    have +-0 and tiny components."""
    src = _random_scene(seed=7, n=300, spread=2.0, radius=0.4, big=False)
    _check(monkeypatch, lambda: R.World(src), w, h, spp, 8, what=f"axis cluster {w}x{h}x{spp}")


def test_leaves_of_up_to_four_spheres(monkeypatch):
    """RT_AMD_LEAF=4: sphere_leaf's loop form runs inside the shared passes."""
    monkeypatch.setenv("RT_AMD_LEAF", "4")
    _, st = _check(monkeypatch, lambda: R.World(S.rtow()), 64, 36, 4, 8, what="rtow leaf 4")
    assert st["sphere_tree"] == 3


def test_rtow_camera_inside_the_sphere_field(monkeypatch):
    """Primary candidate lists and walks mixed in one wave."""
    def moved():
        world = R.World(S.rtow())
        world.move_camera(0.5, -1.5, -9.0)
        return world
    _check(monkeypatch, moved, 80, 60, 4, 8, what="rtow moved")


def test_the_accumulation_kinds_keep_the_immediate_walk():
    """(their corner instances did not take the deferred walk)"""
    world = R.World(S.rtow())
    w, h = 32, 18
    acc = world.accumulator(w, h, 4)
    acc.add(4)
    assert world.leaf_defer() == 0
    acc.close()
    _lean_deferred(world, w, h, 4, 8)
