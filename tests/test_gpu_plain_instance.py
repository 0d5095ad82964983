"""The plain instance of the lean deferred-leaf kernel (trace_body.h trace_body
kPlain): the loop's tests of launch constants are decided at
compile time for launches that satisfy render.h trace_plain_ok, every other
launch runs the instance it ran before.  Nothing a sample computes changes, so
every comparison here is on the raw bits of the lean frame (stats=False)
against three references -- the brute-force kernel, the counting frame and the
lean frame of a fresh World under RT_AMD_PLAIN=0 (the generic instance).
World.trace_plain() (rt_trace_plain) says which instance the last frame launch
ran: a frame meant for the plain instance asserts 1, a fall-back asserts 0, so
no case can test the other kernel unnoticed.  A build without the instance
fails here, it does not skip."""
import numpy as np
import pytest

import raytracer_amd as R
import scenes as S
from test_gpu_corner_tree import TREE_CORNER, _brute, _random_scene
from test_gpu_parity import assert_bits_equal, render_kept

pytestmark = pytest.mark.gpu


def _lean(world, w, h, spp, depth, plain, **kw):
    lean, st = world.render(w, h, spp, depth, stats=False, **kw)
    assert st is None
    got = world.trace_plain()
    assert got == plain, f"{w}x{h}x{spp}: rt_trace_plain = {got}, expected {plain}"
    return lean


def _check(monkeypatch, make_world, w, h, spp, depth, ref=None, what="", plain=1):
    """The lean frame of make_world(), which must run the plain instance
    (plain=0: must not), against brute force, the counting frame and the
    generic lean frame of a fresh world.  Returns the brute-force reference."""
    world = make_world()
    ref = ref or _brute(world, w, h, spp, depth)
    lean = _lean(world, w, h, spp, depth, plain)
    assert_bits_equal(lean, ref[0], f"{what}: plain lean frame vs brute force")
    out, st = render_kept(world, w, h, spp, depth)  # counting == lean == kept samples
    assert st["sphere_tree"] == TREE_CORNER, st["sphere_tree"]
    assert world.trace_plain() == 0  # (the last launch kept its samples: no ring)
    assert_bits_equal(lean, out, f"{what}: plain lean frame vs counting frame")
    assert st["rays"] == ref[1]["rays"]
    monkeypatch.setenv("RT_AMD_PLAIN", "0")
    off_world = make_world()
    off = _lean(off_world, w, h, spp, depth, 0)
    assert off_world.leaf_defer() in (2, 3)  # (the generic deferred-leaf instance)
    monkeypatch.delenv("RT_AMD_PLAIN")
    assert_bits_equal(lean, off, f"{what}: plain vs generic lean frame")
    return ref


# 64 x 36: the launch takes chunks of max(64, 4 spp) jobs (frame.cpp plan_launch:
# 64-job chunks at least, 4 whole pixels at least), so spp 4 gives 16-pixel
# chunks, 48 plane lanes of 64 -- the smallest spp >= 4 already selects the
# instance; spp 64 gives the 4-pixel chunks of 256 jobs.
@pytest.mark.parametrize("depth", [8, 1])
@pytest.mark.parametrize("spp", [64, 4])
def test_rtow(monkeypatch, spp, depth):
    _check(monkeypatch, lambda: R.World(S.rtow()), 64, 36, spp, depth, what=f"rtow spp {spp} d{depth}")


def test_rtow_odd_frame_short_last_chunks_and_partial_refill(monkeypatch):
    """1089 pixels in 5 partitions of 16-pixel chunks: no partition is a whole
    number of chunks, and the last refill of a wave is partial."""
    _check(monkeypatch, lambda: R.World(S.rtow()), 33, 33, 4, 8, what="rtow 33x33")


@pytest.mark.parametrize("plain,case", [
    # ties: exact duplicates, the lower index must win
    (1, dict(seed=2, n=300, spread=3.0, radius=0.6, dup=40)),
    # large magnitudes (the exact-division guards' fallback blocks are still in
    # the instance).  A camera with a coordinate of 1000 or more gets no primary
    # sphere lists (bvh.cpp sphere_list_params: far-off cameras walk the tree),
    # so by the predicate's own rule this frame runs the generic instance ...
    (0, dict(seed=4, n=200, spread=5.0, radius=0.4, offset=(3000.0, -2000.0, 1500.0),
             cam=(3000.0, -2000.0, 1500.0))),
    # ... and the same cluster just inside that limit runs the plain one
    (1, dict(seed=4, n=200, spread=5.0, radius=0.4, offset=(990.0, -980.0, 970.0),
             cam=(990.0, -980.0, 970.0))),
])
def test_dense_random_scenes(monkeypatch, plain, case):
    src = _random_scene(**case)
    _check(monkeypatch, lambda: R.World(src), 48, 32, 4, 8, what=f"seed {case['seed']}", plain=plain)


def test_rtow_camera_inside_the_sphere_field(monkeypatch):
    """Primary candidate lists and walks mixed in one wave."""
    def moved():
        world = R.World(S.rtow())
        world.move_camera(0.5, -1.5, -9.0)
        return world
    _check(monkeypatch, moved, 80, 60, 4, 8, what="rtow moved")


# ---- launches the predicate turns away: the generic instance, the same bits
@pytest.mark.parametrize("w,h,spp,why", [
    (64, 36, 6, "spp not a multiple of 4: pixel-lane resolve"),
    (64, 36, 1, "spp 1: the sample divider is the identity"),
    (1, 36, 4, "width 1: the width divider is the identity, u divides by zero"),
    (64, 1, 4, "height 1: v divides by zero"),
])
def test_fallback_frame_shapes(w, h, spp, why):
    world = R.World(S.rtow())
    ref = _brute(world, w, h, spp, 8)
    assert_bits_equal(_lean(world, w, h, spp, 8, 0), ref[0], why)


def test_fallback_replay_mode():
    w, h, spp = 64, 36, 4
    states = np.random.default_rng(11).integers(1, 2**32, w * h * spp, dtype=np.uint64).astype(np.uint32)
    world = R.World(S.rtow())
    ref, st = world.render(w, h, spp, 8, mode=R.RNG_REPLAY, replay=states, accel=R.ACCEL_BRUTE)
    assert st["accel"] == R.ACCEL_BRUTE
    lean = _lean(world, w, h, spp, 8, 0, mode=R.RNG_REPLAY, replay=states)
    assert_bits_equal(lean, ref, "REPLAY lean frame vs brute force")
    _lean(world, w, h, spp, 8, 1)  # (and COUNTER again on the same world: the plain instance)


def test_fallback_ungated_walks(monkeypatch):
    monkeypatch.setenv("RT_AMD_WALK_MIN", "0")
    world = R.World(S.rtow())
    ref = _brute(world, 64, 36, 4, 8)
    assert_bits_equal(_lean(world, 64, 36, 4, 8, 0), ref[0], "walk_min 0")


def test_fallback_accumulation_pass():
    world = R.World(S.rtow())
    w, h = 64, 36
    ref = _brute(world, w, h, 4, 8)
    _lean(world, w, h, 4, 8, 1)
    acc = world.accumulator(w, h, 4)
    out, _ = acc.add(4)
    assert world.trace_plain() == 0
    acc.close()
    assert_bits_equal(out, ref[0], "accumulated frame of 4 samples vs brute force")
