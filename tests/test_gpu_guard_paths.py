"""The fallbacks of csrc/exactdiv.h in waves that mix guard outcomes.

unit, divide_by and xsqrt run their fast sequence in every lane and reach
HIP's divide / sqrtf through one wave-wide test, selecting per lane inside
that block.  A frame of ordinary scenes never enters the block, and the
exhaustive checks of tools/exactdiv_check run every lane the same way, so
neither meets a wave in which some lanes take the fallback and some do not.

  * tools/guard_mix_check: one wave per (lane pattern, edge value) pair for
    each helper, raw bits against `/` and sqrtf on the device and on the host.
  * tools/exactdiv_check root: for all 2^32 sums, the length rule of xunit3
    (the unguarded root, sqrtf when it fails the denominator guard) has the
    bits of sqrtf.
  * Two scenes (tests/guard_scenes.py; tests/test_guard_scenes.py asserts on
    the CPU that 20 % to 80 % of their primary rays end on the edge primitive):
    frames of 64 x 8 pixels, 4 samples, depth 4, by the default search and by
    brute force, against the oracle on raw bits.  Scene A's 2^41 sphere sends
    divide_by through its fallback beside ordinary hits.  Scene B's camera
    offset of 2^-42 is absorbed when the grammar builds the camera frame, so
    it brings no tiny vector to unit (guard_scenes.py says why); that case,
    with huge, zero and non-finite vectors, is guard_mix_check's.

On an MI355X: guard_mix_check 56 waves, 800 of 3584 lanes outside the guards,
0 mismatches; scene a walks the corner tree with 3,219 tests of the big-sphere
list, scene b walks it with none (its glass ball is in the tree)."""
import os
import subprocess

import numpy as np
import pytest

import guard_scenes as G
import oracle as O
import raytracer_amd as R
from test_gpu_parity import assert_bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = G.FRAME


def _tool(name, *args):
    exe = os.path.join(ROOT, "tools", name)
    assert os.path.exists(exe), "build with `make -C rust-swift-raytracer_amd`"
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    return r


def test_helpers_in_waves_that_mix_guard_outcomes():
    r = _tool("guard_mix_check")
    assert r.returncode == 0 and "guard_mix OK" in r.stdout, r.stdout + r.stderr
    for name in ("divide_by", "unit", "xsqrt"):
        assert f"{name}: 0 mismatches with the device's plain form, 0 with the host" in r.stdout


def test_unit_length_rule_equals_sqrtf_for_every_input():
    r = _tool("exactdiv_check", "root")
    assert r.returncode == 0 and "exactdiv root OK" in r.stdout, r.stdout + r.stderr
    assert "unit root: all 2^32 sums, 0 mismatches" in r.stdout


_SCENES = {"a": G.scene_a, "b": G.scene_b}
_MEMO = {}


def _oracle(name):
    if name not in _MEMO:
        img, st, _ = O.Scene(_SCENES[name]()).render(W, H, SPP, DEPTH, mode=O.RNG_COUNTER, nthreads=4)
        _MEMO[name] = (img, st["rays"])
    return _MEMO[name]


@pytest.mark.parametrize("accel", ["default", "brute"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_scene_frames_equal_the_oracle(name, accel):
    img, rays = _oracle(name)
    world = R.World(_SCENES[name]())
    kw = dict(accel=R.ACCEL_BRUTE) if accel == "brute" else {}
    out, st = world.render(W, H, SPP, DEPTH, mode=R.RNG_COUNTER, **kw)
    lean, _ = world.render(W, H, SPP, DEPTH, mode=R.RNG_COUNTER, stats=False, **kw)  # (the kernel a frame ships with)
    print(f"scene {name} {accel}: accel {st['accel']} sphere_tree {st['sphere_tree']} "
          f"big_sphere_tests {st['big_sphere_tests']} rays {st['rays']}")
    if accel == "brute":
        assert st["accel"] == R.ACCEL_BRUTE and st["sphere_tree"] == 0
    else:
        assert st["accel"] == R.ACCEL_BVH and st["sphere_tree"] != 0
        if name == "a":
            assert st["big_sphere_tests"] > 0  # (the 2^41 sphere is in the brute-force list: spheres_big)
    assert_bits_equal(out, img, f"scene {name} {accel}: frame vs the oracle")
    assert_bits_equal(lean, img, f"scene {name} {accel}: lean frame vs the oracle")
    assert st["rays"] == rays
    assert np.asarray(img).any()
