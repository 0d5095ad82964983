"""Scenes with unusual but legal values (tests/scene_values.py) on the GPU, bit
for bit: negative, zero and non-finite radii, six refraction indices (NaN and
infinite directions from the second bounce on), unclamped fuzz and colours,
degenerate and non-finite triangles, coincident primitives, a camera inside a
glass ball.  Every case carries a background large enough for the trees, so
the tree walks, the primary lists and the SERIAL scatter count meet these
values, not only brute force.

The expectation is the oracle (pinned against the numpy restatement at these
values by tests/test_scene_values.py, which also asserts that the edge
primitives are visible in these frames).  Frames and ray counts are compared
on raw bits; per-sample colours on bits with NaN equal to NaN (a NaN's sign
and payload differ between x86 and gfx950, and no frame shows them: `as u8`
maps every NaN to 0).

PATHS records what the frames of each case ran with on an MI355X."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scene_values as V
from test_gpu_accum import Expect, _run, assert_sums_equal
from test_gpu_adapt import check, colours, restate
from test_gpu_adapt import run as run_adaptive
from test_gpu_corner_tree import TREE_CORNER, TREE_GLOBAL, _brute
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order, render_kept

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = V.FRAME
NJOBS = W * H * SPP

# What the default frames (section a) ran with: sphere_tree (3: LDS corner
# records, 2: LDS box records), primary_lists, tri_bvh, and whether the
# brute-force list of big and non-finite spheres was tested.
PATHS = {
    # name: (sphere_tree, primary_lists, tri_bvh, big_sphere_tests > 0)
    "hollow": (3, 1, 0, False),
    "zero_r": (3, 1, 0, False),
    "ir": (3, 1, 0, False),
    "fuzz_col": (3, 1, 0, False),
    "nonfinite": (3, 1, 0, True),       # (the three non-finite balls: 22,029 tests)
    "big_mix": (3, 1, 0, True),         # (the ball above 8 x median: one test per ray, 8,681)
    "coincident": (3, 1, 0, False),
    "cam_inside": (3, 1, 0, True),      # (the radius-2 glass ball is above 8 x median: 16,419)
    "tri_degenerate": (2, 1, 1, False),
    "tri_tie": (2, 1, 1, False),
    "edit_ir": (3, 1, 0, False),
    "edit_fuzz_col": (3, 1, 0, False),
}
# primary_lists is 1 in every sphere case, also after move_camera(0.3, -0.2, -1.0):
# where a ball straddles the camera plane (cam_inside; hollow after the move)
# the device build still delivers records, and every one of them says "walk"
# (the host build, which RT_AMD_SPL_CHECK compares with, then has no lists).


def assert_samples_equal(got, want, what):
    """Sample colours: bits, NaN equal to NaN (test_gpu_accum.assert_sums_equal's rule)."""
    assert_sums_equal(np.ascontiguousarray(got[:, :3]), np.ascontiguousarray(want[:, :3]), what)


# ---- one world, one oracle scene and one oracle frame per case ----------------------

_MEMO = {}


def _pair(name):
    """(R.World, O.Scene) of the case, edits applied; built once."""
    key = ("pair", name)
    if key not in _MEMO:
        case = V.case(name)
        world, scene = R.World(case.src), O.Scene(case.src)
        assert world.num_spheres == scene.num_spheres and world.num_triangles == scene.num_triangles
        case.apply_edits(world, scene)
        _MEMO[key] = (world, scene)
    return _MEMO[key]


def _oracle(name, w=W, h=H, spp=SPP, mode=O.RNG_COUNTER):
    """The oracle's frame, samples (in the GPU's order) and ray count; computed once."""
    key = ("oracle", name, w, h, spp, mode)
    if key not in _MEMO:
        _, scene = _pair(name)
        img, st, _, smp = scene.render(w, h, spp, DEPTH, mode=mode, nthreads=8 if mode == O.RNG_COUNTER else 1,
                                       record_samples=True)
        _MEMO[key] = (img, oracle_samples_to_gpu_order(smp, w, h, spp), st["rays"])
    return _MEMO[key]


def _fresh_world(name):
    case = V.case(name)
    world = R.World(case.src)
    case.apply_edits(world)
    return world


def _assert_equals_oracle(name, world, out, st, what):
    img, smp, rays = _oracle(name)
    assert_bits_equal(out, img, f"{what}: frame vs the oracle")
    assert_samples_equal(world.read_samples(NJOBS), smp, f"{what}: samples vs the oracle")
    assert st["rays"] == rays, (what, st["rays"], rays)


def _assert_tree_paths(name, st, what):
    assert st["accel"] == R.ACCEL_BVH and st["sphere_tree"] != 0, (what, st["accel"], st["sphere_tree"])
    if V.case(name).soup:
        assert st["tri_bvh"] == 1, what
    if name == "nonfinite":
        assert st["big_sphere_tests"] > 0, what


# ---- a. oracle parity -----------------------------------------------------------------

@pytest.mark.parametrize("name", V.TABLE_CASES + V.EDIT_CASES)
def test_oracle_parity(name):
    world, _ = _pair(name)
    out, st = render_kept(world, W, H, SPP, DEPTH)  # counting == lean == kept-samples frames
    print(f"PATH {name}: sphere_tree {st['sphere_tree']} primary_lists {st['primary_lists']} "
          f"tri_bvh {st['tri_bvh']} big_sphere_tests {st['big_sphere_tests']}")
    _assert_equals_oracle(name, world, out, st, name)
    _assert_tree_paths(name, st, name)
    if name in PATHS:
        assert (st["sphere_tree"], st["primary_lists"], st["tri_bvh"], st["big_sphere_tests"] > 0) == PATHS[name]
    ref, rst, ref_s = _brute(world, W, H, SPP, DEPTH)
    img, smp, rays = _oracle(name)
    assert_bits_equal(ref, img, f"{name}: brute-force frame vs the oracle")
    assert_samples_equal(ref_s, smp, f"{name}: brute-force samples vs the oracle")
    assert rst["rays"] == rays


# ---- b. every layout ------------------------------------------------------------------

SPHERE_LAYOUTS = [dict(RT_AMD_CORNER="0"), dict(RT_AMD_LDS="0"), dict(RT_AMD_LEAF="1"),
                  dict(RT_AMD_SPHERE_LISTS="0"), dict(RT_AMD_PRIMARY_LISTS="0")]
SOUP_LAYOUTS = [dict(RT_AMD_TRI_WIDE="0"), dict(RT_AMD_TRI_CELLS="2.5")]


def _layouts():
    for name in V.TABLE_CASES:
        case = V.case(name)
        envs = SPHERE_LAYOUTS + (SOUP_LAYOUTS if case.soup else []) + [dict(RT_AMD_BIG_K=k) for k in case.big_k]
        for env in envs:
            yield pytest.param(name, env, id=f"{name}-" + "-".join(f"{k[7:]}={v}" for k, v in env.items()))


@pytest.mark.parametrize("name,env", list(_layouts()))
def test_every_layout(monkeypatch, name, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    world = _fresh_world(name)  # (leaf size, big_k and the cell trees are load-time knobs)
    out, st = render_kept(world, W, H, SPP, DEPTH)
    what = f"{name} {env}"
    _assert_equals_oracle(name, world, out, st, what)
    _assert_tree_paths(name, st, what)
    if "RT_AMD_CORNER" in env:
        assert st["sphere_tree"] != TREE_CORNER
    if "RT_AMD_LDS" in env:
        assert st["sphere_tree"] == TREE_GLOBAL
    if "RT_AMD_SPHERE_LISTS" in env and not V.case(name).soup:
        assert st["primary_lists"] == 0
    if env.get("RT_AMD_BIG_K") == "1e9":
        assert st["big_sphere_tests"] == 0  # (every sphere of big_mix is in the tree)
    if env.get("RT_AMD_BIG_K") == "2":
        assert st["big_sphere_tests"] > 0


# ---- c. device sphere lists ---------------------------------------------------------------

@pytest.mark.parametrize("name", V.SPHERE_CASES)
def test_device_sphere_lists_equal_the_host_build(monkeypatch, name):
    """RT_AMD_SPL_CHECK=1: the frame fails unless every device-built list equals
    the host build's.  A case may legitimately have no lists (a ball straddling
    the camera plane or a non-finite one sends every pixel to the walk): either
    way the frame equals brute force."""
    monkeypatch.setenv("RT_AMD_SPL_CHECK", "1")
    world = _fresh_world(name)  # (a fresh world: its lists are built, and checked, by this frame)
    out, st = render_kept(world, W, H, SPP, DEPTH)
    _assert_equals_oracle(name, world, out, st, f"{name}, lists checked")
    if name in PATHS:
        assert st["primary_lists"] == PATHS[name][1]
    world.move_camera(0.3, -0.2, -1.0)
    ref, rst, ref_s = _brute(world, W, H, SPP, DEPTH)
    out, st2 = render_kept(world, W, H, SPP, DEPTH)
    print(f"LISTS {name}: primary_lists {st['primary_lists']}, after the move {st2['primary_lists']}")
    assert_bits_equal(out, ref, f"{name}: frame after the move vs brute force")
    assert_samples_equal(world.read_samples(NJOBS), ref_s, f"{name}: samples after the move vs brute force")
    assert st2["rays"] == rst["rays"] and st2["sphere_tree"] != 0


# ---- d. SERIAL ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ir", "fuzz_col", "hollow", "tri_degenerate"] + V.EDIT_CASES)
def test_serial_stream(name):
    """The GPU finds each sample's start state from a count of scatter draws: a
    NaN path, an absorbed metal ray or fuzz 100 must advance it as the
    reference's stream advances (3 draws per diffuse or metal scatter, none per
    dielectric)."""
    w, h, spp = 33, 17, 3
    world, _ = _pair(name)
    img, _, rays = _oracle(name, w, h, spp, mode=O.RNG_SERIAL)
    out, st = world.render(w, h, spp, DEPTH, mode=R.RNG_SERIAL)
    assert_bits_equal(out, img, f"{name}: SERIAL frame vs the oracle")
    assert st["rays"] == rays


# ---- e. degenerate frames ---------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 5), (5, 1), (1, 1)])
@pytest.mark.parametrize("name", ["ir", "tri_degenerate"])
def test_degenerate_frames(name, w, h):
    world, _ = _pair(name)
    img, _, rays = _oracle(name, w, h, SPP)
    out, st = world.render(w, h, SPP, DEPTH)
    assert_bits_equal(out, img, f"{name} {w}x{h}: frame vs the oracle")
    assert st["rays"] == rays


# ---- accumulators on frames with NaN, negative and above-1 samples ---------------------------------

ACC_W, ACC_H, ACC_STRIDE = 40, 24, 16
SPLITS = [(4, 4, 4, 4), (3, 5, 8)]
TOL, BIAS, MIN_SAMPLES = 0.08, 0.05, 8

# Pixels still active after each decision pass (N >= 8) of the numpy
# restatement, of 960: measured on the CPU.  Few pixels stay (the 5 % to 60 % band of
# test_gpu_adapt does not hold: ir's list is mostly its 27 or 28 NaN pixels,
# 2.9 % of the frame, which never leave it).
ACTIVE = {
    ("ir", (4, 4, 4, 4)): [55, 42, 36],             # 5.7 %, 4.4 %, 3.8 %
    ("ir", (3, 5, 8)): [55, 36],                    # 5.7 %, 3.8 %
    ("fuzz_col", (4, 4, 4, 4)): [134, 109, 91],     # 14.0 %, 11.4 %, 9.5 %
    ("fuzz_col", (3, 5, 8)): [134, 91],             # 14.0 %, 9.5 %
}


def _expect(name):
    key = ("expect", name)
    if key not in _MEMO:
        _MEMO[key] = Expect(O.Scene(V.case(name).src), ACC_W, ACC_H, ACC_STRIDE, DEPTH)
    return _MEMO[key]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["ir", "fuzz_col"])
def test_plain_accumulator(name, split):
    exp = _expect(name)
    smp = colours(exp, ACC_STRIDE)
    if name == "ir":
        assert np.isnan(smp).any() and np.isnan(exp.sums(ACC_STRIDE)).any()
    else:
        assert (smp < 0).any() and (smp > 1).any() and (exp.sums(ACC_STRIDE) < 0).any()
    world, _ = _pair(name)
    acc = world.accumulator(ACC_W, ACC_H, ACC_STRIDE, depth=DEPTH)
    out, _ = _run(acc, split, exp, f"{name} ")  # (frame and sums after every pass)
    assert acc.samples == ACC_STRIDE
    assert_bits_equal(out, world.render(ACC_W, ACC_H, ACC_STRIDE, DEPTH)[0], f"{name}: final vs the one-shot frame")


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("name", ["ir", "fuzz_col"])
def test_adaptive_accumulator(name, split):
    """The decision e <= lim * lim is false for a NaN pixel, which stays listed
    for ever; a pixel with a negative mean has lim = tol * (m + bias) negative
    and then squared.  A kernel that restates the decision differently
    (!(e > lim * lim), fmaxf on a NaN, a contracted q * inv - m * m) diverges at
    these pixels."""
    exp = _expect(name)
    states = restate(exp, split, TOL, BIAS, MIN_SAMPLES)
    decided = [s for s in states if s["N"] >= MIN_SAMPLES]
    assert [len(s["active"]) for s in decided] == ACTIVE[name, split]
    before = np.arange(ACC_W * ACC_H)  # (the list a decision pass starts with)
    seen = left = 0
    for s in states:
        nan = np.flatnonzero(np.isnan(s["sums"]).any(axis=1) | np.isnan(s["sumsq"]))
        assert np.isin(nan, s["active"]).all(), "a NaN pixel left the list"
        if s["N"] >= MIN_SAMPLES:
            a = s["sums"][before]
            m = ((a[:, 0] + a[:, 1]) + a[:, 2]) * (np.float32(1.0) / np.float32(s["N"]))
            if name == "ir":
                seen += np.count_nonzero(np.isnan(m))
            else:
                seen += np.count_nonzero(m < 0)
                left += np.count_nonzero(~np.isin(before[m < 0], s["active"]))
        before = s["active"]
    assert seen > 0, "no NaN sum (ir) or negative luminance mean (fuzz_col) met a decision"
    if name == "fuzz_col":
        assert 0 < left < seen  # (pixels with a negative mean on both sides of the decision)
    world, _ = _pair(name)
    acc = world.accumulator(ACC_W, ACC_H, ACC_STRIDE, depth=DEPTH)
    acc.set_adaptive(TOL, BIAS, MIN_SAMPLES)
    run_adaptive(acc, exp, split, states, f"{name} adaptive")  # list, counts, sums, sumsq, frame per pass
    check(acc, exp, states[-1], None, f"{name} adaptive, at the end")
