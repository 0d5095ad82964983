"""Every trace-kernel instance of the library, run once and compared with the
oracle on raw bits (render.hip compiles one instance per TraceVariant; the host
picks one per launch from the scene's shape, the call and a few environment
knobs).

One case per key that rt_trace_instances reports.  The test does not ask the
library which instance a launch should run: it restates render.h's key formula
and normalisation rules (key_of, normalise), derives from the target variant a
scene, a knob set and a call (steer), restates what that steering asks for
from the knobs' documented meaning (asked), and requires

    key_of(normalise(asked(steer(target)))) == target key

on the CPU, for every key (test_every_instance_is_targeted).  On the GPU each
case clears the handle's launched set (rt_trace_launched), makes the call,
compares its results with the oracle's and requires that the set holds exactly
the target key.

Scenes: six, one per combination of {fewer than 16, at least 16} spheres and
{0, 1 to 15, at least 16} triangles: 16 primitives is where bvh.cpp starts to
build a tree.  test_scenes_are_meaningful checks each on the oracle alone: its
counted frame has at least 1.25 rays per sample, and where it has both kinds
of primitive, the frame changes when either kind is deleted.  The figures it
measured (40 x 24 x 8, depth 6) are in SCENES below, with the tolerance each
scene's adaptive cases run at (ADAPT_TOL), chosen so that the restatement
alone satisfies test_gpu_adapt.assert_tests_the_list."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from test_gpu_accum import Expect, assert_sums_equal
from test_gpu_adapt import BIAS, assert_tests_the_list, restate
from test_gpu_adapt import run as run_adaptive
from test_gpu_corner_tree import _random_scene
from test_gpu_parity import assert_bits_equal

W, H, SPP, DEPTH = 40, 24, 8, 6  # 7680 jobs: several waves per workgroup refill more than once
ACCUM_STRIDE, ACCUM_SPLIT = 8, (3, 1, 4)  # passes of 3 and 1 fold on pixel lanes, of 4 on plane lanes
ADAPT_STRIDE, ADAPT_SPLIT, ADAPT_MIN = 16, (4, 4, 4, 4), 8

# ---- render.h, restated --------------------------------------------------------

BRUTE, GLOBAL, BOX, CORNER = range(4)
LEAN, COUNTED, SERIAL, ACCUM, ADAPT = range(5)
SEARCHES = ("brute", "global", "box", "corner")
KINDS = ("lean", "counted", "serial", "accum", "adapt")
IMMEDIATE, DEFERRED, PLAIN = "immediate", "deferred", "plain"
GRID_KEYS = 4 * 2 * 4 * 5
KEY_DEFERRED, KEY_PLAIN = GRID_KEYS, GRID_KEYS + 1

Variant = namedtuple("Variant", "search step mesh kind leaf")


def key_of(v):
    """((search * 2 + step) * 4 + mesh) * 5 + kind, then the deferred-leaf
    instance and its plain twin (the lean whole-walk corner kernel's only)."""
    if v.leaf == IMMEDIATE:
        return ((v.search * 2 + v.step) * 4 + v.mesh) * 5 + v.kind
    assert (v.search, v.step, v.mesh, v.kind) == (CORNER, 0, 0, LEAN), v
    return KEY_DEFERRED if v.leaf == DEFERRED else KEY_PLAIN


def variant_at(key):
    if key in (KEY_DEFERRED, KEY_PLAIN):
        return Variant(CORNER, 0, 0, LEAN, PLAIN if key == KEY_PLAIN else DEFERRED)
    assert 0 <= key < GRID_KEYS, key
    return Variant(key // 40, key // 20 % 2, key // 5 % 4, key % 5, IMMEDIATE)


def normalise(v, plain_ok):
    """The instance that serves a request: SERIAL on the wide walk runs the
    binary walk; corner records serve only sphere-only, non-SERIAL launches;
    deferred leaves exist only for the lean whole-walk corner kernel; the plain
    instance runs only where the launch satisfies trace_plain_ok."""
    search, step, mesh, kind, leaf = v
    if kind == SERIAL and mesh == 3:
        mesh = 2
    if search == CORNER and (mesh != 0 or kind == SERIAL):
        search = BOX
    deferred = leaf != IMMEDIATE and search == CORNER and not step and mesh == 0 and kind == LEAN
    leaf = IMMEDIATE if not deferred else PLAIN if leaf == PLAIN and plain_ok else DEFERRED
    return Variant(search, step, mesh, kind, leaf)


def name_of(v):
    leaf = "" if v.leaf == IMMEDIATE else "-" + v.leaf
    return f"{SEARCHES[v.search]}-step{v.step}-mesh{v.mesh}-{KINDS[v.kind]}{leaf}"


# ---- the scenes ---------------------------------------------------------------------

def _soup(n, spheres, **kw):
    return S.triangle_soup(7, n, spread=1.5, size=1.0, spheres=spheres, **kw)


# name: (source, spheres, triangles, rays per sample of the oracle's counted frame)
SCENES = {
    # (the ground sphere of _random_scene counts: 11 and 41 spheres)
    "few spheres": (lambda: _random_scene(seed=5, n=10, spread=1.5, radius=0.8), 11, 0, 1.58),
    "many spheres": (lambda: _random_scene(seed=5, n=40, spread=1.5, radius=0.5), 41, 0, 1.77),
    "few spheres, few triangles": (lambda: _soup(8, 8, big=4), 8, 12, 1.73),
    "many spheres, few triangles": (lambda: _soup(8, 40, big=4), 40, 12, 1.82),
    "few spheres, many triangles": (lambda: _soup(300, 8, grid=6), 8, 372, 2.06),
    "many spheres, many triangles": (lambda: _soup(300, 40, grid=6), 40, 372, 2.23),
}
# The tolerance each scene's adaptive cases run at (bias 0.05, min_samples 8):
# the one at which the restatement keeps 5 % to 60 % of the pixels active at
# every decision, with some list length that is no multiple of 8.
ADAPT_TOL = {
    "few spheres": 0.06,  # (0.08 ends at exactly 5 %: 120, 69, 48 of 960)
    "many spheres": 0.08,
    "few spheres, few triangles": 0.08,
    "many spheres, few triangles": 0.08,
    "few spheres, many triangles": 0.08,
    "many spheres, many triangles": 0.08,
}
TREE_MIN = 16  # primitives from which bvh.cpp builds a tree (spheres and triangles alike)


def scene_of(many_spheres, triangles):
    """triangles: 0 none, 1 fewer than 16, 2 at least 16"""
    return (f"{'many' if many_spheres else 'few'} spheres" +
            ("", ", few triangles", ", many triangles")[triangles])


_memo = {}


def source(scene):
    if ("src", scene) not in _memo:
        _memo["src", scene] = SCENES[scene][0]()
    return _memo["src", scene]


def without(src, what):
    """The scene text less its `sphere` or `triangle` lines."""
    return "".join(line + "\n" for line in src.splitlines() if not line.startswith(what + " "))


def oracle_frame(scene, mode):
    """(frame, stats) of the oracle at the cases' size, once per (scene, mode)."""
    if ("frame", scene, mode) not in _memo:
        img, st, _ = O.Scene(source(scene)).render(W, H, SPP, DEPTH, mode=mode, nthreads=4)
        img.setflags(write=False)
        _memo["frame", scene, mode] = (img, st)
    return _memo["frame", scene, mode]


def expect(scene, stride):
    if ("expect", scene, stride) not in _memo:
        _memo["expect", scene, stride] = Expect(O.Scene(source(scene)), W, H, stride, DEPTH)
    return _memo["expect", scene, stride]


def adaptive_states(scene):
    if ("states", scene) not in _memo:
        _memo["states", scene] = restate(expect(scene, ADAPT_STRIDE), ADAPT_SPLIT, ADAPT_TOL[scene], BIAS,
                                         ADAPT_MIN)
    return _memo["states", scene]


@pytest.mark.parametrize("scene", list(SCENES))
def test_scenes_are_meaningful(scene):
    _, nsph, ntri, rays_per_sample = SCENES[scene]
    src = source(scene)
    ref = O.Scene(src)
    assert (ref.num_spheres, ref.num_triangles) == (nsph, ntri)
    world = R.World(src)  # (the product's parser agrees; host only)
    assert (world.num_spheres, world.num_triangles) == (nsph, ntri)
    # on the side of the 16-primitive thresholds its name says, whatever a builder keeps out of its tree
    many_spheres, triangles = scene.startswith("many"), 2 if "many tri" in scene else 1 if "few tri" in scene else 0
    big = int((np.abs(world.spheres()[:, 3]) > 8 * np.median(np.abs(world.spheres()[:, 3]))).sum())
    assert (nsph - big >= TREE_MIN) if many_spheres else (nsph < TREE_MIN)
    assert (ntri == 0, 0 < ntri < TREE_MIN, ntri >= TREE_MIN)[triangles]
    img, st = oracle_frame(scene, O.RNG_COUNTER)
    assert st["samples"] == W * H * SPP
    got = st["rays"] / st["samples"]
    print(f"{scene}: {got:.3f} rays per sample")
    assert got >= 1.25, f"{scene}: {got:.3f} rays per sample"
    assert round(got, 2) == rays_per_sample, f"{scene}: SCENES says {rays_per_sample}, measured {got:.3f}"
    if ntri:
        for what in ("sphere", "triangle"):
            other, _, _ = O.Scene(without(src, what)).render(W, H, SPP, DEPTH, mode=O.RNG_COUNTER, nthreads=4)
            changed = int((other != img).any(axis=2).sum())
            assert changed >= W * H // 50, f"{scene}: deleting the {what}s changes {changed} pixels"


@pytest.mark.parametrize("scene", list(SCENES))
def test_adaptive_tolerances_test_the_list(scene):
    assert_tests_the_list(adaptive_states(scene), W * H, ADAPT_MIN, scene)


# ---- steering ---------------------------------------------------------------------

Steer = namedtuple("Steer", "scene env kind")


def steer(target):
    """The scene, the knobs (all read at device setup or per frame: a fresh World per
    case) and the call that should run the instance `target`."""
    env = {"RT_AMD_STEP": str(target.step)}  # (always stated: its default depends on the scene)
    if target.search == GLOBAL:
        env["RT_AMD_LDS"] = "0"
    if target.search == BOX and target.mesh == 0:
        env["RT_AMD_CORNER"] = "0"
    if target.mesh == 2:
        env["RT_AMD_TRI_WIDE"] = "0"
    if target.search == CORNER and not target.step and target.kind == LEAN:
        if target.leaf == IMMEDIATE:
            env["RT_AMD_LEAF_DEFER"] = "0"
        if target.leaf == DEFERRED:
            env["RT_AMD_PLAIN"] = "0"
    return Steer(scene_of(target.search != BRUTE, min(target.mesh, 2)), env, target.kind)


def asked(st):
    """What that steering asks for, from the scene's shape and the knobs' documented
    meaning, before render.h's rules."""
    _, nsph, ntri, _ = SCENES[st.scene]
    env = st.env
    search = (BRUTE if nsph < TREE_MIN else GLOBAL if env.get("RT_AMD_LDS") == "0" else
              BOX if env.get("RT_AMD_CORNER") == "0" else CORNER)
    mesh = 0 if ntri == 0 else 1 if ntri < TREE_MIN else 2 if env.get("RT_AMD_TRI_WIDE") == "0" else 3
    leaf = IMMEDIATE if env.get("RT_AMD_LEAF_DEFER") == "0" else DEFERRED if env.get("RT_AMD_PLAIN") == "0" else PLAIN
    return Variant(search, int(env["RT_AMD_STEP"]), mesh, st.kind, leaf)


# trace_plain_ok for the lean frame of these cases: COUNTER, no counters, one rank, fused
# resolve, spp % 4 == 0, neither spp nor the width 1, depth >= 1, whole-walk chunks of 8 pixels
PLAIN_OK = SPP % 4 == 0 and SPP > 1 and W > 1 and DEPTH >= 1


def predicted_key(target):
    return key_of(normalise(asked(steer(target)), PLAIN_OK))


def instance_keys():
    return [int(k) for k in np.flatnonzero(R.trace_instances())]


# key -> the line of host code that keeps any steering from reaching it (at most 6)
UNREACHABLE = {}

# The keys rt_trace_instances reports are the variants that are their own normal form
# (test_every_instance_is_targeted asserts the two lists equal): the cases are listed
# from the rules, so that collecting them needs no built library.
OWN_NORMAL_FORM = [k for k in range(GRID_KEYS + 2) if key_of(normalise(variant_at(k), True)) == k]
TARGETS = [k for k in OWN_NORMAL_FORM if k not in UNREACHABLE]


def test_every_instance_is_targeted():
    """(no device: rt_trace_instances reads the table)"""
    have = instance_keys()
    assert len(R.trace_instances()) == GRID_KEYS + 3 and len(have) == 2 * (3 * 19 + 4) + 2
    assert len(UNREACHABLE) <= 6
    assert have == OWN_NORMAL_FORM
    assert all(key_of(variant_at(k)) == k for k in have)
    targeted = {k for k in TARGETS if predicted_key(variant_at(k)) == k}
    assert targeted == set(TARGETS), [name_of(variant_at(k)) for k in set(TARGETS) - targeted]
    assert targeted | set(UNREACHABLE) == set(have) and not targeted & set(UNREACHABLE)
    assert len({name_of(variant_at(k)) for k in have}) == len(have)


def test_entry_points_without_a_device():
    L = R.lib()
    assert L.rt_trace_instances(None, 0) == GRID_KEYS + 3
    short = np.full(8, 7, np.uint8)  # (n bytes at most are written)
    assert L.rt_trace_instances(short.ctypes.data_as(C.POINTER(C.c_uint8)), 5) == GRID_KEYS + 3
    assert short.tolist() == [1, 1, 1, 1, 1, 7, 7, 7]
    assert L.rt_trace_launched(None, -1, None, 0, 0) == -1
    assert "rt_trace_launched" in R.last_error()


# ---- the cases ----------------------------------------------------------------------

def launched(world, kind=None):
    keys = {int(k) for k in np.flatnonzero(world.trace_launched(clear=True))}
    return keys if kind is None else {k for k in keys if k < GRID_KEYS and variant_at(k).kind == kind}


@pytest.mark.gpu
@pytest.mark.parametrize("key", TARGETS, ids=lambda k: name_of(variant_at(k)))
def test_instance(monkeypatch, key):
    target = variant_at(key)
    what = name_of(target)
    st = steer(target)
    assert predicted_key(target) == key, what
    for k, v in st.env.items():
        monkeypatch.setenv(k, v)
    world = R.World(source(st.scene))
    assert launched(world) == set(), what  # (device setup launches nothing; the set starts empty)
    if st.kind in (LEAN, COUNTED):
        img, ost = oracle_frame(st.scene, O.RNG_COUNTER)
        out, got = world.render(W, H, SPP, DEPTH, stats=st.kind == COUNTED)
        ran = launched(world)
        assert_bits_equal(out, img, f"{what}: frame vs the oracle's COUNTER frame")
        if st.kind == COUNTED:
            assert (got["samples"], got["rays"]) == (ost["samples"], ost["rays"]), what
    elif st.kind == SERIAL:
        img, ost = oracle_frame(st.scene, O.RNG_SERIAL)
        out, got = world.render(W, H, SPP, DEPTH, mode=R.RNG_SERIAL)
        ran = launched(world, SERIAL)  # (the frame that replays the found states has a key of its own)
        assert_bits_equal(out, img, f"{what}: frame vs the oracle's SERIAL frame")
        assert got["rays"] == ost["rays"], what
    elif st.kind == ACCUM:
        exp = expect(st.scene, ACCUM_STRIDE)
        acc = world.accumulator(W, H, ACCUM_STRIDE, depth=DEPTH)
        for n in ACCUM_SPLIT:
            out, _ = acc.add(n)
            N = acc.samples
            assert_bits_equal(out, exp.frame(N), f"{what}: frame after {N} samples")
            assert_sums_equal(acc.sums(), exp.sums(N), f"{what}: sums after {N} samples")
        ran = launched(world)
        acc.close()
    else:
        exp, states = expect(st.scene, ADAPT_STRIDE), adaptive_states(st.scene)
        assert_tests_the_list(states, W * H, ADAPT_MIN, what)
        acc = world.accumulator(W, H, ADAPT_STRIDE, depth=DEPTH)
        acc.set_adaptive(ADAPT_TOL[st.scene], BIAS, ADAPT_MIN)
        run_adaptive(acc, exp, ADAPT_SPLIT, states, what)
        ran = launched(world)
        acc.close()
    assert ran == {key}, f"{what}: launched {sorted(name_of(variant_at(k)) for k in ran)}"
    world.close()
