"""The plain instance's shading paths (trace_body.h RT_PLAIN_STEPS 8..64,
DESIGN.md 5.1 "the shading block"): a path ends inside the shading block -- the
depth test sits where the bounce is counted, the sample store in the block --
a shading lane is sky or sphere, the first big sphere is read with the set-up's
parameters and the sample store takes one scalar base.  Nothing a sample
computes changes, so every comparison is on the raw RGBA8 bytes of the plain
lean frame against the brute-force frame, the counting frame and the
RT_AMD_PLAIN=0 frame of a fresh world (test_gpu_plain_instance._check);
World.trace_plain() says which instance ran.  COUNTER mode, frames of at most
96 x 54.

No diffuse sphere whose scatter takes keep_normal is here: that needs a drawn
unit vector within 1e-8 of -normal in every component at once, a sixth of the
spacing of f32 values near 1 (6e-8), so it takes an exact cancellation in all
three components; no input that does it is known, and the case is left out."""
import numpy as np
import pytest

import raytracer_amd as R
import scenes as S
from test_gpu_corner_tree import TREE_CORNER, _brute
from test_gpu_parity import assert_bits_equal, render_kept
from test_gpu_plain_instance import _check, _lean

pytestmark = pytest.mark.gpu

W, H = 64, 36


def _rtow():
    return R.World(S.rtow())


# ---- depth: where a path ends
# depth 1: every path that scatters ends at its first ++bounce; depth 2: the
# first scattered ray is the last; 3 and 8: both kinds of end in one wave
@pytest.mark.parametrize("spp", [4, 8])
@pytest.mark.parametrize("depth", [1, 2, 3, 8])
def test_rtow_depths(monkeypatch, depth, spp):
    _check(monkeypatch, _rtow, W, H, spp, depth, what=f"rtow d{depth} spp {spp}")


def test_depth_zero_is_black_and_not_plain():
    """Bounce 0 is exhausted before any hit: the frame does not ask for the instance."""
    world = _rtow()
    lean = _lean(world, W, H, 4, 0, 0)
    px = np.ascontiguousarray(lean).reshape(-1, 4)
    assert (px[:, :3] == 0).all() and (px[:, 3] != 0).all()
    out, st = render_kept(world, W, H, 4, 0)
    assert_bits_equal(lean, out, "depth 0: lean vs counting frame")
    assert st["rays"] == 0
    _lean(world, W, H, 4, 1, 1)  # (and depth 1 on the same world: the plain instance)


# ---- every material kind
KINDS = ["Diffuse color 0.7 0.5 0.3", "Metal color 0.9 0.8 0.7 fuzz 0.9",
         "Dielectric ir 1.5", "Metal color 0.6 0.6 0.9 fuzz 0.0", "Diffuse color 0.2 0.9 0.4"]


def _cluster(seed, n, radius, big=(), jitter=False, spread=3.0):
    """n spheres of one radius (jitter: 0.3..1 of it) in front of the camera,
    after the spheres of `big` (centre offset, radius)."""
    rng = np.random.default_rng(seed)
    lines = ["camera origin 0.000000 0.000000 0.000000 aspect 1.777780;"]
    lines += [f"material K{i} : {k};" for i, k in enumerate(KINDS)]
    sph = [(x, y, z, r, i % len(KINDS)) for i, (x, y, z, r) in enumerate(big)]
    for _ in range(n):
        c = rng.uniform(-spread, spread, 3) + np.array([0.0, 0.0, -spread - 2.0])
        r = radius * (rng.uniform(0.3, 1.0) if jitter else 1.0)
        sph.append((c[0], c[1], c[2], r, int(rng.integers(0, len(KINDS)))))
    for (x, y, z, r, k) in sph:
        lines.append(f"sphere center {x:.6f} {y:.6f} {z:.6f} radius {r:.6f} material K{k};")
    return "\n".join(lines) + "\n"


def _nbig(st):
    return st["big_sphere_tests"] // st["rays"]


def _counting(world, w, h, spp, depth):
    out, st = world.render(w, h, spp, depth)
    assert st["sphere_tree"] == TREE_CORNER
    return out, st


def test_every_material_kind(monkeypatch):
    """Emitters in view of the camera (a primary ray ends at bounce 0 with
    !next), fuzzy metal (scattered below the surface: dot(v, n) < 0 ends the
    path), mirrors, glass and diffuse spheres, under a ground sphere."""
    src = _cluster(21, 90, 0.55, big=[(0.0, -1004.0, -5.0, 1000.0)], jitter=True)

    def make():
        world = R.World(src)
        for i in range(3, world.num_spheres, 6):  # every sixth sphere emits
            world.set_material(i, 3, (4.0, 3.0, 2.0))
        return world
    world = make()
    # the paths the scene is for do occur: some primary rays see an emitter,
    # and frames of depth 1 and 8 differ (paths go on past the first hit)
    kinds = world.first_hit(W, H)["prim"]
    emit = {i + 1 for i in range(3, world.num_spheres, 6)}
    assert np.isin(kinds, list(emit)).any(), "no emitter is hit by a primary ray"
    for depth in (8, 2):
        _check(monkeypatch, make, W, H, 8, depth, what=f"materials d{depth}")


# ---- big spheres: 0, 1 (RTOW, above) and 3
def test_no_big_sphere(monkeypatch):
    src = _cluster(5, 120, 0.35)
    _, st = _counting(R.World(src), W, H, 4, 8)
    assert _nbig(st) == 0
    _check(monkeypatch, lambda: R.World(src), W, H, 4, 8, what="equal radii")


def test_rtow_has_one_big_sphere():
    _, st = _counting(_rtow(), W, H, 4, 8)
    assert _nbig(st) == 1


def test_three_big_spheres(monkeypatch):
    # radii 30, 8 and 1000 against a median of 0.35: all above 8 x the median
    big = [(0.0, -1004.0, -5.0, 1000.0), (-14.0, 2.0, -40.0, 30.0), (6.0, 5.0, -16.0, 8.0)]
    src = _cluster(6, 120, 0.35, big=big)
    _, st = _counting(R.World(src), W, H, 4, 8)
    assert _nbig(st) == 3
    _check(monkeypatch, lambda: R.World(src), W, H, 4, 8, what="three big spheres")


# ---- chunk mixes: ring accounting with several slots finishing at one refill
def test_short_last_chunks_and_small_chunks(monkeypatch):
    """8-pixel chunks at spp 4 (half a wave's lanes each, so a refill point
    sees finished lanes of several ring slots), in a frame whose partitions
    end in short chunks."""
    monkeypatch.setenv("RT_AMD_CHUNK", "32")
    world = _rtow()
    _, st = _counting(world, 93, 41, 4, 8)
    assert st["launch_chunk"] == 32
    _check(monkeypatch, _rtow, 93, 41, 4, 8, what="93x41, 8-pixel chunks")


# ---- the counting kernel is not touched: its counters for a C2-shaped small frame
def test_counters_of_a_c2_shaped_frame():
    _, st = _counting(_rtow(), 96, 54, 64, 8)
    assert (st["rays"], st["bvh_node_tests"], st["bvh_sphere_tests"]) == C2_SMALL_COUNTERS


# (rays, bvh_node_tests, bvh_sphere_tests) of the 96 x 54 x 64 depth-8 RTOW
# counting frame, recorded from the commit before the shading paths changed
C2_SMALL_COUNTERS = (556938, 4882986, 607764)
