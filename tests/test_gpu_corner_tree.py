"""The LDS sphere tree as octant corner records (bvh.h SphereBVH::corner,
sphere_search.h sphere_node_corner): sphere-only frame kernels walk them when the
image fits a workgroup's LDS share, everything else keeps the box records.
The layout changes work per node, never a sample: every comparison is
bit-exact, and the BVH counters equal the box records' (the same nodes in the
same order with the same skip decisions).  RtRenderStats::sphere_tree says
what a frame walked: 0 none, 1 global, 2 LDS box records, 3 LDS corner records."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order, render_kept

pytestmark = pytest.mark.gpu

TREE_GLOBAL, TREE_BOX, TREE_CORNER = 1, 2, 3


def _random_scene(seed, n, spread, radius, offset=(0.0, 0.0, 0.0), dup=0, big=True, cam=(0.0, 0.0, 0.0)):
    """(shaped like test_gpu_parity's: a cluster in front of the camera, an
    optional ground sphere kept out of the tree, exact duplicates)"""
    rng = np.random.default_rng(seed)
    kinds = ["Diffuse color 0.7 0.5 0.3", "Metal color 0.9 0.8 0.7 fuzz 0.05",
             "Dielectric ir 1.5", "Metal color 0.6 0.6 0.9 fuzz 0.0"]
    lines = [f"camera origin {cam[0]:.6f} {cam[1]:.6f} {cam[2]:.6f} aspect 1.5;"]
    lines += [f"material K{i} : {k};" for i, k in enumerate(kinds)]
    sph = []
    if big:
        sph.append((offset[0], offset[1] - 1000.0, offset[2], 999.0, 0))
    for _ in range(n):
        c = rng.uniform(-spread, spread, 3) + np.array(offset) + np.array([0, 0, -spread - 2])
        sph.append((c[0], c[1], c[2], radius * rng.uniform(0.3, 1.0), int(rng.integers(0, 4))))
    sph += sph[1:1 + dup]  # exact duplicates: equal t, the lower index must win
    for (x, y, z, r, k) in sph:
        lines.append(f"sphere center {x:.6f} {y:.6f} {z:.6f} radius {r:.6f} material K{k};")
    return "\n".join(lines) + "\n"


def _brute(world, w, h, spp, depth=8):
    out, st = world.render(w, h, spp, depth, accel=R.ACCEL_BRUTE, keep_samples=True)
    assert st["accel"] == R.ACCEL_BRUTE and st["sphere_tree"] == 0
    return out, st, world.read_samples(w * h * spp)


def test_rtow_corner_records_equal_brute_force_oracle_and_box_records(monkeypatch):
    src = S.rtow()
    w, h, spp, depth = 64, 36, 4, 8
    world = R.World(src)
    ref, rst, ref_s = _brute(world, w, h, spp, depth)
    img, ost, _, smp = O.Scene(src).render(w, h, spp, depth, mode=O.RNG_COUNTER, nthreads=8,
                                           record_samples=True)
    lean, _ = world.render(w, h, spp, depth, stats=False)
    assert_bits_equal(lean, ref, "lean corner frame vs brute force")
    assert_bits_equal(lean, img, "lean corner frame vs the oracle's COUNTER frame")
    out, st = render_kept(world, w, h, spp, depth)  # (counting, lean and kept-samples frames agree)
    assert st["sphere_tree"] == TREE_CORNER and st["accel"] == R.ACCEL_BVH
    assert 0 < st["sphere_tree_lds_bytes"] <= 81920
    assert_bits_equal(out, ref, "counting corner frame vs brute force")
    smp_c = world.read_samples(w * h * spp)
    assert_bits_equal(smp_c, ref_s, "kept samples vs brute force")
    assert_bits_equal(smp_c[:, :3], oracle_samples_to_gpu_order(smp, w, h, spp)[:, :3], "kept samples vs oracle")
    assert st["rays"] == rst["rays"] == ost["rays"]
    # the box records: a fresh world with the layout forced off
    monkeypatch.setenv("RT_AMD_CORNER", "0")
    box = R.World(src)
    bout, bst = render_kept(box, w, h, spp, depth)
    assert bst["sphere_tree"] == TREE_BOX
    assert_bits_equal(bout, out, "box-record frame vs corner-record frame")
    assert_bits_equal(box.read_samples(w * h * spp), smp_c, "box-record samples vs corner-record samples")
    for key in ("bvh_node_tests", "bvh_sphere_tests", "rays"):
        assert bst[key] == st[key], (key, bst[key], st[key])
    assert st["bvh_node_tests"] > 0 and st["bvh_sphere_tests"] > 0


@pytest.mark.parametrize("case", [
    dict(seed=1, n=400, spread=6.0, radius=0.3),
    dict(seed=2, n=300, spread=3.0, radius=0.6, dup=40),
    dict(seed=4, n=200, spread=5.0, radius=0.4, offset=(3000.0, -2000.0, 1500.0),
         cam=(3000.0, -2000.0, 1500.0)),
    dict(seed=5, n=250, spread=2.0, radius=0.5, big=False, cam=(0.0, 0.0, -4.0)),
])
def test_random_scenes_corner_records_equal_brute_force(case):
    world = R.World(_random_scene(**case))
    w, h, spp = 96, 64, 8
    ref, rst, ref_s = _brute(world, w, h, spp)
    out, st = render_kept(world, w, h, spp, 8)  # counting == lean == kept
    assert st["sphere_tree"] == TREE_CORNER
    assert_bits_equal(out, ref, "corner frames vs brute force")
    assert_bits_equal(world.read_samples(w * h * spp), ref_s, "samples")
    assert st["rays"] == rst["rays"]


def test_tree_too_large_for_corner_records_keeps_another_layout():
    """n=500 at leaf size 2: the 128-B records do not fit a workgroup's share."""
    world = R.World(_random_scene(seed=3, n=500, spread=20.0, radius=0.05))
    w, h, spp = 96, 64, 8
    ref, rst, ref_s = _brute(world, w, h, spp)
    out, st = render_kept(world, w, h, spp, 8)
    assert st["sphere_tree"] in (TREE_GLOBAL, TREE_BOX)
    assert_bits_equal(out, ref, "frames vs brute force")
    assert_bits_equal(world.read_samples(w * h * spp), ref_s, "samples")
    assert st["rays"] == rst["rays"]


def test_rtow_camera_inside_the_sphere_field():
    """Primary candidate lists and walks mixed in one frame."""
    world = R.World(S.rtow())
    world.move_camera(0.5, -1.5, -9.0)
    w, h, spp = 80, 60, 4
    ref, _, _ = _brute(world, w, h, spp)
    lean, _ = world.render(w, h, spp, 8, stats=False)
    assert_bits_equal(lean, ref, "lean frame after the move vs brute force")
    _, st = world.render(w, h, spp, 8)
    assert st["sphere_tree"] == TREE_CORNER


def test_mesh_scene_keeps_the_box_records(monkeypatch):
    src = S.triangle_soup(41, 400, spheres=40)
    w, h, spp = 48, 27, 2
    out, st = render_kept(R.World(src), w, h, spp, 8)
    assert st["sphere_tree"] != TREE_CORNER and st["sphere_tree"] != 0
    monkeypatch.setenv("RT_AMD_CORNER", "0")
    off, ost = render_kept(R.World(src), w, h, spp, 8)
    assert_bits_equal(off, out, "mesh frame with and without RT_AMD_CORNER=0")
    assert ost["sphere_tree"] == st["sphere_tree"] and ost["rays"] == st["rays"]
    ref, rst = R.World(src).render(w, h, spp, 8, accel=R.ACCEL_BRUTE)
    assert_bits_equal(out, ref, "mesh frame vs brute force")
