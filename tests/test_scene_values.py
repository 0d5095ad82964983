"""The oracle at unusual but legal scene values (tests/scene_values.py): the
C++ oracle and the numpy restatement agree on every frame byte and sample bit,
so the expected answer of tests/test_gpu_scene_values.py is well defined; and
the conditions that keep those GPU cases from being empty hold, on the oracle
alone: the edge primitives are visible, NaN occurs but rarely, frames have
content."""
import subprocess

import numpy as np
import pytest

import oracle as O
import pyref as P
import scene_values as V
from test_bvh_host import checker, list_checker  # noqa: F401 (fixtures: the compiled checkers)
from test_bvh_host import run as run_checker

F = np.float32
SOUP_TRIANGLES = 30  # (+ the edge triangles: at most 40, what pyref renders in seconds)


def _pyref_material(kind, rgb, param):
    col = tuple(F(x) for x in rgb) + (F(1.0),)
    return {V.DIFFUSE: ("Diffuse", col), V.METAL: ("Metal", col, F(param)),
            V.DIELECTRIC: ("Dielectric", F(param))}[kind]


@pytest.mark.parametrize("name", V.TABLE_CASES + V.EDIT_CASES)
def test_oracle_matches_numpy_restatement(name):
    case = V.case(name, SOUP_TRIANGLES)
    w, h, spp, depth = 16, 12, 3, 8
    cam, world = P.parse(case.src)
    assert len(world["triangles"]) <= 40
    scene = O.Scene(case.src)
    assert scene.num_spheres == len(world["spheres"]) and scene.num_triangles == len(world["triangles"])
    case.apply_edits(scene)
    for (i, kind, rgb, param) in case.edits:
        c, r, _ = world["spheres"][i]
        world["spheres"][i] = (c, r, _pyref_material(kind, rgb, param))
    ps = np.zeros((w * h * spp, 4), np.float32)
    a = P.ray_trace(world, cam, w, h, spp, depth, samples=ps)
    b, _, _, smp = scene.render(w, h, spp, depth, record_samples=True)
    assert np.array_equal(a, b)
    assert np.array_equal(ps.view(np.uint32), smp.view(np.uint32))


def test_sixty_nines_parse_to_infinity():
    assert np.isposinf(P.dec_to_f32(V.NINES)) and np.isneginf(P.dec_to_f32("-" + V.NINES))
    sph = O.Scene(V.case("nonfinite").src).spheres()[-4:]
    assert np.isposinf(sph[0, 0]) and np.isposinf(sph[1, 3])
    assert np.isfinite(sph[2, 3]) and np.isposinf(sph[2, 3] * sph[2, 3])
    tri = O.Scene(V.case("tri_degenerate").src).triangles()
    assert np.isposinf(tri[:, :9]).sum() == 1


# ---- the conditions on the GPU cases, on the oracle alone ------------------------

_MEMO = {}


def _counter(name):
    """(frame, samples[:, :3]) of the case and samples of its base at the GPU cases' frame."""
    if name not in _MEMO:
        case = V.case(name)
        w, h, spp, depth = V.FRAME
        scene = O.Scene(case.src)
        case.apply_edits(scene)
        img, _, _, smp = scene.render(w, h, spp, depth, mode=O.RNG_COUNTER, nthreads=8, record_samples=True)
        _, _, _, base = O.Scene(case.base).render(w, h, spp, depth, mode=O.RNG_COUNTER, nthreads=8,
                                                  record_samples=True)
        _MEMO[name] = (img, smp[:, :3].copy(), base[:, :3].copy())
    return _MEMO[name]


def _share(mask):
    return float(np.count_nonzero(mask)) / mask.size


@pytest.mark.parametrize("name", V.TABLE_CASES + V.EDIT_CASES)
def test_edge_primitives_are_visible(name):
    img, smp, base = _counter(name)
    nan = np.isnan(smp) & np.isnan(base)
    differ = ((smp.view(np.uint32) != base.view(np.uint32)) & ~nan).any(axis=1)
    print(f"{name}: {100 * _share(differ):.1f} % of the samples differ from the base scene")
    assert _share(differ) >= 0.01


@pytest.mark.parametrize("name", V.TABLE_CASES + V.EDIT_CASES)
def test_frames_have_content(name):
    img, _, _ = _counter(name)
    rgba = np.unique(img.reshape(-1, 4), axis=0)
    assert len(rgba) >= 32, len(rgba)


@pytest.mark.parametrize("name", ["ir", "edit_ir"])
def test_nan_occurs_but_rarely(name):
    _, smp, _ = _counter(name)
    share = _share(np.isnan(smp).any(axis=1))
    print(f"{name}: {100 * share:.1f} % NaN samples")
    assert 0.0 < share <= 0.10


@pytest.mark.parametrize("name", ["fuzz_col", "edit_fuzz_col"])
def test_negative_and_above_one_samples_occur(name):
    _, smp, _ = _counter(name)
    neg, big = _share((smp < 0).any(axis=1)), _share((smp > 1).any(axis=1))
    print(f"{name}: {100 * neg:.1f} % negative, {100 * big:.1f} % above 1")
    assert neg > 0.0 and big > 0.0


# ---- the host-built trees and lists of these scenes (tests/bvh_check.cpp, sphere_list_check.cpp) ----

@pytest.mark.parametrize("leaf", [2, 1])
@pytest.mark.parametrize("name", V.TABLE_CASES)
def test_host_trees_hold_every_primitive(checker, tmp_path, name, leaf):
    case = V.case(name)
    out = run_checker(checker, tmp_path, case.src, leaf, cells=2.5 if case.soup and leaf == 1 else None)
    assert "OK" in out
    nsph = O.Scene(case.src).num_spheres
    # (a tree, not the fallback below 16 tree spheres)
    assert f"spheres {nsph} nodes " in out and f"spheres {nsph} nodes 0" not in out


@pytest.mark.parametrize("move", [None, (0.3, -0.2, -1.0)])
@pytest.mark.parametrize("name", V.SPHERE_CASES)
def test_primary_sphere_lists_cover_every_candidate(list_checker, tmp_path, name, move):
    path = tmp_path / "scene.txt"
    path.write_text(V.case(name).src)
    args = [list_checker, str(path), str(V.FRAME[0]), str(V.FRAME[1])] + ([str(x) for x in move] if move else [])
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


def test_coincident_spheres_lowest_index_wins():
    """The frame of the three coincident balls is the frame of the first alone."""
    case = V.case("coincident")
    lines = case.src.strip("\n").split("\n")
    sph = [i for i, ln in enumerate(lines) if ln.startswith("sphere")]
    first_only = "\n".join(ln for i, ln in enumerate(lines) if i not in sph[-2:]) + "\n"
    assert O.Scene(first_only).num_spheres == O.Scene(case.src).num_spheres - 2
    w, h, spp, depth = V.FRAME
    a, sa, _, sma = O.Scene(case.src).render(w, h, spp, depth, mode=O.RNG_COUNTER, nthreads=8, record_samples=True)
    b, sb, _, smb = O.Scene(first_only).render(w, h, spp, depth, mode=O.RNG_COUNTER, nthreads=8,
                                               record_samples=True)
    assert np.array_equal(a, b) and np.array_equal(sma.view(np.uint32), smb.view(np.uint32))
    assert sa["rays"] == sb["rays"]


def test_big_mix_radii_straddle_the_cut():
    """8 x the median radius, as the tree build takes it (doubles of the f32 radii)."""
    r = np.sort(V.radii(V.case("big_mix").src).astype(np.float64))
    assert len(r) == 62
    cut = 8.0 * r[len(r) // 2]
    assert r[-3] < r[-2] <= cut < r[-1]
    assert cut - r[-2] < 0.001 and r[-1] - cut < 0.001
    # three partitions: RT_AMD_BIG_K=2 keeps both out of the tree, the default one, 1e9 none
    assert np.count_nonzero(r > 2.0 * r[len(r) // 2]) == 2 and np.count_nonzero(r > cut) == 1
