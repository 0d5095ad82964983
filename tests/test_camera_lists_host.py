"""Host check of the primary-ray list builders under oriented cameras (no GPU):
tests/camera_list_check.cpp compiled with g++ against csrc/bvh.cpp +
csrc/scene.cpp.  For every camera of tests/camera_cases.py, at 48 x 32 and at
50 x 30 (a partial last strip), every tree sphere with a candidate root is on
its pixel's list (or the pixel walks) and every camera-origin record whose
padded box a primary ray meets is on the pixel's strip list or on `always`.
Mirrored (det > 0) and singular (det = 0) cameras get no lists."""
import os
import subprocess

import numpy as np
import pytest

import camera_cases as CC
import scene_values as V
import scenes as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc")
SIZES = [(48, 32), (50, 30)]
SCENES = {"rtow": (S.rtow, CC.RTOW), "field": (V.field, CC.FIELD), "soup": (V.soup, CC.SOUP)}
CASES = [(s, c) for s, (_, tab) in SCENES.items() for c in tab]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("camlists")
    exe = str(d / "camera_list_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "camera_list_check.cpp"), os.path.join(CSRC, "bvh.cpp"),
                    os.path.join(CSRC, "scene.cpp"), "-o", exe], check=True)
    paths = {}
    for name, (src, _) in SCENES.items():
        paths[name] = str(d / f"{name}.txt")
        with open(paths[name], "w") as fh:
            fh.write(src())
    return exe, paths


def run(checker, scene, w, h, cam):
    exe, paths = checker
    bits = [f"{b:08x}" for b in np.asarray(cam, np.float32).view(np.uint32)]
    res = subprocess.run([exe, paths[scene], str(w), str(h)] + bits, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("spheres ") and lines[1].startswith("triangles ")
    return lines


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene,name", CASES)
def test_lists_cover_every_candidate(checker, scene, name, w, h):
    cam = CC.camera(SCENES[scene][1], name)
    assert CC.det(cam) < 0  # what every constructor gives
    sph, tri = run(checker, scene, w, h, cam)
    print(f"{scene}/{name} {w}x{h}: {sph}; {tri}")
    assert sph.startswith("spheres OK") or sph == "spheres no lists"
    if scene == "soup":  # 300 triangles: a tree, and a regular camera has lists
        assert tri.startswith("triangles OK")
        assert " rays %d " % (w * h * 8) in tri
    else:
        assert tri == "triangles no tree"


def test_some_oriented_camera_lists_and_some_walks(checker):
    """The cases are not all of one kind: the book's view lists every pixel's
    candidates, a ball across the camera plane makes every pixel walk, and the
    soup's `inside` camera has `always` records."""
    sph, _ = run(checker, "rtow", 48, 32, CC.camera(CC.RTOW, "book"))
    assert sph.startswith("spheres OK") and int(sph.split("candidates ")[1].split()[0]) > 0
    sph, _ = run(checker, "field", 48, 32, CC.camera(CC.FIELD, "inside"))
    assert sph == "spheres no lists"
    _, tri = run(checker, "soup", 48, 32, CC.camera(CC.SOUP, "inside"))
    assert int(tri.split("always ")[1]) > 0 and int(tri.split("met ")[1].split()[0]) > 0


def test_the_gpu_list_cases_are_what_they_claim(checker, tmp_path):
    """The scenes of tests/test_gpu_tri_lists.py, on the host build that the device
    build must reproduce: the spliced soup has a record on every strip and
    `always` records under the scene's own camera, and the camera behind the
    soup has lists whose offsets are all 0."""
    exe, paths = checker
    paths["spliced"] = str(tmp_path / "spliced.txt")
    with open(paths["spliced"], "w") as fh:
        fh.write(CC.spliced_soup())
    default = CC.new_at((0, 0, 0), CC.ASPECT)
    _, plain = run(checker, "soup", 48, 32, default)
    _, tri = run(checker, "spliced", 48, 32, default)
    assert tri.startswith("triangles OK") and int(tri.split("always ")[1]) > int(plain.split("always ")[1])
    # (the spanning triangle alone adds one item to each of the 6 x 32 strips)
    listed = [int(t.split("listed ")[1].split()[0]) for t in (plain, tri)]
    assert listed[1] >= listed[0] + 6 * 32
    o, t, up, deg = CC.ALL_BEHIND
    _, tri = run(checker, "soup", 48, 32, CC.look_at(o, t, up, CC.radians(deg)))
    assert tri.startswith("triangles OK") and " listed 0 always 0" in tri


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("kind", ["mirrored", "singular"])
def test_mirrored_and_singular_cameras_get_no_lists(checker, scene, kind):
    base = CC.camera(SCENES[scene][1], "roll")
    cam = getattr(CC, kind)(base)
    assert CC.det(cam) > 0 if kind == "mirrored" else CC.det(cam) == 0
    sph, tri = run(checker, scene, 48, 32, cam)
    assert sph == "spheres no lists"
    assert tri == ("triangles no lists" if scene == "soup" else "triangles no tree")
