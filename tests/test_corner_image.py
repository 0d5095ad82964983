"""The sphere tree's corner records (bvh.h SphereBVH::corner, no GPU):
tests/corner_image_check.cpp compiled with g++ against csrc/bvh.cpp +
csrc/scene.cpp.  Every slot is its octant's near corner (and the opposite
octant's far corner), links and leaf words decode to the tree's, and a host
emulation of the kernel's corner step walks the same nodes with the same skip
decisions as an emulation of the box step, for rays that include +-0 and
< 1e-20 direction components and origins inside leaf boxes.  -ffp-contract=off:
the emulations' mul / add / fmaf stay the operations the kernel runs.  The
sanitizer leg runs the same program built with -fsanitize=address,undefined."""
import os
import subprocess

import pytest

import scenes as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc")


def _build(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "corner_image_check.cpp"), os.path.join(CSRC, "bvh.cpp"),
                    os.path.join(CSRC, "scene.cpp"), "-pthread", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("corner") / "corner_image_check"))


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
    return r.stdout


def test_rtow_corner_image(checker, tmp_path):
    """The C2 / C3 scene: the image matches the tree, both steps walk alike, and
    image + prims + ids fit the 81,920 B of a lean sphere workgroup."""
    path = tmp_path / "rtow.txt"
    path.write_text(S.rtow())
    out = _run(checker, str(path), "budget")
    assert "nodes 555 prims 485" in out


def test_random_corner_images(checker):
    """20-480 spheres: exact duplicates, no big sphere, a set at (3000, -2000, 1500)."""
    assert "trees 6" in _run(checker, "--random")


def test_corner_image_check_under_sanitizers(tmp_path):
    exe = _build(str(tmp_path / "corner_image_check_san"),
                 ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    path = tmp_path / "rtow.txt"
    path.write_text(S.rtow())
    _run(exe, str(path), "budget")
