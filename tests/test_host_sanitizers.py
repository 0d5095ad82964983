"""AddressSanitizer + UndefinedBehaviorSanitizer run of the host side
(SURVEY.md 5): the scene parser (csrc/scene.cpp, parser.rs:54-381 grammar with
hand-decoded UTF-8) and the BVH / primary-list builders (csrc/bvh.cpp) under
tests/host_fuzz.cpp -- the committed scenes, ~byte-level mutations of them
(bit flips, insertions, truncations, splices, malformed UTF-8) and random
scenes with degenerate, duplicate, huge and non-finite geometry.  Any
sanitizer report (including float->int casts out of range) fails the test."""
import os
import subprocess

import pytest

import scenes as S
from conftest import ROOT

CSRC = os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc")
SCENES = [os.path.join(ROOT, "scenes", n) for n in
          ("world.txt", "c_raytracer_world.txt", "three_spheres.txt", "rtow.txt")]


def test_parser_and_builders_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "host_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", f"-I{CSRC}", os.path.join(ROOT, "tests", "host_fuzz.cpp"),
                    os.path.join(CSRC, "bvh.cpp"), os.path.join(CSRC, "scene.cpp"), "-o", exe],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for seed in (1, 2):
        r = subprocess.run([exe, "10", str(seed)] + SCENES, capture_output=True, text=True,
                           timeout=300, env=env)
        assert r.returncode == 0, r.stdout + r.stderr[-4000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        counts = dict(zip(r.stdout.split()[::2], map(int, r.stdout.split()[1::2])))
        assert counts["parsed"] > 1000 and counts["triangles"] > 1000


def test_builder_thread_pools_under_tsan(tmp_path):
    """ThreadSanitizer run of the host builders' thread pools: the pooled subtree
    build of a large tree (csrc/bvh.cpp Builder::build_root) and the two pools of
    the per-origin-cell trees (build_triangle_cells: the cells' trees, then their
    quantisation).  tests/bvh_check.cpp with csrc/bvh.cpp and csrc/scene.cpp is
    built with -fsanitize=thread and run as a program of its own, so the
    structural checks run on the trees the racing threads would have spoiled.
    The list build behind std::async in csrc/primary_lists.cpp needs the HIP
    headers and a device and is not part of this run."""
    workers = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    if workers < 2:  # (std::thread::hardware_concurrency() == 1: no pool starts)
        pytest.skip("one hardware thread: the builders start no thread pool here")
    exe = str(tmp_path / "bvh_check_tsan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-pthread", f"-I{CSRC}",
                    os.path.join(ROOT, "tests", "bvh_check.cpp"), os.path.join(CSRC, "bvh.cpp"),
                    os.path.join(CSRC, "scene.cpp"), "-o", exe], check=True)
    cases = [("mesh", S.mesh(nx=100, ny=80), ["2"], "triangles 16000 tree 16000"),
             ("soup", S.triangle_soup(seed=13, n=300, spheres=200, grid=12), ["1", "1.3"], "cells ")]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1")
    for name, text, args, expect in cases:
        path = tmp_path / f"{name}.txt"
        path.write_text(text)
        r = subprocess.run([exe, str(path)] + args, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout}{r.stderr[-4000:]}"
        assert "OK" in r.stdout and expect in r.stdout, f"{name}: {r.stdout}"
        assert "ThreadSanitizer" not in r.stderr, f"{name}:\n{r.stderr[-4000:]}"
