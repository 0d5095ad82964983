"""CPU tests of the geometry edit's C-ABI (rt_world_set_sphere_geometry;
include/raytracer_amd.h): the symbol is declared, exported, listed and bound; the
edit works without a GPU and reads back through rt_world_sphere; every rejected
argument answers with a negative code and a message naming the call; a C11 caller
compiles against the header.  And of rt_move_run's, the moved-sphere resolve on host
arrays: its arguments are checked, rt_clamp_run's and the two tables', before any
device is looked for, and a machine without a GPU fails loudly under its name."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT, scene_text
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")
NEW = ["rt_device_setups", "rt_move_run", "rt_world_set_sphere_geometry"]
W, H = 8, 6
F = np.float32
INF = float("inf")


def test_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert set(NEW) <= set(names)
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in NEW if not hasattr(lib, n)]
    assert set(NEW) <= set(R.EXPORTS)
    for n in NEW:
        assert getattr(R.lib(), n).argtypes is not None, n
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(NEW) <= exported
    # the version script exports the rt_ family as a whole
    with open(os.path.join(ROOT, "rust-swift-raytracer_amd", "csrc", "exports.map")) as fh:
        assert "rt_*;" in fh.read()


def _fails(rc, name, word):
    err = R.last_error()
    assert rc < 0, (name, rc)
    assert err.startswith(name + ":") and word in err, (name, err)


def test_edit_without_a_gpu_reads_back():
    w = R.World(scene_text("three_spheres.txt"))
    before = w.spheres()
    for g in ((0.25, -0.125, -2.0, 0.75), (0.0, 0.0, -1.0, -0.5), (1.0, 2.0, 3.0, 0.0), (INF, 0.0, -INF, INF),
              (-0.0, 1e-40, 3e38, 1e-45)):
        w.set_sphere(1, g[:3], g[3])
        after = w.spheres()
        assert after[1, :4].tobytes() == np.array(g, F).tobytes()
        assert after[1, 4:].tobytes() == before[1, 4:].tobytes()      # the material stays
        assert np.delete(after, 1, 0).tobytes() == np.delete(before, 1, 0).tobytes()  # and every other sphere
    assert w.num_spheres == 4
    # a material edit and a geometry edit of the same sphere keep each other's half
    w.set_material(1, 1, (0.1, 0.2, 0.3), 0.4)
    w.set_sphere(1, (0.5, 0.5, -1.5), 0.25)
    assert w.spheres()[1].tobytes() == np.array([0.5, 0.5, -1.5, 0.25, 1, 0.1, 0.2, 0.3, 1.0, 0.4], F).tobytes()
    w.close()


def test_rejected_edits():
    L = R.lib()
    w = R.World(scene_text("three_spheres.txt"))
    before = w.spheres()
    g = np.array([0.0, 0.0, -1.0, 0.5], F)
    name = "rt_world_set_sphere_geometry"
    _fails(L.rt_world_set_sphere_geometry(None, 0, R._fp(g)), name, "null world handle")
    _fails(L.rt_world_set_sphere_geometry(w.handle, 0, None), name, "geometry")
    _fails(L.rt_world_set_sphere_geometry(w.handle, 4, R._fp(g)), name, "out of range")
    _fails(L.rt_world_set_sphere_geometry(w.handle, 1 << 40, R._fp(g)), name, "out of range")
    for k in range(4):
        bad = g.copy()
        bad[k] = np.nan
        _fails(L.rt_world_set_sphere_geometry(w.handle, 1, R._fp(bad)), name, "NaN")
        with pytest.raises(ValueError, match="NaN"):
            w.set_sphere(1, bad[:3], bad[3])
    with pytest.raises(ValueError, match="out of range"):
        w.set_sphere(4, (0, 0, 0), 1.0)
    assert w.spheres().tobytes() == before.tobytes()  # a refused edit changes nothing
    w.close()


def test_device_setups_without_a_device():
    w = R.World(scene_text("three_spheres.txt"))
    assert w.device_setups() == 0
    w.set_sphere(1, (0.0, 0.0, -1.5), 0.5)
    w.set_material(1, 0, (0.1, 0.2, 0.3))
    assert w.device_setups() == 0  # an edit sets nothing up
    _fails(R.lib().rt_device_setups(None), "rt_device_setups", "null argument")
    w.close()


def _run_args(ns=3):
    return dict(cam=np.zeros(12, F), prgbl=np.zeros((H, W, 4), F), prec=np.zeros((H, W), R.FIRST_HIT_DTYPE),
                rgb=np.zeros((H, W, 3), F), n=np.ones((H, W), np.uint32), rec=np.zeros((H, W), R.FIRST_HIT_DTYPE),
                out=np.zeros((H, W, 4), F), box=np.zeros((H, W, 6), F), s0=np.ones((ns, 4), F),
                s1=np.full((ns, 4), 2, F))


def _run(c=None, w=W, h=H, o=None, ns=3, **none):
    """rt_move_run with whole arguments but those named in none, which are NULL."""
    a = _run_args(max(min(ns, 3), 1))
    p = {k: (None if none.get(k) else v.ctypes.data) for k, v in a.items()}
    return R.lib().rt_move_run(w, h, C.byref(o) if o is not None else None, C.byref(c) if c is not None else None,
                               p["cam"], p["prgbl"], p["prec"], p["rgb"], p["n"], p["rec"], p["out"], p["box"],
                               p["s0"], p["s1"], ns, -1)


def test_move_run_arguments():
    name = "rt_move_run"
    # history_run_check under this entry's name: rt_clamp_run's rejections
    for w, h in ((0, 8), (8, 0), (1 << 16, 1 << 15), (1 << 40, 1 << 40), (1 << 33, 1 << 31)):
        _fails(_run(w=w, h=h), name, "size")
    _fails(_run(o=R.history_options(max_history=0.5)), name, "max_history")
    _fails(_run(o=R.history_options(sigma_z=0.0)), name, "sigma_z")
    for field, value in (("gamma", -1.0), ("gamma", float("nan")), ("gamma", INF), ("radius", 0), ("radius", 4),
                         ("flags", 2)):
        c = R.clamp_options()
        setattr(c, field, value)
        _fails(_run(c), name, field)
    _fails(_run(cam=True), name, "prev_cam")
    _fails(_run(prec=True), name, "prev_records")
    _fails(_run(rgb=True), name, "null input: rgb")
    _fails(_run(n=True), name, "null input: n")
    _fails(_run(rec=True), name, "null input: records")
    _fails(_run(out=True), name, "out_rgbl")
    # the tables: NULL with nspheres > 0 names the argument; nspheres below 2^32
    _fails(_run(s0=True), name, "null input: prev_spheres")
    _fails(_run(s1=True), name, "null input: spheres")
    _fails(_run(s0=True, s1=True), name, "prev_spheres")
    _fails(_run(ns=1, s1=True), name, "null input: spheres")
    for ns in (1 << 32, (1 << 32) + 1, 1 << 40, (1 << 64) - 1):
        _fails(_run(ns=ns), name, "nspheres")
        _fails(_run(ns=ns, s0=True, s1=True), name, "nspheres")
    # the order: the image and the options before the tables
    _fails(_run(w=0, s0=True), name, "size")
    _fails(_run(rgb=True, s0=True), name, "rgb")
    # the binding's own checks
    rgb, n, rec = np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE)
    with pytest.raises(ValueError, match="nspheres x 4"):
        R.move_run(rgb, n, rec, np.zeros((3, 4), F), np.zeros((2, 4), F))
    with pytest.raises(ValueError, match="nspheres x 4"):
        R.move_run(rgb, n, rec, np.zeros((3, 4), F), None)
    with pytest.raises(ValueError, match="nspheres x 4"):
        R.move_run(rgb, n, rec, np.zeros(6, F), np.zeros(6, F))
    with pytest.raises(ValueError):
        R.move_run(rgb, n[:, 1:], rec, None, None)
    with pytest.raises(R.RenderError, match="rt_move_run: radius"):
        R.move_run(rgb, n, rec, None, None, clamp=dict(radius=4))


def test_move_run_legal_arguments_get_as_far_as_the_device():
    """NULL tables with nspheres 0, whole tables with nspheres 0, a NULL box and an absent
    prev are legal: such a call gets as far as the device."""
    for kw in (dict(), dict(ns=0), dict(ns=0, s0=True, s1=True), dict(box=True), dict(prgbl=True),
               dict(prgbl=True, cam=True, prec=True), dict(ns=1)):
        rc = _run(**kw)
        err = R.last_error()
        if R.device_count() > 0:
            assert rc == 0, (kw, err)
        else:
            assert rc < 0 and "no HIP device" in err and err.startswith("rt_move_run:"), (kw, err)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_move_run_fails_loudly_without_gpu():
    rc = _run()
    err = R.last_error()
    assert rc < 0 and "no HIP device" in err and err.startswith("rt_move_run:"), (rc, err)
    nan = np.full((2, 4), np.nan, F)
    with pytest.raises(R.RenderError, match="rt_move_run: .*no HIP device"):
        R.move_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE), nan, nan)


def test_move_run_c11_caller(tmp_path):
    src = tmp_path / "move_run.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtClampOptions c;
  RtHistoryOptions o;
  rt_clamp_default_options(&c);
  rt_history_default_options(&o);
  float rgb[4 * 4 * 3] = {0}, rgbl[4 * 4 * 4] = {0}, box[4 * 4 * 6] = {0}, cam[12] = {0};
  const float was[2 * 4] = {0.0f, 0.0f, -1.0f, 0.5f, 1.0f, 0.0f, -1.0f, 0.25f};
  const float now[2 * 4] = {0.1f, 0.0f, -1.0f, 0.5f, 1.0f, 0.0f, -1.0f, 0.5f};
  uint32_t n[16] = {0};
  RtFirstHit rec[16];
  memset(rec, 0, sizeof rec);
  if (rt_move_run(0, 4, &o, &c, cam, rgbl, rec, rgb, n, rec, rgbl, box, was, now, 2, -1) >= 0) return 1;
  if (rt_move_run(4, 4, &o, &c, cam, rgbl, rec, rgb, n, rec, rgbl, box, NULL, now, 2, -1) >= 0) return 2;
  if (!strstr(rt_last_error(), "prev_spheres")) return 3;
  if (rt_move_run(4, 4, NULL, NULL, cam, rgbl, rec, rgb, n, rec, rgbl, NULL, was, NULL, 2, -1) >= 0) return 4;
  if (sizeof(size_t) == 8 &&
      rt_move_run(4, 4, &o, &c, cam, rgbl, rec, rgb, n, rec, rgbl, box, was, now, (size_t)1 << 32, -1) >= 0)
    return 5;
  c.radius = 4;
  if (rt_move_run(4, 4, &o, &c, NULL, NULL, NULL, rgb, n, rec, rgbl, box, NULL, NULL, 0, -1) >= 0) return 6;
  printf("%s\n", rt_last_error());
  return 0;
}
""")
    exe = tmp_path / "move_run"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert got.startswith("rt_move_run: radius")


def test_c11_caller(tmp_path):
    src = tmp_path / "move.c"
    src.write_text(r"""
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  Rust_WorldHandle *h = load_world(
      "camera origin 0.0 0.0 0.0 aspect 1.5;\n"
      "material M : Diffuse color 0.5 0.5 0.5;\n"
      "sphere center 0.0 0.0 -1.0 radius 0.5 material M;\n");
  if (!h) return 1;
  const float g[4] = {0.25f, 0.5f, -2.0f, -0.75f}, bad[4] = {0.0f, NAN, 0.0f, 1.0f};
  float out[10];
  if (rt_world_set_sphere_geometry(h, 0, g) != 0) return 2;
  if (rt_world_sphere(h, 0, out) != 0 || out[0] != g[0] || out[1] != g[1] || out[2] != g[2] || out[3] != g[3]) return 3;
  if (out[4] != 0.0f || out[5] != 0.5f) return 4;
  if (rt_world_set_sphere_geometry(h, 1, g) >= 0) return 5;
  if (rt_world_set_sphere_geometry(h, 0, bad) >= 0) return 6;
  if (rt_world_set_sphere_geometry(h, 0, NULL) >= 0) return 7;
  if (rt_world_set_sphere_geometry(NULL, 0, g) >= 0) return 8;
  printf("%s\n", rt_last_error());
  rt_free_world(h);
  return 0;
}
""")
    exe = tmp_path / "move"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}", "-lm"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert got.startswith("rt_world_set_sphere_geometry: null world handle")
