"""CPU tests of the first-hit C-ABI (rt_first_hit_*, include/raytracer_amd.h):
the symbols are declared, exported, listed and bound; the record is 32 bytes in
C, ctypes and numpy alike; every validation rule answers with a negative code
and a message naming the argument before any device is looked for; a machine
without a GPU fails loudly; a C11 caller compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT, scene_text
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

FIRST_HIT = ["rt_first_hit", "rt_first_hit_default_options", "rt_first_hit_device", "rt_first_hit_pick",
             "rt_first_hit_view", "rt_first_hit_view_device"]


@pytest.fixture(scope="module")
def world():
    return R.World(scene_text("world.txt"))


def _opts(**kw):
    o = R.FirstHitOptions()
    R.lib().rt_first_hit_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _calls(world, w, h, o, out=True, view=R.VIEW_NORMAL, col=0, row=0, which=None):
    """(name, return code, message) of every entry point on the same arguments
    (host buffers of 64 x 64 pixels; out=False: a null output)."""
    L = R.lib()
    hd = world.handle if world is not None else None
    rec = np.zeros(64 * 64, R.FIRST_HIT_DTYPE)
    px = np.zeros((64 * 64, 4), np.uint8)
    one = R.RtFirstHit()
    po = C.byref(o) if o is not None else None
    calls = {
        "rt_first_hit": lambda: L.rt_first_hit(hd, w, h, po, rec.ctypes.data if out else None),
        # (a host pointer stands in for device memory: validation fails before anything reads it)
        "rt_first_hit_device": lambda: L.rt_first_hit_device(hd, w, h, po, rec.ctypes.data if out else None, None),
        "rt_first_hit_pick": lambda: L.rt_first_hit_pick(hd, w, h, col, row, po, C.byref(one) if out else None),
        "rt_first_hit_view": lambda: L.rt_first_hit_view(
            hd, w, h, po, view, px.ctypes.data_as(C.POINTER(R.ColorU8)) if out else None),
        "rt_first_hit_view_device": lambda: L.rt_first_hit_view_device(
            hd, w, h, po, view, px.ctypes.data if out else None, None),
    }
    res = []
    for name, f in calls.items():
        if which is None or name in which:
            rc = f()
            res.append((name, rc, R.last_error()))
    return res


def _all_fail(res, word):
    assert res
    for name, rc, err in res:
        assert rc < 0, (name, rc)
        assert word in err and name in err, (name, err)


RECT_CALLS = ("rt_first_hit", "rt_first_hit_device", "rt_first_hit_view", "rt_first_hit_view_device")
VIEW_CALLS = ("rt_first_hit_view", "rt_first_hit_view_device")


def test_first_hit_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert [n for n in names if n.startswith("rt_first_hit")] == FIRST_HIT
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in FIRST_HIT if not hasattr(lib, n)]
    assert set(FIRST_HIT) <= set(R.EXPORTS)
    for n in FIRST_HIT:
        assert getattr(R.lib(), n).argtypes is not None, n  # prototypes set


def test_first_hit_record_is_32_bytes_everywhere():
    assert C.sizeof(R.RtFirstHit) == 32
    dt = R.FIRST_HIT_DTYPE
    assert dt.itemsize == 32
    for name in ("prim", "t", "normal", "position"):
        assert dt.fields[name][1] == getattr(R.RtFirstHit, name).offset, name
    assert [dt.fields[n][1] for n in ("prim", "t", "normal", "position")] == [0, 4, 8, 20]
    assert dt["prim"] == np.uint32 and dt["t"] == np.float32
    assert dt["normal"].shape == (3,) and dt["position"].shape == (3,)


def test_first_hit_default_options():
    o = R.FirstHitOptions(su=9.0, sv=9.0, x0=1, y0=2, w=3, h=4, device=5, accel=6)
    R.lib().rt_first_hit_default_options(C.byref(o))
    assert (o.su, o.sv) == (0.5, 0.5)
    assert (o.x0, o.y0, o.w, o.h) == (0, 0, 0, 0)
    assert o.device == -1 and o.accel == R.ACCEL_AUTO
    assert (R.VIEW_NORMAL, R.VIEW_DEPTH, R.VIEW_ALBEDO, R.VIEW_PRIM) == (0, 1, 2, 3)


def test_first_hit_null_handle_and_null_output(world):
    _all_fail(_calls(None, 8, 8, _opts()), "null world handle")
    _all_fail(_calls(world, 8, 8, _opts(), out=False), "null output")
    _all_fail(_calls(world, 8, 8, None, out=False), "null output")  # (opts NULL = the defaults)


def test_first_hit_frame_size(world):
    _all_fail(_calls(world, 0, 8, _opts()), "frame size")
    _all_fail(_calls(world, 8, 0, _opts()), "frame size")
    _all_fail(_calls(world, 1 << 16, 1 << 15, _opts()), "frame size")  # width * height == 2^31
    _all_fail(_calls(world, 1 << 40, 1 << 40, _opts()), "frame size")  # (a product that wraps to 0 in 64 bits ...)
    _all_fail(_calls(world, 1 << 33, 1 << 31, _opts()), "frame size")  # (... and one that wraps exactly)


def test_first_hit_rectangle(world):
    for rect in ((0, 0, 9, 1), (0, 0, 1, 9), (8, 0, 1, 1), (0, 8, 1, 1), (4, 4, 5, 1), (4, 4, 1, 5),
                 (0xFFFFFFFF, 0, 2, 1), (0, 0xFFFFFFFF, 1, 2)):
        o = _opts(x0=rect[0], y0=rect[1], w=rect[2], h=rect[3])
        _all_fail(_calls(world, 8, 8, o, which=RECT_CALLS), "rectangle")
    for rect in ((0, 0, 0, 3), (0, 0, 3, 0), (1, 1, 0, 0), (1, 0, 0, 0)):
        o = _opts(x0=rect[0], y0=rect[1], w=rect[2], h=rect[3])
        _all_fail(_calls(world, 8, 8, o, which=RECT_CALLS), "rectangle")


def test_first_hit_offsets(world):
    for bad in (1.0, -0.25, float("nan"), float("inf"), float(np.nextafter(np.float32(0), np.float32(-1)))):
        _all_fail(_calls(world, 8, 8, _opts(su=bad)), "su")
        _all_fail(_calls(world, 8, 8, _opts(sv=bad)), "sv")


def test_first_hit_unknown_view_and_accel(world):
    for view in (-1, 4, 1 << 20):
        _all_fail(_calls(world, 8, 8, _opts(), view=view, which=VIEW_CALLS), "view")
    for accel in (-1, 3):
        _all_fail(_calls(world, 8, 8, _opts(accel=accel)), "accel")


def test_first_hit_pick_outside_the_frame(world):
    for col, row in ((8, 0), (0, 6), (1 << 40, 0), (0, 1 << 40)):
        _all_fail(_calls(world, 8, 6, _opts(), col=col, row=row, which=("rt_first_hit_pick",)), "pick")
    # the rectangle in opts is ignored by a pick: a bad one is no error of its own
    (_, rc, err), = _calls(world, 8, 6, _opts(x0=100, w=0, h=7), col=8, row=0, which=("rt_first_hit_pick",))
    assert rc < 0 and "pick" in err and "rectangle" not in err


def test_first_hit_python_wrappers_raise(world):
    with pytest.raises(R.RenderError, match="su"):
        world.first_hit(8, 8, su=1.0)
    with pytest.raises(R.RenderError, match="rectangle"):
        world.first_hit(8, 8, rect=(4, 4, 8, 8))
    with pytest.raises(R.RenderError, match="pick"):
        world.pick(8, 8, 8, 8)
    with pytest.raises(R.RenderError, match="view"):
        world.first_hit_view(8, 8, 7)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_first_hit_fails_loudly_without_gpu(world):
    for name, rc, err in _calls(world, 8, 8, _opts()):
        assert rc < 0 and "no HIP device" in err, (name, rc, err)
    with pytest.raises(R.RenderError, match="no HIP device"):
        world.first_hit(8, 8)
    with pytest.raises(R.RenderError, match="no HIP device"):
        world.pick(8, 8, 3, 3)
    with pytest.raises(R.RenderError, match="no HIP device"):
        world.first_hit_view(8, 8, R.VIEW_PRIM)


def test_first_hit_layout_and_c11_caller(tmp_path):
    src = tmp_path / "first_hit.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
_Static_assert(sizeof(RtFirstHit) == 32, "RtFirstHit");
_Static_assert(offsetof(RtFirstHit, t) == 4 && offsetof(RtFirstHit, normal) == 8 &&
               offsetof(RtFirstHit, position) == 20, "RtFirstHit fields");
int main(void) {
  RtFirstHitOptions o;
  rt_first_hit_default_options(&o);
  printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(RtFirstHitOptions), offsetof(RtFirstHitOptions, x0),
         offsetof(RtFirstHitOptions, h), offsetof(RtFirstHitOptions, device),
         offsetof(RtFirstHitOptions, accel), o.device, o.accel);
  if (o.su != 0.5f || o.sv != 0.5f || o.x0 || o.y0 || o.w || o.h) return 1;
  RtFirstHit rec[16];
  Rust_ColorU8 px[16];
  if (rt_first_hit(NULL, 4, 4, &o, rec) >= 0) return 2;
  if (rt_first_hit_device(NULL, 4, 4, NULL, rec, NULL) >= 0) return 3;
  if (rt_first_hit_pick(NULL, 4, 4, 1, 2, &o, rec) >= 0) return 4;
  if (rt_first_hit_view(NULL, 4, 4, &o, RT_VIEW_NORMAL, px) >= 0) return 5;
  if (rt_first_hit_view_device(NULL, 4, 4, &o, RT_VIEW_PRIM, px, NULL) >= 0) return 6;
  if (RT_VIEW_DEPTH != 1 || RT_VIEW_ALBEDO != 2) return 7;
  return 0;
}
""")
    exe = tmp_path / "first_hit"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    F = R.FirstHitOptions
    assert [int(x) for x in got] == [C.sizeof(F), F.x0.offset, F.h.offset, F.device.offset, F.accel.offset,
                                     -1, R.ACCEL_AUTO]
