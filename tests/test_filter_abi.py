"""CPU tests of the edge-aware filter's C-ABI (rt_filter_*, include/raytracer_amd.h):
the symbols are declared, exported, listed and bound; the defaults; every
validation rule answers with a negative code and a message naming the call and
the argument before any device is looked for; a machine without a GPU fails
loudly; a C11 caller compiles against the header and sees the ctypes layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

FILTER = ["rt_filter_accum", "rt_filter_accum_device", "rt_filter_create", "rt_filter_default_options",
          "rt_filter_free", "rt_filter_run", "rt_filter_run_device"]
W, H = 8, 6


def test_filter_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert [n for n in names if n.startswith("rt_filter")] == FILTER
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in FILTER if not hasattr(lib, n)]
    assert set(FILTER) <= set(R.EXPORTS)
    for n in FILTER:
        assert getattr(R.lib(), n).argtypes is not None, n  # prototypes set
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(FILTER) <= exported


def test_filter_default_options():
    o = R.FilterOptions(levels=9, sigma_l=9.0, sigma_z=9.0, normal_squarings=9, flags=9)
    R.lib().rt_filter_default_options(C.byref(o))
    assert (o.levels, o.sigma_l, o.normal_squarings, o.flags) == (3, 0.5, 5, 0)
    assert np.float32(o.sigma_z) == np.float32(0.02)
    assert R.FILTER_SAME_PRIM == 1
    p = R.filter_options(levels=2, same_prim=True)
    assert (p.levels, p.flags, p.sigma_l) == (2, 1, 0.5)


@pytest.fixture(scope="module")
def flt():
    f = R.Filter(W, H)
    yield f
    f.close()


def _buffers():
    return (np.zeros((H, W, 3), np.float32), np.zeros((H, W), R.FIRST_HIT_DTYPE), np.zeros((H, W, 3), np.float32),
            np.zeros((H, W, 4), np.uint8))


def _run_calls(f, o, rgb=True, rec=True, out=(True, True)):
    """(name, return code, message) of both run entry points on the same arguments
    (host pointers stand in for device memory: validation fails before anything reads them)."""
    L = R.lib()
    c, g, oc, op = _buffers()
    po = C.byref(o) if o is not None else None
    args = (c.ctypes.data if rgb else None, g.ctypes.data if rec else None, oc.ctypes.data if out[0] else None,
            op.ctypes.data if out[1] else None)
    res = []
    rc = L.rt_filter_run(f, po, *args)
    res.append(("rt_filter_run", rc, R.last_error()))
    rc = L.rt_filter_run_device(f, po, *args, None)
    res.append(("rt_filter_run_device", rc, R.last_error()))
    return res


def _accum_calls(acc, o, out=(True, True)):
    L = R.lib()
    _, _, oc, op = _buffers()
    po = C.byref(o) if o is not None else None
    args = (oc.ctypes.data if out[0] else None, op.ctypes.data if out[1] else None)
    res = []
    rc = L.rt_filter_accum(acc, po, *args)
    res.append(("rt_filter_accum", rc, R.last_error()))
    rc = L.rt_filter_accum_device(acc, po, *args, None)
    res.append(("rt_filter_accum_device", rc, R.last_error()))
    return res


def _all_fail(res, word):
    assert res
    for name, rc, err in res:
        assert rc < 0, (name, rc)
        assert word in err and err.startswith(name + ":"), (name, err)


def test_filter_create_rejects_sizes():
    L = R.lib()
    for w, h in ((0, 8), (8, 0), (1 << 16, 1 << 15), (1 << 40, 1 << 40), (1 << 33, 1 << 31)):
        assert not L.rt_filter_create(w, h, -1), (w, h)
        err = R.last_error()
        assert err.startswith("rt_filter_create:") and "size" in err, err
    with pytest.raises(R.RenderError, match="size"):
        R.Filter(0, 4)
    f = L.rt_filter_create((1 << 31) - 1, 1, -1)  # (the largest image: nothing is allocated yet)
    assert f
    L.rt_filter_free(f)
    L.rt_filter_free(None)


def test_filter_null_arguments(flt):
    o = R.filter_options()
    _all_fail(_run_calls(None, o), "null filter")
    _all_fail(_run_calls(flt._f, o, rgb=False), "rgb")
    _all_fail(_run_calls(flt._f, o, rgb=False), "null input")
    _all_fail(_run_calls(flt._f, o, rec=False), "records")
    _all_fail(_run_calls(flt._f, o, rec=False), "null input")
    _all_fail(_run_calls(flt._f, o, out=(False, False)), "null output")
    _all_fail(_run_calls(flt._f, None, out=(False, False)), "null output")  # (opts NULL = the defaults)
    _all_fail(_accum_calls(None, o), "null accumulator")


BAD_OPTIONS = [("levels", -1), ("levels", 9), ("levels", 1 << 30),
               ("sigma_l", 0.0), ("sigma_l", -1.0), ("sigma_l", float("nan")), ("sigma_l", float("inf")),
               ("sigma_z", 0.0), ("sigma_z", -0.02), ("sigma_z", float("nan")), ("sigma_z", float("inf")),
               ("normal_squarings", -1), ("normal_squarings", 9),
               ("flags", 2), ("flags", 3), ("flags", 1 << 31)]


@pytest.mark.parametrize("field,value", BAD_OPTIONS)
def test_filter_option_ranges(flt, field, value):
    o = R.filter_options()
    setattr(o, field, value)
    _all_fail(_run_calls(flt._f, o), field)


def test_filter_option_range_ends_pass_validation(flt):
    """The ends of the ranges are legal: such a call gets as far as the device."""
    c, g, oc, op = _buffers()
    for kw in (dict(levels=0), dict(levels=8), dict(normal_squarings=0), dict(normal_squarings=8),
               dict(flags=1), dict(sigma_l=1e-45), dict(sigma_z=3.4028234663852886e38)):
        o = R.filter_options(**kw)
        # (the host entry only: the device entry would read these host pointers on a GPU machine)
        rc = R.lib().rt_filter_run(flt._f, C.byref(o), c.ctypes.data, g.ctypes.data, oc.ctypes.data, op.ctypes.data)
        err = R.last_error()
        if R.device_count() > 0:
            assert rc == 0, (kw, err)
        else:
            assert rc < 0 and "no HIP device" in err, (kw, err)


def test_filter_python_wrappers_raise(flt):
    c, g, _, _ = _buffers()
    with pytest.raises(R.RenderError, match="levels"):
        flt.run(c, g, levels=9)
    with pytest.raises(R.RenderError, match="null output"):
        flt.run(c, g, want_rgb=False, want_rgba=False)
    with pytest.raises(TypeError):
        flt.run(c, g, sigma=1.0)
    with pytest.raises(ValueError):
        flt.run(c[:2], g)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_filter_fails_loudly_without_gpu(flt):
    c, g, oc, op = _buffers()
    L = R.lib()
    f = L.rt_filter_create(W, H, -1)  # (creating needs no device ...)
    assert f
    rc = L.rt_filter_run(f, None, c.ctypes.data, g.ctypes.data, oc.ctypes.data, op.ctypes.data)
    err = R.last_error()
    L.rt_filter_free(f)
    assert rc < 0 and "no HIP device" in err and err.startswith("rt_filter_run:"), (rc, err)  # (... running does)
    with pytest.raises(R.RenderError, match="no HIP device"):
        flt.run(c, g)


def test_filter_layout_and_c11_caller(tmp_path):
    src = tmp_path / "filter.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtFilterOptions o;
  rt_filter_default_options(&o);
  printf("%zu %zu %zu %zu %zu %zu %d %d %u\n", sizeof(RtFilterOptions), offsetof(RtFilterOptions, levels),
         offsetof(RtFilterOptions, sigma_l), offsetof(RtFilterOptions, sigma_z),
         offsetof(RtFilterOptions, normal_squarings), offsetof(RtFilterOptions, flags), (int)o.levels,
         (int)o.normal_squarings, (unsigned)o.flags);
  if (o.sigma_l != 0.5f || o.sigma_z != 0.02f) return 1;
  if (RT_FILTER_SAME_PRIM != 1) return 2;
  float rgb[4 * 4 * 3] = {0};
  RtFirstHit rec[16];
  Rust_ColorU8 px[16];
  if (rt_filter_create(0, 4, -1) != NULL) return 3;
  RtFilter *f = rt_filter_create(4, 4, -1);
  if (!f) return 4;
  if (rt_filter_run(NULL, &o, rgb, rec, rgb, px) >= 0) return 5;
  if (rt_filter_run(f, &o, rgb, rec, NULL, NULL) >= 0) return 6;
  if (rt_filter_run_device(f, NULL, NULL, rec, rgb, px, NULL) >= 0) return 7;
  if (rt_filter_accum(NULL, &o, rgb, px) >= 0) return 8;
  if (rt_filter_accum_device(NULL, NULL, rgb, px, NULL) >= 0) return 9;
  rt_filter_free(f);
  return 0;
}
""")
    exe = tmp_path / "filter"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    F = R.FilterOptions
    assert [int(x) for x in got] == [C.sizeof(F), F.levels.offset, F.sigma_l.offset, F.sigma_z.offset,
                                     F.normal_squarings.offset, F.flags.offset, 3, 5, 0]
