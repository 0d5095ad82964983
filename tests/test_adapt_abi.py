"""CPU tests of the adaptive-accumulation C-ABI (rt_adapt_*,
include/raytracer_amd.h): the symbols are declared, exported
and bound, the defaults are the documented ones, a null accumulator and bad
options fail with a message, and a C11 caller compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np

import raytracer_amd as R
from conftest import ROOT
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

ADAPT = ["rt_adapt_active", "rt_adapt_default_options", "rt_adapt_disable", "rt_adapt_enable",
         "rt_adapt_read_active", "rt_adapt_read_counts", "rt_adapt_read_sumsq"]


def test_adapt_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert sorted(n for n in names if n.startswith("rt_adapt_")) == ADAPT
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in ADAPT if not hasattr(lib, n)]
    assert set(ADAPT) <= set(R.EXPORTS)
    L = R.lib()
    for n in ADAPT:
        assert getattr(L, n).argtypes is not None, n  # prototypes set
    for n in ("set_adaptive", "active", "counts", "sumsq", "active_list"):
        assert hasattr(R.Accumulator, n), n


def test_adapt_default_options():
    o = R.AdaptOptions(1.0, 1.0, 99)
    R.lib().rt_adapt_default_options(C.byref(o))
    assert (o.tolerance, o.bias, o.min_samples) == (np.float32(0.05), np.float32(0.05), 8)


def test_adapt_calls_on_null_accumulator_fail():
    L = R.lib()
    assert L.rt_adapt_enable(None, None) < 0 and "rt_adapt_enable: null accumulator" in R.last_error()
    assert L.rt_adapt_disable(None) < 0 and "rt_adapt_disable: null accumulator" in R.last_error()
    assert L.rt_adapt_active(None) < 0 and "null accumulator" in R.last_error()
    buf = np.zeros(4, np.uint32)
    u32 = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.rt_adapt_read_counts(None, u32) < 0 and "null accumulator" in R.last_error()
    assert L.rt_adapt_read_sumsq(None, buf.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))) < 0
    assert L.rt_adapt_read_active(None, u32, 4) < 0 and "null accumulator" in R.last_error()


def test_adapt_enable_rejects_bad_options_with_a_message():
    """(the options are checked before the accumulator, so no GPU is needed)"""
    L = R.lib()
    for kw, word in (({"tolerance": -0.5}, "tolerance"), ({"tolerance": float("nan")}, "tolerance"),
                     ({"tolerance": float("inf")}, "finite"), ({"bias": -1.0}, "bias"),
                     ({"bias": float("nan")}, "bias"), ({"bias": float("inf")}, "finite"),
                     ({"min_samples": 0}, "min_samples"), ({"min_samples": 1}, "min_samples")):
        o = R.AdaptOptions()
        L.rt_adapt_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        assert L.rt_adapt_enable(None, C.byref(o)) < 0
        err = R.last_error()
        assert "rt_adapt_enable" in err and word in err and "null accumulator" not in err, (kw, err)
    # good options reach the accumulator check
    o = R.AdaptOptions(0.0, 0.0, 2)
    assert L.rt_adapt_enable(None, C.byref(o)) < 0 and "null accumulator" in R.last_error()


def test_adapt_options_layout_and_c11_caller(tmp_path):
    src = tmp_path / "adapt.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtAdaptOptions o;
  rt_adapt_default_options(&o);
  printf("%zu %zu %zu %zu %.9g %.9g %u\n", sizeof(RtAdaptOptions), offsetof(RtAdaptOptions, tolerance),
         offsetof(RtAdaptOptions, bias), offsetof(RtAdaptOptions, min_samples), (double)o.tolerance,
         (double)o.bias, (unsigned)o.min_samples);
  RtAccum *acc = NULL;
  uint32_t u[4];
  float f[4];
  if (rt_adapt_enable(acc, &o) >= 0 || rt_adapt_enable(acc, NULL) >= 0 || rt_adapt_disable(acc) >= 0) return 1;
  if (rt_adapt_active(acc) >= 0 || rt_adapt_read_counts(acc, u) >= 0 || rt_adapt_read_sumsq(acc, f) >= 0) return 2;
  if (rt_adapt_read_active(acc, u, 4) >= 0) return 3;
  o.min_samples = 1;
  if (rt_adapt_enable(acc, &o) >= 0) return 4;
  return 0;
}
""")
    exe = tmp_path / "adapt"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got[:4]] == [C.sizeof(R.AdaptOptions), R.AdaptOptions.tolerance.offset,
                                         R.AdaptOptions.bias.offset, R.AdaptOptions.min_samples.offset]
    assert C.sizeof(R.AdaptOptions) == 12
    assert [np.float32(float(x)) for x in got[4:6]] == [np.float32(0.05)] * 2 and int(got[6]) == 8
