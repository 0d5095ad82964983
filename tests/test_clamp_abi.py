"""CPU tests of the history clamp's C-ABI (rt_clamp_*, include/raytracer_amd.h): the
symbols are declared, exported, listed and bound; the defaults; every validation
rule that needs no accumulator answers with a negative code and a message naming
the call and the argument before any device is looked for; a machine without a
GPU fails loudly; a C11 caller compiles against the header and sees the ctypes
layout.  (The rules that need an accumulator are in test_gpu_clamp.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

CLAMP = ["rt_clamp_default_options", "rt_clamp_disable", "rt_clamp_enable", "rt_clamp_run"]
W, H = 8, 6
F = np.float32
FLT_MAX = 3.4028234663852886e38


def test_clamp_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert [n for n in names if n.startswith("rt_clamp")] == CLAMP
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in CLAMP if not hasattr(lib, n)]
    assert set(CLAMP) <= set(R.EXPORTS)
    for n in CLAMP:
        assert getattr(R.lib(), n).argtypes is not None, n  # prototypes set
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(CLAMP) <= exported


def test_clamp_default_options():
    o = R.ClampOptions(gamma=9.0, radius=9, flags=9)
    R.lib().rt_clamp_default_options(C.byref(o))
    assert (o.gamma, o.radius, o.flags) == (1.5, 1, 0)
    p = R.clamp_options(gamma=2, radius=3)
    assert (p.gamma, p.radius, p.flags) == (2.0, 3, 0)
    assert R.clamp_options(keep_on_edit=True).flags == R.CLAMP_KEEP_ON_EDIT == 1
    assert R.clamp_options(flags=R.CLAMP_KEEP_ON_EDIT).flags == 1
    with pytest.raises(TypeError):
        R.clamp_options(sigma=1.0)


def _fails(rc, name, word):
    err = R.last_error()
    assert rc < 0, (name, rc)
    assert err.startswith(name + ":") and word in err, (name, err)


def test_clamp_null_accumulator():
    L = R.lib()
    o = R.clamp_options()
    _fails(L.rt_clamp_enable(None, C.byref(o)), "rt_clamp_enable", "null accumulator")
    _fails(L.rt_clamp_enable(None, None), "rt_clamp_enable", "null accumulator")
    _fails(L.rt_clamp_disable(None), "rt_clamp_disable", "null accumulator")


def _run_args(w=W, h=H):
    return dict(cam=np.zeros(12, F), prgbl=np.zeros((h, w, 4), F), prec=np.zeros((h, w), R.FIRST_HIT_DTYPE),
                rgb=np.zeros((h, w, 3), F), n=np.ones((h, w), np.uint32), rec=np.zeros((h, w), R.FIRST_HIT_DTYPE),
                out=np.zeros((h, w, 4), F), box=np.zeros((h, w, 6), F))


def _run(c, w=W, h=H, o=None, **none):
    a = _run_args()
    p = {k: (None if none.get(k) else v.ctypes.data) for k, v in a.items()}
    return R.lib().rt_clamp_run(w, h, C.byref(o) if o is not None else None, C.byref(c) if c is not None else None,
                                p["cam"], p["prgbl"], p["prec"], p["rgb"], p["n"], p["rec"], p["out"], p["box"], -1)


BAD_OPTIONS = [("gamma", -1.0), ("gamma", -1e-45), ("gamma", float("nan")), ("gamma", float("inf")),
               ("radius", 0), ("radius", 4), ("radius", -1),
               ("flags", 2), ("flags", 3), ("flags", 0x80000000)]


@pytest.mark.parametrize("field,value", BAD_OPTIONS)
def test_clamp_option_ranges(field, value):
    c = R.clamp_options()
    setattr(c, field, value)
    _fails(R.lib().rt_clamp_enable(None, C.byref(c)), "rt_clamp_enable", field)  # (before the accumulator)
    _fails(_run(c), "rt_clamp_run", field)


def test_clamp_run_arguments():
    c = R.clamp_options()
    for w, h in ((0, 8), (8, 0), (1 << 16, 1 << 15), (1 << 40, 1 << 40), (1 << 33, 1 << 31)):
        _fails(_run(c, w, h), "rt_clamp_run", "size")  # (checked before anything is read)
    _fails(_run(c, o=R.history_options(max_history=0.5)), "rt_clamp_run", "max_history")
    _fails(_run(c, o=R.history_options(sigma_z=0.0)), "rt_clamp_run", "sigma_z")
    _fails(_run(c, cam=True), "rt_clamp_run", "prev_cam")
    _fails(_run(c, prec=True), "rt_clamp_run", "prev_records")
    _fails(_run(c, rgb=True), "rt_clamp_run", "rgb")
    _fails(_run(c, n=True), "rt_clamp_run", "null input: n")
    _fails(_run(c, rec=True), "rt_clamp_run", "records")
    _fails(_run(c, out=True), "rt_clamp_run", "out_rgbl")
    with pytest.raises(ValueError):
        R.clamp_run(np.zeros((H, W, 3), F), np.ones((H, W - 1), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE))
    with pytest.raises(R.RenderError, match="radius"):
        R.clamp_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE),
                    clamp=dict(radius=4))
    with pytest.raises(TypeError):
        R.clamp_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE),
                    clamp=dict(sigma=1))


def test_clamp_option_range_ends_pass_validation():
    """The ends of the ranges are legal, a null box and an absent prev too: such a call gets as far as the device."""
    for kw in (dict(gamma=0.0), dict(gamma=FLT_MAX), dict(radius=1), dict(radius=3), dict(keep_on_edit=True), None):
        c = R.clamp_options(**kw) if kw is not None else None
        for none in (dict(), dict(box=True), dict(prgbl=True), dict(prgbl=True, cam=True, prec=True)):
            rc = _run(c, **none)
            err = R.last_error()
            if R.device_count() > 0:
                assert rc == 0, (kw, err)
            else:
                assert rc < 0 and "no HIP device" in err, (kw, err)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_clamp_fails_loudly_without_gpu():
    rc = _run(None)
    err = R.last_error()
    assert rc < 0 and "no HIP device" in err and err.startswith("rt_clamp_run:"), (rc, err)
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.clamp_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE))


def test_clamp_layout_and_c11_caller(tmp_path):
    src = tmp_path / "clamp.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtClampOptions c;
  RtHistoryOptions o;
  rt_clamp_default_options(&c);
  rt_history_default_options(&o);
  printf("%zu %zu %zu %zu %zu\n", sizeof(RtClampOptions), offsetof(RtClampOptions, gamma),
         offsetof(RtClampOptions, radius), offsetof(RtClampOptions, flags), sizeof(RtHistoryOptions));
  if (c.gamma != 1.5f || c.radius != 1 || c.flags != 0 || RT_CLAMP_KEEP_ON_EDIT != 1) return 1;
  float rgb[4 * 4 * 3] = {0}, rgbl[4 * 4 * 4] = {0}, box[4 * 4 * 6] = {0}, cam[12] = {0};
  uint32_t n[16] = {0};
  RtFirstHit rec[16];
  if (rt_clamp_enable(NULL, &c) >= 0) return 2;
  if (rt_clamp_enable(NULL, NULL) >= 0) return 3;
  if (rt_clamp_disable(NULL) >= 0) return 4;
  if (rt_clamp_run(0, 4, &o, &c, cam, rgbl, rec, rgb, n, rec, rgbl, box, -1) >= 0) return 5;
  c.radius = 4;
  if (rt_clamp_run(4, 4, &o, &c, cam, rgbl, rec, rgb, n, rec, rgbl, NULL, -1) >= 0) return 6;
  c.radius = 1;
  c.flags = 2;
  if (rt_clamp_run(4, 4, NULL, &c, cam, rgbl, rec, rgb, n, rec, rgbl, box, -1) >= 0) return 7;
  return 0;
}
""")
    exe = tmp_path / "clamp"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    O = R.ClampOptions
    assert [int(x) for x in got] == [C.sizeof(O), O.gamma.offset, O.radius.offset, O.flags.offset,
                                     C.sizeof(R.HistoryOptions)]
    assert C.sizeof(R.HistoryOptions) == 8  # RtHistoryOptions keeps its layout
