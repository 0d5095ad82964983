"""CPU tests of the temporal reprojection's C-ABI (rt_history_*, include/raytracer_amd.h):
the symbols are declared, exported, listed and bound; the defaults; every
validation rule that needs no accumulator answers with a negative code and a
message naming the call and the argument before any device is looked for; a
machine without a GPU fails loudly; a C11 caller compiles against the header and
sees the ctypes layout.  (An accumulator cannot be created without a GPU: the
rules that need one -- a history that is not enabled, no samples held, a freed
world -- are in test_gpu_history.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

HISTORY = ["rt_history_default_options", "rt_history_disable", "rt_history_enable", "rt_history_read_length",
           "rt_history_reset", "rt_history_resolve", "rt_history_resolve_device", "rt_history_run"]
W, H = 8, 6
F = np.float32


def test_history_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert [n for n in names if n.startswith("rt_history")] == HISTORY
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in HISTORY if not hasattr(lib, n)]
    assert set(HISTORY) <= set(R.EXPORTS)
    for n in HISTORY:
        assert getattr(R.lib(), n).argtypes is not None, n  # prototypes set
    out = subprocess.run(["nm", "-D", "--defined-only", R.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    assert set(HISTORY) <= exported


def test_history_default_options():
    o = R.HistoryOptions(max_history=9.0, sigma_z=9.0)
    R.lib().rt_history_default_options(C.byref(o))
    assert o.max_history == 32.0
    assert np.float32(o.sigma_z) == np.float32(0.02)
    f = R.filter_options()
    assert np.float32(o.sigma_z) == np.float32(f.sigma_z)  # (the filter's default, same meaning)
    p = R.history_options(max_history=4)
    assert (p.max_history, np.float32(p.sigma_z)) == (4.0, np.float32(0.02))
    with pytest.raises(TypeError):
        R.history_options(sigma=1.0)


def _fails(rc, name, word):
    err = R.last_error()
    assert rc < 0, (name, rc)
    assert err.startswith(name + ":") and word in err, (name, err)


def _outputs():
    return np.zeros((H, W, 3), F), np.zeros((H, W, 4), np.uint8)


def test_history_null_accumulator():
    L = R.lib()
    rgb, px = _outputs()
    o = R.history_options()
    _fails(L.rt_history_enable(None, C.byref(o)), "rt_history_enable", "null accumulator")
    _fails(L.rt_history_enable(None, None), "rt_history_enable", "null accumulator")
    _fails(L.rt_history_disable(None), "rt_history_disable", "null accumulator")
    _fails(L.rt_history_reset(None), "rt_history_reset", "null accumulator")
    _fails(L.rt_history_resolve(None, None, rgb.ctypes.data, px.ctypes.data), "rt_history_resolve",
           "null accumulator")
    _fails(L.rt_history_resolve_device(None, None, rgb.ctypes.data, px.ctypes.data, None),
           "rt_history_resolve_device", "null accumulator")
    _fails(L.rt_history_read_length(None, rgb.ctypes.data), "rt_history_read_length", "null accumulator")


def test_history_resolve_outputs_and_filter_options():
    """Both outputs null and the filter's options are a caller's mistake whatever the accumulator."""
    L = R.lib()
    rgb, px = _outputs()
    for name, call in (("rt_history_resolve", lambda f, a, b: L.rt_history_resolve(None, f, a, b)),
                       ("rt_history_resolve_device", lambda f, a, b: L.rt_history_resolve_device(None, f, a, b, None))):
        _fails(call(None, None, None), name, "null output")
        _fails(call(C.byref(R.filter_options()), None, None), name, "null output")
        for field, value in (("levels", 9), ("levels", -1), ("sigma_l", 0.0), ("sigma_l", float("nan")),
                             ("sigma_z", float("inf")), ("sigma_z", -1.0), ("normal_squarings", 9), ("flags", 2)):
            f = R.filter_options()
            setattr(f, field, value)
            _fails(call(C.byref(f), rgb.ctypes.data, px.ctypes.data), name, field)
        # either output alone is enough to get as far as the accumulator
        _fails(call(None, rgb.ctypes.data, None), name, "null accumulator")
        _fails(call(None, None, px.ctypes.data), name, "null accumulator")


BAD_OPTIONS = [("max_history", 0.0), ("max_history", 0.999), ("max_history", -4.0), ("max_history", float("nan")),
               ("max_history", float("inf")),
               ("sigma_z", 0.0), ("sigma_z", -0.02), ("sigma_z", float("nan")), ("sigma_z", float("inf"))]


def _run_args(w=W, h=H):
    return dict(cam=np.zeros(12, F), prgbl=np.zeros((h, w, 4), F), prec=np.zeros((h, w), R.FIRST_HIT_DTYPE),
                rgb=np.zeros((h, w, 3), F), n=np.ones((h, w), np.uint32), rec=np.zeros((h, w), R.FIRST_HIT_DTYPE),
                out=np.zeros((h, w, 4), F))


def _run(o, w=W, h=H, **none):
    a = _run_args()
    p = {k: (None if none.get(k) else v.ctypes.data) for k, v in a.items()}
    return R.lib().rt_history_run(w, h, C.byref(o) if o is not None else None, p["cam"], p["prgbl"], p["prec"],
                                  p["rgb"], p["n"], p["rec"], p["out"], -1)


@pytest.mark.parametrize("field,value", BAD_OPTIONS)
def test_history_option_ranges(field, value):
    o = R.history_options()
    setattr(o, field, value)
    _fails(R.lib().rt_history_enable(None, C.byref(o)), "rt_history_enable", field)  # (before the accumulator)
    _fails(_run(o), "rt_history_run", field)


def test_history_run_arguments():
    o = R.history_options()
    for w, h in ((0, 8), (8, 0), (1 << 16, 1 << 15), (1 << 40, 1 << 40), (1 << 33, 1 << 31)):
        _fails(_run(o, w, h), "rt_history_run", "size")  # (checked before anything is read)
    _fails(_run(o, cam=True), "rt_history_run", "prev_cam")
    _fails(_run(o, prec=True), "rt_history_run", "prev_records")
    _fails(_run(o, rgb=True), "rt_history_run", "rgb")
    _fails(_run(o, n=True), "rt_history_run", "null input: n")
    _fails(_run(o, rec=True), "rt_history_run", "records")
    _fails(_run(o, out=True), "rt_history_run", "out_rgbl")
    with pytest.raises(ValueError):
        R.history_run(np.zeros((H, W, 3), F), np.ones((H, W - 1), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE))
    with pytest.raises(R.RenderError, match="max_history"):
        R.history_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE),
                      max_history=0.5)


def test_history_option_range_ends_pass_validation():
    """The ends of the ranges are legal: such a call gets as far as the device."""
    for kw in (dict(max_history=1.0), dict(max_history=3.4028234663852886e38), dict(sigma_z=1e-45),
               dict(sigma_z=3.4028234663852886e38), None):
        o = R.history_options(**kw) if kw is not None else None
        for none in (dict(), dict(prgbl=True), dict(prgbl=True, cam=True, prec=True)):  # (prev may be absent)
            rc = _run(o, **none)
            err = R.last_error()
            if R.device_count() > 0:
                assert rc == 0, (kw, err)
            else:
                assert rc < 0 and "no HIP device" in err, (kw, err)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_history_fails_loudly_without_gpu():
    rc = _run(None)
    err = R.last_error()
    assert rc < 0 and "no HIP device" in err and err.startswith("rt_history_run:"), (rc, err)
    with pytest.raises(R.RenderError, match="no HIP device"):
        R.history_run(np.zeros((H, W, 3), F), np.ones((H, W), np.uint32), np.zeros((H, W), R.FIRST_HIT_DTYPE))


def test_history_layout_and_c11_caller(tmp_path):
    src = tmp_path / "history.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtHistoryOptions o;
  rt_history_default_options(&o);
  printf("%zu %zu %zu\n", sizeof(RtHistoryOptions), offsetof(RtHistoryOptions, max_history),
         offsetof(RtHistoryOptions, sigma_z));
  if (o.max_history != 32.0f || o.sigma_z != 0.02f) return 1;
  float rgb[4 * 4 * 3] = {0}, rgbl[4 * 4 * 4] = {0}, cam[12] = {0};
  uint32_t n[16] = {0};
  RtFirstHit rec[16];
  Rust_ColorU8 px[16];
  if (rt_history_enable(NULL, &o) >= 0) return 2;
  if (rt_history_disable(NULL) >= 0) return 3;
  if (rt_history_reset(NULL) >= 0) return 4;
  if (rt_history_resolve(NULL, NULL, rgb, px) >= 0) return 5;
  if (rt_history_resolve_device(NULL, NULL, rgb, px, NULL) >= 0) return 6;
  if (rt_history_read_length(NULL, rgb) >= 0) return 7;
  if (rt_history_run(0, 4, &o, cam, rgbl, rec, rgb, n, rec, rgbl, -1) >= 0) return 8;
  o.max_history = 0.5f;
  if (rt_history_run(4, 4, &o, cam, rgbl, rec, rgb, n, rec, rgbl, -1) >= 0) return 9;
  return 0;
}
""")
    exe = tmp_path / "history"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    O = R.HistoryOptions
    assert [int(x) for x in got] == [C.sizeof(O), O.max_history.offset, O.sigma_z.offset]
