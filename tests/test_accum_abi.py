"""CPU tests of the progressive-accumulation C-ABI (rt_accum_*,
include/raytracer_amd.h): the symbols are exported and bound, creation rejects
bad arguments with a message before it looks for a device, a machine without
a GPU fails loudly, and a C11 caller compiles against the header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import raytracer_amd as R
from conftest import ROOT, scene_text
from test_abi import declared_functions

INC = os.path.join(ROOT, "include")

ACCUM = ["rt_accum_add", "rt_accum_add_device", "rt_accum_create", "rt_accum_default_options",
         "rt_accum_free", "rt_accum_read", "rt_accum_reset", "rt_accum_samples"]


def _create(world, w, h, **kw):
    """rt_accum_create with the defaults overridden by kw -> (pointer or None, error text)."""
    L = R.lib()
    o = R.AccumOptions()
    L.rt_accum_default_options(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    a = L.rt_accum_create(world.handle if world is not None else None, w, h, C.byref(o))
    return a, R.last_error()


def test_accum_symbols_declared_exported_and_bound():
    names = declared_functions("raytracer_amd.h")
    assert [n for n in names if n.startswith("rt_accum_")] == ACCUM
    lib = C.CDLL(R.LIB_PATH)
    assert not [n for n in ACCUM if not hasattr(lib, n)]
    assert set(ACCUM) <= set(R.EXPORTS)
    assert R.lib().rt_accum_add.argtypes is not None  # prototypes set


def test_accum_default_options():
    o = R.AccumOptions()
    R.lib().rt_accum_default_options(C.byref(o))
    assert (o.max_ray_bounces, o.rng_mode, o.seed) == (8, R.RNG_COUNTER, R.DEFAULT_SEED)
    assert o.sample_stride >= 1 and o.device == -1 and o.accel == R.ACCEL_AUTO and not o.replay_states


def test_accum_create_rejects_bad_arguments_with_a_message():
    world = R.World(scene_text("world.txt"))
    a, err = _create(None, 8, 8)
    assert not a and "null world handle" in err
    a, err = _create(world, 8, 8, sample_stride=0)
    assert not a and "sample_stride" in err
    a, err = _create(world, 8, 8, rng_mode=R.RNG_SERIAL)
    assert not a and "RT_RNG_SERIAL" in err
    a, err = _create(world, 8, 8, rng_mode=R.RNG_REPLAY)
    assert not a and "replay table missing" in err
    a, err = _create(world, 0, 8)
    assert not a and "frame size" in err
    with pytest.raises(R.RenderError, match="sample_stride"):
        world.accumulator(8, 8, 0)
    with pytest.raises(R.RenderError, match="RT_RNG_SERIAL"):
        world.accumulator(8, 8, 4, mode=R.RNG_SERIAL)


def test_accum_calls_on_null_accumulator_fail():
    L = R.lib()
    assert L.rt_accum_add(None, 1, None, None) < 0 and "null accumulator" in R.last_error()
    assert L.rt_accum_add_device(None, 1, None, None, None) < 0
    assert L.rt_accum_samples(None) < 0
    px = np.zeros(3, np.float32)
    assert L.rt_accum_read(None, px.ctypes.data_as(C.POINTER(C.c_float))) < 0
    assert L.rt_accum_reset(None) < 0
    L.rt_accum_free(None)


@pytest.mark.skipif(R.device_count() > 0, reason="a GPU is present")
def test_accum_fails_loudly_without_gpu():
    world = R.World(scene_text("world.txt"))
    with pytest.raises(R.RenderError, match="no HIP device"):
        world.accumulator(8, 8, 4).add(1)


def test_accum_options_layout_and_c11_caller(tmp_path):
    src = tmp_path / "accum.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include "raytracer.h"
#include "raytracer_amd.h"
int main(void) {
  RtAccumOptions o;
  rt_accum_default_options(&o);
  o.sample_stride = 16;
  printf("%zu %zu %zu %zu %zu\n", sizeof(RtAccumOptions), offsetof(RtAccumOptions, replay_states),
         offsetof(RtAccumOptions, sample_stride), offsetof(RtAccumOptions, device),
         offsetof(RtAccumOptions, accel));
  RtAccum *acc = rt_accum_create(NULL, 4, 4, &o);
  if (acc != NULL) return 1;
  Rust_ColorU8 px[16];
  float sums[48];
  RtRenderStats st;
  if (rt_accum_add(acc, 1, px, &st) >= 0) return 2;
  if (rt_accum_add_device(acc, 1, NULL, NULL, NULL) >= 0) return 3;
  if (rt_accum_samples(acc) >= 0 || rt_accum_read(acc, sums) >= 0 || rt_accum_reset(acc) >= 0) return 4;
  rt_accum_free(acc);
  return 0;
}
""")
    exe = tmp_path / "accum"
    libdir = os.path.dirname(R.LIB_PATH)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{INC}", "-o", str(exe), str(src),
                    f"-L{libdir}", "-lraytracer", f"-Wl,-rpath,{libdir}"], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [C.sizeof(R.AccumOptions), R.AccumOptions.replay_states.offset,
                                     R.AccumOptions.sample_stride.offset, R.AccumOptions.device.offset,
                                     R.AccumOptions.accel.offset]
