"""CPU tests of bench.py's --gpus handling (no GPU needed).

The driver runs `python bench.py --gpus N` (one process drives N GPUs through
the library's multi-device mode) and `torch.distributed.run --nproc-per-node N
bench.py --gpus N` (one rank per GPU).  A rank count that differs from --gpus,
or more GPUs than are visible, must stop the bench before any GPU work instead
of silently timing fewer GPUs.
"""
import os
import subprocess
import sys

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True,
                          timeout=300)


def test_launcher_rank_count_must_equal_gpus():
    r = _run(["--gpus", "2", "--steps", "1"], {"WORLD_SIZE": "3", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 2 but the launcher started 3 ranks" in r.stderr


def test_more_gpus_than_visible_is_refused():
    import raytracer_amd as R

    n = R.device_count() + 1
    r = _run(["--gpus", str(n), "--steps", "1"], {})
    assert r.returncode != 0
    assert f"--gpus {n} but only" in r.stderr


def test_gpus_must_be_positive():
    r = _run(["--gpus", "0"], {})
    assert r.returncode != 0 and "--gpus must be >= 1" in r.stderr


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_spp_and_depth_override_the_config():
    """--spp / --depth (and the reference CLI's samples= / ray_depth=,
    main.rs:23-45) replace the config's spp and depth; the defaults keep the
    config's, so the driver's bench line is unchanged."""
    b = _bench_module()
    _, W, H, spp, depth = b.workload(b.parse_args([]))
    assert (W, H, spp, depth) == (1920, 1080, 64, 8)
    _, W, H, spp, depth = b.workload(b.parse_args(["--spp", "16", "--depth", "4"]))
    assert (W, H, spp, depth) == (1920, 1080, 16, 4)
    _, _, _, spp, depth = b.workload(b.parse_args(["--config", "c3", "--depth", "5"]))
    assert (spp, depth) == (256, 5)
    # the reference's argument syntax: leading digits only (parser.rs:90-104)
    _, _, _, spp, depth = b.workload(b.parse_args(["samples=32", "ray_depth=3x"]))
    assert (spp, depth) == (32, 3)


def test_plain_run_is_the_default_and_full_is_an_option():
    b = _bench_module()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = b.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    r = _run(["--steps", "0"], {})
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_writes_the_frame_or_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: the RGBA8 frame as float32 [rows, W, 4]; a frame over the
    byte budget as the same seeded pixel sample on every call, within the budget."""
    import numpy as np
    import torch

    b = _bench_module()
    w, h = 37, 11
    px = np.random.default_rng(5).integers(0, 256, h * w * 4, dtype=np.uint8)
    frame = torch.from_numpy(np.concatenate([px, np.zeros(64, np.uint8)]))  # (a longer buffer)
    b.dump_outputs(str(tmp_path / "a"), frame, w, h)
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and got.shape == (h, w, 4)
    assert np.array_equal(got, px.reshape(h, w, 4).astype(np.float32))
    assert b.DUMP_MAX_BYTES == 64 << 20
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 100 * 16)
    b.dump_outputs(str(tmp_path / "b"), frame, w, h)
    b.dump_outputs(str(tmp_path / "c"), frame, w, h)
    s1, s2 = np.load(tmp_path / "b" / "frame.npy"), np.load(tmp_path / "c" / "frame.npy")
    assert s1.dtype == np.float32 and s1.shape == (100, 4) and s1.nbytes <= 100 * 16
    assert np.array_equal(s1, s2)
    # every sampled pixel is a pixel of the frame, in ascending pixel order
    rows = px.reshape(h * w, 4).astype(np.float32)
    pos = 0
    for p in s1:
        while not np.array_equal(rows[pos], p):
            pos += 1
        pos += 1


def test_bad_spp_and_reference_args_are_refused():
    r = _run(["--spp", "0"], {})
    assert r.returncode != 0 and "--spp must be >= 1" in r.stderr
    r = _run(["samples=abc"], {})
    assert r.returncode != 0 and "cannot parse 'samples=abc'" in r.stderr
    r = _run(["ray_depth=99999999999"], {})
    assert r.returncode != 0 and "cannot parse" in r.stderr
