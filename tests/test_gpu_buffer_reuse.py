"""One world handle, many frames: the device buffers behind it grow, are reused
at a smaller size and are uploaded again under a new version, and every frame
is still the oracle's, byte for byte.

The rest of the suite mostly renders a fresh World per frame, so a buffer that
keeps a stale size, a list left over from the last camera, or a pointer that
means "none" and is not reset would pass it.  Here each of three scenes keeps
one World through four frame sizes (small, large, small again, odd), and at
every size runs every path that owns scratch: the fused resolve with and
without stats, the sample slab (RT_FLAG_KEEP_SAMPLES, then rt_read_samples),
REPLAY from a host table, and SERIAL.  Between sizes the sphere scene switches
its primary lists from the device build to the host build and back, and the
triangle scene does the same for its strip lists and moves its camera, so the
camera records and the lists go into buffers that already exist.  Each scene
ends with an accumulator on the same handle, adaptive and then plain.

A frame rendered without stats is only enqueued, so the last test keeps
frames in flight across camera moves: the camera records and host-built lists
of the next frame must not land in buffers that the frame before still reads."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from conftest import scene_text
from test_gpu_accum import Expect, assert_sums_equal
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order

pytestmark = pytest.mark.gpu

DEPTH = 8
FRAMES = [(16, 12, 2), (64, 48, 4), (16, 12, 1), (33, 17, 3)]  # width, height, spp: in this order

SCENES = {
    "c_raytracer_world": lambda: scene_text("c_raytracer_world.txt"),
    "rtow": S.rtow,
    "triangle_soup": lambda: S.triangle_soup(7, 300, spheres=40, grid=6),
}
# frames (indices into FRAMES) rendered with the host's list builds
HOST_LIST_FRAMES = (1, 2)
HOST_LISTS_ENV = {
    "rtow": {"RT_AMD_GPU_LISTS": "0", "RT_AMD_SYNC_LISTS": "1"},
    "triangle_soup": {"RT_AMD_GPU_TRI_LISTS": "0"},
}
# camera moves before a frame (triangle scene): once under the host lists, once under the device's
CAMERA_MOVES = {2: (0.25, 0.125, -0.5), 3: (-0.5, 0.0, 0.25)}


def _all_paths(world, ref, w, h, spp, what):
    img, ost, _, smp = ref.render(w, h, spp, DEPTH, mode=O.RNG_COUNTER, record_samples=True, nthreads=4)
    simg, sst, states = ref.render(w, h, spp, DEPTH, mode=O.RNG_SERIAL, record_states=True)

    out, st = world.render(w, h, spp, DEPTH)
    assert_bits_equal(out, img, f"{what}: fused resolve, counted")
    assert st["rays"] == ost["rays"] and st["fused_resolve"] == 1, what
    out, st = world.render(w, h, spp, DEPTH, stats=False)
    assert_bits_equal(out, img, f"{what}: fused resolve, no stats")
    assert st is None

    out, st = world.render(w, h, spp, DEPTH, keep_samples=True)
    assert_bits_equal(out, img, f"{what}: slab and resolve kernel")
    assert st["rays"] == ost["rays"] and st["fused_resolve"] == 0, what
    assert_bits_equal(world.read_samples(w * h * spp)[:, :3], oracle_samples_to_gpu_order(smp, w, h, spp)[:, :3],
                      f"{what}: samples read back")

    out, st = world.render(w, h, spp, DEPTH, mode=R.RNG_REPLAY, replay=states)
    assert_bits_equal(out, simg, f"{what}: REPLAY from a host table")
    assert st["rays"] == sst["rays"], what
    out, _ = world.render(w, h, spp, DEPTH, mode=R.RNG_REPLAY, replay=states, stats=False)
    assert_bits_equal(out, simg, f"{what}: REPLAY from a host table, no stats")

    out, st = world.render(w, h, spp, DEPTH, mode=R.RNG_SERIAL)
    assert_bits_equal(out, simg, f"{what}: SERIAL")
    assert st["rays"] == sst["rays"], what
    out, _ = world.render(w, h, spp, DEPTH, mode=R.RNG_SERIAL, stats=False)
    assert_bits_equal(out, simg, f"{what}: SERIAL, no stats")


@pytest.mark.parametrize("name", list(SCENES))
def test_one_handle_through_sizes_paths_and_versions(name, monkeypatch):
    src = SCENES[name]()
    world, ref = R.World(src), O.Scene(src)
    for k, (w, h, spp) in enumerate(FRAMES):
        host_lists = k in HOST_LIST_FRAMES and name in HOST_LISTS_ENV
        for var, val in HOST_LISTS_ENV.get(name, {}).items():
            if host_lists:
                monkeypatch.setenv(var, val)
            else:
                monkeypatch.delenv(var, raising=False)
        if name == "triangle_soup" and k in CAMERA_MOVES:
            world.move_camera(*CAMERA_MOVES[k])
            ref.set_camera(world.camera())
        what = f"{name} frame {k} ({w}x{h}x{spp}{', host lists' if host_lists else ''})"
        _all_paths(world, ref, w, h, spp, what)
        if name == "triangle_soup":
            # (the last launch was a frame's: 1 host build, 2 device build, 0 no lists)
            assert world.primary_tri_lists() == (1 if host_lists else 2), what

    # an accumulator on the same handle: adaptive passes, then the plain fold of 4
    w, h, _ = FRAMES[-1]
    exp = Expect(ref, w, h, 4, DEPTH)
    acc = world.accumulator(w, h, 4, depth=DEPTH)
    acc.set_adaptive()
    for n in (1, 2, 1):
        acc.add(n)
    assert acc.samples == 4
    full = acc.counts() == 4  # (pixels the rule stopped early hold fewer)
    assert_sums_equal(acc.sums()[full], exp.sums(4)[full], f"{name}: adaptive sums after 1 + 2 + 1")
    acc.reset()
    acc.set_adaptive(enable=False)
    out, _ = acc.add(4)
    assert acc.samples == 4
    assert_bits_equal(out, exp.frame(4), f"{name}: accumulated frame of 4")
    assert_sums_equal(acc.sums(), exp.sums(4), f"{name}: sums of one pass of 4")
    acc.close()
    # ... and the handle still renders frames
    w, h, spp = FRAMES[0]
    img, _, _ = ref.render(w, h, spp, DEPTH, mode=O.RNG_COUNTER, nthreads=4)
    assert_bits_equal(world.render(w, h, spp, DEPTH, stats=False)[0], img, f"{name}: a frame after the accumulator")


# ---- frames in flight across camera moves ---------------------------------

MOVES = [None, (0.25, 0.125, -0.5), (-0.5, 0.0, 0.25), (0.25, -0.125, 0.25)]


@pytest.mark.parametrize("name,lists", [("triangle_soup", "device"), ("triangle_soup", "host"), ("rtow", "host")])
def test_frames_in_flight_across_camera_moves(name, lists, monkeypatch):
    """rt_render_device without stats on a non-blocking stream, four frames
    back to back with a camera move before each but the first, one host wait
    at the end: every frame is the oracle's for its own camera."""
    import torch

    if lists == "host":
        for var, val in HOST_LISTS_ENV[name].items():
            monkeypatch.setenv(var, val)
    src = SCENES[name]()
    w, h, spp = 96, 64, 16
    # the cameras and the oracle's frames first, so that the enqueues below follow each other closely
    ref, twin, want = O.Scene(src), R.World(src), []
    for move in MOVES:
        if move:
            twin.move_camera(*move)
        ref.set_camera(twin.camera())
        want.append(ref.render(w, h, spp, DEPTH, mode=O.RNG_COUNTER, nthreads=4)[0])
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    outs = [torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda") for _ in MOVES]
    world = R.World(src)
    torch.cuda.synchronize()
    for move, out in zip(MOVES, outs):
        if move:
            world.move_camera(*move)
        world.render_device(w, h, out.data_ptr(), stream.cuda_stream, spp=spp, depth=DEPTH, device=0, stats=False)
    torch.cuda.synchronize()
    for k, (out, img) in enumerate(zip(outs, want)):
        assert_bits_equal(out.cpu().numpy().reshape(h, w, 4), img, f"{name}, {lists} lists: frame {k} of {len(MOVES)}")
