"""The forked sky kernel (DESIGN.md 5.3b, 4 "Stream ordering"): a frame with sky
rows and a trace launch runs sky_rows_kernel on the device's side stream, behind
a fork point on the frame's stream and beside the trace launches, and the frame's
stream waits for it before the frame's end is recorded.  Nothing a sample
computes changes: every comparison is on raw RGBA8 bytes.

Expected bytes.  Small frames: the brute-force kernel and the counting frame
(neither has sky rows), as tests/test_gpu_sky_rows.py takes them.  Heavy frames
(4096 samples, which keep the GPU busy while the host enqueues behind them): the
solo render -- the same request rendered synchronously on a fresh World under
RT_AMD_SKY_FORK=0 with nothing else in flight, the method of
tests/test_gpu_streams.py.

World.sky_forked() (rt_sky_forked) says whether the last frame launch forked: a
case that means to fork asserts 1 on the frame it checks, a case that must not
asserts 0.  A camera's sky rows are known once its first frame is enqueued
(classify_pending_sky_rows), so a frame meant to fork follows a priming frame
of the same camera and size, which traces every row.

The ordering cases enqueue on non-blocking torch streams with no host wait
between the calls, and assert the "in flight" witness of test_gpu_streams.py
where the case depends on it: an event behind the earlier work has not completed
when the later call returns.  JOIN_* is sized by measurement
(profiles/sky_fork/times.txt): its sky kernel ends well after its trace launch,
so a copy enqueued behind a frame that did not join reads unfinished sky rows
(seen once with the join taken out of a local build: the case fails on bytes).
"""
import math

import numpy as np
import pytest

import camera_cases as CC
import raytracer_amd as R
import scenes as S
import test_gpu_first_hit as FH
from test_gpu_corner_tree import _brute
from test_gpu_parity import assert_bits_equal
from test_gpu_sky_rows import _expect, _rtow_with
from test_gpu_streams import B as ONE_SAMPLE
from test_gpu_streams import as_frame, assert_in_flight, enqueue, frame_buf, gpu, mark, memo, oracle_frame, source

pytestmark = pytest.mark.gpu

# the cameras of test_gpu_sky_rows.py's test_cameras
CAMS = {
    "up": lambda wd: wd.look_at((0, 2, 13), (0, 3, 14), CC.Y, float(CC.radians(50)), 1.5),
    "down": lambda wd: wd.look_at((0, 6, 0.5), (0, 0, 0), CC.Y, float(CC.radians(50)), 1.5),
    "roll": lambda wd: wd.look_at((0, 2, 13), (0, 2, 0), (1, 1, 0), float(CC.radians(60)), 1.5),
    "fov": lambda wd: wd.vertical_fov((0, 2, 13), float(CC.radians(50)), 1.5),
}
HEAVY = dict(spp=4096, depth=8)      # a frame that outlasts the host calls behind it (profiles/streams/times.txt)
H_W, H_H = 480, 270
LIGHT = dict(spp=4, depth=8)
# the join case: tilted up until only the last rows are traced (profiles/sky_fork/times.txt)
JOIN_W, JOIN_H, JOIN_SPP, JOIN_PITCH, JOIN_ROWS = 480, 270, 4096, 23.5, 268


def tilt_up(pitch_deg):
    """The rtow camera's place, looking over the field at pitch_deg above the horizontal."""
    ty = 2.0 + 13.0 * math.tan(math.radians(pitch_deg))
    return lambda wd: wd.look_at((0, 2, 13), (0, ty, 0), CC.Y, float(CC.radians(50)), 1.5)


def solo_off(monkeypatch, key, make_world, w, h, spp, depth):
    """The solo render under RT_AMD_SKY_FORK=0, once per request."""
    def make():
        monkeypatch.setenv("RT_AMD_SKY_FORK", "0")
        world = make_world()
        out, _ = world.render(w, h, spp, depth, device=0, stats=False)
        assert world.sky_forked() == 0
        world.close()
        monkeypatch.delenv("RT_AMD_SKY_FORK")
        return out
    return memo(("solo off", key, w, h, spp, depth), make)


def primed(make_world, w, h, out, stream_ptr=0, **frame):
    """A world whose next frame of this size has its sky rows: one frame rendered, the device idle."""
    import torch

    world = make_world()
    enqueue(world, w, h, out, stream_ptr, **(frame or LIGHT))
    torch.cuda.synchronize()
    out.zero_()
    torch.cuda.synchronize()
    return world


# ---- 1. same bytes ---------------------------------------------------------------------------

def check_same_bytes(monkeypatch, make_world, w, h, spp, depth, rows, fork, what):
    """The second lean frame of make_world() against brute force, the counting frame
    and the RT_AMD_SKY_FORK=0 frame of a fresh world.  fork: what sky_forked() must
    say of it (None: 1 exactly when some but not all rows are sky)."""
    world = make_world()
    ref = _brute(world, w, h, spp, depth)[0]
    world.render(w, h, spp, depth, stats=False)
    lean, _ = world.render(w, h, spp, depth, stats=False)
    n, forked = world.sky_rows(), world.sky_forked()
    _expect(n, h, rows, what)
    print(f"{what}: sky_forked = {forked}")
    assert forked == (int(0 < n < h) if fork is None else fork), (what, n, forked)
    assert_bits_equal(lean, ref, f"{what}: forked frame vs brute force")
    counted, _ = world.render(w, h, spp, depth)
    assert world.sky_forked() == 0 and world.sky_rows() == 0  # (a counted frame has no sky kernel)
    assert_bits_equal(lean, counted, f"{what}: forked frame vs counting frame")
    monkeypatch.setenv("RT_AMD_SKY_FORK", "0")
    off_world = make_world()
    off_world.render(w, h, spp, depth, stats=False)
    off, _ = off_world.render(w, h, spp, depth, stats=False)
    assert off_world.sky_rows() == n and off_world.sky_forked() == 0
    monkeypatch.delenv("RT_AMD_SKY_FORK")
    assert_bits_equal(lean, off, f"{what}: forked frame vs the one-stream frame")


@pytest.mark.parametrize("depth", [8, 1])
@pytest.mark.parametrize("spp", [1, 6, 64])
@pytest.mark.parametrize("w,h", [(64, 36), (93, 41)])
def test_1_forked_frames_have_the_same_bytes(monkeypatch, w, h, spp, depth):
    check_same_bytes(monkeypatch, lambda: R.World(S.rtow()), w, h, spp, depth, "some", 1,
                     f"rtow {w}x{h}x{spp} d{depth}")


@pytest.mark.parametrize("name,rows,fork", [("fov", "some", 1), ("roll", "any", None), ("up", "all", 0),
                                            ("down", "none", 0)])
def test_1_cameras(monkeypatch, name, rows, fork):
    check_same_bytes(monkeypatch, _rtow_with(CAMS[name]), 64, 36, 4, 8, rows, fork, f"camera {name}")


# ---- 2. the join -------------------------------------------------------------------------------

def test_2_a_copy_behind_the_frame_sees_its_sky_rows(monkeypatch):
    torch, (s,) = gpu(1)
    w, h, frame = JOIN_W, JOIN_H, dict(spp=JOIN_SPP, depth=8)
    make = _rtow_with(tilt_up(JOIN_PITCH))
    want = solo_off(monkeypatch, "join", make, w, h, **frame)
    out, copy = frame_buf(torch, w, h), frame_buf(torch, w, h)
    world = primed(make, w, h, out, s.cuda_stream)

    enqueue(world, w, h, out, s.cuda_stream, **frame)
    e = mark(torch, s)
    with torch.cuda.stream(s):
        copy.copy_(out, non_blocking=True)
    running = not e.query()
    n, forked = world.sky_rows(), world.sky_forked()
    torch.cuda.synchronize()

    print(f"join: sky_rows = {n} of {h}")
    assert forked == 1 and n == JOIN_ROWS, (n, forked)
    assert_bits_equal(as_frame(copy, w, h), want, "join: the copy enqueued behind the frame")
    assert_bits_equal(as_frame(out, w, h), want, "join: the frame")
    assert_in_flight(running, "join")
    world.close()


# ---- 3. the fork point -------------------------------------------------------------------------

def test_3_the_sky_kernel_does_not_run_ahead_of_the_stream(monkeypatch):
    """A heavy frame into X, a fill of Y, a forking frame into Y: the sky kernel starts
    behind the fill, or the fill would overwrite its rows."""
    torch, (s,) = gpu(1)
    w, h = H_W, H_H
    make = lambda: R.World(source("rtow"))  # noqa: E731
    want_x = solo_off(monkeypatch, "rtow", make, w, h, **HEAVY)
    want_y = oracle_frame("rtow", w, h, **ONE_SAMPLE)
    x, y = frame_buf(torch, w, h), frame_buf(torch, w, h)
    world = primed(make, w, h, y, s.cuda_stream)

    enqueue(world, w, h, x, s.cuda_stream, **HEAVY)
    e = mark(torch, s)
    assert world.sky_forked() == 1
    with torch.cuda.stream(s):
        y.fill_(0x5A)
    enqueue(world, w, h, y, s.cuda_stream, **ONE_SAMPLE)
    running = not e.query()
    n, forked = world.sky_rows(), world.sky_forked()
    torch.cuda.synchronize()

    assert forked == 1 and 0 < n < h, (n, forked)
    assert_in_flight(running, "fork point")
    assert_bits_equal(as_frame(y, w, h), want_y, "fork point: the frame behind the fill against the oracle")
    assert_bits_equal(as_frame(x, w, h), want_x, "fork point: the heavy frame against its solo render")
    world.close()


# ---- 4. two streams, one buffer ----------------------------------------------------------------

@pytest.mark.parametrize("role_a", ["user", "library"])
def test_4_two_streams_one_buffer(monkeypatch, role_a):
    """A forking frame on stream A, then, with the camera moved up (other sky rows), a
    priming frame and a forking frame on stream B, all into one buffer: B's frame."""
    torch, (sA, sB) = gpu(2)
    w, h = H_W, H_H
    make = lambda: R.World(source("rtow"))  # noqa: E731

    def make_moved():
        world = make()
        world.move_camera(0.0, 4.0, 0.0)
        return world

    want = _brute(make_moved(), w, h, LIGHT["spp"], LIGHT["depth"])[0]
    pa = sA.cuda_stream if role_a == "user" else 0
    out = frame_buf(torch, w, h)
    world = primed(make, w, h, out, pa)

    enqueue(world, w, h, out, pa, **HEAVY)
    e_a = mark(torch, sA) if role_a == "user" else None
    rows_a, forked_a = world.sky_rows(), world.sky_forked()
    world.move_camera(0.0, 4.0, 0.0)
    enqueue(world, w, h, out, sB.cuda_stream, **LIGHT)  # (every row traced: the rows are classified behind it)
    assert world.sky_forked() == 0
    enqueue(world, w, h, out, sB.cuda_stream, **LIGHT)
    e_b = mark(torch, sB)
    running = not (e_a if e_a is not None else e_b).query()
    rows_b, forked_b = world.sky_rows(), world.sky_forked()
    torch.cuda.synchronize()

    what = f"one buffer, A on the {role_a} stream"
    print(f"{what}: rows {rows_a} then {rows_b}")
    assert forked_a == 1 and forked_b == 1 and 0 < rows_a < rows_b < h, (rows_a, rows_b, forked_a, forked_b)
    assert_in_flight(running, what)
    if e_a is not None:
        assert e_a.elapsed_time(e_b) >= 0, f"{what}: B ended before A"
    assert_bits_equal(as_frame(out, w, h), want, f"{what}: the buffer is B's frame")
    world.close()


# ---- 5. back to back ---------------------------------------------------------------------------

def test_5_three_forking_frames_back_to_back(monkeypatch):
    torch, (s,) = gpu(1)
    w, h = H_W, H_H  # (at 93 x 41 two of these cameras have the same 21 sky rows)
    frame = LIGHT
    lifts = (0.0, 2.0, 4.0)  # (the camera's height over its first place: higher, more sky rows)

    def make_at(lift):
        def make():
            world = R.World(source("rtow"))
            if lift:
                world.move_camera(0.0, lift, 0.0)
            return world
        return make

    want = [_brute(make_at(lift)(), w, h, frame["spp"], frame["depth"])[0] for lift in lifts]
    outs = [frame_buf(torch, w, h) for _ in lifts]
    scratch = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    torch.cuda.synchronize()
    rows = []
    for k, out in enumerate(outs):
        if k:
            world.move_camera(0.0, lifts[k] - lifts[k - 1], 0.0)
        enqueue(world, w, h, scratch, s.cuda_stream, **frame)  # (the priming frame of this camera)
        enqueue(world, w, h, out, s.cuda_stream, **frame)
        assert world.sky_forked() == 1
        rows.append(world.sky_rows())
    torch.cuda.synchronize()
    print(f"back to back: rows {rows}")
    assert len(set(rows)) == len(rows) and all(0 < n < h for n in rows), rows
    for k, out in enumerate(outs):
        assert_bits_equal(as_frame(out, w, h), want[k], f"back to back: frame {k} against brute force")
    world.close()


# ---- 6. behind the fence -----------------------------------------------------------------------

EDIT = (0, 1, (0.7, 0.6, 0.5), 0.2, False)  # (test_gpu_streams.py EDITS["rtow"][0]: the ground, seen by many pixels)


def test_6_first_hit_and_an_edit_behind_a_forked_frame(monkeypatch):
    torch, (sA, sB) = gpu(2)
    w, h = 64, 36
    make = lambda: R.World(source("rtow"))  # noqa: E731
    want_heavy = solo_off(monkeypatch, "rtow", make, w, h, **HEAVY)
    want_rec = memo(("sky fork records", w, h), lambda: FH.restate(source("rtow"), w, h))
    want_edit = oracle_frame("rtow", w, h, LIGHT["spp"], LIGHT["depth"], edits=(EDIT,))
    out_heavy, out_edit = frame_buf(torch, w, h), frame_buf(torch, w, h)
    d_rec = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
    world = primed(make, w, h, out_heavy, sA.cuda_stream)
    world.first_hit_device(w, h, d_rec.data_ptr(), sB.cuda_stream, device=0)
    torch.cuda.synchronize()
    d_rec.zero_()
    torch.cuda.synchronize()

    enqueue(world, w, h, out_heavy, sA.cuda_stream, **HEAVY)
    e = mark(torch, sA)
    forked = world.sky_forked()
    world.first_hit_device(w, h, d_rec.data_ptr(), sB.cuda_stream, device=0)
    running = not e.query()
    i, kind, rgb, param, tri = EDIT
    world.set_material(i, kind, rgb, param, triangle=tri)
    enqueue(world, w, h, out_edit, sA.cuda_stream, **LIGHT)
    torch.cuda.synchronize()

    what = "behind the fence"
    assert forked == 1
    assert_in_flight(running, what)
    assert_bits_equal(as_frame(out_heavy, w, h), want_heavy, f"{what}: the forked frame against its solo render")
    FH.assert_records(np.frombuffer(d_rec.cpu().numpy().tobytes(), R.FIRST_HIT_DTYPE).reshape(h, w), want_rec,
                      f"{what}: first-hit records")
    assert_bits_equal(as_frame(out_edit, w, h), want_edit, f"{what}: the edited world's frame against the oracle")
    world.close()


def test_6_a_world_closed_with_its_forked_frame_in_flight(monkeypatch):
    torch, (s,) = gpu(1)
    w, h = H_W, H_H
    make = lambda: R.World(source("rtow"))  # noqa: E731
    want = oracle_frame("rtow", w, h, **ONE_SAMPLE)
    out = frame_buf(torch, w, h)
    world = primed(make, w, h, out, s.cuda_stream)
    fresh = make()

    enqueue(world, w, h, out, s.cuda_stream, **HEAVY)
    e = mark(torch, s)
    forked = world.sky_forked()
    running = not e.query()
    world.close()
    enqueue(fresh, w, h, out, s.cuda_stream, **ONE_SAMPLE)
    torch.cuda.synchronize()

    assert forked == 1
    assert_in_flight(running, "closed world")
    assert_bits_equal(as_frame(out, w, h), want, "closed world: the fresh world's frame against the oracle")
    fresh.close()


# ---- 7. off ------------------------------------------------------------------------------------

def test_7_off_keeps_the_one_stream_order(monkeypatch):
    w, h, spp = 64, 36, 6
    monkeypatch.setenv("RT_AMD_SKY_FORK", "0")
    world = R.World(S.rtow())
    ref = _brute(world, w, h, spp)[0]
    world.render(w, h, spp, 8, stats=False)
    lean, _ = world.render(w, h, spp, 8, stats=False)
    assert 0 < world.sky_rows() < h and world.sky_forked() == 0
    assert_bits_equal(lean, ref, "RT_AMD_SKY_FORK=0 vs brute force")
    monkeypatch.delenv("RT_AMD_SKY_FORK")
    lean, _ = world.render(w, h, spp, 8, stats=False)
    assert world.sky_forked() == 1
    assert_bits_equal(lean, ref, "the forked frame of the same world vs brute force")
