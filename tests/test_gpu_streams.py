"""Stream ordering on one device (raytracer_amd.h: "frames enqueued on different
streams of one device are ordered: the later waits for the earlier, they share
the device's scratch").  Calls here follow each other on different streams with
no host wait in between, the earlier one still running when the later one is
enqueued, and every output is still the expected one.

Every call is only enqueued (stats=False or a *_device entry), on non-blocking
torch streams or on the library's own stream (stream_ptr 0), into torch tensors
of its own.  Everything expected is computed before the first enqueue.

Expected values.  The oracle (raw bits: assert_bits_equal, Expect,
assert_sums_equal, filter_ref, test_gpu_adapt's and test_gpu_first_hit's
restatements) for every light frame, pass, record and filter result.  The solo
render -- the same request rendered synchronously on a fresh World with nothing
else in flight -- only for the heavy frame "A": 480 x 270 at 4096 samples in
cases (a) and (c), and the 4096-sample frames that put the light calls of (b),
(d), (e) and (g) behind a running kernel.  That path is pinned to the oracle at small
sizes by the rest of the suite; what is under test here is ordering.  A is sized
by measurement (profiles/streams/times.txt): its trace time alone is far above
the host time of the call enqueued behind it.

Two witnesses, both asserted, in every case but (f) (the adaptive passes of (d)
wait on the host by themselves, so only their order is asserted):
  in flight  an event recorded behind the earlier call has not completed when
             the later call returns -- else the case tested nothing, and says so;
  ordered    with timing events behind both calls, the later call's work ends
             no earlier than the earlier call's (elapsed_time >= 0).
The library's own stream takes no caller's event.  Where the earlier frame runs
on it, "in flight" is read off the later call's event (that call waits for the
frame) and "ordered" is the later call ending at least half the frame's solo
trace time after the pair began; where the later frame runs on it, a third
light frame on a user stream, which waits for the library's stream in turn,
carries the event.

Which wait or lock each case goes through (csrc/; the three fences, device_fence.h
and DESIGN.md 4, "Stream ordering": d->done the device's, a.done / acc.done the accumulator's, f.done
the filter's; a wait is fence.wait(stream), the host's wait fence.sync()):
  (a) frame after frame            frame.cpp render_frame: the device's scratch (d->done)
  (b) the slab path                the same wait; d->samples and the resolve kernel
  (c) REPLAY after COUNTER         the same wait before the pass's launches; an
                                   accumulator owns its table, so d->replay's upload is
                                   reached only by the "frame" variant (rt_render_device)
  (d) an accumulator on three      frame.cpp enqueue_launches (acc.done before a pass),
      streams, then a filter       filter.cpp AccumRead::begin, for filter_accum (a.done before
                                   the filter reads the sums; f.done: the second filter run, on
                                   another stream), first_hit.cpp (d->done before the records),
                                   filter.cpp filter_enqueue (f.done again, a stand-alone run's
                                   only wait), accum.cpp accum_read (the host waits)
      filter between frames        AccumRead::begin (d->done before finish records it
                                   again on the filter's stream)
      adaptive                     accum.cpp accum_add (a.done before the frame's copy of
                                   a pass that traced nothing); accum_records' wait before
                                   new records (f.done) after a reset
  (e) first-hit between frames     first_hit.cpp and frame.cpp, both directions
  (f) two worlds                   no wait: nothing is shared
  (g) edits with frames in flight  WorldState::mu and the release of the device state
  (h) SERIAL behind a frame        serial_states.cpp serial_find_states (d->done before its
                                   first pass); SERIAL waits on the host, so the witness is
                                   that the frame before it has ended when it returns
  (i) a stand-alone filter         filter.cpp filter_run (f.done before the host entry's staging
                                   copies) and RtFilter::mu; the host entry waits, so the
                                   witness is as in (h)
  (j) history resolves on two      AccumRead::begin, for history.cpp history_resolve (a.done: the
      streams behind a pass        pass, then the first resolve's snapshots; f.done: the first
                                   resolve's staging; d->done), history_read_length (the host waits)
  (g') geometry edits with         capi.cpp edit_begin, for rt_world_set_sphere_geometry: the
      frames in flight             host waits on d->done before the tree and the packed spheres
                                   change (the library waits on its own event, which a caller's
                                   event behind it may outlast: the frames' bits are the witness)
  (j') a geometry edit with a      the same host wait, on the d->done that AccumRead::finish recorded
      move-path resolve in flight  behind the resolve (it reads the device's sphere array);
                                   history.cpp upload_prev_spheres (the host waits on a.done: the pass)
Every wait on a fence in frame.cpp, accum.cpp, filter.cpp, first_hit.cpp, history.cpp and
serial_states.cpp is reached by a case.  Frames captured into a graph and replayed, which
the fences do not order, are in tests/test_gpu_capture.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import clamp_ref as CR
import filter_ref as FR
import history_ref as HR
import move_cases as MC
import move_ref as MR
import oracle as O
import raytracer_amd as R
import scenes as S
import test_gpu_adapt as AD
import test_gpu_first_hit as FH
from conftest import scene_text
from test_gpu_accum import Expect, assert_sums_equal
from test_gpu_filter import assert_same, synthetic
from test_gpu_history import same_bits
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order

pytestmark = pytest.mark.gpu

NT = max(1, min(16, len(os.sched_getaffinity(0))))  # oracle threads
A_W, A_H, A_SPP, A_DEPTH = 480, 270, 4096, 8       # the heavy frame (profiles/streams/times.txt)
B = dict(spp=1, depth=5, seed=99)                    # the light frame enqueued behind it
C3 = dict(spp=1, depth=3, seed=7)                    # ... and a third one
DT = R.FIRST_HIT_DTYPE

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def source(name):
    return memo(("src", name), {"rtow": S.rtow, "soup": lambda: S.triangle_soup(7, 300, spheres=40, grid=6),
                                "three_spheres": lambda: scene_text("three_spheres.txt")}[name])


def oracle_frame(name, w, h, spp, depth, seed=R.DEFAULT_SEED, edits=()):
    def make():
        ref = O.Scene(source(name))
        for e in edits:
            ref.set_material(*e[:-1], triangle=e[-1])
        return ref.render(w, h, spp, depth, mode=O.RNG_COUNTER, seed=seed, nthreads=NT)[0]
    return memo(("oracle", name, w, h, spp, depth, seed, tuple(edits)), make)


def solo(name, w, h, spp, depth, seed=R.DEFAULT_SEED):
    """The solo render: (frame, its trace time in ms), once per request."""
    def make():
        world = R.World(source(name))
        out, st = world.render(w, h, spp, depth, seed=seed, device=0)
        world.close()
        return out, st["trace_ms"]
    return memo(("solo", name, w, h, spp, depth, seed), make)


def gpu(nstreams):
    import torch

    torch.cuda.set_device(0)
    return torch, [torch.cuda.Stream() for _ in range(nstreams)]


def frame_buf(torch, w, h):
    return torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")


def as_frame(t, w, h):
    return t.cpu().numpy().reshape(h, w, 4)


def mark(torch, stream):
    e = torch.cuda.Event(enable_timing=True)
    e.record(stream)
    return e


def assert_in_flight(running, what):
    assert running, (f"{what}: the earlier call had finished when the later call returned, so nothing was "
                     "enqueued behind a running kernel and the case tested nothing")


def assert_ordered(events, what):
    """events: [(name, event)] in call order, read after a synchronise."""
    for (na, ea), (nb, eb) in zip(events, events[1:]):
        ms = ea.elapsed_time(eb)
        assert ms >= 0, f"{what}: {nb} ended {-ms:.3f} ms before {na}"


def enqueue(world, w, h, out, stream_ptr, spp, depth, seed=R.DEFAULT_SEED, **kw):
    assert world.render_device(w, h, out.data_ptr(), stream_ptr, spp=spp, depth=depth, seed=seed, device=0,
                               stats=False, **kw) is None


# ---- (a) frame then frame ------------------------------------------------------------------

@pytest.mark.parametrize("role_a,role_b", [("user", "user"), ("library", "user"), ("user", "library")])
def test_a_frame_behind_a_running_frame(role_a, role_b):
    torch, (sA, sB, sC) = gpu(3)
    w, h = A_W, A_H
    want_a, a_ms = solo("rtow", w, h, A_SPP, A_DEPTH)
    want_b, want_c = oracle_frame("rtow", w, h, **B), oracle_frame("rtow", w, h, **C3)
    pa = sA.cuda_stream if role_a == "user" else 0
    pb = sB.cuda_stream if role_b == "user" else 0
    out_a, out_b, out_c = (frame_buf(torch, w, h) for _ in range(3))
    world = R.World(source("rtow"))
    enqueue(world, w, h, out_b, pb, **B)  # (the scene upload, the lists, B's kernel: done before the pair)
    torch.cuda.synchronize()
    out_b.zero_()
    torch.cuda.synchronize()

    what = f"A on the {role_a} stream, B on the {role_b} stream"
    e0 = mark(torch, sB)
    enqueue(world, w, h, out_a, pa, A_SPP, A_DEPTH)
    e_a = mark(torch, sA) if role_a == "user" else None
    enqueue(world, w, h, out_b, pb, **B)
    e_b = mark(torch, sB) if role_b == "user" else None
    running = not (e_a if e_a is not None else e_b).query()
    e_c = None
    if role_b == "library":  # (its event: a frame on a user stream that waits for the library's)
        enqueue(world, w, h, out_c, sC.cuda_stream, **C3)
        e_c = mark(torch, sC)
    torch.cuda.synchronize()

    assert_in_flight(running, what)
    if role_a == "user":
        assert_ordered([("A", e_a), ("B", e_b) if e_b is not None else ("the frame behind B", e_c)], what)
    else:
        ms = e0.elapsed_time(e_b)
        assert ms >= 0.5 * a_ms, f"{what}: B ended {ms:.3f} ms after the pair began, A alone traces {a_ms:.3f} ms"
    assert_bits_equal(as_frame(out_a, w, h), want_a, f"{what}: A against its solo render")
    assert_bits_equal(as_frame(out_b, w, h), want_b, f"{what}: B against the oracle")
    if e_c is not None:
        assert_bits_equal(as_frame(out_c, w, h), want_c, f"{what}: the frame behind B against the oracle")
    world.close()


# ---- (b) the slab path ---------------------------------------------------------------------

def test_b_slab_frames_on_two_streams():
    """Both frames keep their samples: the slab and the resolve kernel are the shared
    scratch.  A (480 x 270 x 64) takes under a millisecond, so it is enqueued behind the
    heavy frame on its own stream: B is enqueued while A has not even begun."""
    torch, (sA, sB) = gpu(2)
    w, h, spp = 480, 270, 64
    want_heavy, _ = solo("rtow", A_W, A_H, A_SPP, A_DEPTH)
    want_a = oracle_frame("rtow", w, h, spp, 8)
    want_b, _, _, smp_b = memo("slab B", lambda: O.Scene(source("rtow")).render(
        w, h, B["spp"], B["depth"], mode=O.RNG_COUNTER, seed=B["seed"], record_samples=True, nthreads=NT))
    out_heavy, out_a, out_b = (frame_buf(torch, w, h) for _ in range(3))
    world = R.World(source("rtow"))
    enqueue(world, w, h, out_a, sA.cuda_stream, spp, 8, keep_samples=True)  # (the slab: allocated for A's size)
    enqueue(world, w, h, out_b, sB.cuda_stream, keep_samples=True, **B)
    torch.cuda.synchronize()
    out_a.zero_(), out_b.zero_()
    torch.cuda.synchronize()

    enqueue(world, A_W, A_H, out_heavy, sA.cuda_stream, A_SPP, A_DEPTH)
    enqueue(world, w, h, out_a, sA.cuda_stream, spp, 8, keep_samples=True)
    e_a = mark(torch, sA)
    enqueue(world, w, h, out_b, sB.cuda_stream, keep_samples=True, **B)
    running = not e_a.query()
    e_b = mark(torch, sB)
    torch.cuda.synchronize()

    assert_in_flight(running, "slab frames")
    assert_ordered([("A", e_a), ("B", e_b)], "slab frames")
    assert_bits_equal(as_frame(out_heavy, A_W, A_H), want_heavy, "slab frames: the heavy frame against its solo render")
    assert_bits_equal(as_frame(out_a, w, h), want_a, "slab frame A against the oracle")
    assert_bits_equal(as_frame(out_b, w, h), want_b, "slab frame B against the oracle")
    assert_bits_equal(world.read_samples(w * h * B["spp"])[:, :3],
                      oracle_samples_to_gpu_order(smp_b, w, h, B["spp"])[:, :3], "the last launch's samples (B's)")
    world.close()


# ---- (c) REPLAY after COUNTER --------------------------------------------------------------

@pytest.mark.parametrize("how", ["accumulator", "frame"])
def test_c_replay_behind_a_counter_frame(how):
    """The table is the reference's own stream (the oracle's SERIAL run).  how = frame:
    rt_render_device with RT_RNG_REPLAY, whose table is uploaded to the device's
    scratch on the call's stream; the binding's render_device takes no table."""
    torch, (sA, sB) = gpu(2)
    w, h, stride = A_W, A_H, 2
    want_a, _ = solo("rtow", w, h, A_SPP, A_DEPTH)
    img, _, states = memo("serial run", lambda: O.Scene(source("rtow")).render(w, h, stride, 8, mode=O.RNG_SERIAL,
                                                                               record_states=True))
    exp = memo("replay expect", lambda: Expect(O.Scene(source("rtow")), w, h, stride, 8, states=states))
    want_b = exp.frame(1) if how == "accumulator" else img
    want_sums = exp.sums(1)
    out_a, out_b = frame_buf(torch, w, h), frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    o, table = R.options(stride, 8, R.RNG_REPLAY, replay=states, device=0)  # (table: alive until the last wait)

    def replay_frame():
        rc = R.lib().rt_render_device(world.handle, w, h, C.byref(o), C.c_void_p(out_b.data_ptr()),
                                      C.c_void_p(sB.cuda_stream), None)
        assert rc == 0, R.last_error()

    acc = None
    if how == "accumulator":
        warm = world.accumulator(w, h, stride, mode=R.RNG_REPLAY, replay=states, device=0)
        warm.add_device(1, out_b.data_ptr(), sB.cuda_stream)
        torch.cuda.synchronize()
        warm.close()
        acc = world.accumulator(w, h, stride, mode=R.RNG_REPLAY, replay=states, device=0)
    else:
        replay_frame()
    torch.cuda.synchronize()
    out_b.zero_()
    torch.cuda.synchronize()

    enqueue(world, w, h, out_a, sA.cuda_stream, A_SPP, A_DEPTH)
    e_a = mark(torch, sA)
    if acc is not None:
        assert acc.add_device(1, out_b.data_ptr(), sB.cuda_stream) is None
    else:
        replay_frame()
    running = not e_a.query()
    e_b = mark(torch, sB)
    torch.cuda.synchronize()
    del table

    what = f"REPLAY {how} behind a COUNTER frame"
    assert_in_flight(running, what)
    assert_ordered([("A", e_a), ("the REPLAY " + how, e_b)], what)
    assert_bits_equal(as_frame(out_a, w, h), want_a, f"{what}: A against its solo render")
    assert_bits_equal(as_frame(out_b, w, h), want_b, f"{what}: the {how} against the oracle")
    if acc is not None:
        assert acc.samples == 1
        assert_sums_equal(acc.sums(), want_sums, f"{what}: sums")
        acc.close()
    world.close()


# ---- (d) one accumulator, several streams ----------------------------------------------------

def test_d_accumulator_passes_and_filter_on_three_streams():
    """Behind a heavy frame on sA: add(3) on sA, add(5) on sB, the filter on sC, a
    second filter run on sA, and rt_accum_read at once, which has to wait by itself."""
    torch, (sA, sB, sC) = gpu(3)
    w, h, stride = 96, 64, 8
    hw, hh = A_W, A_H
    want_heavy, _ = solo("rtow", hw, hh, A_SPP, A_DEPTH)
    exp = memo("d expect", lambda: Expect(O.Scene(source("rtow")), w, h, stride, 8))
    exp.frame(3), exp.sums(8)
    out_heavy = frame_buf(torch, hw, hh)
    out_3, out_8, px_c, px_a = (frame_buf(torch, w, h) for _ in range(4))
    rgb_c = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    world = R.World(source("rtow"))
    warm = world.accumulator(w, h, stride, device=0)  # (the pass's and the filter's kernels and buffers)
    warm.add_device(2, out_3.data_ptr(), sB.cuda_stream)
    warm.filtered_device(rgb_c.data_ptr(), px_c.data_ptr(), sC.cuda_stream)
    torch.cuda.synchronize()
    warm.close()
    for t in (out_3, px_c, rgb_c):
        t.zero_()
    acc = world.accumulator(w, h, stride, device=0)
    torch.cuda.synchronize()

    enqueue(world, hw, hh, out_heavy, sA.cuda_stream, A_SPP, A_DEPTH)
    assert acc.add_device(3, out_3.data_ptr(), sA.cuda_stream) is None
    e1 = mark(torch, sA)
    assert acc.add_device(5, out_8.data_ptr(), sB.cuda_stream) is None
    e2 = mark(torch, sB)
    acc.filtered_device(rgb_c.data_ptr(), px_c.data_ptr(), sC.cuda_stream)
    e3 = mark(torch, sC)
    acc.filtered_device(0, px_a.data_ptr(), sA.cuda_stream, levels=1)
    e4 = mark(torch, sA)
    running = not e1.query()
    sums = acc.sums()  # (no synchronise before it)
    held = acc.samples
    torch.cuda.synchronize()

    what = "accumulator on three streams"
    assert_in_flight(running, what)
    assert_ordered([("add(3)", e1), ("add(5)", e2), ("the filter", e3), ("the second filter run", e4)], what)
    assert held == 8
    assert_sums_equal(sums, exp.sums(8), f"{what}: sums read with no wait before")
    assert_bits_equal(as_frame(out_heavy, hw, hh), want_heavy, f"{what}: the heavy frame against its solo render")
    assert_bits_equal(as_frame(out_3, w, h), exp.frame(3), f"{what}: frame after add(3)")
    assert_bits_equal(as_frame(out_8, w, h), exp.frame(8), f"{what}: frame after add(5)")
    rec = world.first_hit(w, h, device=0)  # (pinned by test_gpu_first_hit.py)
    rgb = FR.means(exp.sums(8), 8)
    got = (rgb_c.cpu().numpy().reshape(h, w, 3), as_frame(px_c, w, h))
    assert_same(got, FR.filter_image(rgb, rec), f"{what}: the filter on sC")
    assert_same((None, as_frame(px_a, w, h)), FR.filter_image(rgb, rec, levels=1), f"{what}: the second run, on sA")
    acc.close()
    world.close()


def test_d_adaptive_accumulator_on_alternating_streams():
    """An adaptive pass with a decision reads the list's length back, so each pass
    waits on the host: no in-flight witness here, the order of the passes only."""
    torch, (sA, sB) = gpu(2)
    w, h, stride, split = 96, 64, 12, (4, 4, 4)
    exp = memo("adaptive expect", lambda: Expect(O.Scene(source("three_spheres")), w, h, stride, 8))
    states = AD.restate(exp, split, 0.08, 0.05, 4)
    assert any(0 < len(s["active"]) < w * h for s in states)
    world = R.World(source("three_spheres"))
    acc = world.accumulator(w, h, stride, device=0)
    acc.set_adaptive(0.08, 0.05, 4)
    outs = [frame_buf(torch, w, h) for _ in split]
    torch.cuda.synchronize()
    events = []
    for k, (n, out) in enumerate(zip(split, outs)):
        s = (sA, sB)[k % 2]
        assert acc.add_device(n, out.data_ptr(), s.cuda_stream) is None
        events.append((f"pass {k}", mark(torch, s)))
    counts, sums, active = acc.counts(), acc.sums(), acc.active_list()
    torch.cuda.synchronize()
    assert_ordered(events, "adaptive passes")
    last = states[-1]
    assert acc.samples == last["N"] and np.array_equal(active, last["active"])
    assert np.array_equal(counts.reshape(-1), last["count"]), "adaptive passes: counts"
    full = counts.reshape(-1) == last["N"]
    assert full.any() and not full.all()
    assert_sums_equal(sums.reshape(-1, 3)[full], last["sums"][full], "adaptive passes: sums at full-count pixels")
    assert_sums_equal(sums.reshape(-1, 3), last["sums"], "adaptive passes: sums")
    for k, (out, st) in enumerate(zip(outs, states)):
        assert_bits_equal(as_frame(out, w, h), AD.expected_frame(exp, st["count"]), f"adaptive pass {k}: frame")
    # the filter after the passes, then a reset, new passes and the filter on another
    # stream: new records are traced behind the filter's last run
    px = [frame_buf(torch, w, h) for _ in range(2)]
    acc.filtered_device(0, px[0].data_ptr(), sA.cuda_stream)
    acc.reset()
    acc.add_device(4, outs[0].data_ptr(), sA.cuda_stream)
    acc.filtered_device(0, px[1].data_ptr(), sB.cuda_stream)
    torch.cuda.synchronize()
    rec = world.first_hit(w, h, device=0)
    for k, st in enumerate((last, states[0])):
        rgb = FR.means(st["sums"].reshape(h, w, 3), st["count"].reshape(h, w))
        assert_same((None, as_frame(px[k], w, h)), FR.filter_image(rgb, rec), f"adaptive: filter run {k}")
    acc.close()
    world.close()


def test_d_adaptive_pass_that_traces_nothing_on_another_stream():
    """With every pixel converged at the first decision the next pass only copies the
    accumulator's frame out: on another stream, behind the pass that wrote it."""
    torch, (sA, sB) = gpu(2)
    w, h = 40, 24
    exp = AD._rtow()
    states = AD.restate(exp, (8, 4), 1e30, AD.BIAS, 8)
    assert len(states[0]["active"]) == 0 and states[1]["traced"] == 0
    acc = AD._rtow_acc(tolerance=1e30)
    first, again = frame_buf(torch, w, h), frame_buf(torch, w, h)
    torch.cuda.synchronize()
    assert acc.add_device(8, first.data_ptr(), sA.cuda_stream) is None
    e1 = mark(torch, sA)
    assert acc.add_device(4, again.data_ptr(), sB.cuda_stream) is None
    e2 = mark(torch, sB)
    torch.cuda.synchronize()
    assert_ordered([("the pass of 8", e1), ("the pass that traces nothing", e2)], "empty list")
    assert acc.samples == 8 and acc.active == 0
    want = AD.expected_frame(exp, states[0]["count"])
    assert_bits_equal(as_frame(first, w, h), want, "empty list: the frame of the first pass")
    assert_bits_equal(as_frame(again, w, h), want, "empty list: the same frame from the pass that traced nothing")
    acc.close()


def test_d_filter_between_frames_on_two_streams():
    """A heavy frame on sA, the filter of an accumulator on sB (its records are current,
    so it traces nothing), then a light frame on sB.  The filter records the device's
    "last work" event on sB; the frame behind it must still wait for the frame on sA."""
    torch, (sA, sB) = gpu(2)
    w, h, stride = 96, 64, 8
    hw, hh = A_W, A_H
    want_a, _ = solo("rtow", hw, hh, A_SPP, A_DEPTH)
    want_b = oracle_frame("rtow", hw, hh, **B)
    exp = memo("d expect", lambda: Expect(O.Scene(source("rtow")), w, h, stride, 8))
    exp.sums(8)
    out_a, out_b = frame_buf(torch, hw, hh), frame_buf(torch, hw, hh)
    px = [frame_buf(torch, w, h) for _ in range(2)]
    world = R.World(source("rtow"))
    acc = world.accumulator(w, h, stride, device=0)
    acc.add_device(8, 0, sB.cuda_stream)
    acc.filtered_device(0, px[0].data_ptr(), sB.cuda_stream)  # (the records are traced here)
    enqueue(world, hw, hh, out_b, sB.cuda_stream, **B)
    torch.cuda.synchronize()
    out_b.zero_()
    torch.cuda.synchronize()

    enqueue(world, hw, hh, out_a, sA.cuda_stream, A_SPP, A_DEPTH)
    e_a = mark(torch, sA)
    acc.filtered_device(0, px[1].data_ptr(), sB.cuda_stream)
    enqueue(world, hw, hh, out_b, sB.cuda_stream, **B)
    running = not e_a.query()
    e_b = mark(torch, sB)
    torch.cuda.synchronize()

    what = "filter between frames"
    assert_in_flight(running, what)
    assert_ordered([("A", e_a), ("the frame behind the filter", e_b)], what)
    assert_bits_equal(as_frame(out_a, hw, hh), want_a, f"{what}: A against its solo render")
    assert_bits_equal(as_frame(out_b, hw, hh), want_b, f"{what}: the frame behind the filter against the oracle")
    want_px = FR.filter_image(FR.means(exp.sums(8), 8), world.first_hit(w, h, device=0))
    for k in range(2):
        assert_same((None, as_frame(px[k], w, h)), want_px, f"{what}: filter run {k}")
    acc.close()
    world.close()


# ---- (e) first-hit records between frames -----------------------------------------------------

def test_e_first_hit_between_frames():
    """Behind a heavy frame on sA: a frame on sA, the records on sB, a frame on sA, then
    the host entry (the library's stream, the device's own buffer).  The strip lists and
    the camera-origin records are bound by both kinds of call."""
    torch, (sA, sB) = gpu(2)
    w, h = 64, 48
    f1, f2 = dict(spp=4, depth=8, seed=R.DEFAULT_SEED), dict(spp=3, depth=5, seed=99)
    want_heavy, _ = solo("soup", w, h, A_SPP, A_DEPTH)
    want_1, want_2 = oracle_frame("soup", w, h, **f1), oracle_frame("soup", w, h, **f2)
    want_rec = FH.restate(source("soup"), w, h)
    out_heavy, out_1, out_2 = (frame_buf(torch, w, h) for _ in range(3))
    d_rec = torch.zeros(w * h * 32, dtype=torch.uint8, device="cuda")
    world = R.World(source("soup"))
    enqueue(world, w, h, out_1, sA.cuda_stream, **f1)  # (the lists of this camera and size: built with a host wait)
    world.first_hit_device(w, h, d_rec.data_ptr(), sB.cuda_stream, device=0)
    world.first_hit(w, h, device=0)
    torch.cuda.synchronize()
    out_1.zero_(), d_rec.zero_()
    torch.cuda.synchronize()

    enqueue(world, w, h, out_heavy, sA.cuda_stream, A_SPP, A_DEPTH)
    enqueue(world, w, h, out_1, sA.cuda_stream, **f1)
    e1 = mark(torch, sA)
    world.first_hit_device(w, h, d_rec.data_ptr(), sB.cuda_stream, device=0)
    e2 = mark(torch, sB)
    enqueue(world, w, h, out_2, sA.cuda_stream, **f2)
    e3 = mark(torch, sA)
    running = not e1.query()
    host_rec = world.first_hit(w, h, device=0)
    torch.cuda.synchronize()

    what = "first-hit between frames"
    assert_in_flight(running, what)
    assert_ordered([("the first frame", e1), ("the records", e2), ("the second frame", e3)], what)
    assert world.primary_tri_lists(device=0) == 2  # (the device's strip lists were bound)
    FH.assert_records(np.frombuffer(d_rec.cpu().numpy().tobytes(), DT).reshape(h, w), want_rec, f"{what}: device records")
    FH.assert_records(host_rec, want_rec, f"{what}: host records")
    assert_bits_equal(as_frame(out_heavy, w, h), want_heavy, f"{what}: the heavy frame against its solo render")
    assert_bits_equal(as_frame(out_1, w, h), want_1, f"{what}: the first frame against the oracle")
    assert_bits_equal(as_frame(out_2, w, h), want_2, f"{what}: the second frame against the oracle")
    world.close()


# ---- (h) SERIAL behind a running frame ---------------------------------------------------------------

def test_h_serial_frame_behind_a_running_frame():
    """SERIAL finds its start states in passes the host waits for, on the library's
    stream here, so nothing can be enqueued behind it and the two witnesses do not
    apply.  Its first pass has to wait for the heavy frame on sA (the passes use the
    slab and the job counters): when the SERIAL call returns, that frame has ended."""
    torch, (sA,) = gpu(1)
    w, h, spp = 24, 18, 4
    want_a, _ = solo("rtow", A_W, A_H, A_SPP, A_DEPTH)
    want, ost, _ = memo("serial small", lambda: O.Scene(source("rtow")).render(w, h, spp, 8, mode=O.RNG_SERIAL))
    out_a = frame_buf(torch, A_W, A_H)
    world = R.World(source("rtow"))
    world.render(w, h, spp, 8, mode=R.RNG_SERIAL, device=0)
    enqueue(world, A_W, A_H, out_a, sA.cuda_stream, **B)
    torch.cuda.synchronize()

    enqueue(world, A_W, A_H, out_a, sA.cuda_stream, A_SPP, A_DEPTH)
    e_a = mark(torch, sA)
    running = not e_a.query()
    out, st = world.render(w, h, spp, 8, mode=R.RNG_SERIAL, device=0)
    ended = e_a.query()
    torch.cuda.synchronize()

    assert_in_flight(running, "SERIAL behind a frame")
    assert ended, "SERIAL behind a frame: the SERIAL frame returned while the frame enqueued before it still ran"
    assert_bits_equal(out, want, "SERIAL behind a frame: the SERIAL frame against the oracle")
    assert st["rays"] == ost["rays"]
    assert_bits_equal(as_frame(out_a, A_W, A_H), want_a, "SERIAL behind a frame: A against its solo render")
    world.close()


# ---- (i) a stand-alone filter: host entry behind its device entry ---------------------------------------

def test_i_filter_host_entry_behind_its_device_entry():
    """rt_filter_run_device on sA, enqueued behind a heavy frame, then rt_filter_run (the
    filter's own stream): its staging copies and levels use the filter's scratch, so it
    has to wait for the device run, and with it for the frame: both have ended when it returns."""
    torch, (sA,) = gpu(1)
    w, h = 37, 23
    rgb, rec = synthetic(w, h)
    want, want_1 = FR.filter_image(rgb, rec), FR.filter_image(rgb, rec, levels=1)
    want_a, _ = solo("rtow", A_W, A_H, A_SPP, A_DEPTH)
    out_a = frame_buf(torch, A_W, A_H)
    d_rgb = torch.from_numpy(rgb.copy()).cuda()
    d_rec = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).cuda()
    d_px = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    flt = R.Filter(w, h, device=0)
    enqueue(world, A_W, A_H, out_a, sA.cuda_stream, **B)
    flt.run(rgb, rec)
    flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), 0, d_px.data_ptr(), sA.cuda_stream, levels=1)
    torch.cuda.synchronize()
    d_px.zero_()
    torch.cuda.synchronize()

    enqueue(world, A_W, A_H, out_a, sA.cuda_stream, A_SPP, A_DEPTH)
    flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), 0, d_px.data_ptr(), sA.cuda_stream, levels=1)
    e = mark(torch, sA)
    running = not e.query()
    got = flt.run(rgb, rec)
    ended = e.query()
    torch.cuda.synchronize()

    what = "filter host entry behind its device entry"
    assert_in_flight(running, what)
    assert ended, f"{what}: the host entry returned while the device run enqueued before it had not ended"
    assert_same(got, want, f"{what}: the host entry")
    assert_same((None, as_frame(d_px, w, h)), want_1, f"{what}: the device entry")
    assert_bits_equal(as_frame(out_a, A_W, A_H), want_a, f"{what}: the heavy frame against its solo render")
    flt.close()
    world.close()


# ---- (f) two worlds, two streams ----------------------------------------------------------------

def test_f_two_worlds_two_streams():
    """The worlds share no scratch and may overlap (no witness): nothing global is shared by accident."""
    torch, streams = gpu(2)
    requests = [dict(spp=4, depth=8, seed=R.DEFAULT_SEED), B, dict(spp=3, depth=3, seed=7), dict(spp=8, depth=8, seed=1234)]
    sizes = {"rtow": (64, 36), "soup": (64, 48)}
    want = {n: [oracle_frame(n, *sizes[n], **r) for r in requests] for n in sizes}
    worlds = {n: R.World(source(n)) for n in sizes}
    outs = {n: [frame_buf(torch, *sizes[n]) for _ in requests] for n in sizes}
    torch.cuda.synchronize()
    for k, r in enumerate(requests):
        for s, n in zip(streams, sizes):
            enqueue(worlds[n], *sizes[n], outs[n][k], s.cuda_stream, **r)
    torch.cuda.synchronize()
    for n in sizes:
        for k in range(len(requests)):
            assert_bits_equal(as_frame(outs[n][k], *sizes[n]), want[n][k], f"two worlds: {n} frame {k}")
        worlds[n].close()


# ---- (g) material edits with frames in flight ------------------------------------------------------

EDITS = {  # (index, kind, rgb, param, triangle) before frames 1, 2, 3: primitives that many pixels see
    "rtow": [(0, 1, (0.7, 0.6, 0.5), 0.2, False), (484, 3, (4.0, 3.0, 1.0), 0.0, False),
             (0, 0, (0.2, 0.6, 0.3), 0.0, False)],
    "soup": [(118, 3, (6.0, 5.0, 2.0), 0.0, True), (5, 1, (0.8, 0.8, 0.3), 0.0, False),
             (39, 3, (1.0, 4.0, 6.0), 0.0, False)],
}


@pytest.mark.parametrize("name", list(EDITS))
def test_g_material_edits_with_frames_in_flight(name):
    """Four frames on one non-blocking stream, an edit before each but the first, one
    host wait at the end.  Frame 0 is heavy (same scene, size and camera), so the
    first edit is made while a frame runs: the edit drops the device's state."""
    torch, (s,) = gpu(1)
    w, h, spp = 96, 64, 16
    want = [solo(name, w, h, A_SPP, A_DEPTH)[0]]
    for k in range(len(EDITS[name])):
        want.append(oracle_frame(name, w, h, spp, A_DEPTH, edits=EDITS[name][:k + 1]))
        before = want[k] if k else oracle_frame(name, w, h, spp, A_DEPTH)
        assert (want[-1] != before).any(axis=2).sum() >= 40, f"{name}: edit {k} changes too few pixels to be seen"
    outs = [frame_buf(torch, w, h) for _ in want]
    world = R.World(source(name))
    enqueue(world, w, h, outs[1], s.cuda_stream, spp, A_DEPTH)
    torch.cuda.synchronize()
    outs[1].zero_()
    torch.cuda.synchronize()

    enqueue(world, w, h, outs[0], s.cuda_stream, A_SPP, A_DEPTH)
    e0 = mark(torch, s)
    running = not e0.query()
    events = [("frame 0", e0)]
    for k, (i, kind, rgb, param, tri) in enumerate(EDITS[name], 1):
        world.set_material(i, kind, rgb, param, triangle=tri)
        enqueue(world, w, h, outs[k], s.cuda_stream, spp, A_DEPTH)
        events.append((f"frame {k}", mark(torch, s)))
    torch.cuda.synchronize()

    assert_in_flight(running, f"{name}: the first edit")
    assert_ordered(events, f"{name}: edited frames")
    assert_bits_equal(as_frame(outs[0], w, h), want[0], f"{name}: frame 0 against its solo render")
    for k in range(1, len(want)):
        assert_bits_equal(as_frame(outs[k], w, h), want[k], f"{name}: frame {k} against the oracle with {k} edits")
    world.close()


# ---- (g') geometry edits with frames in flight ------------------------------------------------------

GEO_EDITS = {  # (sphere, offset from the scene file's centre, factor on its radius) before frames 1, 2, 3
    "rtow": [(484, (0.0, 0.4, 0.0), 1.25), (485, (0.3, 0.0, 0.5), 0.75), (484, (0.0, -0.2, 0.3), 1.0)],
    "soup": [(5, (0.2, 0.1, 0.0), 1.25), (39, (-0.2, 0.0, 0.1), 0.75), (5, (0.0, -0.1, 0.0), 1.0)],
}


def geo_steps(name):
    """[(sphere, centre, radius, the scene text after this edit and those before it)]"""
    src = text = source(name)
    steps = []
    for i, off, factor in GEO_EDITS[name]:
        c, r = MC.geometry(src, i)
        c, r = c + np.array(off, np.float32), np.float32(r * np.float32(factor))
        text = MC.edited(text, i, c, r)
        steps.append((i, c, r, text))
    return steps


def oracle_text_frame(key, text, w, h, spp, depth):
    return memo(("oracle text", key, w, h, spp, depth),
                lambda: O.Scene(text).render(w, h, spp, depth, mode=O.RNG_COUNTER, seed=R.DEFAULT_SEED, nthreads=NT)[0])


@pytest.mark.parametrize("name", list(GEO_EDITS))
def test_g_geometry_edits_with_frames_in_flight(name):
    """Case (g) with rt_world_set_sphere_geometry: the first edit is made while the heavy
    frame 0 runs, and the call waits for it on the host before the tree and the packed
    spheres change; each light frame is the oracle's of the edited scene text."""
    torch, (s,) = gpu(1)
    w, h, spp = 96, 64, 16
    steps = geo_steps(name)
    want = [solo(name, w, h, A_SPP, A_DEPTH)[0]]
    for k, (_, _, _, text) in enumerate(steps):
        want.append(oracle_text_frame((name, k), text, w, h, spp, A_DEPTH))
        before = want[k] if k else oracle_frame(name, w, h, spp, A_DEPTH)
        assert (want[-1] != before).any(axis=2).sum() >= 40, f"{name}: edit {k} changes too few pixels to be seen"
    outs = [frame_buf(torch, w, h) for _ in want]
    world = R.World(source(name))
    enqueue(world, w, h, outs[1], s.cuda_stream, spp, A_DEPTH)
    torch.cuda.synchronize()
    outs[1].zero_()
    torch.cuda.synchronize()

    enqueue(world, w, h, outs[0], s.cuda_stream, A_SPP, A_DEPTH)
    e0 = mark(torch, s)
    running = not e0.query()
    events = [("frame 0", e0)]
    for k, (i, c, r, _) in enumerate(steps, 1):
        world.set_sphere(i, c, r)
        enqueue(world, w, h, outs[k], s.cuda_stream, spp, A_DEPTH)
        events.append((f"frame {k}", mark(torch, s)))
    torch.cuda.synchronize()

    assert_in_flight(running, f"{name}: the first geometry edit")
    assert_ordered(events, f"{name}: frames after geometry edits")
    assert_bits_equal(as_frame(outs[0], w, h), want[0], f"{name}: frame 0 against its solo render")
    for k in range(1, len(want)):
        assert_bits_equal(as_frame(outs[k], w, h), want[k], f"{name}: frame {k} against the oracle of the edited text")
    world.close()


# ---- (j) history resolves behind an accumulator's pass --------------------------------------------------

@pytest.mark.parametrize("clamp", [None, dict(gamma=1.0, radius=2)], ids=["plain", "clamp"])
def test_j_history_resolves_behind_a_running_pass(clamp):
    """The set-up resolves 3 samples of a camera moved aside, so the history holds that
    view.  Then, back at the scene's camera and behind a heavy frame on sA: add(2) on sA,
    the resolve on sB, a second, filtered resolve on sC (it reads the prev the first one
    made of the set-up's view, rewrites the same cur and runs the filter behind the first
    one's use of its staging), and rt_history_read_length at once, which waits by itself."""
    torch, (sA, sB, sC) = gpu(3)
    w, h, stride = 96, 64, 8
    hw, hh = A_W, A_H
    want_heavy, _ = solo("rtow", hw, hh, A_SPP, A_DEPTH)
    world = R.World(source("rtow"))
    cam0 = world.camera()
    world.translate_camera(0.02, 0.0, 0.0)
    cam_p = world.camera()

    def expect():
        moved = O.Scene(source("rtow"))
        moved.set_camera(cam_p)
        sums_p = Expect(moved, w, h, stride, 8).sums(3)
        rec_p = world.first_hit(w, h, device=0)  # (pinned by test_gpu_first_hit.py)
        world.set_camera(cam0)
        rec = world.first_hit(w, h, device=0)
        world.set_camera(cam_p)
        ref = HR.History() if clamp is None else CR.ClampHistory(clamp=clamp)
        ref.resolve(sums_p, np.full((h, w), 3, np.uint32), rec_p, cam_p, 0)
        rgb, px, length = ref.resolve(exp.sums(2), np.full((h, w), 2, np.uint32), rec, cam0, 0)
        assert (length > 2).any(), "no pixel takes history: the resolves would not read prev"
        return rgb, px, length, FR.filter_image(rgb, rec)

    exp = memo("d expect", lambda: Expect(O.Scene(source("rtow")), w, h, stride, 8))
    want_rgb, want_px, want_len, want_filtered = memo(("j expect", str(clamp)), expect)
    out_heavy = frame_buf(torch, hw, hh)
    out_2, px_1, px_2 = (frame_buf(torch, w, h) for _ in range(3))
    rgb_1, rgb_2 = (torch.zeros(h * w * 3, dtype=torch.float32, device="cuda") for _ in range(2))
    acc = world.accumulator(w, h, stride, device=0)
    acc.history_enable()
    if clamp is not None:
        acc.clamp_enable(**clamp)
    acc.add_device(3, out_2.data_ptr(), sB.cuda_stream)  # (the moved camera's view; every kernel and buffer)
    acc.resolved_device(rgb_2.data_ptr(), px_2.data_ptr(), sC.cuda_stream, filter={})
    acc.resolved_device(rgb_1.data_ptr(), px_1.data_ptr(), sB.cuda_stream)
    world.set_camera(cam0)
    enqueue(world, hw, hh, out_heavy, sA.cuda_stream, **B)
    torch.cuda.synchronize()
    for t in (out_heavy, out_2, px_1, px_2, rgb_1, rgb_2):
        t.zero_()
    torch.cuda.synchronize()

    enqueue(world, hw, hh, out_heavy, sA.cuda_stream, A_SPP, A_DEPTH)
    assert acc.add_device(2, out_2.data_ptr(), sA.cuda_stream) is None
    e1 = mark(torch, sA)
    acc.resolved_device(rgb_1.data_ptr(), px_1.data_ptr(), sB.cuda_stream)
    e2 = mark(torch, sB)
    acc.resolved_device(rgb_2.data_ptr(), px_2.data_ptr(), sC.cuda_stream, filter={})
    e3 = mark(torch, sC)
    running = not e1.query()
    length = acc.history_length()  # (no synchronise before it)
    held = acc.samples
    torch.cuda.synchronize()

    what = f"history resolves on two streams ({'clamp' if clamp else 'plain'})"
    assert_in_flight(running, what)
    assert_ordered([("add(2)", e1), ("the resolve", e2), ("the filtered resolve", e3)], what)
    assert held == 2
    same_bits(length, want_len, f"{what}: history_length read with no wait before")
    assert_bits_equal(as_frame(out_heavy, hw, hh), want_heavy, f"{what}: the heavy frame against its solo render")
    assert_bits_equal(as_frame(out_2, w, h), exp.frame(2), f"{what}: frame after add(2)")
    same_bits(rgb_1.cpu().numpy().reshape(h, w, 3), want_rgb, f"{what}: the resolve on sB, out_rgb")
    assert as_frame(px_1, w, h).tobytes() == want_px.tobytes(), f"{what}: the resolve on sB, RGBA8"
    got = (rgb_2.cpu().numpy().reshape(h, w, 3), as_frame(px_2, w, h))
    assert_same(got, want_filtered, f"{what}: the filtered resolve on sC")
    acc.close()
    world.close()


# ---- (j') a geometry edit with a move-path resolve in flight --------------------------------------------

def test_j_geometry_edit_with_a_move_resolve_in_flight():
    """A resolve that follows a moved sphere reads the device's sphere array and the
    accumulator's table of prev's spheres.  It is enqueued on sB behind a heavy pass of
    its accumulator (on sA) and a heavy frame of the same world (on sB); then the sphere
    is moved again, on the host, with no wait; then add and a second resolve.  The
    resolve's own call waits on the host for the accumulator's pass (it rewrites the
    table's staging: history.cpp upload_prev_spheres), so what is still running when it
    returns, and when the edit is made, is the frame in front of it on sB.

    Everything expected comes from a twin world that goes through the same calls one at
    a time, before the first enqueue: its sums, records and spheres, restated by
    MoveHistory."""
    torch, (sA, sB) = gpu(2)
    w, h, hw, hh = 96, 64, A_W, A_H
    src = source("three_spheres")
    ball = 1
    c, r = MC.geometry(src, ball)
    d = np.array([0.05, 0.02, 0.0], np.float32)
    clamp = dict(gamma=1.0, radius=2, keep_on_edit=True)
    cap = 65536.0  # max_history

    def session():
        world = R.World(src)
        acc = world.accumulator(w, h, A_SPP + 8, device=0)
        acc.history_enable(max_history=cap)  # (above the pass's samples: its resolve still blends)
        acc.clamp_enable(**clamp)
        return world, acc

    def expect():
        world, acc = session()
        ref = MR.MoveHistory(max_history=cap, clamp=clamp)
        want = []
        for edit, (k, centre) in enumerate(((2, None), (A_SPP, c + d), (1, c + d + d))):
            if centre is not None:
                world.set_sphere(ball, centre, r)
            acc.add(k, stats=False)
            rec = world.first_hit(w, h, device=0)
            want.append(ref.resolve(acc.sums(), np.full((h, w), k, np.uint32), rec, world.camera(), edit,
                                    world.spheres()[:, :4]))
            if edit == 1:
                heavy = world.render(hw, hh, A_SPP, A_DEPTH, device=0)[0]
            if edit:
                on = rec["prim"] == ball + 1
                assert ref.prev["spheres"].tobytes() != world.spheres()[:, :4].tobytes()  # (the motion path)
                assert on.sum() > 100 and (want[-1][2][on] > k).any(), "the ball takes no history: nothing to follow"
        acc.close()
        world.close()
        return want, heavy

    want, want_heavy = memo("j' expect", expect)
    world, acc = session()
    out_heavy = frame_buf(torch, hw, hh)
    px_1, px_2 = frame_buf(torch, w, h), frame_buf(torch, w, h)
    rgb_1, rgb_2 = (torch.zeros(h * w * 3, dtype=torch.float32, device="cuda") for _ in range(2))
    acc.add(2, stats=False)
    rgb_0, px_0 = acc.resolved()
    torch.cuda.synchronize()

    world.set_sphere(ball, c + d, r)
    assert acc.add_device(A_SPP, 0, sA.cuda_stream) is None
    e1 = mark(torch, sA)
    enqueue(world, hw, hh, out_heavy, sB.cuda_stream, A_SPP, A_DEPTH)
    acc.resolved_device(rgb_1.data_ptr(), px_1.data_ptr(), sB.cuda_stream)
    e2 = mark(torch, sB)
    running = not e2.query()
    world.set_sphere(ball, c + d + d, r)  # (no synchronise before it: the call waits by itself)
    assert acc.add_device(1, 0, sA.cuda_stream) is None
    acc.resolved_device(rgb_2.data_ptr(), px_2.data_ptr(), sB.cuda_stream)
    e3 = mark(torch, sB)
    length = acc.history_length()
    torch.cuda.synchronize()

    what = "a geometry edit with a move-path resolve in flight"
    assert_in_flight(running, what)
    assert_ordered([("the heavy pass", e1), ("the first resolve", e2), ("the second resolve", e3)], what)
    same_bits(rgb_0, want[0][0], f"{what}: the set-up's resolve")
    assert px_0.tobytes() == want[0][1].tobytes()
    assert_bits_equal(as_frame(out_heavy, hw, hh), want_heavy, f"{what}: the heavy frame against the twin's")
    for k, (rgb, px) in enumerate(((rgb_1, px_1), (rgb_2, px_2)), 1):
        same_bits(rgb.cpu().numpy().reshape(h, w, 3), want[k][0], f"{what}: resolve {k}, out_rgb")
        assert as_frame(px, w, h).tobytes() == want[k][1].tobytes(), f"{what}: resolve {k}, RGBA8"
    same_bits(length, want[2][2], f"{what}: history_length after the second resolve")
    acc.close()
    world.close()
