"""Several host threads in one process (raytracer_amd.h: "calls from several host
threads on one handle are serialised by a lock"; the error string is per thread).

At most four Python threads, released together by a barrier; ctypes drops the
GIL around every library call, so the calls overlap.  An exception in a thread
is kept and raised again by the test.  Everything expected is the oracle's
(nthreads <= 4), Expect's or filter_ref's and is computed before the threads
start.

What each case goes through (csrc/):
  (a) one world, four threads      WorldState::mu around whole frames (render_frame_host),
                                   COUNTER counted and uncounted, the slab, and SERIAL (all on
                                   the library's stream: the lock alone keeps them apart)
  (b) four worlds, four threads    nothing shared: device states, the filters' RtFilter::mu,
                                   the launched-instance sets
  (c) errors are per thread        the thread-local error string (device_state.cpp g_error)
  (d) an accumulator's lifetime    WorldState::mu (passes against reads), g_accum_mu and
                                   rt_free_world's wait for the calls under way

rt_read_samples reads "the last trace launch" of its world, whoever launched it.
A thread that renders with keep_samples and then reads the samples can hold no
expectation across other threads' frames on the same world, so in (a) that
thread has a world of its own (same scene, same device); the other three share one.
"""
import threading

import numpy as np
import pytest

import filter_ref as FR
import oracle as O
import raytracer_amd as R
import scenes as S
import test_gpu_first_hit as FH
from conftest import scene_text
from test_gpu_accum import Expect, assert_sums_equal
from test_gpu_filter import assert_same
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order

pytestmark = pytest.mark.gpu

DEPTH = 8
SOURCES = {
    "rtow": S.rtow,
    "c_raytracer_world": lambda: scene_text("c_raytracer_world.txt"),
    "three_spheres": lambda: scene_text("three_spheres.txt"),
    "soup": lambda: S.triangle_soup(7, 300, spheres=40, grid=6),
}


def run_threads(*bodies, timeout=120):
    """Runs bodies[k](k) on a thread each, released together; raises the first exception."""
    assert len(bodies) <= 4
    barrier = threading.Barrier(len(bodies))
    errors = [None] * len(bodies)

    def main(k):
        try:
            barrier.wait(timeout)
            bodies[k](k)
        except BaseException as e:  # (raised again below, in the test's thread)
            errors[k] = e

    threads = [threading.Thread(target=main, args=(k,)) for k in range(len(bodies))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout)
    assert not any(t.is_alive() for t in threads), "a thread did not return"
    for k, e in enumerate(errors):
        if e is not None:
            raise AssertionError(f"thread {k}: {e!r}") from e


# ---- (a) one world, four threads ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["rtow", "c_raytracer_world"])
def test_a_one_world_four_threads(name):
    src = SOURCES[name]()
    ref = O.Scene(src)
    counted = ref.render(40, 24, 8, DEPTH, mode=O.RNG_COUNTER, nthreads=4)  # (frame, stats, ...)
    lean = ref.render(33, 17, 3, DEPTH, mode=O.RNG_COUNTER, nthreads=4)
    kept = ref.render(16, 12, 2, DEPTH, mode=O.RNG_COUNTER, record_samples=True, nthreads=4)
    serial = ref.render(24, 18, 4, DEPTH, mode=O.RNG_SERIAL)
    kept_samples = oracle_samples_to_gpu_order(kept[3], 16, 12, 2)[:, :3]
    world, own = R.World(src), R.World(src)  # (own: the read_samples thread's, module docstring)
    world.render(8, 8, 1, 1, device=0)
    own.render(8, 8, 1, 1, device=0)
    loops = 5

    def counted_frames(k):
        for i in range(loops):
            out, st = world.render(40, 24, 8, DEPTH, device=0)
            assert_bits_equal(out, counted[0], f"{name}: counted frame, loop {i}")
            assert st["rays"] == counted[1]["rays"] and st["samples"] == 40 * 24 * 8, (name, i, st["rays"])

    def lean_frames(k):
        for i in range(loops):
            out, st = world.render(33, 17, 3, DEPTH, stats=False, device=0)
            assert st is None
            assert_bits_equal(out, lean[0], f"{name}: frame without stats, loop {i}")

    def kept_frames(k):
        for i in range(loops):
            out, st = own.render(16, 12, 2, DEPTH, keep_samples=True, device=0)
            assert_bits_equal(out, kept[0], f"{name}: slab frame, loop {i}")
            assert st["rays"] == kept[1]["rays"] and st["fused_resolve"] == 0
            assert_bits_equal(own.read_samples(16 * 12 * 2, device=0)[:, :3], kept_samples,
                              f"{name}: samples read back, loop {i}")

    def serial_frames(k):
        for i in range(loops):
            out, st = world.render(24, 18, 4, DEPTH, mode=R.RNG_SERIAL, device=0)
            assert_bits_equal(out, serial[0], f"{name}: SERIAL frame, loop {i}")
            assert st["rays"] == serial[1]["rays"], (name, i, st["rays"])

    run_threads(counted_frames, lean_frames, kept_frames, serial_frames)
    world.close()
    own.close()


# ---- (b) four worlds, four threads ----------------------------------------------------------------

def test_b_four_worlds_four_threads():
    w, h, spp, stride = 32, 20, 4, 8
    names = ["three_spheres", "rtow", "soup", "rtow"]
    srcs = {n: SOURCES[n]() for n in set(names)}
    want = {}
    for n, src in srcs.items():
        ref = O.Scene(src)
        frame, ost, _ = ref.render(w, h, spp, DEPTH, mode=O.RNG_COUNTER, nthreads=4)
        exp = Expect(ref, w, h, stride, DEPTH)
        exp.frame(3), exp.frame(8), exp.sums(8)
        rec = FH.restate(src, w, h)
        rgb = FR.means(exp.sums(8), 8)
        want[n] = dict(frame=frame, rays=ost["rays"], exp=exp, rec=rec, filtered=FR.filter_image(rgb, rec))
    instances = R.trace_instances()
    worlds = [R.World(srcs[n]) for n in names]

    def body(k):
        n, world, x = names[k], worlds[k], want[names[k]]
        what = f"world {k} ({n})"
        out, st = world.render(w, h, spp, DEPTH, device=0)
        assert_bits_equal(out, x["frame"], f"{what}: frame")
        assert st["rays"] == x["rays"], what
        acc = world.accumulator(w, h, stride, depth=DEPTH, device=0)
        out, _ = acc.add(3)
        assert_bits_equal(out, x["exp"].frame(3), f"{what}: accumulated frame of 3")
        out, _ = acc.add(5)
        assert_bits_equal(out, x["exp"].frame(8), f"{what}: accumulated frame of 8")
        assert acc.samples == 8
        assert_sums_equal(acc.sums(), x["exp"].sums(8), f"{what}: sums")
        assert_same(acc.filtered(), x["filtered"], f"{what}: filtered()")
        FH.assert_records(world.first_hit(w, h, device=0), x["rec"], f"{what}: first-hit records")
        launched = world.trace_launched(clear=True, device=0)
        assert launched.any(), f"{what}: no instance recorded"
        assert not (launched & ~instances).any(), f"{what}: a key outside rt_trace_instances"
        assert not world.trace_launched(device=0).any(), f"{what}: the set was not cleared"
        acc.close()

    run_threads(body, body, body, body)
    for world in worlds:
        world.close()


# ---- (c) errors are per thread ---------------------------------------------------------------------

def test_c_errors_are_per_thread():
    src = SOURCES["rtow"]()
    frame = O.Scene(src).render(40, 24, 4, DEPTH, mode=O.RNG_COUNTER, nthreads=4)[0]
    bad_world, good_world = R.World(src), R.World(src)
    good_world.render(8, 8, 1, 1, device=0)
    flt = R.Filter(8, 8, device=0)
    acc = bad_world.accumulator(8, 8, 4, device=0)
    rgb, rec = np.zeros((8, 8, 3), np.float32), np.zeros((8, 8), R.FIRST_HIT_DTYPE)
    done = threading.Event()
    words = ("levels", "exceed", "ndevices")

    def errors(k):
        try:
            for i in range(20):
                with pytest.raises(R.RenderError, match="rt_filter_run: levels must be 0 to 8"):
                    flt.run(rgb, rec, levels=9)
                assert R.last_error() == "rt_filter_run: levels must be 0 to 8"
                with pytest.raises(R.RenderError, match="rt_accum_add: 0 \\+ 5 samples exceed"):
                    acc.add(5)
                assert R.last_error().startswith("rt_accum_add: 0 + 5 samples exceed")
                with pytest.raises(R.RenderError, match="ndevices renders the whole frame"):
                    bad_world.render_device(8, 8, 0, 0, spp=1, depth=1, rank=1, nranks=2, ndevices=1, device=0,
                                            stats=False)
                assert R.last_error() == "ndevices renders the whole frame: rank/nranks must be 0/1"
        finally:
            done.set()

    def frames(k):
        n = 0
        while n < 5 or not done.is_set():
            assert R.last_error() == "", f"another thread's error: {R.last_error()!r}"
            out, _ = good_world.render(40, 24, 4, DEPTH, device=0)
            assert_bits_equal(out, frame, f"frame {n} next to a thread of errors")
            assert not any(x in R.last_error() for x in words), R.last_error()
            n += 1
            assert n < 10000

    run_threads(errors, frames)
    assert acc.samples == 0
    acc.close()
    flt.close()
    bad_world.close()
    good_world.close()


# ---- (d) an accumulator's lifetime across threads ------------------------------------------------------

def test_d_accumulator_reads_next_to_passes_then_a_freed_world():
    src = SOURCES["rtow"]()
    w, h, stride, split = 24, 16, 16, (1, 2, 3, 2, 4, 4)
    exp = Expect(O.Scene(src), w, h, stride, DEPTH)
    ends = np.cumsum(split).tolist()
    sums = {0: np.zeros((h, w, 3), np.float32), **{n: exp.sums(n) for n in ends}}
    frames = {n: exp.frame(n) for n in ends}
    world = R.World(src)
    acc = world.accumulator(w, h, stride, depth=DEPTH, device=0)
    assert acc.samples == 0
    done = threading.Event()

    def adds(k):
        try:
            for n, end in zip(split, ends):
                out, _ = acc.add(n)
                assert_bits_equal(out, frames[end], f"frame after {end} samples")
        finally:
            done.set()

    def reads(k):
        loops = 0
        while loops < 5 or not done.is_set():
            n1 = acc.samples
            got = acc.sums()
            n2 = acc.samples
            assert acc.active == w * h
            assert n1 <= n2 and n1 in sums and n2 in sums, (n1, n2)
            # the sums of a completed pass: of some N held between the two reads of N
            held = [n for n in sums if n1 <= n <= n2 and got.tobytes() == sums[n].tobytes()]
            assert held, f"sums read between N = {n1} and N = {n2} are those of no completed pass"
            loops += 1
            assert loops < 100000
        assert_sums_equal(acc.sums(), sums[ends[-1]], "sums after the last pass")

    run_threads(adds, reads)
    assert acc.samples == stride

    # the world is freed on one thread while the other keeps calling the accumulator
    closed = threading.Event()
    calls = {"before": 0, "after": 0}

    def close(k):
        world.close()
        closed.set()

    def keep_calling(k):
        after = 0
        while after < 20:
            was_closed = closed.is_set()
            for call in (lambda: acc.samples, acc.sums, lambda: acc.active, lambda: acc.add(1)):
                try:
                    call()
                except R.RenderError as e:
                    assert "world was freed" in str(e) or (not was_closed and "exceed" in str(e)), str(e)
                else:
                    assert not was_closed, "a call on the accumulator of a freed world succeeded"
            calls["after" if was_closed else "before"] += 1
            after += was_closed

    run_threads(keep_calling, close)
    assert calls["after"] == 20
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.filtered()
    acc.close()
