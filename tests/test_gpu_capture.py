"""Frames captured into a HIP graph and replayed (raytracer_amd.h, rt_render_device:
"Capture"; DESIGN.md 4, "Capture").  tests/hip_graph.py begins and ends the captures
(thread-local mode, on non-blocking torch streams) and launches the graphs.

Expected bytes: the oracle's COUNTER frame of the same request, raw RGBA8 bits (for
REPLAY: the oracle's SERIAL frame of the table's states), as in tests/test_gpu_parity.py,
all computed before the first enqueue.  Every output buffer is filled with 0x5A on the
stream in front of every replay and every eager frame, so a launch that writes nothing
cannot pass on an earlier launch's bytes, and where replays follow each other without a
host wait a device-to-device copy behind each keeps its frame; one wait at the end.
A captured request's seed is never rendered outside the capture.

NULL STREAM.  Nothing here runs on the legacy null stream (torch's default stream) between
two launches of one executable graph: fills and copies go to the non-blocking stream that
launches.  Measured while writing this file (profiles/capture/null_stream.txt): with a
torch fill_ and clone on the default stream between two launches of the same graph, and no
library call at all in between, the second and third launch left every traced row
untouched (4864 of 9216 bytes poison, the sky kernel's 17 rows written); with the same
operations on the launching stream every launch is right.  The library has no part in
that sequence, so it is left to the runtime; a caller is told in INTEGRATION.md.

What each case fails on when the host runtime is wrong:
  a  the graph is not the one-stream chain (a fork inside a capture, a fence's event node),
     or work ran during the capture
  b  the job counters' parity: the second replay takes the set its first replay spent,
     finds no job and traces nothing (the parent commit: in replays 2 and 3, 4858 of 9216
     bytes differ and 4864 are poison -- the 19 traced rows; the sky kernel, which takes no
     job, still writes its 17 rows: profiles/capture/parent_case_b.txt)
  c  a capture flips the host's parity or marks a set clean that no launch zeroed: the
     eager frame behind it writes nothing
  d  two graphs sharing the captured set's fill; lists or rings that a graph's nodes name,
     rebuilt or freed by the warm-up of another size
  e  a launch of a multi-launch graph without its fill node; the slab path's samples
  f  triangle frames: the device lists of the warm frame, walked by the replays
  g  the REPLAY table's copy node
  h  a cold request that enqueues a node, or that leaves the host believing the lists of
     the new camera are built (the parent commit: the next eager frame walks the old
     camera's lists)
  i  a refused call that changed something
  j  a graph's nodes outliving the world whose buffers they name (never launched here)
"""
import ctypes as C
import os

import numpy as np
import pytest

import hip_graph as G
import oracle as O
import raytracer_amd as R
from conftest import scene_text
from test_gpu_parity import assert_bits_equal, oracle_samples_to_gpu_order
from test_gpu_streams import as_frame, enqueue, frame_buf, gpu, memo, oracle_frame, source

pytestmark = pytest.mark.gpu

NT = max(1, min(16, len(os.sched_getaffinity(0))))  # oracle threads
POISON = 0x5A
RTOW = (64, 36, dict(spp=4, depth=8))   # sky rows from the second frame on, corner records in LDS
SOUP = (48, 32, dict(spp=4, depth=8))   # triangle trees, device strip lists
WARM_SEED = 11                           # (no captured frame uses it)
COLD = "outside the capture"             # what rt_last_error says of a cold request


def poison(torch, s, out):
    with torch.cuda.stream(s):
        out.fill_(POISON)


def keep(torch, s, out):
    """A copy of out behind what s holds, on s."""
    with torch.cuda.stream(s):
        return out.clone()


def warm(torch, world, w, h, out, stream_ptr, frames=2, **frame):
    """The request rendered outside a capture (twice: the second frame has its sky rows), the device idle."""
    for _ in range(frames):
        enqueue(world, w, h, out, stream_ptr, **dict(frame, seed=WARM_SEED))
    torch.cuda.synchronize()


def capture(world, w, h, out, s, **frame):
    with G.Capture(s.cuda_stream) as cap:
        enqueue(world, w, h, out, s.cuda_stream, **frame)
    return cap


def replay(torch, s, cap, out):
    """Poison, one replay, the kept copy: all on s, no host wait."""
    poison(torch, s, out)
    cap.launch()
    return keep(torch, s, out)


def eager(torch, s, world, w, h, out, stream_ptr, **frame):
    """The same for a frame outside a capture (on the library's stream: waits on the host around it)."""
    if stream_ptr == 0:  # (the fill and the copy stay on s: see NULL STREAM in the module's docstring)
        torch.cuda.synchronize()
        poison(torch, s, out)
        torch.cuda.synchronize()
        enqueue(world, w, h, out, 0, **frame)
        torch.cuda.synchronize()
        t = keep(torch, s, out)
        torch.cuda.synchronize()
        return t
    poison(torch, s, out)
    enqueue(world, w, h, out, stream_ptr, **frame)
    return keep(torch, s, out)


def check_all(kept, w, h, what):
    """kept: [(name, tensor, expected frame)], read after a synchronise."""
    bad = []
    for name, t, want in kept:
        got = as_frame(t, w, h)
        n = int((got != want).sum())
        print(f"{what}: {name}: {n} of {got.size} bytes differ, {int((got == POISON).sum())} are 0x5A")
        if n:
            bad.append(name)
    for name, t, want in kept:
        assert_bits_equal(as_frame(t, w, h), want, f"{what}: {name}")
    assert not bad


def try_frame(world, w, h, out, stream_ptr, stats=False, **opts):
    """rt_render_device -> (rc, rt_last_error) without raising."""
    o, table = R.options(device=0, L=world._L, **opts)
    st = R.RenderStats()
    rc = world._L.rt_render_device(world.handle, w, h, C.byref(o), C.c_void_p(out.data_ptr()),
                                   C.c_void_p(stream_ptr or None), C.byref(st) if stats else None)
    del table
    return rc, R.last_error()


# ---- a. the shape of a captured frame -------------------------------------------------------

def test_a_shape_of_a_captured_frame(monkeypatch):
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    want = oracle_frame("rtow", w, h, seed=21, **frame)
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    poison(torch, s, out)
    torch.cuda.synchronize()

    cap = capture(world, w, h, out, s, seed=21, **frame)
    rows, forked = world.sky_rows(), world.sky_forked()
    torch.cuda.synchronize()
    during = out.cpu().numpy()
    types = cap.chain()  # (asserts one root, edges == nodes - 1, no node with two successors)
    print("captured frame:", [G.TYPE_NAMES.get(t, t) for t in types], f"sky rows {rows}")
    assert 0 < rows < h and forked == 0, (rows, forked)
    assert (during == POISON).all(), "work ran during the capture"
    assert types.count(G.KERNEL) == 1 + 1, types  # (the sky kernel and one trace launch)
    assert types == [G.KERNEL, G.MEMSET, G.KERNEL], types  # (... behind the captured set's fill)

    monkeypatch.setenv("RT_AMD_SKY_FORK", "0")
    off = capture(world, w, h, out, s, seed=21, **frame)
    monkeypatch.delenv("RT_AMD_SKY_FORK")
    assert off.chain() == types
    kept = [("the replay", replay(torch, s, cap, out), want),
            ("the RT_AMD_SKY_FORK=0 graph's replay", replay(torch, s, off, out), want)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "shape")
    cap.close(), off.close()
    world.close()


# ---- b. three replays back to back ----------------------------------------------------------

def test_b_three_replays_back_to_back():
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    want = oracle_frame("rtow", w, h, seed=22, **frame)
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    cap = capture(world, w, h, out, s, seed=22, **frame)
    kept = [(f"replay {k + 1}", replay(torch, s, cap, out), want) for k in range(3)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "back to back")
    cap.close()
    world.close()


# ---- c. a capture does not disturb the eager frames -----------------------------------------

@pytest.mark.parametrize("eager_on", ["the same stream", "the library's stream"])
def test_c_capture_between_eager_frames(eager_on):
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    seeds = dict(G=30, e1=31, e2=32, e3=33)
    want = {k: oracle_frame("rtow", w, h, seed=v, **frame) for k, v in seeds.items()}
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    ptr = s.cuda_stream if eager_on == "the same stream" else 0
    wait = torch.cuda.synchronize if ptr == 0 else (lambda: None)
    warm(torch, world, w, h, out, ptr, **frame)

    def eager_frame(k):
        return (f"eager frame {k}", eager(torch, s, world, w, h, out, ptr, seed=seeds[k], **frame), want[k])

    def replay_g(k):
        wait()
        t = replay(torch, s, cap, out)
        wait()
        return (f"replay {k}", t, want["G"])

    cap = capture(world, w, h, out, s, seed=seeds["G"], **frame)  # (not launched yet)
    kept = [eager_frame("e1"), replay_g(1), eager_frame("e2"), replay_g(2), replay_g(3), eager_frame("e3")]
    torch.cuda.synchronize()
    check_all(kept, w, h, f"eager frames on {eager_on}")
    cap.close()
    world.close()


# ---- d. two graphs of one world -------------------------------------------------------------

def test_d_two_graphs_two_seeds():
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    want = [oracle_frame("rtow", w, h, seed=seed, **frame) for seed in (41, 42)]
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    caps = [capture(world, w, h, out, s, seed=seed, **frame) for seed in (41, 42)]
    kept = [(f"G{g + 1} (launch {k})", replay(torch, s, caps[g], out), want[g]) for k, g in enumerate((0, 1, 0, 0, 1))]
    torch.cuda.synchronize()
    check_all(kept, w, h, "two seeds")
    for cap in caps:
        cap.close()
    world.close()


@pytest.mark.parametrize("sizes", [((64, 36), (48, 27)), ((48, 27), (80, 45))],
                         ids=["smaller second", "larger second"])
def test_d_two_graphs_two_sizes(sizes):
    """Each size is warmed and captured in turn.  The second size's warm-up rebuilds the
    device's primary lists and, where it is the larger, grows the sample rings: the first
    graph's nodes still name the old ones, which the device state therefore keeps
    (DeviceState::retire).  Without that, smaller second: every launch of G1 differed from
    the oracle in 50 of 9216 bytes -- pixels tested against another frame's candidate
    spheres (profiles/capture/capture_two_sizes_before.txt)."""
    torch, (s,) = gpu(1)
    _, _, frame = RTOW
    want = [oracle_frame("rtow", w, h, seed=43 + g, **frame) for g, (w, h) in enumerate(sizes)]
    outs = [frame_buf(torch, w, h) for w, h in sizes]
    world = R.World(source("rtow"))
    caps = []
    for g, (w, h) in enumerate(sizes):
        warm(torch, world, w, h, outs[g], s.cuda_stream, **frame)
        caps.append(capture(world, w, h, outs[g], s, seed=43 + g, **frame))
    kept = [[], []]
    for k, g in enumerate((0, 1, 0, 0, 1)):
        kept[g].append((f"G{g + 1} (launch {k})", replay(torch, s, caps[g], outs[g]), want[g]))
    torch.cuda.synchronize()
    for g, (w, h) in enumerate(sizes):
        check_all(kept[g], w, h, f"two sizes, {w}x{h}")
    for cap in caps:
        cap.close()
    world.close()


def test_d_two_graphs_two_cameras_of_a_triangle_scene():
    """The same for a camera move on the soup: the camera-origin records and the device's
    strip lists that the first graph's nodes name are kept when the move replaces them."""
    torch, (s,) = gpu(1)
    w, h, frame = SOUP
    shift = (0.3, 0.2, 0.5)
    probe = R.World(source("soup"))
    cams = [probe.camera()]
    probe.move_camera(*shift)
    cams.append(probe.camera())
    probe.close()

    def oracle_at(g):
        def make():
            ref = O.Scene(source("soup"))
            ref.set_camera(cams[g])
            return ref.render(w, h, frame["spp"], frame["depth"], mode=O.RNG_COUNTER, seed=46 + g, nthreads=NT)[0]
        return memo(("capture soup camera", g), make)
    want = [oracle_at(0), oracle_at(1)]
    out = frame_buf(torch, w, h)
    world = R.World(source("soup"))
    caps = []
    for g in range(2):
        if g:
            world.move_camera(*shift)
        warm(torch, world, w, h, out, s.cuda_stream, **frame)
        caps.append(capture(world, w, h, out, s, seed=46 + g, **frame))
        assert world.primary_tri_lists() == 2
    kept = [(f"G{g + 1} (launch {k})", replay(torch, s, caps[g], out), want[g]) for k, g in enumerate((0, 1, 0, 0, 1))]
    torch.cuda.synchronize()
    check_all(kept, w, h, "two cameras")
    for cap in caps:
        cap.close()
    world.close()


# ---- e. several launches; the slab path -----------------------------------------------------

def test_e_a_frame_of_several_launches(monkeypatch):
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    rows_per_launch = 8
    want = oracle_frame("rtow", w, h, seed=51, **frame)
    out = frame_buf(torch, w, h)
    monkeypatch.setenv("RT_AMD_SLAB_JOBS", str(w * frame["spp"] * rows_per_launch))
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    cap = capture(world, w, h, out, s, seed=51, **frame)
    launches = -(-(h - world.sky_rows()) // rows_per_launch)
    types = cap.chain()
    print("several launches:", [G.TYPE_NAMES.get(t, t) for t in types], f"sky rows {world.sky_rows()}")
    assert launches >= 2 and types.count(G.KERNEL) == 1 + launches, (launches, types)
    assert types.count(G.MEMSET) == launches, types  # (every launch behind its own fill)
    kept = [(f"replay {k + 1}", replay(torch, s, cap, out), want) for k in range(2)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "several launches")
    cap.close()
    world.close()


def test_e_the_slab_path_and_its_samples():
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    spp = frame["spp"]
    want, _, _, smp = memo("capture slab", lambda: O.Scene(source("rtow")).render(
        w, h, spp, frame["depth"], mode=O.RNG_COUNTER, seed=52, record_samples=True, nthreads=NT))
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, keep_samples=True, **frame)
    cap = capture(world, w, h, out, s, seed=52, keep_samples=True, **frame)
    types = cap.chain()
    assert types.count(G.KERNEL) == 2, types  # (the trace launch and resolve_kernel; no sky kernel on this path)
    kept = [(f"replay {k + 1}", replay(torch, s, cap, out), want) for k in range(2)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "slab path")
    assert_bits_equal(world.read_samples(w * h * spp)[:, :3], oracle_samples_to_gpu_order(smp, w, h, spp)[:, :3],
                      "slab path: the samples a replay left")
    cap.close()
    world.close()


# ---- f. triangles ---------------------------------------------------------------------------

def test_f_triangles_with_device_lists():
    torch, (s,) = gpu(1)
    w, h, frame = SOUP
    want = oracle_frame("soup", w, h, seed=61, **frame)
    out = frame_buf(torch, w, h)
    world = R.World(source("soup"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    cap = capture(world, w, h, out, s, seed=61, **frame)
    assert world.primary_tri_lists() == 2
    cap.chain()
    kept = [(f"replay {k + 1}", replay(torch, s, cap, out), want) for k in range(2)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "triangles")
    cap.close()
    world.close()


# ---- g. REPLAY ------------------------------------------------------------------------------

def test_g_replay_mode_with_the_table_kept_alive():
    torch, (s,) = gpu(1)
    w, h, spp = 40, 30, 3
    src = scene_text("c_raytracer_world.txt")
    want, _, states = memo("capture replay", lambda: O.Scene(src).render(w, h, spp, 8, mode=O.RNG_SERIAL,
                                                                       record_states=True))
    out = frame_buf(torch, w, h)
    world = R.World(src)
    o, table = R.options(spp, 8, R.RNG_REPLAY, replay=states, device=0)  # (table: alive until the graph is gone)

    def frame():
        rc = world._L.rt_render_device(world.handle, w, h, C.byref(o), C.c_void_p(out.data_ptr()),
                                       C.c_void_p(s.cuda_stream), None)
        assert rc == 0, R.last_error()

    frame(), frame()
    torch.cuda.synchronize()
    with G.Capture(s.cuda_stream) as cap:
        frame()
    types = cap.chain()
    assert types.count(G.MEMCPY) == 1, types  # (the table's copy node)
    kept = [(f"replay {k + 1}", replay(torch, s, cap, out), want) for k in range(2)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "REPLAY")
    cap.close()
    del table
    world.close()


# ---- h. cold requests -----------------------------------------------------------------------

def _move(world):
    world.move_camera(0.0, 1.5, -2.0)


def _turn(world):
    x, y, z = (float(v) for v in world.camera()[:3])  # (the origin stays: only the view turns)
    world.look_at((x, y, z), (x + 0.3, y - 0.1, z - 1.0), vfov=float(np.radians(70.0)))


COLD_CASES = {
    "after move_camera": ("rtow", RTOW, _move, None),
    "after a turn in place": ("soup", SOUP, _turn, None),
    "after a resize to a larger frame": ("rtow", RTOW, None, (80, 45)),
    "on a fresh world": ("rtow", RTOW, None, None),
}


@pytest.mark.parametrize("case", list(COLD_CASES))
def test_h_cold_requests_are_refused_cleanly(case):
    torch, (s,) = gpu(1)
    name, (w0, h0, frame), change, resize = COLD_CASES[case]
    w, h = resize or (w0, h0)
    probe = R.World(source(name))  # (the camera after the change: host work only)
    if change:
        change(probe)
    cam = probe.camera()
    probe.close()

    def make():
        ref = O.Scene(source(name))
        ref.set_camera(cam)
        return ref.render(w, h, frame["spp"], frame["depth"], mode=O.RNG_COUNTER, seed=71, nthreads=NT)[0]
    want = memo(("capture cold", case), make)
    out = frame_buf(torch, max(w, w0), max(h, h0))[: w * h * 4]

    def prepare():
        world = R.World(source(name))
        if case != "on a fresh world":
            warm(torch, world, w0, h0, out, s.cuda_stream, **frame)
        if change:
            change(world)
        return world

    # what the first frame of this request reports on a world that never met a capture
    plain = prepare()
    enqueue(plain, w, h, out, s.cuda_stream, seed=71, **frame)
    expect_rows, expect_ptl = plain.sky_rows(), plain.primary_tri_lists()
    torch.cuda.synchronize()
    plain.close()

    world = prepare()
    with G.Capture(s.cuda_stream) as cap:
        rc, msg = try_frame(world, w, h, out, s.cuda_stream, seed=71, **frame)
    print(f"{case}: rc {rc}, {msg!r}")
    assert rc < 0 and COLD in msg, (rc, msg)
    assert cap.nodes() == [], [G.TYPE_NAMES.get(cap.node_type(n)) for n in cap.nodes()]
    cap.close()
    kept = [("the next eager frame", eager(torch, s, world, w, h, out, s.cuda_stream, seed=71, **frame), want)]
    rows, ptl = world.sky_rows(), world.primary_tri_lists()
    torch.cuda.synchronize()
    check_all(kept, w, h, case)
    assert (rows, ptl) == (expect_rows, expect_ptl), (rows, ptl, expect_rows, expect_ptl)
    world.close()


# ---- i. refusals ----------------------------------------------------------------------------

def test_i_calls_that_are_never_captured():
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    acc = world.accumulator(w, h, 8, device=0)
    acc.add_device(2, out.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    assert acc.samples == 2
    calls = {
        "rt_accum_add_device": lambda: (acc._L.rt_accum_add_device(acc._a, 2, C.c_void_p(out.data_ptr()),
                                                                   C.c_void_p(s.cuda_stream), None), R.last_error()),
        "stats": lambda: try_frame(world, w, h, out, s.cuda_stream, stats=True, **frame),
        "SERIAL": lambda: try_frame(world, w, h, out, s.cuda_stream, mode=R.RNG_SERIAL, **frame),
        "ndevices=1": lambda: try_frame(world, w, h, out, s.cuda_stream, ndevices=1, **frame),
    }
    for what, call in calls.items():
        with G.Capture(s.cuda_stream) as cap:
            rc, msg = call()
        print(f"{what}: rc {rc}, {msg!r}")
        assert rc < 0 and "cannot be captured" in msg, (what, rc, msg)
        assert cap.nodes() == [], what
        cap.close()
        assert acc.samples == 2, what
    # ... and everything still works outside a capture
    want = oracle_frame("rtow", w, h, seed=81, **frame)
    kept = [("an eager frame behind the refusals", eager(torch, s, world, w, h, out, s.cuda_stream, seed=81, **frame),
             want)]
    torch.cuda.synchronize()
    check_all(kept, w, h, "refusals")
    acc.close()
    world.close()


# ---- j. a world edited or closed while its graph exists -------------------------------------

@pytest.mark.parametrize("how", ["edited", "closed"])
def test_j_a_graph_that_outlives_its_world(how):
    """The contract: destroy the graph before the edit or the free.  A caller who did
    not must still be able to drop the graph unlaunched and go on."""
    torch, (s,) = gpu(1)
    w, h, frame = RTOW
    edit = (0, 1, (0.7, 0.6, 0.5), 0.2, False)  # (test_gpu_streams.py EDITS["rtow"][0])
    want = oracle_frame("rtow", w, h, seed=91, edits=(edit,) if how == "edited" else (), **frame)
    out = frame_buf(torch, w, h)
    world = R.World(source("rtow"))
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    stale = capture(world, w, h, out, s, seed=90, **frame)
    if how == "edited":
        i, kind, rgb, param, tri = edit
        world.set_material(i, kind, rgb, param, triangle=tri)
    else:
        world.close()
        world = R.World(source("rtow"))
    stale.close()  # (never launched)
    warm(torch, world, w, h, out, s.cuda_stream, **frame)
    cap = capture(world, w, h, out, s, seed=91, **frame)
    kept = [("the fresh capture's replay", replay(torch, s, cap, out), want)]
    torch.cuda.synchronize()
    check_all(kept, w, h, f"world {how}")
    cap.close()
    world.close()
