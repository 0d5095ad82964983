"""Progressive accumulation (rt_accum_*): a frame refined pass
by pass is, bit for bit, the frame that was never split.

A pixel is an in-order f32 fold of its samples (common.rs:333-341); a fold
stopped after sample k and continued from the stored f32 sum gives the bits of
a fold that never stopped.  So every comparison here is on raw bits: against
the one-shot frame of the same library, and against the oracle's REPLAY frame
at spp N fed the table states[(row W + col) N + s] = seed or state of the
accumulator's job (row W + col) S + s.  The expected sums are the sequential
np.float32 fold of the oracle's per-sample colours."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from conftest import scene_text
from test_gpu_corner_tree import TREE_BOX, TREE_CORNER, TREE_GLOBAL, _random_scene
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

SEED = R.DEFAULT_SEED


def _seeds(seed, jobs):
    """rt_sample_seed over an array of u64 jobs (the splitmix64 finaliser)."""
    with np.errstate(over="ignore"):
        g = np.uint64(0x9E3779B97F4A7C15)
        z = jobs.astype(np.uint64) + np.uint64(seed) * g + g
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        r = (z ^ (z >> np.uint64(32))).astype(np.uint32)
    return np.where(r == 0, np.uint32(2547549), r)


def test_seed_helper_is_the_oracles():
    jobs = np.array([0, 1, 17, 1 << 20, (1 << 32) + 5, (31 << 28) + 3], np.uint64)
    assert _seeds(SEED, jobs).tolist() == [O.sample_seed(SEED, int(j)) for j in jobs]
    assert _seeds(7, jobs).tolist() == [O.sample_seed(7, int(j)) for j in jobs]


class Expect:
    """The oracle's view of an accumulation of `scene` (an O.Scene) at w x h,
    stride S: frame(N) and sums(N) for N held samples, computed once per N."""

    def __init__(self, scene, w, h, stride, depth, seed=SEED, states=None):
        self.scene, self.w, self.h, self.S, self.depth = scene, w, h, stride, depth
        self.seed, self.states = seed, states  # states: REPLAY table at stride S
        self._memo = {}

    def table(self, n):
        pix = np.arange(self.w * self.h, dtype=np.uint64)[:, None]
        jobs = pix * np.uint64(self.S) + np.arange(n, dtype=np.uint64)[None, :]  # (64-bit jobs)
        if self.states is not None:
            return np.ascontiguousarray(self.states[jobs.reshape(-1).astype(np.int64)])
        return _seeds(self.seed, jobs.reshape(-1))

    def _get(self, n):
        if n not in self._memo:
            img, _, _, smp = self.scene.render(self.w, self.h, n, self.depth, mode=O.RNG_REPLAY,
                                               replay=self.table(n), record_samples=True, nthreads=4)
            c = smp.reshape(self.h, self.w, n, 4)[::-1, :, :, :3]  # top row first
            acc = np.zeros((self.h, self.w, 3), np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                for s in range(n):
                    acc = acc + c[:, :, s, :]  # the in-order f32 fold
            self._memo[n] = (img, acc)
        return self._memo[n]

    def frame(self, n):
        return self._get(n)[0]

    def sums(self, n):
        return self._get(n)[1]


def assert_sums_equal(a, b, what):
    """Bits, with NaN equal to NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    nan = np.isnan(a) & np.isnan(b)
    bad = np.argwhere((a.view(np.uint32) != b.view(np.uint32)) & ~nan)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first at {bad[:5].tolist()}"


def _run(acc, split, exp=None, what=""):
    """Adds the passes of `split`; with exp, checks frame and sums after every pass."""
    out = st = None
    for n in split:
        out, st = acc.add(n)
        if exp is not None:
            N = acc.samples
            assert_bits_equal(out, exp.frame(N), f"{what}{split}: frame after {N} samples")
            assert_sums_equal(acc.sums(), exp.sums(N), f"{what}{split}: sums after {N} samples")
    return out, st


# ---- 1. pass splits, COUNTER ------------------------------------------------

_RTOW = {}


def _rtow_expect():
    if not _RTOW:
        _RTOW["exp"] = Expect(O.Scene(S.rtow()), 64, 36, 16, 8)
        _RTOW["one"] = R.World(S.rtow()).render(64, 36, 16, 8)[0]
    return _RTOW["exp"], _RTOW["one"]


@pytest.mark.parametrize("split", [(16,), (4, 4, 8), (3, 5, 8), (1,) * 16, (8, 1, 7)])
def test_pass_splits_counter(split):
    exp, one = _rtow_expect()
    acc = R.World(S.rtow()).accumulator(64, 36, 16, depth=8)
    assert acc.samples == 0 and not acc.sums().any()
    out, st = _run(acc, split, exp)
    assert acc.samples == 16
    assert_bits_equal(out, one, f"{split}: final frame vs the one-shot frame at spp 16")
    assert st["sphere_tree"] == TREE_CORNER and st["fused_resolve"] == 1 and st["rays"] == 0
    assert st["samples"] == 64 * 36 * split[-1] and st["trace_launches"] == 1


# ---- 2. REPLAY reproduces the reference's stream ----------------------------

def test_replay_reproduces_the_reference_stream():
    src = scene_text("world.txt")
    w, h, stride, depth = 33, 17, 6, 8
    ref = O.Scene(src)
    img, _, states = ref.render(w, h, stride, depth, mode=O.RNG_SERIAL, record_states=True)
    exp = Expect(ref, w, h, stride, depth, states=states)
    acc = R.World(src).accumulator(w, h, stride, depth=depth, mode=R.RNG_REPLAY, replay=states)
    acc.add(1)
    out, _ = acc.add(2)
    assert_bits_equal(out, exp.frame(3), "after the second pass")
    assert_sums_equal(acc.sums(), exp.sums(3), "sums after the second pass")
    out, _ = acc.add(3)
    assert_bits_equal(out, img, "final frame vs the oracle's SERIAL frame")
    assert_sums_equal(acc.sums(), exp.sums(6), "final sums")


# ---- 3. every kernel family's accumulation instance --------------------------

def _emissive_edits(n):
    return [(i, 3, (0.9, 0.7, 0.4)) for i in range(1, n, 3)]


FAMILIES = {
    # name: (source, env, accel, size, sphere_tree or None, edits)
    "corner": (lambda: S.rtow(), {}, R.ACCEL_AUTO, (40, 24), TREE_CORNER, None),
    "box": (lambda: S.rtow(), {"RT_AMD_CORNER": "0"}, R.ACCEL_AUTO, (40, 24), TREE_BOX, None),
    "global": (lambda: S.rtow(), {"RT_AMD_LDS": "0"}, R.ACCEL_AUTO, (40, 24), TREE_GLOBAL, None),
    "brute": (lambda: S.rtow(), {}, R.ACCEL_BRUTE, (40, 24), 0, None),
    "c_raytracer": (lambda: scene_text("c_raytracer_world.txt"), {}, R.ACCEL_AUTO, (40, 30), 0, None),
    "soup": (lambda: S.triangle_soup(41, 400, spheres=40), {}, R.ACCEL_AUTO, (48, 27), None, None),
    "emissive": (lambda: _random_scene(seed=1, n=400, spread=6.0, radius=0.3), {}, R.ACCEL_AUTO, (48, 32),
                 TREE_CORNER, _emissive_edits),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_family(monkeypatch, family):
    make, env, accel, (w, h), tree, edits = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    src = make()
    world, ref = R.World(src), O.Scene(src)
    if edits:
        for (i, kind, rgb) in edits(world.num_spheres):
            world.set_material(i, kind, rgb)
            ref.set_material(i, kind, rgb)
    one, ost = world.render(w, h, 8, 8, accel=accel)
    exp = Expect(ref, w, h, 8, 8)
    acc = world.accumulator(w, h, 8, depth=8, accel=accel)
    out, st = acc.add(3)
    assert_bits_equal(out, exp.frame(3), f"{family}: first pass vs the oracle")
    assert_sums_equal(acc.sums(), exp.sums(3), f"{family}: first pass sums")
    # the intended path ran: the search and workgroup size of the lean frame
    assert st["sphere_tree"] == ost["sphere_tree"] and st["accel"] == ost["accel"]
    assert st["launch_block_threads"] == ost["launch_block_threads"]
    assert st["tri_bvh"] == ost["tri_bvh"] and st["fused_resolve"] == 1
    if tree is not None:
        assert st["sphere_tree"] == tree
    if family == "soup":
        assert st["tri_bvh"] == 1
    acc.add(1)
    out, _ = acc.add(4)
    assert_bits_equal(out, one, f"{family}: final frame vs the one-shot frame")
    assert_sums_equal(acc.sums(), exp.sums(8), f"{family}: final sums")


# ---- 4. both resolve shapes and the odd ends ---------------------------------

_BRIGHT_SRC = _random_scene(seed=2, n=300, spread=3.0, radius=0.6)


def _bright_pair():
    """test_gpu_lean_state's "bright" world (emitters at 40.0: channels
    saturate) and its oracle twin."""
    world, ref = R.World(_BRIGHT_SRC), O.Scene(_BRIGHT_SRC)
    for i in range(1, world.num_spheres, 3):
        world.set_material(i, 3, (40.0, 3.0, 0.6))
        ref.set_material(i, 3, (40.0, 3.0, 0.6))
    return world, ref


@pytest.mark.parametrize("split", [(4, 4), (8, 8), (3, 5), (5, 3, 4, 4)])
def test_resolve_shapes_within_one_accumulation(split):
    """Passes of n % 4 == 0 fold on plane lanes, the others on pixel lanes."""
    world, ref = _bright_pair()
    w, h, stride = 24, 10, sum(split)
    exp = Expect(ref, w, h, stride, 8)
    out, _ = _run(world.accumulator(w, h, stride), split, exp, "bright ")
    assert (out[..., 0] == 255).any() and (out[..., :3] < 255).any()
    assert_bits_equal(out, world.render(w, h, stride, 8)[0], "bright: final vs one-shot")


@pytest.mark.parametrize("w", [4, 5, 6, 7, 9, 10, 11])
def test_resolve_last_chunk_of_1_to_7_pixels(monkeypatch, w):
    """One partition of 8-pixel chunks over 3 w pixels: the last chunk holds 1 to 7."""
    world, ref = _bright_pair()
    split = (8, 4, 3, 1)
    exp = Expect(ref, w, 3, sum(split), 8)
    acc = world.accumulator(w, 3, sum(split))
    monkeypatch.setenv("RT_AMD_PARTS", "1")
    for n in split:
        monkeypatch.setenv("RT_AMD_CHUNK", str(8 * n))
        out, st = acc.add(n)
        assert st["launch_chunk"] == 8 * n and st["launch_parts"] == 1
        N = acc.samples
        assert_bits_equal(out, exp.frame(N), f"w {w}: frame after {N}")
        assert_sums_equal(acc.sums(), exp.sums(N), f"w {w}: sums after {N}")


@pytest.mark.parametrize("pix", ["1", "3", "64"])
def test_resolve_chunk_knob(monkeypatch, pix):
    monkeypatch.setenv("RT_AMD_RESOLVE_PIX", pix)
    world, ref = _bright_pair()
    exp = Expect(ref, 24, 10, 12, 8)
    _run(world.accumulator(24, 10, 12), (4, 3, 1, 4), exp, f"pix {pix} ")


def test_depth_0_is_an_all_zero_frame_after_every_pass():
    world, _ = _bright_pair()
    acc = world.accumulator(24, 10, 8, depth=0)
    for n in (4, 3, 1):
        out, _ = acc.add(n)
        assert not out[..., :3].any() and (out[..., 3] == 255).all()
        assert not acc.sums().any()
    assert_bits_equal(out, world.render(24, 10, 8, 0)[0], "depth 0")


@pytest.mark.parametrize("w,h", [(1, 5), (5, 1), (1, 1)])
def test_degenerate_frames_nan_directions(w, h):
    """(width - 1) or (height - 1) = 0: the camera divisions give NaN and infinite directions."""
    src = _random_scene(seed=7, n=300, spread=2.0, radius=0.4, big=False)
    world = R.World(src)
    exp = Expect(O.Scene(src), w, h, 8, 8)
    out, _ = _run(world.accumulator(w, h, 8), (4, 1, 3), exp, f"{w}x{h} ")
    assert_bits_equal(out, world.render(w, h, 8, 8)[0], f"{w}x{h}: final vs one-shot")


# ---- 5. several launches per pass -------------------------------------------

def test_several_launches_per_pass(monkeypatch):
    src = scene_text("rtow.txt")
    w, h, split = 50, 20, (8, 3, 5)
    one = R.World(src).accumulator(w, h, 16)
    frames = [(one.add(n)[0], one.sums()) for n in split]
    many = R.World(src).accumulator(w, h, 16)
    for n, (frame, sums) in zip(split, frames):
        monkeypatch.setenv("RT_AMD_SLAB_JOBS", str(w * n * 3))  # 3 rows per launch
        out, st = many.add(n)
        assert st["trace_launches"] == 7
        assert_bits_equal(out, frame, f"slabbed pass of {n}")
        assert_sums_equal(many.sums(), sums, f"slabbed pass of {n}: sums")
    monkeypatch.delenv("RT_AMD_SLAB_JOBS")
    assert_bits_equal(frames[-1][0], R.World(src).render(w, h, 16, 8)[0], "final vs one-shot")


# ---- 6. 64-bit job indices --------------------------------------------------

def test_64_bit_job_indices():
    src = scene_text("world.txt")
    w, h, stride = 8, 4, 1 << 28  # W H S = 2^33
    exp = Expect(O.Scene(src), w, h, stride, 8)
    assert int(exp.table(4).size) == w * h * 4
    acc = R.World(src).accumulator(w, h, stride)
    out, _ = acc.add(2)
    assert_bits_equal(out, exp.frame(2), "2 of 2^28")
    out, _ = acc.add(2)
    assert_bits_equal(out, exp.frame(4), "4 of 2^28")
    assert_sums_equal(acc.sums(), exp.sums(4), "sums")
    # the same pixels at a 32-bit stride start other streams
    small = R.World(src).accumulator(w, h, 4)
    assert (small.add(4)[0] != out).any()


# ---- 7. splitting above 4096 ------------------------------------------------

def test_requests_above_4096_are_split():
    world = R.World(S.rtow())
    acc = world.accumulator(12, 5, 4100)
    out, st = acc.add(4100)
    assert acc.samples == 4100
    assert st["trace_launches"] == 2 and st["samples"] == 12 * 5 * 4100
    assert_bits_equal(out, world.render(12, 5, 4100, 8)[0], "4100 samples in one add")


# ---- 8. resets ----------------------------------------------------------------

def test_resets():
    src = S.rtow()
    w, h = 40, 24
    world = R.World(src)
    acc = world.accumulator(w, h, 16)
    first, _ = acc.add(4)
    first_sums = acc.sums()
    acc.add(4)
    assert acc.samples == 8
    # a camera move
    world.move_camera(0.5, -0.25, -1.0)
    assert acc.samples == 0 and not acc.sums().any()
    out, _ = acc.add(4)
    assert acc.samples == 4
    fresh = R.World(src)
    fresh.move_camera(0.5, -0.25, -1.0)
    facc = fresh.accumulator(w, h, 16)
    moved, _ = facc.add(4)
    assert_bits_equal(out, moved, "after a camera move")
    assert_sums_equal(acc.sums(), facc.sums(), "sums after a camera move")
    assert (out != first).any()
    # a scene edit
    acc.add(4)
    world.set_material(3, 1, (0.9, 0.2, 0.2), 0.1)
    fresh.set_material(3, 1, (0.9, 0.2, 0.2), 0.1)
    out, _ = acc.add(4)
    assert acc.samples == 4 and facc.samples == 0
    edited, _ = facc.add(4)
    assert_bits_equal(out, edited, "after set_material")
    assert_sums_equal(acc.sums(), facc.sums(), "sums after set_material")
    # an explicit reset
    acc.add(2)
    acc.reset()
    assert acc.samples == 0 and not acc.sums().any()
    out, _ = acc.add(4)
    assert acc.samples == 4
    assert_bits_equal(out, edited, "after reset()")
    # back at the first camera and material: nothing of the abandoned accumulations survives
    world.move_camera(-0.5, 0.25, 1.0)
    orig = R.World(src)
    assert_bits_equal(world.camera(), orig.camera(), "camera moved back")
    m = orig.spheres()[3]
    world.set_material(3, int(m[4]), m[5:8], float(m[9]))
    out, _ = acc.add(4)
    assert acc.samples == 4
    assert_bits_equal(out, first, "moved back: the very first pass again")
    assert_sums_equal(acc.sums(), first_sums, "moved back: sums")


# ---- 9. limits ------------------------------------------------------------------

def test_limits():
    world = R.World(S.rtow())
    acc = world.accumulator(16, 9, 6)
    out, _ = acc.add(4)
    sums = acc.sums()
    with pytest.raises(R.RenderError, match="exceed"):
        acc.add(3)
    for n in (0, -1):
        with pytest.raises(R.RenderError, match="at least 1"):
            acc.add(n)
    assert acc.samples == 4
    assert_sums_equal(acc.sums(), sums, "sums after refused passes")
    full, _ = acc.add(2)
    assert_bits_equal(full, world.render(16, 9, 6, 8)[0], "the refused passes traced nothing")
    with pytest.raises(R.RenderError, match="exceed"):
        acc.add(1)


def test_world_freed_before_its_accumulator():
    world = R.World(S.rtow())
    acc = world.accumulator(16, 9, 4)
    acc.add(1)
    world.close()
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.add(1)
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.sums()
    acc.close()


# ---- 10. device output and streams ----------------------------------------------

def test_device_output_on_a_torch_stream():
    import torch

    src = S.rtow()
    w, h = 40, 24
    host = R.World(src).accumulator(w, h, 8)
    host.add(3)
    ref, _ = host.add(5)
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = R.World(src).accumulator(w, h, 8)
    t = torch.zeros((h, w, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        assert acc.add_device(3, t.data_ptr(), stream.cuda_stream) is None
        assert acc.add_device(5, t.data_ptr(), stream.cuda_stream) is None
    stream.synchronize()
    assert_bits_equal(t.cpu().numpy(), ref, "two enqueued passes on a torch stream")
    assert acc.samples == 8
    assert_sums_equal(acc.sums(), host.sums(), "sums")
    # d_rgba NULL: accumulate only
    only = R.World(src).accumulator(w, h, 8)
    only.add_device(3, 0)
    out, _ = only.add(5)
    assert_bits_equal(out, ref, "accumulate-only pass, then a host pass")


# ---- 11. an unrelated frame between passes --------------------------------------

def test_unrelated_frame_between_passes():
    src = S.rtow()
    w, h = 40, 24
    plain = R.World(src).accumulator(w, h, 8)
    plain.add(4)
    ref, _ = plain.add(4)
    world = R.World(src)
    acc = world.accumulator(w, h, 8)
    acc.add(4)
    other, _ = world.render(64, 36, 16, 8)  # the shared scratch: rings, counters, output tile
    kept, _ = world.render(21, 13, 5, 8, keep_samples=True)
    out, _ = acc.add(4)
    assert_bits_equal(out, ref, "accumulation around unrelated frames")
    assert_sums_equal(acc.sums(), plain.sums(), "sums")
    assert_bits_equal(other, R.World(src).render(64, 36, 16, 8)[0], "the unrelated frame itself")
