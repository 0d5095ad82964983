"""Adaptive accumulation (rt_adapt_*): the accumulator stops
sampling pixels that have converged, and every pixel still carries exactly the
reference's in-order fold of its own samples.

The expectation is a numpy float32 restatement of the contract (`restate`), run
on the oracle's per-sample colours at the accumulator's stride in COUNTER mode
(test_gpu_accum.Expect's table) or on the reference's SERIAL states.  After
every pass the active list, the counts, the three sums, sumsq and the frame
(pixel p = the oracle's REPLAY frame at spp count[p]) are compared on raw bits,
NaN equal to NaN.  Cases that claim to test the list first assert, on the
restatement alone, that 5 % to 60 % of the pixels stay active at each decision
and that some list length is no multiple of 8."""
import numpy as np
import pytest

import oracle as O
import raytracer_amd as R
import scenes as S
from conftest import scene_text
from test_gpu_accum import FAMILIES, Expect, assert_sums_equal
from test_gpu_corner_tree import _random_scene
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
TOL, BIAS = 0.08, 0.05


# ---- the restatement ----------------------------------------------------------

def colours(exp, n):
    """The oracle's per-sample colours of exp's accumulation, samples 0..n-1 of
    every pixel: float32[h * w, n, 3], top row first (memoised on exp)."""
    memo = exp.__dict__.setdefault("_colours", {})
    if n not in memo:
        _, _, _, smp = exp.scene.render(exp.w, exp.h, n, exp.depth, mode=O.RNG_REPLAY, replay=exp.table(n),
                                        record_samples=True, nthreads=4)
        c = smp.reshape(exp.h, exp.w, n, 4)[::-1, :, :, :3]
        memo[n] = np.ascontiguousarray(c, dtype=f32).reshape(exp.h * exp.w, n, 3)
    return memo[n]


def restate(exp, split, tolerance, bias, min_samples):
    """DESIGN.md 5.7 in numpy float32, one rounded operation per step -> the
    state after every pass: dict(N, active, count, sums, sumsq, traced)."""
    c = colours(exp, sum(split))
    npix = exp.w * exp.h
    sums, q = np.zeros((npix, 3), f32), np.zeros(npix, f32)
    count = np.zeros(npix, np.uint32)
    active = np.arange(npix, dtype=np.uint32)
    tol, bias = f32(tolerance), f32(bias)
    N, states = 0, []
    with np.errstate(invalid="ignore", over="ignore"):
        for n in split:
            traced = 0
            if active.size:
                traced = int(active.size) * n
                for s in range(N, N + n):
                    x = c[active, s, :]
                    sums[active] = sums[active] + x
                    y = (x[:, 0] + x[:, 1]) + x[:, 2]
                    q[active] = q[active] + y * y
                N += n
                count[active] = N
                if N >= min_samples:
                    inv = f32(1.0) / f32(N)
                    a = sums[active]
                    m = ((a[:, 0] + a[:, 1]) + a[:, 2]) * inv
                    v = q[active] * inv - m * m
                    v = np.where(v < 0, f32(0.0), v)
                    e = v * inv
                    lim = tol * (m + bias)
                    active = active[~(e <= lim * lim)]
            states.append(dict(N=N, active=active.copy(), count=count.copy(), sums=sums.copy(), sumsq=q.copy(),
                               traced=traced))
    assert sums.dtype == q.dtype == f32
    return states


def assert_tests_the_list(states, npix, min_samples, what):
    """The condition on a case that claims to test the list (module docstring)."""
    decided = [len(s["active"]) for s in states if s["N"] >= min_samples]
    assert decided, what
    shares = [n / npix for n in decided]
    assert all(0.05 <= x <= 0.60 for x in shares), f"{what}: active shares {shares}"
    assert any(n % 8 for n in decided), f"{what}: list lengths {decided}"


def expected_frame(exp, count):
    out = np.zeros((exp.h, exp.w, 4), np.uint8)
    cnt = count.reshape(exp.h, exp.w)
    for n in np.unique(cnt):
        assert n > 0
        out[cnt == n] = exp.frame(int(n))[cnt == n]
    return out


def check(acc, exp, st, out, what):
    """The accumulator's whole state, and the frame `out` it delivered, against state st."""
    assert acc.samples == st["N"], what
    assert acc.active == len(st["active"]), f"{what}: active {acc.active} != {len(st['active'])}"
    got = acc.active_list()
    assert got.dtype == np.uint32 and np.array_equal(got, st["active"]), f"{what}: active list"
    assert np.array_equal(acc.counts().reshape(-1), st["count"]), f"{what}: counts"
    assert_sums_equal(acc.sums().reshape(-1, 3), st["sums"], f"{what}: sums")
    assert_sums_equal(acc.sumsq().reshape(-1), st["sumsq"], f"{what}: sumsq")
    if out is not None:
        assert_bits_equal(out, expected_frame(exp, st["count"]), f"{what}: frame")


def run(acc, exp, split, states, what, stats=None):
    out = st = None
    for k, (n, want) in enumerate(zip(split, states)):
        out, st = acc.add(n)
        assert st["samples"] == want["traced"], f"{what}: pass {k} traced {st['samples']} != {want['traced']}"
        if stats is not None:
            stats.append(st)
        check(acc, exp, want, out, f"{what} pass {k} of {split}")
    return out, st


# ---- 1. pass splits on RTOW -------------------------------------------------------

_MEMO = {}


def _rtow():
    if "rtow" not in _MEMO:
        _MEMO["rtow"] = Expect(O.Scene(S.rtow()), 40, 24, 24, 8)
    return _MEMO["rtow"]


def _rtow_acc(tolerance=TOL, bias=BIAS, min_samples=8):
    acc = R.World(S.rtow()).accumulator(40, 24, 24, depth=8)
    acc.set_adaptive(tolerance, bias, min_samples)
    return acc


@pytest.mark.parametrize("split,min_samples", [((4,) * 6, 8), ((3,) * 8, 6), ((8, 4, 3, 1, 4, 4), 8)])
def test_pass_splits(split, min_samples):
    """(passes of 3 and 1 fold on pixel lanes, the others on plane lanes)"""
    exp = _rtow()
    states = restate(exp, split, TOL, BIAS, min_samples)
    assert_tests_the_list(states, 40 * 24, min_samples, f"rtow {split}")
    acc = _rtow_acc(min_samples=min_samples)
    assert acc.active == 40 * 24 and acc.samples == 0
    assert not acc.counts().any() and not acc.sumsq().any()
    assert np.array_equal(acc.active_list(), np.arange(40 * 24, dtype=np.uint32))
    run(acc, exp, split, states, "rtow")
    assert acc.samples == 24
    with pytest.raises(R.RenderError, match="exceed"):
        acc.add(1)


# ---- 2. every kernel family ---------------------------------------------------------

# The tolerance each family's frame is tested at: 0.08 unless the restatement
# leaves too few pixels active with it (the soup's triangles are flat diffuse
# faces: 8 -> 1 % at 0.08).
FAMILY_TOL = {"soup": 0.03}
FAMILY_SPLIT, FAMILY_MIN = (4, 4, 4, 4), 8


def _family_expect(family):
    make, env, accel, (w, h), tree, edits = FAMILIES[family]
    key = ("family", "rtow" if family in ("corner", "box", "global", "brute") else family)
    if key not in _MEMO:
        src = make()
        ref = O.Scene(src)
        if edits:
            for (i, kind, rgb) in edits(R.World(src).num_spheres):
                ref.set_material(i, kind, rgb)
        _MEMO[key] = Expect(ref, w, h, sum(FAMILY_SPLIT), 8)
    return _MEMO[key]


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_kernel_family(monkeypatch, family):
    make, env, accel, (w, h), tree, edits = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    exp = _family_expect(family)
    tol = FAMILY_TOL.get(family, TOL)
    states = restate(exp, FAMILY_SPLIT, tol, BIAS, FAMILY_MIN)
    assert_tests_the_list(states, w * h, FAMILY_MIN, family)
    world = R.World(make())
    if edits:
        for (i, kind, rgb) in edits(world.num_spheres):
            world.set_material(i, kind, rgb)
    _, pst = world.accumulator(w, h, sum(FAMILY_SPLIT), depth=8, accel=accel).add(4)
    acc = world.accumulator(w, h, sum(FAMILY_SPLIT), depth=8, accel=accel)
    acc.set_adaptive(tol, BIAS, FAMILY_MIN)
    stats = []
    run(acc, exp, FAMILY_SPLIT, states, family, stats)
    for st in stats[:3]:  # (full and partial lists: the plain pass's path)
        for k in ("sphere_tree", "accel", "launch_block_threads", "tri_bvh", "fused_resolve"):
            assert st[k] == pst[k], (family, k)
    if tree is not None:
        assert stats[0]["sphere_tree"] == tree
    if family == "soup":
        assert stats[0]["tri_bvh"] == 1


# ---- 3. the last chunk of a list ---------------------------------------------------

# The tolerances whose lists (RTOW 40 x 24, passes of 4) have, by the
# restatement, lengths of every residue 1 to 7 mod 8 between them: 0.08 gives
# 331, 297, 260, 222 (3, 1, 4, 6), 0.07 gives 338, 321, 285, 255 (2, 1, 5, 7).
LAST_CHUNK = (0.08, 0.07)


def _traced_residues(states):
    return {len(s["active"]) % 8 for s in states[:-1] if len(s["active"])}


def test_last_chunk_cases_cover_1_to_7():
    exp = _rtow()
    got = set()
    for tol in LAST_CHUNK:
        got |= _traced_residues(restate(exp, (4,) * 6, tol, BIAS, 8))
    assert got >= set(range(1, 8)), sorted(got)


@pytest.mark.parametrize("tolerance", list(LAST_CHUNK))
def test_last_chunk_of_1_to_7_pixels(monkeypatch, tolerance):
    """One partition of 8-pixel chunks over the list: its last chunk holds length mod 8 pixels."""
    exp = _rtow()
    split = (4,) * 6
    states = restate(exp, split, tolerance, BIAS, 8)
    assert_tests_the_list(states, 40 * 24, 8, f"tolerance {tolerance}")
    acc = _rtow_acc(tolerance=tolerance)
    monkeypatch.setenv("RT_AMD_PARTS", "1")
    monkeypatch.setenv("RT_AMD_CHUNK", str(8 * 4))
    stats = []
    run(acc, exp, split, states, f"tolerance {tolerance}", stats)
    assert all(st["launch_chunk"] == 32 and st["launch_parts"] == 1 for st in stats)


@pytest.mark.parametrize("n", [3, 1])
def test_last_chunk_pixel_lanes(monkeypatch, n):
    """The same through the pixel-lane resolve (passes of 3 and of 1)."""
    exp = _rtow()
    split = (8,) + (n,) * (5 if n == 3 else 8)
    states = restate(exp, split, TOL, BIAS, 8)
    assert_tests_the_list(states, 40 * 24, 8, f"passes of {n}")
    assert _traced_residues(states) - {0}
    acc = _rtow_acc()
    monkeypatch.setenv("RT_AMD_PARTS", "1")
    out = None
    for k, (m, want) in enumerate(zip(split, states)):
        monkeypatch.setenv("RT_AMD_CHUNK", str(8 * m))
        out, st = acc.add(m)
        assert st["launch_chunk"] == 8 * m and st["launch_parts"] == 1
        check(acc, exp, want, out, f"passes of {n}: pass {k}")


# ---- 4. min_samples >= S: a plain accumulator with a fourth fold --------------------

def test_min_samples_above_the_stride_is_a_plain_accumulation():
    exp = _rtow()
    split = (8, 4, 3, 1, 4, 4)
    states = restate(exp, split, TOL, BIAS, 25)
    plain = R.World(S.rtow()).accumulator(40, 24, 24, depth=8)
    acc = _rtow_acc(min_samples=25)
    for n, want in zip(split, states):
        ref, _ = plain.add(n)
        out, st = acc.add(n)
        assert st["samples"] == 40 * 24 * n
        assert_bits_equal(out, ref, f"frame after {acc.samples} vs the plain accumulator")
        assert_sums_equal(acc.sums(), plain.sums(), f"sums after {acc.samples}")
        assert len(want["active"]) == 40 * 24
        check(acc, exp, want, out, f"after {acc.samples}")
    assert acc.active == 40 * 24 and (acc.counts() == 24).all()


# ---- 5. the empty list ------------------------------------------------------------

def test_empty_list():
    exp = _rtow()
    states = restate(exp, (8, 4), 1e30, BIAS, 8)
    assert len(states[0]["active"]) == 0 and states[1]["N"] == 8 and states[1]["traced"] == 0
    acc = _rtow_acc(tolerance=1e30)
    out, st = acc.add(8)
    assert st["samples"] == 40 * 24 * 8 and st["trace_launches"] == 1
    check(acc, exp, states[0], out, "first decision")
    assert acc.active == 0 and acc.active_list().size == 0
    again, st = acc.add(4)
    assert st["samples"] == 0 and st["trace_launches"] == 0
    assert_bits_equal(again, out, "the pass that traced nothing delivers the same frame")
    check(acc, exp, states[1], again, "after the empty pass")
    assert acc.samples == 8
    with pytest.raises(R.RenderError, match="exceed"):
        acc.add(17)


# ---- 6. degenerate frames -----------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 5), (5, 1), (1, 1)])
def test_degenerate_frames_nan_pixels_never_converge(w, h):
    src = _random_scene(seed=7, n=300, spread=2.0, radius=0.4, big=False)
    exp = Expect(O.Scene(src), w, h, 8, 8)
    split = (4, 1, 3)
    states = restate(exp, split, TOL, BIAS, 2)
    for st in states:
        nan = np.flatnonzero(np.isnan(st["sums"]).any(axis=1) | np.isnan(st["sumsq"]))
        assert np.isin(nan, st["active"]).all(), "a NaN pixel left the list"
    acc = R.World(src).accumulator(w, h, 8)
    acc.set_adaptive(TOL, BIAS, 2)
    run(acc, exp, split, states, f"{w}x{h}")
    assert acc.samples == 8


# ---- 7. REPLAY ------------------------------------------------------------------------

def test_replay_of_the_reference_stream():
    src = scene_text("world.txt")
    w, h, stride, depth = 33, 17, 6, 8
    ref = O.Scene(src)
    _, _, table = ref.render(w, h, stride, depth, mode=O.RNG_SERIAL, record_states=True)
    exp = Expect(ref, w, h, stride, depth, states=table)
    split = (2, 2, 2)
    states = restate(exp, split, TOL, BIAS, 2)
    assert_tests_the_list(states, w * h, 2, "replay")
    acc = R.World(src).accumulator(w, h, stride, depth=depth, mode=R.RNG_REPLAY, replay=table)
    acc.set_adaptive(TOL, BIAS, 2)
    run(acc, exp, split, states, "replay")


# ---- 8. several launches per pass ------------------------------------------------------

def test_several_launches_per_pass(monkeypatch):
    exp = _rtow()
    split = (4,) * 6
    states = restate(exp, split, TOL, BIAS, 8)
    acc = _rtow_acc()
    prev = 40 * 24
    for k, (n, want) in enumerate(zip(split, states)):
        monkeypatch.setenv("RT_AMD_SLAB_JOBS", str(n * 100))  # 100 list entries per launch
        out, st = acc.add(n)
        assert st["trace_launches"] == -(-prev // 100) and st["samples"] == prev * n
        check(acc, exp, want, out, f"slabbed pass {k}")
        prev = len(want["active"])
    assert prev % 100  # (the last launch of some pass was a partial range)


# ---- 9. 64-bit job indices ---------------------------------------------------------------

def test_64_bit_job_indices():
    src = scene_text("world.txt")
    w, h, stride = 8, 4, 1 << 28  # W H S = 2^33
    exp = Expect(O.Scene(src), w, h, stride, 8)
    split = (2, 2)
    states = restate(exp, split, TOL, BIAS, 2)
    acc = R.World(src).accumulator(w, h, stride)
    acc.set_adaptive(TOL, BIAS, 2)
    run(acc, exp, split, states, "stride 2^28")


# ---- 10. resets ---------------------------------------------------------------------------

def test_resets():
    src = S.rtow()
    w, h = 40, 24
    exp = _rtow()
    states = restate(exp, (8, 4), TOL, BIAS, 8)
    world = R.World(src)
    acc = world.accumulator(w, h, 24)
    acc.set_adaptive(TOL, BIAS, 8)
    run(acc, exp, (8, 4), states, "before the move")
    assert 0 < acc.active < w * h
    for what in ("enable", "disable"):
        with pytest.raises(R.RenderError, match="holds 12 samples"):
            acc.set_adaptive(TOL, BIAS, 8, enable=what == "enable")
    # a camera move: the full list, zero counts
    world.move_camera(0.5, -0.25, -1.0)
    assert acc.samples == 0 and acc.active == w * h
    assert not acc.counts().any() and not acc.sumsq().any() and not acc.sums().any()
    assert np.array_equal(acc.active_list(), np.arange(w * h, dtype=np.uint32))
    fresh = R.World(src)
    fresh.move_camera(0.5, -0.25, -1.0)
    facc = fresh.accumulator(w, h, 24)
    facc.set_adaptive(TOL, BIAS, 8)

    def same(out, fout, what):
        assert_bits_equal(out, fout, f"{what}: frame")
        assert acc.samples == facc.samples and acc.active == facc.active, what
        assert np.array_equal(acc.active_list(), facc.active_list()), what
        assert np.array_equal(acc.counts(), facc.counts()), what
        assert_sums_equal(acc.sums(), facc.sums(), f"{what}: sums")
        assert_sums_equal(acc.sumsq(), facc.sumsq(), f"{what}: sumsq")

    same(acc.add(8)[0], facc.add(8)[0], "after a camera move")
    assert 0 < acc.active < w * h
    same(acc.add(4)[0], facc.add(4)[0], "after a camera move, second pass")
    # a material edit
    world.set_material(3, 1, (0.9, 0.2, 0.2), 0.1)
    fresh.set_material(3, 1, (0.9, 0.2, 0.2), 0.1)
    assert acc.samples == 0 and acc.active == w * h and not acc.counts().any()
    same(acc.add(8)[0], facc.add(8)[0], "after set_material")
    assert (acc.counts() == 8).all()
    # an explicit reset keeps the adaptive setting
    acc.reset()
    facc.reset()
    assert acc.samples == 0 and acc.active == w * h
    same(acc.add(8)[0], facc.add(8)[0], "after reset()")
    same(acc.add(4)[0], facc.add(4)[0], "after reset(), second pass")
    assert 0 < acc.active < w * h
    # ... and disable gives the plain accumulator back
    acc.reset()
    acc.set_adaptive(enable=False)
    plain = fresh.accumulator(w, h, 24)
    assert_bits_equal(acc.add(12)[0], plain.add(12)[0], "disabled: a plain pass")
    assert acc.active == w * h
    with pytest.raises(R.RenderError, match="not adaptive"):
        acc.counts()


# ---- 11. interleaving ------------------------------------------------------------------------

def test_frames_and_plain_passes_between_adaptive_passes():
    exp = _rtow()
    split = (8, 4, 4)
    states = restate(exp, split, TOL, BIAS, 8)
    world = R.World(S.rtow())
    acc = world.accumulator(40, 24, 24)
    acc.set_adaptive(TOL, BIAS, 8)
    plain = world.accumulator(40, 24, 24)
    twin = R.World(S.rtow()).accumulator(40, 24, 24)
    for k, (n, want) in enumerate(zip(split, states)):
        out, _ = acc.add(n)
        check(acc, exp, want, out, f"pass {k}")
        other, _ = world.render(64, 36, 16, 8)  # the shared scratch: rings, counters, output tile
        world.render(21, 13, 5, 8, keep_samples=True)
        pout, _ = plain.add(n)
        assert_bits_equal(pout, twin.add(n)[0], f"the plain accumulator's pass {k}")
        check(acc, exp, want, None, f"pass {k}, after the unrelated work")
    assert_bits_equal(other, R.World(S.rtow()).render(64, 36, 16, 8)[0], "the unrelated frame itself")
    assert_sums_equal(plain.sums(), twin.sums(), "the plain accumulator's sums")


# ---- 12. device output ---------------------------------------------------------------------------

def test_device_output_on_a_torch_stream():
    import torch

    exp = _rtow()
    split = (8, 4, 4)
    states = restate(exp, split, TOL, BIAS, 8)
    dev = torch.device("cuda", torch.cuda.current_device())
    acc = _rtow_acc()
    t = torch.zeros((24, 40, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    for k, (n, want) in enumerate(zip(split, states)):
        with torch.cuda.stream(stream):
            assert acc.add_device(n, t.data_ptr(), stream.cuda_stream) is None
        stream.synchronize()
        check(acc, exp, want, t.cpu().numpy(), f"device pass {k}")
    # d_rgba NULL: accumulate only, then a host pass delivers every pixel
    only = _rtow_acc()
    only.add_device(8, 0)
    out, _ = only.add(4)
    check(only, exp, states[1], out, "accumulate-only pass, then a host pass")
