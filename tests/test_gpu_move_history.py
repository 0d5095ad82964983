"""The history resolve that follows a moved sphere, on the GPU (RT_CLAMP_KEEP_ON_EDIT
across rt_world_set_sphere_geometry), bit for bit against the numpy
restatement of its contract (move_ref.py).

Outputs are compared as raw f32 bits and raw bytes; any NaN equals any NaN.
Nothing expected comes from the library's resolve: the accumulator cases take its
inputs (sums, counts, first-hit records, the camera's floats, the spheres' floats,
each pinned by its own suite) and restate the resolve over them.
"""
import numpy as np
import pytest

import filter_ref as FR
import move_cases as MC
import move_ref as MR
import raytracer_amd as R
import scene_values as V
from conftest import scene_text
from test_gpu_clamp import Session
from test_gpu_history import orbit, same_bits, scene_source

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)

# ---- 1. accumulator sessions ----------------------------------------------------------------

class MoveSession(Session):
    """test_gpu_clamp.Session with the restatement that remembers sphere tables."""

    def __init__(self, src, w, h, adaptive=False, clamp=None):
        super().__init__(src, w, h, adaptive, clamp=None)
        self.ref = MR.MoveHistory()
        if clamp is not None:
            self.clamp(**clamp)

    def move(self, i, c, r):
        self.world.set_sphere(i, c, r)
        self.edit += 1

    def recolour(self, i, rgb):
        self.world.set_material(i, 0, rgb)
        self.edit += 1

    def resolve(self, what, ref=None):
        acc = self.acc
        n = self.samples()
        rec = self.world.first_hit(self.w, self.h)
        want = self.ref.resolve(acc.sums(), n, rec, self.world.camera(), self.edit, self.world.spheres()[:, :4])
        rgb, px = acc.resolved()
        length = acc.history_length()
        same_bits(rgb, want[0], f"{what}: out_rgb")
        assert px.tobytes() == want[1].tobytes(), f"{what}: RGBA8"
        same_bits(length, want[2], f"{what}: history_length")
        return rgb, px, length, n, rec


def ball_of(which, src):
    """(sphere index, centre, radius) of the sphere the session drags."""
    i = 1 if which == "three_spheres.txt" else V._visible(src, 1)[0]
    c, r = MC.geometry(src, i)
    return i, c, r


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
@pytest.mark.parametrize("which,w,h,target,radius", [("three_spheres.txt", 48, 32, (0.0, 0.0, -1.0), 1.0),
                                                     ("soup", 40, 24, (0.0, 0.0, -3.0), 3.0)])
def test_sessions_follow_the_ball(which, w, h, target, radius, adaptive):
    import torch

    src = scene_source(which)
    i, c, r = ball_of(which, src)
    s = MoveSession(src, w, h, adaptive, clamp=dict(gamma=1.0, radius=2, keep_on_edit=True))
    what = f"{which} {'adaptive' if adaptive else 'plain'}"
    shares = []

    def took(length, n, rec, label):
        ball = rec["prim"] == i + 1
        share = float((length[ball] > n.astype(F)[ball]).mean()) if ball.any() else float("nan")
        shares.append((label, int(ball.sum()), share))
        return ball, share

    orbit(s.world, 0, w, h, target, radius)
    s.add(2)
    s.resolve(f"{what}: first resolve")
    d = np.array([0.05, 0.02, 0.0], F)
    s.move(i, c + d, r)
    s.add(1)
    rgb, px, length, n, rec = s.resolve(f"{what}: the ball moved")
    ball, share = took(length, n, rec, "moved")
    assert ball.any() and share > 0
    if which == "three_spheres.txt":
        assert ball.sum() > 50 and share > 0.5
    # the device entry on a caller's stream: the host entry's bytes (the same prev, cur recomputed)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out = torch.zeros(h, w, 3, dtype=torch.float32, device="cuda")
        d_px = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
    st.synchronize()
    s.acc.resolved_device(d_out.data_ptr(), d_px.data_ptr(), st.cuda_stream)
    s.acc.resolved_device(d_out.data_ptr(), d_px.data_ptr(), st.cuda_stream)  # (twice: the staging is reused)
    st.synchronize()
    same_bits(d_out.cpu().numpy(), rgb, "device entry")
    assert d_px.cpu().numpy().tobytes() == px.tobytes()
    # again under the same camera, with another radius
    s.move(i, c + d + d, F(r * F(1.125)))
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: moved again, same camera")
    ball, share = took(length, n, rec, "moved again")
    assert ball.any() and share > 0
    if which == "three_spheres.txt":
        assert share > 0.5
    # the ball and the camera
    s.move(i, c + d + d + d, r)
    orbit(s.world, 2, w, h, target, radius)
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: the ball and the camera moved")
    ball, share = took(length, n, rec, "ball and camera")
    assert ball.any() and share > 0
    if which == "three_spheres.txt":
        assert share > 0.5
    # away and back to the value cur remembers, with no resolve in between: nothing moved
    s.move(i, c, r)
    s.move(i, c + d + d + d, r)
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: moved back to a remembered value")
    assert s.ref.prev["spheres"].tobytes() == s.world.spheres()[:, :4].tobytes()
    ball, share = took(length, n, rec, "back")
    assert ball.any() and share > 0
    # a material edit of the moved ball: the guides stay true
    s.recolour(i, (0.1, 0.2, 0.9))
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: the moved ball recoloured")
    ball, share = took(length, n, rec, "recoloured")
    assert ball.any() and share > 0
    # a filtered resolve after one more move filters the followed out with the same records
    s.move(i, c + d, r)
    s.add(1)
    rgb, _, length, n, rec = s.resolve(f"{what}: moved after the recolouring")
    ball, share = took(length, n, rec, "moved after recolouring")
    assert ball.any() and share > 0
    want = FR.filter_image(rgb, rec)
    got = s.acc.resolved(filter=dict())
    same_bits(got[0], want[0], f"{what}: filtered")
    assert got[1].tobytes() == want[1].tobytes()
    # values at the contract's edges, each seen from the side where the ball is visible now
    # and prev remembers the odd value: an infinite centre (P' is not finite: no history on
    # the ball), radius 0 (k = 0: every pixel maps to c0) and a negative radius (k < 0)
    for label, odd in (("inf centre", (np.array([INF, c[1], c[2]], F), r)), ("zero radius", (c + d, F(0.0))),
                       ("negative radius", (c + d, -r))):
        s.move(i, *odd)
        s.add(1)
        s.resolve(f"{what}: {label}")
        s.move(i, c + d + d, r)
        s.add(1)
        _, _, length, n, rec = s.resolve(f"{what}: back from {label}")
        ball, share = took(length, n, rec, f"back from {label}")
        assert s.ref.prev["spheres"].tobytes() != s.world.spheres()[:, :4].tobytes()  # (the motion path)
        # prev never saw the ball (an infinite centre, radius 0: no pixel of prev carries its
        # prim id), so by the prim-id test none of its pixels can take history
        if label in ("inf centre", "zero radius"):
            assert ball.any() and share == 0.0
    # the flag cleared: an edit drops both snapshots, as without a clamp
    s.clamp(gamma=1.0, radius=2)
    s.move(i, c, r)
    s.add(1)
    _, px, length, n, _ = s.resolve(f"{what}: flag cleared, the ball moved")
    assert (length == n.astype(F)).all() and px.tobytes() == s.frame.tobytes()
    # the clamp disabled: likewise
    s.clamp(gamma=1.0, radius=2, keep_on_edit=True)
    s.add(1)
    s.resolve(f"{what}: flag set again")
    s.unclamp()
    s.move(i, c + d, r)
    s.add(1)
    _, _, length, n, _ = s.resolve(f"{what}: clamp disabled, the ball moved")
    assert (length == n.astype(F)).all()
    print(f"shares of the ball's pixels taking history, {what}: " +
          ", ".join(f"{label} {share:.3f} of {count}" for label, count, share in shares))
    s.close()


SIZES = [(1, 1), (1, 7), (7, 1), (9, 9), (70, 50)]  # test_gpu_history.SIZES: partial tiles, one pixel


@pytest.mark.parametrize("gamma,radius", [(0.0, 1), (1.5, 3)])
@pytest.mark.parametrize("w,h", SIZES)
def test_sessions_at_sizes_off_the_tile(w, h, gamma, radius):
    """The motion kernel where lanes fall outside the image and the box is cut by its
    edges: a move under one camera, one with the camera, and one seen from behind."""
    src = scene_text("three_spheres.txt")
    i, c, r = ball_of("three_spheres.txt", src)
    s = MoveSession(src, w, h, clamp=dict(gamma=gamma, radius=radius, keep_on_edit=True))
    what = f"{w}x{h} g{gamma} r{radius}"
    orbit(s.world, 0, w, h)
    s.add(2)
    s.resolve(f"{what}: first")
    d = np.array([0.05, 0.02, 0.0], F)
    s.move(i, c + d, r)
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: moved")
    assert s.ref.prev["spheres"].tobytes() != s.world.spheres()[:, :4].tobytes()  # (the motion path)
    ball = rec["prim"] == i + 1
    if (w, h) == (70, 50):
        assert ball.sum() > 100 and (length[ball] > n.astype(F)[ball]).mean() > 0.5
    s.move(i, c + d + d, F(r * F(0.875)))
    orbit(s.world, 3, w, h)
    s.add(1)
    s.resolve(f"{what}: the ball and the camera")
    # the far side: every point prev saw is behind or off the new view's taps
    s.move(i, c + d, r)
    orbit(s.world, 180, w, h)
    s.add(1)
    s.resolve(f"{what}: from behind")
    s.close()


def test_session_with_nan_samples():
    """scene_values' `ir` case (refraction indices that give NaN and infinite samples): the
    sums, the box and the blend carry NaN through the motion kernel as the contract says."""
    case = V.case("ir")
    w, h = 45, 27
    s = MoveSession(case.src, w, h, clamp=dict(gamma=1.5, radius=1, keep_on_edit=True))
    i = s.world.num_spheres - 4  # one of the spliced glass balls, in front of the field
    g = s.world.spheres()[i]
    s.add(4)
    rgb, _, _, _, _ = s.resolve("ir: first")
    assert np.isnan(rgb).any()
    for step in (1, 2):
        s.move(i, g[:3] + np.array([0.04 * step, 0.0, 0.0], F), g[3])
        s.add(2)
        rgb, _, length, n, rec = s.resolve(f"ir: move {step}")
        assert s.ref.prev["spheres"].tobytes() != s.world.spheres()[:, :4].tobytes()
    assert np.isnan(rgb).any() and (length > n.astype(F)).any()
    s.close()


# ---- 1b. the host's sparse maps: several spheres, several accumulators, the flag set late ---------

def differing(s):
    """The sphere indices whose entries differ between the table that the next resolve's
    prev remembers and the world's table now, by the restatement's bookkeeping alone."""
    ref = s.ref
    cam = np.array(s.world.camera(), F).reshape(12)
    p = ref.cur if ref.cur is not None and (ref.cur["cam"].tobytes() != cam.tobytes() or
                                            ref.cur["edit"] != s.edit) else ref.prev
    now = np.ascontiguousarray(s.world.spheres()[:, :4])
    return set(np.flatnonzero((p["spheres"].view(np.uint32) != now.view(np.uint32)).any(axis=1)).tolist())


def took_on(length, n, rec, i):
    on = rec["prim"] == i + 1
    return bool((length[on] > n.astype(F)[on]).any())


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
def test_session_with_several_moved_spheres(adaptive):
    """Three spheres of the 60-sphere field: two moved for one resolve; a third moved and
    the first one moved away and back to what prev remembers; one moved twice with no
    resolve in between.  Each step's map of moved spheres is another subset."""
    src = V.field()
    w, h = 48, 32
    s = MoveSession(src, w, h, adaptive, clamp=dict(gamma=1.0, radius=2, keep_on_edit=True))
    what = f"field {'adaptive' if adaptive else 'plain'}"
    prims, counts = np.unique(s.world.first_hit(w, h)["prim"], return_counts=True)
    counts = np.where((prims >= 1) & (prims <= s.world.num_spheres), counts, 0)
    a, b, c = (int(p) - 1 for p in prims[np.argsort(-counts)][:3])
    assert np.sort(counts)[-3] >= 8, "three spheres that first_hit shows"
    (ca, ra), (cb, rb), (cc, rc) = (MC.geometry(src, i) for i in (a, b, c))
    d = np.array([0.03, 0.02, 0.0], F)
    s.add(2)
    s.resolve(f"{what}: first")
    s.move(a, ca + d, ra)
    s.move(b, cb - d, F(rb * F(1.125)))
    s.add(1)
    assert differing(s) == {a, b}
    _, _, length, n, rec = s.resolve(f"{what}: A and B moved")
    assert took_on(length, n, rec, a) and took_on(length, n, rec, b) and took_on(length, n, rec, c)
    s.move(c, cc + d, rc)
    s.move(a, ca, ra)
    s.move(a, ca + d, ra)  # (back to the value the last resolve's snapshot remembers)
    s.add(1)
    assert differing(s) == {c}
    _, _, length, n, rec = s.resolve(f"{what}: C moved, A away and back")
    assert took_on(length, n, rec, a) and took_on(length, n, rec, c)
    s.move(b, cb, rb)
    s.move(b, cb + d, F(rb * F(0.875)))
    s.add(1)
    assert differing(s) == {b}
    _, _, length, n, rec = s.resolve(f"{what}: B moved twice")
    assert took_on(length, n, rec, b)
    # all three and the camera, then nothing but the camera
    for i, (ci, ri) in ((a, (ca, ra)), (b, (cb, rb)), (c, (cc, rc))):
        s.move(i, ci - d, ri)
    s.world.translate_camera(0.02, 0.0, 0.0)
    s.add(1)
    assert differing(s) == {a, b, c}
    s.resolve(f"{what}: three spheres and the camera")
    s.world.translate_camera(0.02, 0.0, 0.0)
    s.add(1)
    assert differing(s) == set()
    s.resolve(f"{what}: the camera alone")
    s.close()


class SharedSession(MoveSession):
    """A MoveSession on a world it shares: the edit count is the world's, kept by the test."""

    def __init__(self, world, edits, w, h, clamp):
        self.world, self._edits = world, edits
        self.acc = world.accumulator(w, h, 64)
        self.adaptive, self.w, self.h, self.frame = False, w, h, None
        self.acc.history_enable()
        self.ref = MR.MoveHistory()
        self.clamp(**clamp)

    @property
    def edit(self):
        return self._edits[0]

    @edit.setter
    def edit(self, v):
        self._edits[0] = v


@pytest.mark.parametrize("w,h", [(40, 24), (9, 9)])
def test_two_accumulators_of_one_world(w, h):
    """Snapshots made at different times remember different sets of moved spheres."""
    src = scene_text("three_spheres.txt")
    world = R.World(src)
    edits = [0]
    clamp = dict(gamma=1.0, radius=1, keep_on_edit=True)
    x, y = SharedSession(world, edits, w, h, clamp), SharedSession(world, edits, w, h, clamp)
    s1, s2 = 1, 2
    (c1, r1), (c2, r2) = MC.geometry(src, s1), MC.geometry(src, s2)
    d = np.array([0.05, 0.02, 0.0], F)
    orbit(world, 0, w, h)
    x.add(2)
    x.resolve(f"{w}x{h} X: first")
    x.move(s1, c1 + d, r1)
    y.add(2)
    y.resolve(f"{w}x{h} Y: first, after s1 moved")
    y.move(s2, c2 - d, F(r2 * F(0.875)))
    x.add(1)
    y.add(1)
    assert differing(x) == {s1, s2} and differing(y) == {s2}
    _, _, length, n, rec = x.resolve(f"{w}x{h} X: remembers s1 and s2")
    if (w, h) == (40, 24):
        assert took_on(length, n, rec, s1) and took_on(length, n, rec, s2)
    _, _, length, n, rec = y.resolve(f"{w}x{h} Y: remembers s2 alone")
    if (w, h) == (40, 24):
        assert took_on(length, n, rec, s1) and took_on(length, n, rec, s2)
    x.acc.close()
    y.move(s1, c1 + d + d, r1)
    y.add(1)
    assert differing(y) == {s1}
    y.resolve(f"{w}x{h} Y: X freed, s1 moved again")
    y.acc.close()
    world.close()


def test_flag_set_after_the_move():
    """The map is kept whatever the flag says when the sphere moves: the flag counts at the resolve."""
    w, h = 48, 32
    src = scene_text("three_spheres.txt")
    i, c, r = ball_of("three_spheres.txt", src)
    d = np.array([0.05, 0.02, 0.0], F)
    s = MoveSession(src, w, h, clamp=dict(gamma=1.0, radius=2))
    orbit(s.world, 0, w, h)
    s.add(2)
    s.resolve("late flag: first, no flag")
    s.move(i, c + d, r)
    s.clamp(gamma=1.0, radius=2, keep_on_edit=True)
    s.add(1)
    assert differing(s) == {i}
    _, _, length, n, rec = s.resolve("late flag: the flag set after the move")
    assert took_on(length, n, rec, i)
    # the mirror: a reset between the move and the resolve leaves no snapshot to follow from
    s.move(i, c + d + d, r)
    s.acc.history_reset()
    s.ref.reset()
    s.add(1)
    _, px, length, n, _ = s.resolve("late flag: reset after a move")
    assert (length == n.astype(F)).all() and px.tobytes() == s.frame.tobytes()
    s.move(i, c + d, r)
    s.add(1)
    assert differing(s) == {i}
    _, _, length, n, rec = s.resolve("late flag: the next move is followed again")
    assert took_on(length, n, rec, i)
    s.close()


# ---- 2. a world without a geometry edit runs what it ran ------------------------------------

def test_no_geometry_edit_is_the_clamp_restatement():
    w, h = 48, 32
    s = Session(scene_text("three_spheres.txt"), w, h, clamp=dict(keep_on_edit=True))  # (ClampHistory's bookkeeping)
    orbit(s.world, 0, w, h)
    s.add(2)
    s.resolve("no move: first")
    orbit(s.world, 2, w, h)
    s.add(1)
    s.resolve("no move: camera")
    s.world.set_material(1, 0, (0.2, 0.9, 0.1))
    s.edit += 1
    s.add(1)
    _, _, length, n, rec = s.resolve("no move: a material edit")
    assert (length[rec["prim"] == 2] > 1).any()
    s.close()


# ---- 3. quality -----------------------------------------------------------------------------

DRAG_BOUND = 0.570  # the midpoint between the measured (b) / (a) = 0.1409 and 1


def mse(a, b, mask):
    return float(np.mean(((a.astype(np.float64) - b) ** 2)[mask]))


def test_quality_of_a_drag():
    """Measured on the GPU (profiles/move/quality.txt).
    three_spheres at 96 x 64, 1 COUNTER sample per step, the ball dragged six steps of
    0.05 in x with a resolve each, against 1024 samples of the final scene.  Over the
    ball's pixels: (a) the 1-sample frame, what a geometry edit shows without the flag;
    (b) the resolve that followed the ball, at the default clamp.  Printed as well: the
    ball's old footprint (pixels it uncovered) and the ground under it."""
    w, h = 96, 64
    world = R.World(scene_text("three_spheres.txt"))
    acc = world.accumulator(w, h, 4)
    acc.history_enable()
    acc.clamp_enable(keep_on_edit=True)
    c, r = MC.geometry(scene_text("three_spheres.txt"), 1)
    acc.add(1, stats=False)
    acc.resolved()
    first = world.first_hit(w, h)
    for step in range(1, 7):
        world.set_sphere(1, c + np.array([0.05 * step, 0.0, 0.0], F), r)
        acc.add(1, stats=False)
        resolved, _ = acc.resolved()
    length = acc.history_length()
    noisy = FR.means(acc.sums(), 1)
    rec = world.first_hit(w, h)
    ref_acc = world.accumulator(w, h, 1024, seed=99)
    ref_acc.add(1024, stats=False)
    ref = FR.means(ref_acc.sums(), 1024).astype(np.float64)
    ball = rec["prim"] == 2
    old = (first["prim"] == 2) & ~ball
    ground = (rec["prim"] == 1) & (np.abs(rec["position"][..., 0] - (c[0] + 0.3)) < 0.75) & \
             (np.abs(rec["position"][..., 2] - c[2]) < 0.75)
    a, b = mse(noisy, ref, ball), mse(resolved, ref, ball)
    print(f"move quality, drag: {int(ball.sum())} pixels of the ball; (a) 1-sample MSE {a:.4g}, (b) followed resolve "
          f"MSE {b:.4g}, (b)/(a) {b / a:.4f}; mean history length on the ball {float(length[ball].mean()):.2f}")
    for name, mask in (("old footprint", old), ("ground under the ball", ground)):
        if mask.any():
            print(f"move quality, drag, {name} ({int(mask.sum())} pixels): 1-sample {mse(noisy, ref, mask):.4g}, "
                  f"resolve {mse(resolved, ref, mask):.4g}, mean length {float(length[mask].mean()):.2f}")
    assert 200 <= ball.sum() <= 1500
    assert b < DRAG_BOUND * a, (a, b)
    acc.close()
    ref_acc.close()
    world.close()
