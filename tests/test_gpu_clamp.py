"""The neighbourhood clamp of the history resolve on the GPU (rt_clamp_*, DESIGN.md
5.10a), bit for bit against the numpy restatement of its contract (clamp_ref.py).

Outputs are compared as raw f32 bits and raw bytes, with one allowance: any NaN
equals any NaN.  Nothing expected comes from the library's resolve: the
accumulator cases take its inputs (sums, counts, first-hit records, the camera's
floats, each pinned by its own suite) and restate the resolve over them.  The
synthetic views, the sessions' scenes and the orbit are test_gpu_history.py's.
"""
import numpy as np
import pytest

import clamp_ref as CR
import filter_ref as FR
import history_ref as HR
import raytracer_amd as R
from conftest import scene_text
from test_gpu_history import PAIRS, SIZES, camera, inputs, memo, orbit, same_bits, scene_source, special, view

pytestmark = pytest.mark.gpu

F = np.float32
INF = F(np.inf)
NAN = F(np.nan)
RADII = (1, 2, 3)
GAMMAS = (0.0, 1.0, 1.5)


def run_both(rgb, n, rec, pcam, prgbl, prec, clamp, what, **opts):
    """rt_clamp_run against the restatement, the box first: a moments mistake is told from a blend mistake."""
    want, wbox = CR.resolve(rgb, n, rec, pcam, prgbl, prec, **{"max_history": 32.0, "sigma_z": 0.02, **opts},
                            clamp=clamp)
    got, box = R.clamp_run(rgb, n, rec, pcam, prgbl, prec, clamp=clamp, **opts)
    same_bits(box, wbox, f"{what}: out_box")
    same_bits(got, want, f"{what}: out_rgbl")
    return got, box


# ---- 1. rt_clamp_run on synthetic views ----------------------------------------------------

@pytest.mark.parametrize("pair", ["identity", "translated", "rotated", "behind", "mirrored"])
@pytest.mark.parametrize("w,h", SIZES)
def test_run_on_synthetic_views(w, h, pair):
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = memo(("inputs", w, h), lambda: inputs(w, h, 7))
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    plain = HR.resolve(rgb, n, rec, pcam, prgbl, prec)
    has = plain[..., 3] > n.astype(F)
    for radius in RADII:
        for gamma in GAMMAS:
            got, box = run_both(rgb, n, rec, pcam, prgbl, prec, dict(gamma=gamma, radius=radius),
                                f"{pair} {w}x{h} r{radius} g{gamma}")
            same_bits(got[..., 3], plain[..., 3], "len is the unclamped resolve's")
            same_bits(got[~has], plain[~has], "pixels without history are untouched")
            if gamma == 0.0:
                same_bits(box[..., :3], box[..., 3:], "gamma 0: lo is hi")
            if (w, h) == (70, 50) and pair in ("identity", "translated", "rotated") and gamma == 1.0:
                changed = (got[..., :3] != plain[..., :3]).any(axis=2)
                assert 0.1 < changed[has].mean() < 0.9  # (test_clamp_ref.py: neither vacuous nor total)
    if (w, h) == (1, 1) and has.all():
        same_bits(got[..., :3], rgb, "1 x 1: the pixel's own mean")


@pytest.mark.parametrize("w,h", SIZES)
def test_run_without_prev_and_without_box(w, h):
    rgb, n, prgbl = memo(("inputs", w, h), lambda: inputs(w, h, 7))
    pcam, ccam = PAIRS["translated"]
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    got, box = run_both(rgb, n, rec, None, None, None, dict(gamma=1.0, radius=2), f"no prev {w}x{h}")
    same_bits(got[..., :3], rgb, "no prev: the means")
    assert (got[..., 3] == n.astype(F)).all()
    # out_box NULL: the same out_rgbl
    want, _ = CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=dict(gamma=1.0, radius=2))
    got, none = R.clamp_run(rgb, n, rec, pcam, prgbl, prec, clamp=dict(gamma=1.0, radius=2), box=False)
    assert none is None
    same_bits(got, want, f"no box {w}x{h}")
    # clamp NULL: the defaults
    want, wbox = CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=dict(gamma=1.5, radius=1))
    got, box = R.clamp_run(rgb, n, rec, pcam, prgbl, prec)
    same_bits(box, wbox, "defaults: out_box")
    same_bits(got, want, "defaults: out_rgbl")


# ---- 2. a seam case that localises an index mistake ----------------------------------------

def test_seams_with_distinct_means():
    """24 x 24 = 3 x 3 tiles, every mean distinct, gamma = 0, radius = 3: out_box is mu,
    so a tap taken from the wrong pixel shows at the pixel and channel where it was taken."""
    w = h = 24
    cam = camera()
    rec = view(cam, w, h)
    rows, cols = np.mgrid[0:h, 0:w]
    base = (cols + 100 * rows).astype(F)
    rgb = np.stack([base, base + F(0.25), base * F(2)], axis=2)
    n = np.ones((h, w), np.uint32)
    prgbl = np.concatenate([rgb[::-1, ::-1], np.full((h, w, 1), 8, F)], axis=2).astype(F)
    _, _, mu = CR.box(rgb, 0.0, 3)
    got, box = run_both(rgb, n, rec, cam, prgbl, rec, dict(gamma=0.0, radius=3), "seams")
    same_bits(box[..., :3], mu, "lo is mu")
    same_bits(box[..., 3:], mu, "hi is mu")
    assert len(np.unique(mu[..., 0])) > 500  # (the means tell the pixels apart)
    has = got[..., 3] > 1
    assert has.any()
    same_bits(got[..., :3][has], (mu + (rgb - mu) * (F(1) / got[..., 3:4]))[has], "gamma 0: hc is mu")


# ---- 3. special values ----------------------------------------------------------------------

def special_clamp():
    rgb, n, rec, pcam, prgbl, prec = (np.copy(a) for a in special())
    rng = np.random.default_rng(13)
    hit = np.argwhere(rec["prim"] != 0)
    pick = [tuple(p) for p in hit[rng.choice(len(hit), 24, replace=False)]]
    vals = (NAN, INF, -INF, F(1e-40), F(-1e-45), F(1e38), F(-1e38), F(3e38))
    for k, p in enumerate(pick):
        rgb[p][k % 3] = vals[k % len(vals)]
    return rgb, n, rec, pcam, prgbl, prec, pick


@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("gamma", [0.0, 1.5, 3.4028234663852886e38])
def test_run_special_values(radius, gamma):
    """NaN, +-inf, denormal and 1e38 means (s2 overflows: the variance is NaN and hc is
    left alone), n = 0, len 0 in prev."""
    rgb, n, rec, pcam, prgbl, prec, pick = memo("special_clamp", special_clamp)
    got, box = run_both(rgb, n, rec, pcam, prgbl, prec, dict(gamma=gamma, radius=radius),
                        f"special r{radius} g{gamma}")
    assert np.isnan(got).any() and np.isinf(got).any() and np.isnan(box).any()
    assert (n == 0).any() and (prgbl[..., 3] == 0).any()
    # the 1e38 mean: 1e38 * 1e38 overflows, inf * ic - mu * mu is inf or NaN, never a finite width
    p = pick[5]
    k = 5 % 3
    assert rgb[p][k] == F(1e38) and not np.isfinite(box[p][3 + k] - box[p][k])
    plain = HR.resolve(rgb, n, rec, pcam, prgbl, prec)
    nanbox = np.isnan(box[..., :3]) & np.isnan(box[..., 3:])
    same_bits(got[..., :3][nanbox], plain[..., :3][nanbox], "a NaN box leaves the resolve alone")
    assert nanbox.any()


def test_run_radius_larger_than_the_image():
    w = h = 2
    pcam, ccam = PAIRS["identity"]
    rgb, n, prgbl = inputs(w, h, 3)
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    got, box = run_both(rgb, n, rec, pcam, prgbl, prec, dict(gamma=1.0, radius=3), "radius 3 at 2 x 2")
    # every pixel's neighbourhood is the whole image: one box
    for at in ((0, 1), (1, 0), (1, 1)):
        same_bits(box[at], box[0, 0], "one box")


# ---- 4. accumulator sequences --------------------------------------------------------------

class Session:
    """An accumulator with a history and a clamp beside the restatement's bookkeeping."""

    def __init__(self, src, w, h, adaptive=False, stride=64, clamp=None, history=True):
        self.world = R.World(src)
        self.acc = self.world.accumulator(w, h, stride)
        if adaptive:
            self.acc.set_adaptive(0.5, 0.05, 2)
        self.adaptive, self.w, self.h, self.edit = adaptive, w, h, 0
        if history:
            self.acc.history_enable()
        self.ref = CR.ClampHistory()
        if clamp is not None:
            self.clamp(**clamp)
        self.frame = None

    def clamp(self, **opts):
        self.acc.clamp_enable(**opts)
        self.ref.clamp = {"gamma": 1.5, "radius": 1, **opts}

    def unclamp(self):
        self.acc.clamp_disable()
        self.ref.clamp = None

    def add(self, k):
        self.frame, _ = self.acc.add(k, stats=False)

    def samples(self):
        return self.acc.counts() if self.adaptive else np.full((self.h, self.w), self.acc.samples, np.uint32)

    def resolve(self, what, ref=None):
        """One resolve checked against the restatement -> (rgb, rgba, len, n, records)."""
        acc = self.acc
        n = self.samples()
        rec = self.world.first_hit(self.w, self.h)
        want = (ref or self.ref).resolve(acc.sums(), n, rec, self.world.camera(), self.edit)
        rgb, px = acc.resolved()
        length = acc.history_length()
        same_bits(rgb, want[0], f"{what}: out_rgb")
        assert px.tobytes() == want[1].tobytes(), f"{what}: RGBA8"
        same_bits(length, want[2], f"{what}: history_length")
        return rgb, px, length, n, rec

    def close(self):
        self.acc.close()
        self.world.close()


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
@pytest.mark.parametrize("which,w,h,target,radius", [("three_spheres.txt", 48, 32, (0.0, 0.0, -1.0), 1.0),
                                                     ("soup", 40, 24, (0.0, 0.0, -3.0), 3.0)])
def test_accumulator_sequences(which, w, h, target, radius, adaptive):
    s = Session(scene_source(which), w, h, adaptive, clamp=dict(gamma=1.0, radius=2))
    what = f"{which} {'adaptive' if adaptive else 'plain'}"
    orbit(s.world, 0, w, h, target, radius)
    s.add(2)
    _, px, length, n, _ = s.resolve(f"{what}: first resolve")
    assert px.tobytes() == s.frame.tobytes() and (length == n.astype(F)).all()  # prev invalid: the last frame
    s.add(2)
    _, px, length, n, _ = s.resolve(f"{what}: same camera")
    assert px.tobytes() == s.frame.tobytes() and (length == n.astype(F)).all()
    orbit(s.world, 2, w, h, target, radius)
    s.add(1)
    rgb, _, length, n, rec = s.resolve(f"{what}: after a move")
    took = length > n.astype(F)
    assert took.any() and not took[rec["prim"] == 0].any()
    # the same state without the clamp: history_ref's bits, and the clamp did bind
    plain = HR.History()
    plain.cur, plain.prev = s.ref.cur, s.ref.prev
    s.unclamp()
    rgb0, _, length0, _, _ = s.resolve(f"{what}: clamp disabled", ref=plain)
    s.ref.cur, s.ref.prev = plain.cur, plain.prev
    same_bits(length0, length, "the clamp leaves len alone")
    assert rgb0.tobytes() != rgb.tobytes(), "the clamp bound nowhere"
    s.clamp(gamma=1.0, radius=2)
    rgb2, _, _, _, _ = s.resolve(f"{what}: clamp enabled again")
    same_bits(rgb2, rgb, "enable and disable drop no snapshot")
    # a filtered resolve filters the clamped out with the same records
    want = FR.filter_image(rgb, rec)
    got = s.acc.resolved(filter=dict())
    same_bits(got[0], want[0], f"{what}: filtered")
    assert got[1].tobytes() == want[1].tobytes()
    same_bits(s.acc.history_length(), length, "filtered: the length")
    # other options reach the kernel from the same state
    s.clamp(gamma=0.0, radius=3)
    s.resolve(f"{what}: gamma 0, radius 3")
    s.clamp(gamma=1.0, radius=2)
    s.add(1)
    s.resolve(f"{what}: same camera after a move")
    # two moves with no resolve in between
    orbit(s.world, 4, w, h, target, radius)
    s.add(1)
    orbit(s.world, 6, w, h, target, radius)
    s.add(1)
    _, _, length, n, _ = s.resolve(f"{what}: two moves, one resolve")
    assert (length > n.astype(F)).any()
    s.close()


# ---- 5. keep on edit -----------------------------------------------------------------------

def test_edit_drops_the_history_without_the_flag():
    w, h = 48, 32
    s = Session(scene_text("three_spheres.txt"), w, h, clamp=dict())
    orbit(s.world, 0, w, h)
    s.add(2)
    s.resolve("no flag: first")
    orbit(s.world, 2, w, h)
    s.add(1)
    _, _, length, n, _ = s.resolve("no flag: moved")
    assert (length > n.astype(F)).any()
    s.world.set_material(1, 0, (0.2, 0.9, 0.1))
    s.edit += 1
    s.add(1)
    _, px, length, n, _ = s.resolve("no flag: after an edit")
    assert (length == n.astype(F)).all() and px.tobytes() == s.frame.tobytes()
    s.close()


def test_keep_on_edit():
    w, h = 48, 32
    s = Session(scene_text("three_spheres.txt"), w, h, clamp=dict(keep_on_edit=True))
    orbit(s.world, 0, w, h)
    s.add(4)
    s.resolve("keep: first")
    orbit(s.world, 2, w, h)
    s.add(1)
    s.resolve("keep: moved")
    # an edit and a move: the snapshots stay, cur becomes prev
    s.world.set_material(1, 0, (0.2, 0.9, 0.1))
    s.edit += 1
    orbit(s.world, 4, w, h)
    s.add(1)
    _, _, length, n, rec = s.resolve("keep: an edit and a move")
    ball = rec["prim"] == 2
    assert ball.sum() > 50 and (length[ball] > n.astype(F)[ball]).any()
    # an edit under the same camera: cur (another edit version) becomes prev, so history is carried
    s.world.set_material(1, 0, (0.9, 0.1, 0.6))
    s.edit += 1
    s.add(1)
    _, _, length, n, rec = s.resolve("keep: an edit, same camera")
    assert (length[rec["prim"] == 2] > 1).any() and (length > n.astype(F)).mean() > 0.5
    s.add(1)
    s.resolve("keep: same camera, same edit")  # (no swap: cur is recomputed from the same prev)
    # the flag taken away: the next edit drops both snapshots, as without a clamp
    s.clamp()
    s.world.set_material(1, 0, (0.3, 0.3, 0.3))
    s.edit += 1
    s.add(1)
    _, _, length, n, _ = s.resolve("keep: flag cleared, an edit")
    assert (length == n.astype(F)).all()
    s.close()


# ---- 6. state rules ------------------------------------------------------------------------

def test_state_rules():
    import torch

    w, h = 48, 32
    # enabled before the history exists: the setting waits for it
    s = Session(scene_text("three_spheres.txt"), w, h, clamp=dict(gamma=0.5, radius=2), history=False)
    acc, world = s.acc, s.world
    orbit(world, 0, w, h)
    s.add(2)
    with pytest.raises(R.RenderError, match="rt_history_resolve: the accumulator's history is not enabled"):
        acc.resolved()
    acc.history_enable()
    s.resolve("state: first")
    orbit(world, 2, w, h)
    s.add(1)
    rgb, px, length, n, rec = s.resolve("state: moved")
    assert (length > n.astype(F)).any()
    # enabled again after the history: other options, no snapshot dropped
    s.clamp(gamma=2.0, radius=1)
    rgb, px, length, n, rec = s.resolve("state: other options")
    with pytest.raises(R.RenderError, match="rt_clamp_enable: radius"):
        acc.clamp_enable(radius=0)
    s.resolve("state: after a refused enable")  # (the setting is as it was)
    # the device entry on a caller's stream: the host entry's bytes
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out = torch.zeros(h, w, 3, dtype=torch.float32, device="cuda")
        d_px = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
    st.synchronize()
    acc.resolved_device(d_out.data_ptr(), d_px.data_ptr(), st.cuda_stream)
    st.synchronize()
    same_bits(d_out.cpu().numpy(), rgb, "device entry")
    assert d_px.cpu().numpy().tobytes() == px.tobytes()
    # the setting survives rt_history_reset, rt_history_disable and rt_history_enable (which drop the snapshots)
    acc.history_reset()
    s.ref.reset()
    s.resolve("state: after history_reset")
    orbit(world, 4, w, h)
    s.add(1)
    rgb1, _, _, _, _ = s.resolve("state: moved after the reset")
    acc.history_disable()
    acc.history_enable()
    s.ref.reset()
    s.resolve("state: history disabled and enabled")
    orbit(world, 6, w, h)
    s.add(1)
    rgb2, _, length, n, _ = s.resolve("state: moved, the clamp still on")
    plain = HR.resolve(FR.means(acc.sums(), n), n, s.ref.cur["rec"], s.ref.prev["cam"], s.ref.prev["rgbl"],
                       s.ref.prev["rec"])
    assert plain[..., :3].tobytes() != rgb2.tobytes()  # (an unclamped resolve would differ)
    world.close()
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.resolved()
    with pytest.raises(R.RenderError, match="rt_clamp_enable: the accumulator's world was freed"):
        acc.clamp_enable()
    with pytest.raises(R.RenderError, match="rt_clamp_disable: the accumulator's world was freed"):
        acc.clamp_disable()
    acc.close()


# ---- 7. full size --------------------------------------------------------------------------

def test_full_size_resolve_after_a_move():
    w, h, top, bottom = 1920, 1080, 508, 572
    world = R.World(scene_text("rtow.txt"))
    acc = world.accumulator(w, h, 4)
    acc.history_enable()
    acc.clamp_enable(radius=1)
    cam0 = world.camera()
    acc.add(2, stats=False)
    rgb0, _ = acc.resolved()
    sums0, rec0 = acc.sums(), world.first_hit(w, h)
    same_bits(rgb0, FR.means(sums0, 2), "first resolve: the means")
    world.translate_camera(0.05, 0.02, 0.0)
    acc.add(1, stats=False)
    sums1, rec1 = acc.sums(), world.first_hit(w, h)
    prgbl = np.concatenate([rgb0, np.full((h, w, 1), 2, F)], axis=2)
    m1 = FR.means(sums1, 1)
    plain = HR.resolve(m1[top:bottom], 1, rec1[top:bottom], cam0, prgbl, rec0)
    for radius in (1, 3):
        acc.clamp_enable(radius=radius)  # (the same prev: a resolve under the same camera recomputes cur)
        rgb1, px1 = acc.resolved()
        length = acc.history_length()
        # the band and `radius` rows on each side for its boxes; prev is whole (taps land anywhere)
        ext = slice(top - radius, bottom + radius)
        want, _ = CR.resolve(m1[ext], 1, rec1[ext], cam0, prgbl, rec0, clamp=dict(gamma=1.5, radius=radius))
        want = want[radius:-radius]
        same_bits(rgb1[top:bottom], want[..., :3], f"band r{radius}: out_rgb")
        same_bits(length[top:bottom], want[..., 3], f"band r{radius}: length")
        assert px1[top:bottom].tobytes() == FR.rgba8(np.ascontiguousarray(want[..., :3])).tobytes()
        assert want[..., :3].tobytes() != plain[..., :3].tobytes()  # (the clamp binds in the band)
        assert np.isfinite(rgb1).all() and (px1[..., 3] == 255).all()
    hit = rec1["prim"] != 0
    assert (length[hit] > 1).mean() > 0.75 and (length[~hit] == 1).all()
    acc.close()


# ---- 8. quality ----------------------------------------------------------------------------

EDIT_BOUND = 0.769   # the midpoint between the measured (c) / (b) = 0.5384 and 1
ORBIT_BOUND = 0.607  # the midpoint between the measured clamped / 1-sample = 0.2133 and 1


def mse(a, b, mask=None):
    d = (a.astype(np.float64) - b) ** 2
    return float(np.mean(d if mask is None else d[mask]))


def edit_sequence(gamma):
    """Six 2 degree orbit steps at 1 sample with a resolve each, the diffuse ball
    recoloured, one more step -> (resolved, the 1-sample means, records, reference)."""
    w, h = 96, 64
    world = R.World(scene_text("three_spheres.txt"))
    acc = world.accumulator(w, h, 4)
    acc.history_enable()
    acc.clamp_enable(gamma=gamma, keep_on_edit=True)
    for step in range(6):
        orbit(world, 2 * step, w, h)
        acc.add(1, stats=False)
        acc.resolved()
    world.set_material(1, 0, (0.1, 0.2, 0.9))
    orbit(world, 12, w, h)
    acc.add(1, stats=False)
    resolved, _ = acc.resolved()
    noisy = FR.means(acc.sums(), 1)
    rec = world.first_hit(w, h)
    ref_acc = world.accumulator(w, h, 1024, seed=99)
    ref_acc.add(1024, stats=False)
    ref = FR.means(ref_acc.sums(), 1024).astype(np.float64)
    acc.close()
    ref_acc.close()
    world.close()
    return resolved, noisy, rec, ref


def test_quality_after_an_edit():
    """Measured on the GPU (profiles/clamp/quality.txt), over the pixels of the recoloured
    ball: (a) the accumulator's 1-sample frame, what an edit shows without KEEP_ON_EDIT;
    (b) the history kept with gamma = 1e30, a box that binds only where the neighbourhood
    is constant: stale colours; (c) the default clamp."""
    stale, noisy, rec, ref = edit_sequence(1e30)
    clamped, noisy_c, rec_c, ref_c = edit_sequence(1.5)
    assert noisy.tobytes() == noisy_c.tobytes() and rec.tobytes() == rec_c.tobytes()
    ball = rec["prim"] == 2
    a, b, c = mse(noisy, ref, ball), mse(stale, ref, ball), mse(clamped, ref, ball)
    print(f"clamp quality, edit: {int(ball.sum())} pixels of the ball; (a) 1-sample MSE {a:.4g}, "
          f"(b) stale history MSE {b:.4g}, (c) default clamp MSE {c:.4g}, (c)/(b) {c / b:.4f}, (c)/(a) {c / a:.4f}")
    assert 200 <= ball.sum() <= 1500
    assert c < EDIT_BOUND * b, (a, b, c)


def test_quality_on_an_orbit():
    """test_gpu_history.py's orbit with the default clamp: all pixels against the 1-sample
    frame (asserted), the metal and glass spheres against the unclamped resolve (reported)."""
    w, h = 96, 64
    world = R.World(scene_text("three_spheres.txt"))
    accs = {False: world.accumulator(w, h, 4), True: world.accumulator(w, h, 4)}
    out = {}
    for on, acc in accs.items():
        acc.history_enable()
        if on:
            acc.clamp_enable()
    for step in range(8):
        orbit(world, 2 * step, w, h)
        for on, acc in accs.items():
            acc.add(1, stats=False)
            out[on], _ = acc.resolved()
    noisy = FR.means(accs[True].sums(), 1)
    rec = world.first_hit(w, h)
    ref_acc = world.accumulator(w, h, 1024, seed=99)
    ref_acc.add(1024, stats=False)
    ref = FR.means(ref_acc.sums(), 1024).astype(np.float64)
    m_noisy, m_plain, m_clamp = mse(noisy, ref), mse(out[False], ref), mse(out[True], ref)
    print(f"clamp quality, orbit: 1-sample MSE {m_noisy:.4g}, unclamped {m_plain:.4g}, clamped {m_clamp:.4g}, "
          f"clamped / 1-sample {m_clamp / m_noisy:.4f}")
    for name, prim in (("metal", 3), ("glass", 4)):
        mask = rec["prim"] == prim
        print(f"clamp quality, orbit, {name} ({int(mask.sum())} pixels): 1-sample {mse(noisy, ref, mask):.4g}, "
              f"unclamped {mse(out[False], ref, mask):.4g}, clamped {mse(out[True], ref, mask):.4g}")
    assert m_clamp < ORBIT_BOUND * m_noisy, (m_clamp, m_noisy)
    for acc in accs.values():
        acc.close()
    ref_acc.close()
    world.close()
