"""Temporal reprojection on the GPU (rt_history_*), bit for bit
against the numpy restatement of its contract (history_ref.py).

Outputs are compared as raw f32 bits and raw bytes, with one allowance: any NaN
equals any NaN.  Nothing expected comes from the library's history: the
accumulator cases take its inputs (sums, counts, first-hit records, the camera's
floats, each pinned by its own suite) and restate the resolve over them.
"""
import numpy as np
import pytest

import filter_ref as FR
import history_ref as HR
import raytracer_amd as R
import scene_values as V
from conftest import scene_text

pytestmark = pytest.mark.gpu

F = np.float32
DT = R.FIRST_HIT_DTYPE
INF = F(np.inf)
NAN = F(np.nan)

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape, got.dtype)
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = (gb != wb) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} f32 values differ, first at {at}: "
                             f"got {got[at]!r} ({gb[at]:#x}), want {want[at]!r} ({wb[at]:#x})")


# ---- 1. rt_history_run on synthetic views ------------------------------------------------

def camera(origin=(0.0, 0.0, 0.0), yaw=0.0, mirror=False, half_w=1.5, half_h=1.0):
    """12 floats of a camera at origin looking down -z turned by yaw about y;
    mirror: horizontal negated and the corner on the other side (det < 0)."""
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    sx = -1.0 if mirror else 1.0
    hv = rot @ np.array([2 * half_w * sx, 0, 0])
    vv = rot @ np.array([0, 2 * half_h, 0])
    a = rot @ np.array([-half_w * sx, -half_h, -1.0])
    o = np.array(origin, np.float64)
    return np.concatenate([o, o + a, hv, vv]).astype(F)


def view(cam, w, h):
    """Records of what the camera sees of a small world: the plane z = -5 in strips
    of three prim ids, sky above y = 3 and where a ray misses the plane.  The
    rays go through the pixel centres (computed in f64: these are inputs)."""
    c = cam.astype(np.float64)
    o, a, hv, vv = c[0:3], c[3:6] - c[0:3], c[6:9], c[9:12]
    rows, cols = np.mgrid[0:h, 0:w]
    u = (cols + 0.5) / max(w - 1, 1)
    v = ((h - 1 - rows) + 0.5) / max(h - 1, 1)
    d = a + u[..., None] * hv + v[..., None] * vv
    with np.errstate(all="ignore"):
        t = (-5.0 - o[2]) / d[..., 2]
    pos = o + t[..., None] * d
    hit = (t > 0) & np.isfinite(t) & (pos[..., 1] < 3.0)
    rec = np.zeros((h, w), DT)
    rec["prim"] = np.where(hit, 1 + np.floor(pos[..., 0]).astype(np.int64) % 3, 0)
    rec["t"] = np.where(hit, t, np.inf)
    rec["position"] = np.where(hit[..., None], pos, 0)
    rec["normal"][..., 2] = np.where(hit, 1, 0)
    return rec


def inputs(w, h, seed):
    rng = np.random.default_rng(seed)
    rgb = rng.random((h, w, 3), dtype=F) * F(2)
    n = rng.integers(1, 5, (h, w)).astype(np.uint32)
    prgbl = rng.random((h, w, 4), dtype=F) * F(2)
    prgbl[..., 3] = rng.integers(1, 40, (h, w)).astype(F)
    return rgb, n, prgbl


def run_both(rgb, n, rec, pcam, prgbl, prec, what, **opts):
    want = HR.resolve(rgb, n, rec, pcam, prgbl, prec, **{"max_history": 32.0, "sigma_z": 0.02, **opts})
    got = R.history_run(rgb, n, rec, pcam, prgbl, prec, **opts)
    same_bits(got, want, what)
    return got


SIZES = [(1, 1), (1, 7), (7, 1), (9, 9), (70, 50)]
PAIRS = {
    "identity": (camera(), camera()),
    "translated": (camera(), camera((0.3, 0.1, 0.2))),
    "rotated": (camera(), camera((0.1, 0.0, 0.0), yaw=0.08)),
    "behind": (camera((0.0, 0.0, -10.0)), camera()),            # every point is behind prev: det < 0 < s
    "mirrored": (camera(mirror=True), camera((0.2, 0.0, 0.0))),  # det > 0 and s > 0: in front
    "mirrored_behind": (camera((0.0, 0.0, -10.0), mirror=True), camera()),  # s < 0 < det
}


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("w,h", SIZES)
def test_run_on_synthetic_views(w, h, pair):
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = memo(("inputs", w, h), lambda: inputs(w, h, 7))
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    got = run_both(rgb, n, rec, pcam, prgbl, prec, f"{pair} {w}x{h}")
    hit = rec["prim"] != 0
    took = got[..., 3] > n.astype(F)
    if (w, h) == (70, 50):
        assert hit.any() and not hit.all()
        front, _, _ = HR.project(pcam, rec["position"], w, h)
        if pair == "identity":
            # every hit pixel finds itself among the taps around its own centre
            assert (took | ~(hit & (prec["prim"] == rec["prim"]))).all() and took[hit].mean() > 0.9
        elif pair in ("translated", "rotated", "mirrored"):
            assert front[hit].all() and took[hit].mean() > 0.5 and not took[hit].all()
        else:
            assert not front[hit].any() and not took.any()
    assert not took[~hit].any()  # sky takes no history
    if "behind" in pair:
        same_bits(got[..., :3], rgb, "behind: the means")


@pytest.mark.parametrize("w,h", SIZES)
def test_run_without_prev(w, h):
    rgb, n, _ = memo(("inputs", w, h), lambda: inputs(w, h, 7))
    rec = view(camera(), w, h)
    got = run_both(rgb, n, rec, None, None, None, f"no prev {w}x{h}")
    same_bits(got[..., :3], rgb, "no prev: the means")
    assert (got[..., 3] == n.astype(F)).all()


def special(w=70, h=50):
    pcam, ccam = PAIRS["translated"]
    rgb, n, prgbl = inputs(w, h, 11)
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    rng = np.random.default_rng(12)
    hit = np.argwhere(rec["prim"] != 0)
    pick = [tuple(p) for p in hit[rng.choice(len(hit), 40, replace=False)]]
    rec["position"][pick[0]] = (NAN, F(0), F(-5))
    rec["position"][pick[1]] = (INF, F(1), F(-5))
    rec["position"][pick[2]] = (NAN,) * 3
    rec["position"][pick[3]] = (-INF, INF, INF)
    rec["position"][pick[4]] = (F(1e38), F(1e38), F(-1e38))
    rec["position"][pick[5]] = (F(1e38), F(0), F(-5))
    rec["position"][pick[6]] = (F(0), F(0), -INF)
    rec["t"][pick[7]] = INF
    rec["t"][pick[8]] = INF
    rec["t"][pick[9]] = NAN
    rec["t"][pick[10]] = F(0)
    rec["normal"][pick[11]] = 0
    rec["normal"][pick[12]] = 0
    rec["normal"][pick[13]] = (NAN, F(0), F(1))
    for k in range(14, 20):
        n[pick[k]] = (33, 100, 4096, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF)[k - 14]  # larger than max_history
    n[pick[20]] = 0                                                                  # (no render holds it: 1/0)
    phit = np.argwhere(prec["prim"] != 0)
    ppick = [tuple(p) for p in phit[rng.choice(len(phit), 160, replace=False)]]
    lens = (F(0), F(-0.0), F(-3), NAN, INF, F(1e-40), F(0.5), F(1e38))
    cols = (NAN, INF, -INF, F(1e-40), F(-1e-45), F(3e38), F(-1.5), F(0))
    for k, p in enumerate(ppick[:80]):
        prgbl[p][3] = lens[k % len(lens)]
    for k, p in enumerate(ppick[80:]):
        prgbl[p][k % 3] = cols[k % len(cols)]
    for k, p in enumerate(pick[21:30]):
        rgb[p][k % 3] = cols[k % len(cols)]
    prec["position"][ppick[0]] = (NAN, NAN, NAN)
    prec["position"][ppick[81]] = (INF, F(0), F(-5))
    return rgb, n, rec, pcam, prgbl, prec


@pytest.mark.parametrize("opts", [dict(), dict(max_history=1.0), dict(max_history=3.0, sigma_z=1e-6),
                                  dict(max_history=3e38, sigma_z=3e38)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_run_special_values(opts):
    rgb, n, rec, pcam, prgbl, prec = memo("special", special)
    got = run_both(rgb, n, rec, pcam, prgbl, prec, f"special {opts}", **opts)
    assert np.isnan(got).any() and np.isinf(got).any()  # (they reach the output: the contract decides where)
    if opts.get("max_history") == 1.0:
        ok = np.isfinite(got[..., 3]) & (n > 0)
        assert (got[..., 3][ok] == n.astype(F)[ok]).all()  # cap = nf: the length never grows
    if not opts:
        assert (got[..., 3] > n.astype(F)).any() and np.nanmax(got[..., 3][n < 32]) <= 32.0


def test_run_exact_edges():
    """Points that project exactly onto fx = -1, fx = width, fx = -0.5 and an integer
    fx (likewise fy), under a camera of powers of two at 9 x 9: u = (x + 1) / 2 for
    a point (x, y, -1), so fx = 4 (x + 1) - 0.5."""
    w = h = 9
    pcam = np.array([0, 0, 0, -1, -1, -1, 2, 0, 0, 0, 2, 0], F)
    xs = np.array([-1.125, 1.375, -1.0, -0.125, -1.0625, 1.25, 0.0], F)  # fx = -1, 9, -0.5, 3, -0.75, 8.5, 3.5
    want_fx = np.array([-1, 9, -0.5, 3, -0.75, 8.5, 3.5], F)
    rec = np.zeros((h, w), DT)
    rec["prim"] = 1
    rec["t"] = 1
    rec["normal"][..., 2] = 1
    rec["position"][..., 2] = -1
    rec["position"][..., 0] = np.resize(xs, (h, w))
    rec["position"][..., 1] = np.resize(xs, (w, h)).T
    front, fx, fy = HR.project(pcam, rec["position"], w, h)
    assert front.all()
    assert fx.tobytes() == np.resize(want_fx, (h, w)).tobytes() and fy.tobytes() == np.resize(want_fx, (w, h)).T.tobytes()
    prec = np.zeros((h, w), DT)
    prec["prim"] = 1
    prec["position"][..., 2] = -1
    rgb, n, prgbl = inputs(w, h, 5)
    got = run_both(rgb, n, rec, pcam, prgbl, prec, "exact edges", sigma_z=1.0)
    took = got[..., 3] > n.astype(F)
    edge = np.isin(fx, (-1, 9)) | np.isin(fy, (-1, 9))
    assert not took[edge].any() and took[~edge].all()
    # an integer fx and fy: the whole weight is on one tap, prev's column 3 of bottom row 3
    whole = np.argwhere((fx == 3) & (fy == 3))
    assert len(whole)
    for at in map(tuple, whole):
        assert got[at][3] == min(F(32), prgbl[h - 1 - 3, 3, 3] + F(n[at]))
        alpha = F(n[at]) / got[at][3]
        for k in range(3):
            assert got[at][k] == prgbl[h - 1 - 3, 3, k] + (rgb[at][k] - prgbl[h - 1 - 3, 3, k]) * alpha


# ---- 2. accumulator sequences -------------------------------------------------------------

def orbit(world, deg, w, h, target=(0.0, 0.0, -1.0), radius=1.0):
    a = np.deg2rad(deg)
    world.look_at((target[0] + radius * np.sin(a), target[1], target[2] + radius * np.cos(a)), target,
                  vfov=np.pi / 2, aspect=w / h)


class Session:
    """An accumulator with a history beside the restatement's bookkeeping."""

    def __init__(self, src, w, h, adaptive=False, stride=64, **opts):
        self.world = R.World(src)
        self.acc = self.world.accumulator(w, h, stride)
        if adaptive:
            self.acc.set_adaptive(0.5, 0.05, 2)
        self.adaptive, self.w, self.h, self.edit = adaptive, w, h, 0
        self.acc.history_enable(**opts)
        self.ref = HR.History(**{"max_history": 32.0, "sigma_z": 0.02, **opts})
        self.frame = None

    def add(self, k):
        self.frame, _ = self.acc.add(k, stats=False)

    def samples(self):
        return self.acc.counts() if self.adaptive else np.full((self.h, self.w), self.acc.samples, np.uint32)

    def resolve(self, what):
        """One resolve checked against the restatement -> (rgb, rgba, len, n, records)."""
        acc = self.acc
        n = self.samples()
        rec = self.world.first_hit(self.w, self.h)
        want = self.ref.resolve(acc.sums(), n, rec, self.world.camera(), self.edit)
        rgb, px = acc.resolved()
        length = acc.history_length()
        same_bits(rgb, want[0], f"{what}: out_rgb")
        assert px.tobytes() == want[1].tobytes(), f"{what}: RGBA8"
        same_bits(length, want[2], f"{what}: history_length")
        return rgb, px, length, n, rec

    def close(self):
        self.acc.close()
        self.world.close()


def scene_source(which):
    return memo("soup", lambda: V.soup(40)) if which == "soup" else scene_text(which)


# Share of the hit pixels that keep history over the 2 degree step of the third
# resolve, by the restatement alone: three_spheres 48 x 32 0.998 of 1112, soup
# 40 x 24 0.894 of 123 (first GPU run; the test asserts the three quarters asked for).
@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "adaptive"])
@pytest.mark.parametrize("which,w,h,target,radius", [("three_spheres.txt", 48, 32, (0.0, 0.0, -1.0), 1.0),
                                                     ("soup", 40, 24, (0.0, 0.0, -3.0), 3.0)])
def test_accumulator_sequences(which, w, h, target, radius, adaptive):
    s = Session(scene_source(which), w, h, adaptive)
    what = f"{which} {'adaptive' if adaptive else 'plain'}"
    orbit(s.world, 0, w, h, target, radius)
    assert (s.acc.history_length() == 0).all()
    s.add(2)
    rgb, px, length, n, rec = s.resolve(f"{what}: first resolve")
    assert px.tobytes() == s.frame.tobytes()  # prev invalid, no filter: the accumulator's last frame
    assert (length == n.astype(F)).all()
    s.add(2)
    _, px, length, n, _ = s.resolve(f"{what}: same camera")  # prev untouched: still none
    assert px.tobytes() == s.frame.tobytes() and (length == n.astype(F)).all()
    orbit(s.world, 2, w, h, target, radius)
    s.add(1)
    _, _, length, n, rec = s.resolve(f"{what}: after a move")
    hit = rec["prim"] != 0
    took = length > n.astype(F)
    share = float(took[hit].mean())
    print(f"history share {what}: {share:.3f} of {int(hit.sum())} hit pixels keep history")
    assert took.any(), "reprojection is off: no pixel took history"
    assert share >= 0.75 and not took[~hit].any()
    if not adaptive:
        assert length.max() == 5.0  # 4 samples of the last view and 1 of this one
    # a second resolve under the same camera: cur is recomputed from the same prev
    s.add(1)
    _, _, length2, _, _ = s.resolve(f"{what}: same camera after a move")
    if not adaptive:
        assert length2.max() == 6.0
    # two moves with no resolve in between: prev is the last view that was resolved
    orbit(s.world, 4, w, h, target, radius)
    s.add(1)
    orbit(s.world, 6, w, h, target, radius)
    s.add(1)
    _, _, length, n, _ = s.resolve(f"{what}: two moves, one resolve")
    assert (length > n.astype(F)).any()
    # an edit drops the history
    s.world.set_material(1, 0, (0.2, 0.9, 0.1))
    s.edit += 1
    s.add(1)
    _, px, length, n, _ = s.resolve(f"{what}: after an edit")
    assert (length == n.astype(F)).all() and px.tobytes() == s.frame.tobytes()
    orbit(s.world, 8, w, h, target, radius)
    s.add(1)
    _, _, length, n, _ = s.resolve(f"{what}: a move after the edit")
    assert (length > n.astype(F)).any()
    s.close()


def test_options_reach_the_kernel():
    w, h = 48, 32
    s = Session(scene_text("three_spheres.txt"), w, h, max_history=3.0, sigma_z=0.005)
    orbit(s.world, 0, w, h)
    s.add(4)
    s.resolve("options: first")
    orbit(s.world, 2, w, h)
    s.add(1)
    _, _, length, _, _ = s.resolve("options: moved")
    assert length.max() == 3.0
    orbit(s.world, 4, w, h)
    s.add(8)
    _, _, length, _, _ = s.resolve("options: more samples than max_history")
    assert (length == 8.0).all()
    s.close()


# ---- 3. state rules ------------------------------------------------------------------------

def test_state_rules():
    import torch

    w, h = 48, 32
    s = Session(scene_text("three_spheres.txt"), w, h)
    acc, world = s.acc, s.world
    orbit(world, 0, w, h)
    with pytest.raises(R.RenderError, match="rt_history_resolve: no samples held"):
        acc.resolved()
    s.add(2)
    s.resolve("state: first")
    orbit(world, 2, w, h)
    with pytest.raises(R.RenderError, match="no samples held"):  # (the move reset the accumulator)
        acc.resolved()
    s.add(1)
    rgb, px, length, n, rec = s.resolve("state: moved")
    assert (length > n.astype(F)).any()
    # filtered: the filter of the unfiltered output with the records; the history keeps the unfiltered one
    for opts in (dict(), dict(levels=2, flags=R.FILTER_SAME_PRIM)):
        want = FR.filter_image(rgb, rec, **opts)
        got = acc.resolved(filter=opts)
        same_bits(got[0], want[0], f"filtered {opts}")
        assert got[1].tobytes() == want[1].tobytes()
        same_bits(acc.history_length(), length, "filtered: the length")
    assert got[0].tobytes() != rgb.tobytes()
    again = acc.resolved()
    same_bits(again[0], rgb, "unfiltered again")
    assert again[1].tobytes() == px.tobytes()
    with pytest.raises(R.RenderError, match="rt_history_resolve: levels"):
        acc.resolved(filter=dict(levels=9))
    # the device entry on a caller's stream: the host entry's bytes
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_out = torch.zeros(h, w, 3, dtype=torch.float32, device="cuda")
        d_px = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
        d_px2 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
    st.synchronize()
    acc.resolved_device(d_out.data_ptr(), d_px.data_ptr(), st.cuda_stream)
    st.synchronize()
    same_bits(d_out.cpu().numpy(), rgb, "device entry")
    assert d_px.cpu().numpy().tobytes() == px.tobytes()
    acc.resolved_device(0, d_px2.data_ptr(), st.cuda_stream, filter=dict())
    acc.resolved_device(d_out.data_ptr(), 0, 0)  # (the library's stream, ordered by the library)
    s.add(1)                                     # (a pass after it, likewise)
    torch.cuda.synchronize()
    assert d_px2.cpu().numpy().tobytes() == FR.filter_image(rgb, rec)[1].tobytes()
    same_bits(d_out.cpu().numpy(), rgb, "device entry, library stream")
    with pytest.raises(R.RenderError, match="rt_history_resolve_device: null output"):
        acc.resolved_device(0, 0, st.cuda_stream)
    s.resolve("state: after the device entries")
    # reset: both snapshots go, the setting stays
    acc.history_reset()
    s.ref.reset()
    assert (acc.history_length() == 0).all()
    _, px, length, n, _ = s.resolve("state: after history_reset")
    assert (length == n.astype(F)).all() and px.tobytes() == s.frame.tobytes()
    # enable again with other options: the snapshots go too
    orbit(world, 4, w, h)
    s.add(1)
    s.resolve("state: moved after the reset")
    acc.history_enable(max_history=4.0)
    s.ref = HR.History(4.0, 0.02)
    _, _, length, n, _ = s.resolve("state: enabled again")
    assert (length == n.astype(F)).all()
    # disabled: every history call but enable says so
    acc.history_disable()
    for call, name in ((acc.resolved, "rt_history_resolve"), (acc.history_length, "rt_history_read_length"),
                       (acc.history_reset, "rt_history_reset")):
        with pytest.raises(R.RenderError, match=f"{name}: the accumulator's history is not enabled"):
            call()
    acc.filtered()  # (the accumulator and its filter are as before)
    acc.history_enable()
    s.ref = HR.History()
    s.resolve("state: enabled after disable")
    world.close()
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.resolved()
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.history_length()
    acc.close()


# ---- 4. quality ----------------------------------------------------------------------------

QUALITY_BOUND = 0.609  # the midpoint between the measured 0.2185 and 1


def test_quality_on_an_orbit():
    """Measured on the GPU (profiles/history/quality.txt): the MSE of the last step's
    unfiltered resolve over the MSE of the accumulator's own 1-sample frame is 0.2185
    (0.002506 against 0.01147, mean history length 5.75 with the sky's 1); asserted
    below the midpoint between that and 1."""
    w, h = 96, 64
    world = R.World(scene_text("three_spheres.txt"))
    acc = world.accumulator(w, h, 4)
    acc.history_enable()
    for step in range(8):
        orbit(world, 2 * step, w, h)
        acc.add(1, stats=False)
        resolved, _ = acc.resolved()
    noisy = FR.means(acc.sums(), 1)
    ref_acc = world.accumulator(w, h, 1024, seed=99)
    ref_acc.add(1024, stats=False)
    ref = FR.means(ref_acc.sums(), 1024).astype(np.float64)
    mse_noisy = float(np.mean((noisy.astype(np.float64) - ref) ** 2))
    mse_resolved = float(np.mean((resolved.astype(np.float64) - ref) ** 2))
    print(f"history quality: 1-sample MSE {mse_noisy:.4g}, resolved MSE {mse_resolved:.4g}, "
          f"ratio {mse_resolved / mse_noisy:.4f}, mean length {float(acc.history_length().mean()):.2f}")
    assert mse_resolved < QUALITY_BOUND * mse_noisy, (mse_resolved, mse_noisy)
    acc.close()
    ref_acc.close()


# ---- 5. full size --------------------------------------------------------------------------

def test_full_size_resolve_after_a_move():
    w, h, band = 1920, 1080, slice(508, 572)
    world = R.World(scene_text("rtow.txt"))
    acc = world.accumulator(w, h, 4)
    acc.history_enable()
    cam0 = world.camera()
    acc.add(2, stats=False)
    rgb0, px0 = acc.resolved()
    sums0, rec0 = acc.sums(), world.first_hit(w, h)
    world.translate_camera(0.05, 0.02, 0.0)
    frame, _ = acc.add(1, stats=False)
    rgb1, px1 = acc.resolved()
    length = acc.history_length()
    sums1, rec1 = acc.sums(), world.first_hit(w, h)
    same_bits(rgb0, FR.means(sums0, 2), "first resolve: the means")
    # the band's rows against the restatement: prev is whole (taps land anywhere), the view is the band
    prgbl = np.concatenate([rgb0, np.full((h, w, 1), 2, F)], axis=2)
    want = HR.resolve(FR.means(sums1, 1)[band], 1, rec1[band], cam0, prgbl, rec0)
    same_bits(rgb1[band], want[..., :3], "band: out_rgb")
    same_bits(length[band], want[..., 3], "band: length")
    assert px1[band].tobytes() == FR.rgba8(np.ascontiguousarray(want[..., :3])).tobytes()
    hit = rec1["prim"] != 0
    assert (length[hit] > 1).mean() > 0.75 and (length[~hit] == 1).all()
    assert np.isfinite(rgb1).all() and (px1[..., 3] == 255).all() and px1.tobytes() != frame.tobytes()
    acc.close()


