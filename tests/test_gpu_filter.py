"""The edge-aware filter on the GPU (rt_filter_*), bit for bit
against the numpy restatement of its contract (filter_ref.py).

Outputs are compared as raw f32 bits and raw bytes, with one allowance: any NaN
equals any NaN.  Nothing expected comes from the library's filter: the
accumulator cases take its inputs (sums, counts, first-hit records, each pinned
by its own suite) and restate the filter over them.
"""
import numpy as np
import pytest

import filter_ref as FR
import raytracer_amd as R
import scene_values as V
from conftest import scene_text

pytestmark = pytest.mark.gpu

F = np.float32
DT = R.FIRST_HIT_DTYPE
INF = F(np.inf)

_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def the_filter(w, h):
    return memo(("filter", w, h), lambda: R.Filter(w, h))


def assert_same(got, want, what):
    """got = (rgb, rgba) of the library, want of the restatement."""
    (g_rgb, g_px), (w_rgb, w_px) = got, want
    if w_rgb is not None and g_rgb is not None:
        assert g_rgb.shape == w_rgb.shape and g_rgb.dtype == F
        gb, wb = g_rgb.view(np.uint32), w_rgb.view(np.uint32)
        bad = (gb != wb) & ~(np.isnan(g_rgb) & np.isnan(w_rgb))
        if bad.any():
            at = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{what}: {int(bad.sum())} f32 values differ, first at {at}: "
                                 f"got {g_rgb[at]!r} ({gb[at]:#x}), want {w_rgb[at]!r} ({wb[at]:#x})")
    if w_px is not None and g_px is not None:
        bad = g_px != w_px
        assert not bad.any(), (what, "rgba", int(bad.sum()), np.argwhere(bad)[:4].tolist())


# ---- 1. synthetic images -----------------------------------------------------------------

def synthetic(w, h, seed=1):
    """Seeded colours in [0, 4) and records built here: a sky band on top, below it
    two planes that meet at a crease (column w // 2), the left one split into
    strips of a few prim ids; unit normals."""
    rng = np.random.default_rng(seed)
    rgb = rng.random((h, w, 3), dtype=F) * F(4)
    rec = np.zeros((h, w), DT)
    ys, xs = np.mgrid[0:h, 0:w]
    xs, ys = xs.astype(F), ys.astype(F)
    jit = (rng.random((h, w, 3), dtype=F) - F(0.5)) * F(0.02)
    sky = ys < h // 5
    right = xs >= w // 2
    s = xs - F(w // 2)
    r2 = F(np.sqrt(F(0.5)))
    pos = np.empty((h, w, 3), F)
    pos[..., 0] = np.where(right, F(w // 2) * F(0.1) + s * F(0.1) * r2, xs * F(0.1))
    pos[..., 1] = -ys * F(0.1)
    pos[..., 2] = np.where(right, F(-5) - s * F(0.1) * r2, F(-5))
    pos = pos + jit
    nrm = np.zeros((h, w, 3), F)
    nrm[..., 2] = np.where(right, r2, F(1))
    nrm[..., 0] = np.where(right, r2, F(0))
    prim = np.where(right, 9, 1 + (np.arange(w)[None, :] // 5) % 3 + 0 * ys.astype(np.int64)).astype(np.uint32)
    t = np.sqrt((pos[..., 0] * pos[..., 0] + pos[..., 1] * pos[..., 1]) + pos[..., 2] * pos[..., 2])
    rec["prim"] = np.where(sky, 0, prim)
    rec["t"] = np.where(sky, INF, t)
    rec["normal"] = np.where(sky[..., None], F(0), nrm)
    rec["position"] = np.where(sky[..., None], F(0), pos)
    return rgb, rec


SIZES = [(1, 1), (3, 2), (37, 23), (100, 70)]
OPTION_SETS = [dict(levels=n) for n in (0, 1, 2, 3, 5, 8)] + [
    dict(flags=R.FILTER_SAME_PRIM), dict(levels=5, flags=R.FILTER_SAME_PRIM),
    dict(normal_squarings=0), dict(normal_squarings=8),
    dict(sigma_l=1e-3), dict(sigma_l=1e3), dict(sigma_z=1e-3), dict(sigma_z=1e3),
    dict(levels=2, sigma_l=1e3, sigma_z=1e3, normal_squarings=0),
]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_images(w, h, opts):
    rgb, rec = memo(("synthetic", w, h), lambda: synthetic(w, h))
    if (w, h) == (100, 70):
        assert rec["prim"].min() == 0 and len(np.unique(rec["prim"])) >= 5  # sky, three strips, the other plane
    want = FR.filter_image(rgb, rec, **opts)
    got = the_filter(w, h).run(rgb, rec, **opts)
    assert_same(got, want, f"{w}x{h} {opts}")
    if opts.get("levels", 3) == 0:
        assert got[0].tobytes() == rgb.tobytes()
    elif w > 1 and opts == dict(levels=3):
        assert got[0].tobytes() != rgb.tobytes()


# ---- 2. special values ---------------------------------------------------------------------

def special(w=37, h=23):
    rgb, rec = synthetic(w, h, seed=2)
    rgb, rec = rgb.copy(), rec.copy()
    vals = [F(np.nan), INF, -INF, F(-1.5), F(0), F(-0.0), F(1e38), F(1e-40)]
    rng = np.random.default_rng(3)
    for k, v in enumerate(vals):
        for n in range(6):
            y, x, c = int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(3))
            rgb[y, x, c] = v
        rgb[(5 + 2 * k) % h, (3 + 4 * k) % w] = v  # (a whole pixel of it)
    hit = np.argwhere(rec["prim"] != 0)
    pick = hit[rng.choice(len(hit), 12, replace=False)]
    rec["position"][tuple(pick[0])] = (F(np.nan), F(0), F(0))
    rec["position"][tuple(pick[1])] = (INF, F(1), F(-5))
    rec["position"][tuple(pick[2])] = (F(np.nan),) * 3
    rec["position"][tuple(pick[3])] = (-INF, INF, INF)
    rec["normal"][tuple(pick[4])] = 0  # a hit pixel with a zero normal
    rec["normal"][tuple(pick[5])] = 0
    rec["t"][tuple(pick[6])] = INF     # a hit pixel with t = inf
    rec["t"][tuple(pick[7])] = INF
    rec["t"][tuple(pick[8])] = F(0)
    rec["t"][tuple(pick[9])] = F(np.nan)
    rec["normal"][tuple(pick[10])] = (F(np.nan), F(0), F(1))
    rec["t"][tuple(pick[11])] = F(1e-40)
    return rgb, rec


@pytest.mark.parametrize("opts", [dict(), dict(levels=1), dict(levels=5, flags=R.FILTER_SAME_PRIM),
                                  dict(normal_squarings=0, sigma_z=1e3, sigma_l=1e3)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) or "defaults")
def test_special_values(opts):
    rgb, rec = memo("special", special)
    want = FR.filter_image(rgb, rec, **opts)
    got = the_filter(37, 23).run(rgb, rec, **opts)
    assert_same(got, want, f"special {opts}")
    assert np.isnan(want[0]).any() and np.isinf(want[0]).any()  # (they reach the output: the contract decides where)


# ---- 3. the device entry -------------------------------------------------------------------

def test_device_entry_with_torch_buffers():
    import torch

    w, h = 100, 70
    rgb, rec = memo(("synthetic", w, h), lambda: synthetic(w, h))
    flt = the_filter(w, h)
    host = flt.run(rgb, rec)
    assert_same(host, FR.filter_image(rgb, rec), "host entry")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_rgb = torch.from_numpy(rgb.copy()).cuda()
        d_rec = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).cuda()
        d_out = torch.zeros(h, w, 3, dtype=torch.float32, device="cuda")
        d_px = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
        d_px2 = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
    s.synchronize()
    flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), d_out.data_ptr(), d_px.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert_same((d_out.cpu().numpy(), d_px.cpu().numpy()), host, "device entry")
    assert d_rgb.cpu().numpy().tobytes() == rgb.tobytes()  # (the input is left alone)
    # only the RGBA8 output
    flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), 0, d_px2.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert_same((None, d_px2.cpu().numpy()), host, "device entry, rgba only")
    # only the f32 output, in place
    flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), d_rgb.data_ptr(), 0, s.cuda_stream)
    s.synchronize()
    assert_same((d_rgb.cpu().numpy(), None), host, "device entry, in place")
    with pytest.raises(R.RenderError, match="null output"):
        flt.run_device(d_rgb.data_ptr(), d_rec.data_ptr(), 0, 0, s.cuda_stream)


# ---- 4. accumulators -----------------------------------------------------------------------

def scene_source(which):
    if which == "soup":
        return memo("soup", lambda: V.soup(40))
    return scene_text(which)


def check_accumulator(world, acc, n, frame, accel, what, **opts):
    """acc holds n samples (n: a count or the plane of counts) and `frame` is its
    last pass's frame; returns the records the restatement used."""
    w, h = acc.width, acc.height
    sums = acc.sums()
    rec = world.first_hit(w, h, accel=accel)
    rgb = FR.means(sums, n)
    want = FR.filter_image(rgb, rec, **opts)
    got = acc.filtered(**opts)
    assert_same(got, want, f"{what}: filtered() against the restatement")
    assert_same(the_filter(w, h).run(rgb, rec, **opts), got, f"{what}: rt_filter_run on the same arrays")
    zero = acc.filtered(levels=0)
    assert zero[1].tobytes() == frame.tobytes(), f"{what}: levels = 0 is not the frame"
    assert_same(zero, (rgb, FR.rgba8(rgb)), f"{what}: levels = 0")
    return rec


@pytest.mark.parametrize("which,w,h", [("three_spheres.txt", 96, 64), ("rtow.txt", 48, 32), ("soup", 48, 32)])
def test_accumulators(which, w, h):
    world = R.World(scene_source(which))
    acc = world.accumulator(w, h, 16)
    frame, _ = acc.add(4)
    check_accumulator(world, acc, 4, frame, R.ACCEL_AUTO, f"{which} 4 samples")
    frame, _ = acc.add(4)
    check_accumulator(world, acc, 8, frame, R.ACCEL_AUTO, f"{which} 8 samples")
    check_accumulator(world, acc, 8, frame, R.ACCEL_AUTO, f"{which} 8 samples, other options", levels=2,
                      flags=R.FILTER_SAME_PRIM, sigma_z=0.5)
    acc.close()


def test_accumulator_validation_and_device_entry():
    import ctypes as C
    import torch

    w, h = 48, 32
    world = R.World(scene_text("rtow.txt"))
    acc = world.accumulator(w, h, 8, accel=R.ACCEL_BRUTE)
    L = R.lib()
    out = np.zeros((h, w, 3), F)
    for name, call in (("rt_filter_accum", lambda o, p: L.rt_filter_accum(acc._a, o, p, None)),
                       ("rt_filter_accum_device", lambda o, p: L.rt_filter_accum_device(acc._a, o, p, None, None))):
        for field, value in (("levels", 9), ("sigma_l", 0.0), ("sigma_z", float("nan")), ("normal_squarings", -1),
                             ("flags", 4)):
            o = R.filter_options()
            setattr(o, field, value)
            assert call(C.byref(o), out.ctypes.data) < 0
            err = R.last_error()
            assert err.startswith(name + ":") and field in err, err
        assert call(None, None) < 0
        assert "null output" in R.last_error() and R.last_error().startswith(name + ":")
    with pytest.raises(R.RenderError, match="no samples held"):
        acc.filtered()
    frame, _ = acc.add(4)
    rec = check_accumulator(world, acc, 4, frame, R.ACCEL_BRUTE, "brute accumulator")
    assert rec.tobytes() == world.first_hit(w, h, accel=R.ACCEL_BVH).tobytes()
    host = acc.filtered()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_out = torch.zeros(h, w, 3, dtype=torch.float32, device="cuda")
        d_px = torch.zeros(h, w, 4, dtype=torch.uint8, device="cuda")
    s.synchronize()
    acc.filtered_device(d_out.data_ptr(), d_px.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert_same((d_out.cpu().numpy(), d_px.cpu().numpy()), host, "rt_filter_accum_device")
    acc.filtered_device(0, d_px.data_ptr(), 0, levels=0)  # (the library's stream)
    acc.add(1)                                            # (a pass after it, ordered by the library)
    torch.cuda.synchronize()
    acc.close()


# ---- 5. adaptive accumulator ---------------------------------------------------------------

def test_adaptive_accumulator():
    w, h = 96, 64
    world = R.World(scene_text("three_spheres.txt"))
    acc = world.accumulator(w, h, 32)
    acc.set_adaptive(0.08, 0.05, 4)
    for _ in range(3):
        frame, _ = acc.add(4)
    counts = acc.counts()
    assert 0 < acc.active < w * h
    assert (counts < acc.samples).any() and (counts == acc.samples).any()  # stopped pixels and active ones
    check_accumulator(world, acc, counts, frame, R.ACCEL_AUTO, "adaptive")
    acc.close()


# ---- 6. state ------------------------------------------------------------------------------

def test_state_camera_moves_edits_and_a_freed_world():
    w, h = 48, 32
    world = R.World(scene_text("rtow.txt"))
    acc = world.accumulator(w, h, 8)
    frame, _ = acc.add(2)
    rec0 = check_accumulator(world, acc, 2, frame, R.ACCEL_AUTO, "first camera")
    world.look_at((3.0, 2.0, 4.0), (0.0, 0.5, 0.0), vfov=0.9, aspect=w / h)
    with pytest.raises(R.RenderError, match="no samples held"):
        acc.filtered()
    with pytest.raises(R.RenderError, match="rt_filter_accum"):
        acc.filtered(levels=0)
    frame, _ = acc.add(2)
    rec1 = check_accumulator(world, acc, 2, frame, R.ACCEL_AUTO, "moved camera")
    assert rec1.tobytes() != rec0.tobytes()
    # an edit: the samples and the records start over (the scene is uploaded again)
    world.set_material(0, 1, (0.9, 0.2, 0.1), 0.0)
    with pytest.raises(R.RenderError, match="no samples held"):
        acc.filtered()
    frame, _ = acc.add(3)
    check_accumulator(world, acc, 3, frame, R.ACCEL_AUTO, "edited scene")
    acc.reset()
    with pytest.raises(R.RenderError, match="no samples held"):
        acc.filtered()
    frame, _ = acc.add(1)
    check_accumulator(world, acc, 1, frame, R.ACCEL_AUTO, "after reset")
    world.close()
    with pytest.raises(R.RenderError, match="world was freed"):
        acc.filtered()
    acc.close()


# ---- 7. quality ----------------------------------------------------------------------------

def test_quality_on_three_spheres():
    """Measured on the GPU: filtered / unfiltered MSE = 0.156 (the restatement alone gave 0.156)."""
    w, h = 96, 64
    src = scene_text("three_spheres.txt")
    world = R.World(src)
    acc = world.accumulator(w, h, 4)
    acc.add(4)
    noisy = FR.means(acc.sums(), 4)
    filtered, _ = acc.filtered()
    ref_acc = world.accumulator(w, h, 1024, seed=99)
    ref_acc.add(1024)
    ref = FR.means(ref_acc.sums(), 1024).astype(np.float64)
    mse_noisy = float(np.mean((noisy.astype(np.float64) - ref) ** 2))
    mse_filtered = float(np.mean((filtered.astype(np.float64) - ref) ** 2))
    print(f"filter quality: unfiltered MSE {mse_noisy:.4g}, filtered MSE {mse_filtered:.4g}, "
          f"ratio {mse_filtered / mse_noisy:.4f}")
    assert mse_filtered < 0.5 * mse_noisy, (mse_filtered, mse_noisy)
    acc.close()
    ref_acc.close()


# ---- 8. full size --------------------------------------------------------------------------

def test_full_size_frame():
    w, h = 1920, 1080
    world = R.World(scene_text("rtow.txt"))
    acc = world.accumulator(w, h, 4)
    frame, _ = acc.add(4)
    rgb5, px5 = acc.filtered(levels=5)
    rgb0, px0 = acc.filtered(levels=0)
    assert np.isfinite(rgb5).all()
    assert px0.tobytes() == frame.tobytes()
    assert rgb5.tobytes() != rgb0.tobytes() and px5.tobytes() != px0.tobytes()
    assert (px5[..., 3] == 255).all()
    acc.close()
