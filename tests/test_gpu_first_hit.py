"""First-hit records, picks and views on the GPU (rt_first_hit_*, DESIGN.md
5.8), bit for bit against a test-side restatement.

The restatement is the contract's four lines in numpy f32: u and v as one
rounded add and one division each, pyref.cast_ray, and pyref.world_hit's two
loops restated with the winner's index kept (over pyref.sphere_hit and
pyref.triangle_intersect).  A few pixels of every restated frame are checked
against the C++ oracle's ro_cast_ray / ro_sphere_hit / ro_triangle_intersect.
Nothing expected comes from the library.  Records are compared as raw bytes.
Restated frames are computed once per (scene, camera, size, offsets) and shared.
"""
import numpy as np
import pytest

import camera_cases as CC
import guard_scenes as G
import oracle as O
import pyref as P
import raytracer_amd as R
import scene_values as V
from conftest import scene_text

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 48, 32
DT = R.FIRST_HIT_DTYPE
ACCELS = (R.ACCEL_BRUTE, R.ACCEL_BVH)
ONE_BELOW = float(np.nextafter(F(1), F(0)))

_MEMO = {}


# ---- the restatement ---------------------------------------------------------------------

def cam_dict(cam12):
    c = [F(x) for x in np.asarray(cam12, F)]
    return {"origin": tuple(c[0:3]), "llc": tuple(c[3:6]), "h": tuple(c[6:9]), "v": tuple(c[9:12])}


def cam_floats(cam):
    return np.array(cam["origin"] + cam["llc"] + cam["h"] + cam["v"], F)


def parsed(src):
    """(camera dict, pyref world) of a scene text; parsed once."""
    key = ("parsed", src)
    if key not in _MEMO:
        _MEMO[key] = P.parse(src)
    return _MEMO[key]


def pixel_ray(cam, width, height, col, row, su, sv):
    """The contract's ray of reference (row, col), row 0 = bottom."""
    u = (F(col) + F(su)) / F(width - 1)
    v = (F(row) + F(sv)) / F(height - 1)
    return P.cast_ray(cam, u, v)


def world_hit_indexed(world, ray, candidates=None):
    """pyref.world_hit (common.rs:237-258) with the winner's index kept:
    (prim, t, normal, position) or None.  candidates (optional list): receives
    (prim, t) of every primitive that alone would be hit in (t_min, +inf)."""
    closest, rec = P.INF, None
    for i, (c, r, _m) in enumerate(world["spheres"]):
        h = P.sphere_hit(c, r, ray, P.T_MIN, closest)
        if h is not None:
            closest = h[0]
            rec = (1 + i, h[0], h[2], h[1])
        if candidates is not None:
            h = P.sphere_hit(c, r, ray, P.T_MIN, P.INF)
            if h is not None:
                candidates.append((1 + i, h[0]))
    ns = len(world["spheres"])
    mclosest, mrec = P.INF, None
    for j, (v0, v1, v2, nrm, _m) in enumerate(world["triangles"]):
        h = P.triangle_intersect(v0, v1, v2, ray, P.T_MIN, closest)
        if h is not None and h[0] < mclosest:
            mclosest = h[0]
            mrec = (1 + ns + j, h[0], nrm, h[1])
        if candidates is not None:
            h = P.triangle_intersect(v0, v1, v2, ray, P.T_MIN, P.INF)
            if h is not None:
                candidates.append((1 + ns + j, h[0]))
    return mrec if mrec is not None else rec


def record_of(hit):
    rec = np.zeros((), DT)
    rec["t"] = np.inf
    if hit is not None:
        rec["prim"], rec["t"], rec["normal"], rec["position"] = hit[0], hit[1], hit[2], hit[3]
    return rec


def oracle_check(world, cam, width, height, col, row, su, sv, rec):
    """The same pixel through the C++ oracle's cast_ray, sphere_hit and
    triangle_intersect (World::hit's loops around them): same record."""
    L = O.lib()
    ray = np.zeros(6, F)
    u = (F(col) + F(su)) / F(width - 1)
    v = (F(row) + F(sv)) / F(height - 1)
    L.ro_cast_ray(O.fptr(cam_floats(cam)), float(u), float(v), O.fptr(ray))
    out = np.zeros(7, F)
    closest, best = F(np.inf), None
    for i, (c, r, _m) in enumerate(world["spheres"]):
        if L.ro_sphere_hit(O.fptr(ray), O.fptr(O.f32arr(c)), float(r), float(P.T_MIN), float(closest), O.fptr(out)):
            closest = out[0]
            best = (1 + i, out[0], out[4:7].copy(), out[1:4].copy())
    ns = len(world["spheres"])
    mclosest, mbest = F(np.inf), None
    for j, (v0, v1, v2, nrm, _m) in enumerate(world["triangles"]):
        if L.ro_triangle_intersect(O.fptr(ray), O.fptr(O.f32arr(v0 + v1 + v2)), float(P.T_MIN), float(closest),
                                   O.fptr(out)) \
                and out[0] < mclosest:
            mclosest = out[0]
            mbest = (1 + ns + j, out[0], np.array(nrm, F), out[1:4].copy())
    want = record_of(mbest if mbest is not None else best)
    assert want.tobytes() == rec.tobytes(), ("restatement vs oracle", col, row, want, rec)


def restate(src, width, height, cam12=None, su=0.5, sv=0.5):
    """The restated records of the whole frame, DT[height, width], top row first."""
    key = ("frame", src, width, height, None if cam12 is None else np.asarray(cam12, F).tobytes(),
           F(su).tobytes(), F(sv).tobytes())
    if key in _MEMO:
        return _MEMO[key]
    cam, world = parsed(src)
    if cam12 is not None:
        cam = cam_dict(cam12)
    out = np.zeros((height, width), DT)
    for row in range(height):
        for col in range(width):
            out[height - 1 - row, col] = record_of(
                world_hit_indexed(world, pixel_ray(cam, width, height, col, row, su, sv)))
    # the oracle's arithmetic on a few pixels: corners, centre, a seeded handful
    rng = np.random.default_rng(width * 1000 + height)
    pts = {(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, height // 2)}
    pts |= {(int(rng.integers(width)), int(rng.integers(height))) for _ in range(6)}
    for col, row in sorted(pts):
        oracle_check(world, cam, width, height, col, row, su, sv, out[height - 1 - row, col])
    out.setflags(write=False)
    _MEMO[key] = out
    return out


def world_of(src):
    key = ("world", src)
    if key not in _MEMO:
        _MEMO[key] = R.World(src)
    return _MEMO[key]


def assert_records(got, want, what):
    assert got.dtype == DT and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(np.frombuffer(got.tobytes(), np.uint8).reshape(got.shape + (32,)) !=
                          np.frombuffer(want.tobytes(), np.uint8).reshape(want.shape + (32,)))
        y, x = int(bad[0][0]), int(bad[0][1])
        raise AssertionError(f"{what}: {len(set(map(tuple, bad[:, :2])))} records differ, first at top row {y} "
                             f"col {x}: got {got[y, x]} want {want[y, x]}")


def check_both_accels(src, width, height, what, look=None, su=0.5, sv=0.5):
    """Records under BRUTE and BVH equal the restatement (so each other)."""
    world = R.World(src)  # (a world of its own: its camera may be swapped)
    cam12 = None
    if look is not None:
        table, name = look
        CC.apply(world, table, name)
        cam12 = CC.camera(table, name)
        assert world.camera().tobytes() == cam12.tobytes(), (what, "camera")
    want = restate(src, width, height, cam12, su, sv)
    for accel in ACCELS:
        got = world.first_hit(width, height, su=su, sv=sv, accel=accel)
        assert_records(got, want, f"{what} accel {accel}")
    return want


RTOW = scene_text("rtow.txt")
THREE = scene_text("three_spheres.txt")


def few_triangles():
    """The 60-ball field plus 5 triangles: below the triangle tree's threshold."""
    tris = [V.triangle((-1.2, -0.8, -2.0), (-0.2, -0.8, -2.0), (-0.7, 0.1, -2.2), "ED"),
            V.triangle((0.3, -0.2, -1.2), (0.9, -0.3, -1.4), (0.5, 0.5, -1.3), "EM"),
            V.triangle((-3.0, -1.5, -6.0), (3.0, -1.5, -6.0), (0.0, 2.5, -6.5), "ED"),
            V.triangle((0.1, 0.6, -1.0), (0.7, 0.7, -1.1), (0.3, 0.95, -0.9), "EM"),
            V.triangle((-0.9, 0.4, -1.1), (-0.4, 0.3, -1.0), (-0.6, 0.8, -1.2), "ED")]
    return V.splice(V.field(), [V.DIFF, V.MIRROR], (), tris)


# ---- 1. brute force and tree, spheres ------------------------------------------------------

def test_spheres_brute_and_tree():
    assert len(parsed(THREE)[1]["spheres"]) < 16 and len(parsed(RTOW)[1]["spheres"]) == 486
    want = check_both_accels(THREE, W, H, "three_spheres")
    assert len(np.unique(want["prim"])) >= 4
    want = check_both_accels(RTOW, W, H, "rtow")
    assert (want["prim"] == 1).any()  # the ground sphere, kept out of the tree
    assert len(np.unique(want["prim"])) > 20
    want = check_both_accels(RTOW, W, H, "rtow book", look=(CC.RTOW, "book"))
    assert len(np.unique(want["prim"])) > 20


# ---- 2. triangles ------------------------------------------------------------------------

@pytest.mark.parametrize("look", [None, "side", "wide"])
def test_triangles_brute_and_tree(look):
    lk = None if look is None else (CC.SOUP, look)
    soup = V.soup(40)
    _, pw = parsed(soup)
    assert len(pw["triangles"]) == 40 and len(pw["spheres"]) == 40
    want = check_both_accels(soup, W, H, f"soup {look}", look=lk)
    ns = 40
    assert (want["prim"] > ns).any() and ((want["prim"] > 0) & (want["prim"] <= ns)).any()
    few = few_triangles()
    assert 0 < len(parsed(few)[1]["triangles"]) < 16
    want = check_both_accels(few, W, H, f"few triangles {look}", look=lk)
    if look is None:
        assert (want["prim"] > 60).any()


@pytest.mark.parametrize("look", [None, "high"])
def test_triangle_lists_and_tree_walk_agree(look, monkeypatch):
    """A scene with a triangle tree takes the frames' primary strip lists, made
    current for the camera of the call; RT_AMD_PRIMARY_LISTS=0 (read at every
    call) leaves the static tree's walk.  Both are the restatement."""
    src = V.soup(40)
    world = R.World(src)
    cam12 = None
    if look is not None:
        CC.apply(world, CC.SOUP, look)
        cam12 = CC.camera(CC.SOUP, look)
    want = restate(src, W, H, cam12)
    assert (want["prim"] > 40).any()
    assert_records(world.first_hit(W, H), want, f"lists {look}")
    monkeypatch.setenv("RT_AMD_PRIMARY_LISTS", "0")
    assert_records(world.first_hit(W, H), want, f"walk {look}")
    monkeypatch.delenv("RT_AMD_PRIMARY_LISTS")
    assert_records(world.first_hit(W, H, rect=(5, 3, 31, 17)), np.ascontiguousarray(want[3:20, 5:36]),
                   f"lists, rectangle {look}")


# ---- 3. ties ------------------------------------------------------------------------------

def axis_candidates(src):
    """Candidates on the ray of pixel (col 23, reference row 15) at 48 x 32: the axis ray."""
    cam, world = parsed(src)
    ray = pixel_ray(cam, W, H, 23, 15, 0.5, 0.5)
    assert [float(x) for x in ray[1]] == [0.0, 0.0, -1.0]
    cands = []
    hit = world_hit_indexed(world, ray, cands)
    return hit, cands


def test_tie_triangle_beats_sphere_and_lower_triangle_wins():
    case = V.case("tri_tie", 40)
    cam, world = parsed(case.src)
    ns = len(world["spheres"])
    assert ns == 41
    # on the restatement alone: sphere 40 and triangle 42 share t on the axis ray
    hit, cands = axis_candidates(case.src)
    ts = dict(cands)
    assert (1 + 40) in ts and (1 + ns + 42) in ts
    assert ts[1 + 40] == ts[1 + ns + 42] == F(1.5)
    assert hit[0] == 1 + ns + 42
    want = check_both_accels(case.src, W, H, "tri_tie")
    assert want[H - 1 - 15, 23]["prim"] == 1 + 41 + 42
    # the duplicated triangle (40 and 41): somewhere both are candidates at equal t
    seen = 0
    for row in range(H):
        for col in range(W):
            if want[H - 1 - row, col]["prim"] != 1 + ns + 40:
                continue
            cands = []
            world_hit_indexed(world, pixel_ray(cam, W, H, col, row, 0.5, 0.5), cands)
            ts = dict(cands)
            assert ts[1 + ns + 40] == ts[1 + ns + 41]
            seen += 1
    assert seen > 0
    assert not (want["prim"] == 1 + ns + 41).any()


def test_tie_lowest_sphere_index_wins():
    case = V.case("coincident")
    hit, cands = axis_candidates(case.src)
    ts = dict(cands)
    # spheres 60, 61, 62 (prims 61, 62, 63) share t on the axis ray
    assert ts[61] == ts[62] == ts[63] == F(1.1683373)
    assert min(t for _p, t in cands) == ts[61]
    assert hit[0] == 61
    want = check_both_accels(case.src, W, H, "coincident")
    assert want[H - 1 - 15, 23]["prim"] == 61
    assert not np.isin(want["prim"], (62, 63)).any()


# ---- 4. unusual values ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hollow", "zero_r", "nonfinite", "cam_inside", "big_mix", "tri_degenerate"])
def test_unusual_values(name):
    case = V.case(name, 40)
    w, h = V.FRAME[0], V.FRAME[1]
    want = check_both_accels(case.src, w, h, name)
    base = restate(case.base, w, h)
    assert want.tobytes() != base.tobytes(), f"{name}: the edge primitives are not visible"


@pytest.mark.parametrize("name", ["scene_a", "scene_b"])
def test_guard_scenes(name):
    src = getattr(G, name)()
    want = check_both_accels(src, 64, 8, name)
    last = len(parsed(src)[1]["spheres"])
    assert (want["prim"] == last).any()  # the edge sphere takes part of the view


# ---- 5. degenerate frames -------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (1, 7), (7, 1)])
def test_degenerate_frames_hit_nothing(size):
    w, h = size
    want = restate(RTOW, w, h)
    assert (want["prim"] == 0).all() and np.isposinf(want["t"]).all()
    assert not want["normal"].any() and not want["position"].any()
    world = world_of(RTOW)
    for accel in ACCELS:
        assert_records(world.first_hit(w, h, accel=accel), want, f"{w}x{h} accel {accel}")


def test_frame_that_is_no_multiple_of_a_wave():
    check_both_accels(RTOW, 37, 23, "rtow 37x23")


# ---- 6. offsets -----------------------------------------------------------------------------

@pytest.mark.parametrize("off", [(0.0, 0.0), (ONE_BELOW, ONE_BELOW)])
def test_offsets(off):
    want = check_both_accels(RTOW, W, H, f"rtow offsets {off}", su=off[0], sv=off[1])
    assert want.tobytes() != restate(RTOW, W, H).tobytes()


# ---- 7. rectangle, pick, device buffer ------------------------------------------------------

def test_rectangles_are_slices_of_the_full_call():
    world = world_of(RTOW)
    full = world.first_hit(W, H)
    assert_records(full, restate(RTOW, W, H), "rtow")
    for rect in ((0, 0, 1, 1), (7, 11, 5, 3), (0, 20, W, 1), (W - 1, 0, 1, H), (0, 0, W, H), (40, 24, 8, 8)):
        x0, y0, w, h = rect
        for accel in ACCELS:
            got = world.first_hit(W, H, rect=rect, accel=accel)
            assert got.shape == (h, w)
            assert_records(got, np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w]), f"rect {rect} accel {accel}")


def test_pick_equals_the_full_call():
    world = world_of(RTOW)
    full = restate(RTOW, W, H)
    rng = np.random.default_rng(20)
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (23, 16)]
    pts += [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(20)]
    for col, row in pts:
        rec = world.pick(W, H, col, row)
        assert rec.tobytes() == full[row, col].tobytes(), (col, row, rec, full[row, col])
    # the rectangle in the options is ignored by a pick
    L = R.lib()
    o = world._first_hit_options(0.5, 0.5, (3, 3, 2, 2), R.ACCEL_AUTO, -1)
    one = R.RtFirstHit()
    import ctypes as C
    assert L.rt_first_hit_pick(world.handle, W, H, 30, 9, C.byref(o), C.byref(one)) == 0
    assert bytes(one) == full[9, 30].tobytes()


def test_device_records_equal_host_records():
    import torch

    world = world_of(RTOW)
    want = restate(RTOW, W, H)
    buf = torch.zeros(W * H * 32, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    world.first_hit_device(W, H, buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    got = np.frombuffer(buf.cpu().numpy().tobytes(), DT).reshape(H, W)
    assert_records(got, want, "first_hit_device")
    # a rectangle into a buffer of its own size
    rect = (7, 11, 5, 3)
    small = torch.zeros(5 * 3 * 32, dtype=torch.uint8, device="cuda")
    world.first_hit_device(W, H, small.data_ptr(), stream.cuda_stream, rect=rect)
    stream.synchronize()
    got = np.frombuffer(small.cpu().numpy().tobytes(), DT).reshape(3, 5)
    assert_records(got, np.ascontiguousarray(want[11:14, 7:12]), "first_hit_device rect")


# ---- 8. camera and edits --------------------------------------------------------------------

@pytest.mark.parametrize("which", ["rtow", "soup"])
def test_records_follow_the_camera_as_it_is_now(which):
    src, table, name = (RTOW, CC.RTOW, "book") if which == "rtow" else (V.soup(40), CC.SOUP, "side")
    world = R.World(src)
    world.render(W, H, 1, 4)  # a frame with the file camera: lists and camera-origin records are built
    assert_records(world.first_hit(W, H), restate(src, W, H), f"{which} file camera")
    world.render(W, H, 1, 4)
    CC.apply(world, table, name)
    cam12 = CC.camera(table, name)
    want = restate(src, W, H, cam12)
    assert want.tobytes() != restate(src, W, H).tobytes()
    for accel in ACCELS:
        assert_records(world.first_hit(W, H, accel=accel), want, f"{which} after look_at, accel {accel}")
    # ... and a frame in between does not change them either
    world.render(W, H, 1, 4)
    assert_records(world.first_hit(W, H), want, f"{which} after look_at and a frame")


def test_material_edit_changes_albedo_only_on_that_sphere():
    world = R.World(RTOW)
    want = restate(RTOW, W, H)
    prims, counts = np.unique(want["prim"][want["prim"] > 1], return_counts=True)
    prim = int(prims[np.argmax(counts)])  # the most visible small sphere
    before = world.first_hit_view(W, H, R.VIEW_ALBEDO)
    world.set_material(prim - 1, 0, (0.125, 0.625, 0.875))
    assert_records(world.first_hit(W, H), want, "records after set_material")
    after = world.first_hit_view(W, H, R.VIEW_ALBEDO)
    mask = want["prim"] == prim
    assert mask.any()
    assert np.array_equal(after[~mask], before[~mask])
    assert (after[mask] == np.array([31, 159, 223, 255], np.uint8)).all()  # c * 255.999 as u8
    assert not np.array_equal(after[mask], before[mask])


# ---- 9. views --------------------------------------------------------------------------------

def as_u8(x):
    """Rust's `f32 as u8` on an array: saturating, NaN -> 0, truncating."""
    x = np.asarray(x, F)
    out = np.zeros(x.shape, np.uint8)
    ok = x > 0
    out[ok & (x >= 255)] = 255
    mid = ok & (x < 255)
    out[mid] = x[mid].astype(np.int64).astype(np.uint8)
    return out


def restate_view(rec, view, world):
    """The view's formulas in numpy f32, one rounded operation per step."""
    h, w = rec.shape
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 3] = 255
    hit = rec["prim"] != 0
    k = F(255.999)
    with np.errstate(all="ignore"):
        if view == R.VIEW_NORMAL:
            rgb = as_u8(((rec["normal"] * F(0.5)) + F(0.5)) * k)
        elif view == R.VIEW_DEPTH:
            d = as_u8((F(1.0) / (F(1.0) + rec["t"])) * k)
            rgb = np.stack([d, d, d], axis=-1)
        elif view == R.VIEW_ALBEDO:
            sph, tri = world.spheres(), world.triangles()
            mats = np.concatenate([np.zeros((1, 6), F), sph[:, 4:10], tri[:, 12:18]])  # row = prim
            m = mats[rec["prim"]]
            col = np.where((m[..., 0] == 2)[..., None], F(1.0), m[..., 1:4]).astype(F)
            rgb = as_u8(col * k)
        else:
            hsh = (rec["prim"].astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
            rgb = np.stack([(hsh >> np.uint64(24)), (hsh >> np.uint64(16)) & np.uint64(255),
                            (hsh >> np.uint64(8)) & np.uint64(255)], axis=-1).astype(np.uint8)
    out[..., :3] = np.where(hit[..., None], rgb, 0)
    return out


@pytest.mark.parametrize("which", ["rtow", "soup"])
@pytest.mark.parametrize("view", [R.VIEW_NORMAL, R.VIEW_DEPTH, R.VIEW_ALBEDO, R.VIEW_PRIM])
def test_views(which, view):
    import torch

    src = RTOW if which == "rtow" else V.soup(40)
    world = world_of(src)
    want = restate_view(restate(src, W, H), view, world)
    assert want[..., :3].any() and len(np.unique(want.reshape(-1, 4), axis=0)) > 3  # (the soup has 4 materials)
    for accel in ACCELS:
        got = world.first_hit_view(W, H, view, accel=accel)
        assert got.tobytes() == want.tobytes(), (which, view, accel, np.argwhere(got != want)[:4])
    buf = torch.zeros(W * H * 4, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    world.first_hit_view_device(W, H, view, buf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert buf.cpu().numpy().tobytes() == want.tobytes(), (which, view, "device")
    rect = (7, 11, 5, 3)
    got = world.first_hit_view(W, H, view, rect=rect)
    assert got.tobytes() == np.ascontiguousarray(want[11:14, 7:12]).tobytes(), (which, view, "rect")


# ---- 10. full size, no restatement -----------------------------------------------------------

def test_full_size_brute_equals_tree():
    world = world_of(RTOW)
    a = world.first_hit(1920, 1080, accel=R.ACCEL_BRUTE)
    b = world.first_hit(1920, 1080, accel=R.ACCEL_BVH)
    assert a.tobytes() == b.tobytes()
    prims = np.unique(a["prim"])
    assert len(prims[prims > 0]) > 100
    # the pick of a pixel of the big frame is that frame's record
    rec = world.pick(1920, 1080, 1000, 700)
    assert rec.tobytes() == a[700, 1000].tobytes()
