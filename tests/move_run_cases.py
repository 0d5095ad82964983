"""Inputs of rt_move_run's tests (a plain helper module, no tests): synthetic views in
which every sphere moved and neighbouring pixels lie on different spheres, shared by
tests/test_move_ref.py (CPU: the cases are neither vacuous nor total, by the
restatement alone) and tests/test_gpu_move_run.py (the kernel against the
restatement, on bits).  Nothing here comes from the library.

The seam construction.  S spheres with random {c0, r0} in prev's table and
c1 = c0 + offset, r1 = r0 * factor (factor in [0.5, 1.5]) in the present one.  prev's
records are test_gpu_history.view(pcam) with sphere ids for prims; the present
records keep the prims, normals and t of view(ccam) and get the position
    P = c1 + (Pw - c0) / k,  k = f32(r0) / f32(r1)        (f64, rounded to f32)
of the world point Pw the pixel shows, so that the contract's P' = c0 + (P - c1) * k
lands on Pw again, on the prev pixels that show it.  A lane that reads another
sphere's entry, swaps the tables or forgets the mapping lands somewhere else.

Two id layouts:
  "mod"      prim = 1 + (pixel index mod S): every pixel on another sphere than its
             neighbours (the identity pair only: both views share the pixel grid);
  "strips"   strips about three of prev's columns wide, cut every three rows so that
             the whole table is used; the id is a function of the world point, so it
             holds under a moved camera, and the 2 x 2 gather blends several taps.
"""
import numpy as np

from test_gpu_history import PAIRS, inputs, view

F = np.float32
INF = F(np.inf)
NAN = F(np.nan)


def tables(S, seed=21):
    """(prev_spheres, spheres) float32[S, 4]: every sphere moved and resized."""
    rng = np.random.default_rng(seed)
    s0 = np.empty((S, 4), F)
    s0[:, :3] = rng.uniform(-3.0, 3.0, (S, 3))
    s0[:, 3] = rng.uniform(0.5, 2.0, S)
    s1 = np.empty((S, 4), F)
    s1[:, :3] = s0[:, :3] + rng.uniform(-1.0, 1.0, (S, 3)).astype(F)
    s1[:, 3] = s0[:, 3] * rng.uniform(0.5, 1.5, S).astype(F)
    assert (s0.view(np.uint32) != s1.view(np.uint32)).any(axis=1).all()
    return s0, s1


def ids(rec, w, h, S, layout):
    """Sphere ids 1 .. S of a view's hit pixels (0: sky)."""
    hit = rec["prim"] != 0
    if layout == "mod":
        k = np.arange(w * h, dtype=np.int64).reshape(h, w) % S
    else:
        pos = rec["position"].astype(np.float64)
        dx, dy = 3 * 15.0 / max(w - 1, 1), 3 * 10.0 / max(h - 1, 1)  # three columns, three rows at z = -5
        k = (np.floor(pos[..., 0] / dx).astype(np.int64) + 5 * np.floor(pos[..., 1] / dy).astype(np.int64)) % S
    return np.where(hit, 1 + k, 0).astype(np.uint32)


def unmap(pw, prim, s0, s1):
    """P of the present records: the point that the contract maps onto pw."""
    i = np.where(prim > 0, prim.astype(np.int64) - 1, 0)
    g0, g1 = s0[i], s1[i]
    with np.errstate(all="ignore"):
        k = (g0[..., 3] / g1[..., 3]).astype(np.float64)
        p = g1[..., :3].astype(np.float64) + (pw.astype(np.float64) - g0[..., :3]) / k[..., None]
    return np.where((prim > 0)[..., None], p, 0).astype(F)


def seam(w, h, S, pair="identity", layout="mod", seed=21):
    """-> dict(rgb, n, rec, pcam, prgbl, prec, s0, s1, world): world the present records
    before the positions were unmapped (what prev would see of them)."""
    assert layout in ("mod", "strips") and (layout == "strips" or pair == "identity")
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = inputs(w, h, 7)
    prec, world = view(pcam, w, h), view(ccam, w, h)
    prec["prim"] = ids(prec, w, h, S, layout)
    world["prim"] = ids(world, w, h, S, layout)
    s0, s1 = tables(S, seed)
    rec = world.copy()
    rec["position"] = unmap(world["position"], world["prim"], s0, s1)
    return dict(rgb=rgb, n=n, rec=rec, pcam=pcam, prgbl=prgbl, prec=prec, s0=s0, s1=s1, world=world)


def took(rgbl, n):
    """Which pixels took history: len > n."""
    return rgbl[..., 3] > np.asarray(n).astype(F)


def rolled(case):
    """Both tables rolled by one entry: what a lane sees that reads sphere prim, not prim - 1."""
    return np.roll(case["s0"], -1, axis=0), np.roll(case["s1"], -1, axis=0)


def half_identical(case):
    """(prev_spheres, spheres) with the first half of the present table equal to prev's on
    bits, and the records to go with them: those spheres' pixels show the world point itself."""
    s0, s1 = case["s0"], case["s1"].copy()
    half = len(s0) // 2
    s1[:half] = s0[:half]
    rec = case["world"].copy()
    rec["position"] = unmap(rec["position"], rec["prim"], s0, s1)
    still = (rec["prim"] >= 1) & (rec["prim"] <= half)
    assert rec["position"][still].tobytes() == case["world"]["position"][still].tobytes()
    return s0, s1, rec, still


def index_edges(w, h, ns):
    """The identity pair's view in strips whose prims are 1, ns, ns + 1 (a triangle's) and
    0xFFFFFFFF in turn (sky: 0), under tables of ns moved spheres: the sphere prims carry
    unmapped positions, every other prim the world point itself.  ns may be 0."""
    pcam, ccam = PAIRS["identity"]
    rgb, n, prgbl = inputs(w, h, 7)
    prec = view(pcam, w, h)
    values = np.array([1, max(ns, 1), ns + 1, 0xFFFFFFFF], np.int64)
    strip = ids(prec, w, h, 4, "strips").astype(np.int64) - 1
    prec["prim"] = np.where(strip >= 0, values[np.maximum(strip, 0)], 0).astype(np.uint32)
    s0, s1 = tables(ns) if ns else (np.zeros((0, 4), F), np.zeros((0, 4), F))
    world = prec.copy()
    rec = world.copy()
    on = (rec["prim"] >= 1) & (rec["prim"] <= ns)
    if ns:
        rec["position"] = np.where(on[..., None], unmap(world["position"], np.where(on, rec["prim"], 0), s0, s1),
                                   world["position"])
    return dict(rgb=rgb, n=n, rec=rec, pcam=pcam, prgbl=prgbl, prec=prec, s0=s0, s1=s1, world=world)


# ---- the special values of the mapping -------------------------------------------------------

# sphere index -> what its entry is made of; each of the first entries replaces {r0, r1}
RADII = [
    ("r1 = 0", None, 0.0), ("r0 = 0", 0.0, None), ("both 0", 0.0, 0.0),
    ("r1 = inf", None, INF), ("r1 = -inf", None, -INF), ("r0 = inf", INF, None), ("both inf", INF, INF),
    ("r0 < 0", -0.75, None), ("r1 < 0", None, -1.25), ("both < 0", -0.75, -1.25),
    ("k overflows", 3e38, 1e-3),
]
TINY_K, TINY_PRODUCT, ZERO_SIGN = len(RADII), len(RADII) + 1, len(RADII) + 2
CENTRES = len(RADII) + 3  # five entries from here: +-inf, 1e38 and NaN in centres


def special_move(w=70, h=50, S=37):
    """The strips seam at 70 x 50 under the translated pair with special values in some
    spheres' entries, non-finite positions and t on sphere prims, n = 0 and len = 0.
    -> (case, names): names[i] says what sphere i's entry holds (None: the seam's)."""
    c = seam(w, h, S, "translated", "strips")
    s0, s1, rec, world = c["s0"], c["s1"], c["rec"], c["world"]
    names = [None] * S
    for i, (name, r0, r1) in enumerate(RADII):
        names[i] = name
        if r0 is not None:
            s0[i, 3] = r0
        if r1 is not None:
            s1[i, 3] = r1
    # a subnormal k and a subnormal product e * k.  Both centres 0, so P' = e * k alone: a
    # subnormal multiple of the world point, which prev's camera (at the origin) projects
    # where it projects the point itself; t is made large so that the taps' plane test,
    # |z_q - P'_z| = 5 <= sigma_z * t, passes.  Flushed to zero, P' is the origin: no history.
    for i, name, r0, scale in ((TINY_K, "subnormal k", 1e-40, 1.0), (TINY_PRODUCT, "subnormal e * k", 1e-30, 2e-11)):
        names[i] = name
        s0[i] = (0.0, 0.0, 0.0, r0)
        s1[i] = (0.0, 0.0, 0.0, 1.0)
        on = world["prim"] == i + 1
        rec["position"][on] = world["position"][on] * F(scale)
        rec["t"][on] = F(1000.0)
    # centres that differ only in the sign of zero: differing bits, so the ten operations run, with k = 1
    names[ZERO_SIGN] = "-0.0 against 0.0"
    s0[ZERO_SIGN] = (0.0, 1.25, -2.5, 1.0)
    s1[ZERO_SIGN] = (-0.0, 1.25, -2.5, 1.0)
    on = world["prim"] == ZERO_SIGN + 1
    rec["position"][on] = world["position"][on]
    for j, (name, tab, col, v) in enumerate((("c1.x = inf", s1, 0, INF), ("c0.y = -inf", s0, 1, -INF),
                                             ("c0.z = 1e38", s0, 2, 1e38), ("c0.x = NaN", s0, 0, NAN),
                                             ("c1 = 1e38, -1e38, inf", s1, slice(0, 3), (1e38, -1e38, INF)))):
        names[CENTRES + j] = name
        tab[CENTRES + j, col] = v
    assert CENTRES + 5 <= S
    # test_gpu_history.special()'s non-finite positions and t on sphere prims that keep the seam's entries
    rng = np.random.default_rng(31)
    plain = np.argwhere(rec["prim"] > CENTRES + 5)
    pick = [tuple(p) for p in plain[rng.choice(len(plain), 24, replace=False)]]
    for k, p in enumerate(((NAN, F(0), F(-5)), (INF, F(1), F(-5)), (NAN,) * 3, (-INF, INF, INF),
                           (F(1e38), F(1e38), F(-1e38)), (F(1e38), F(0), F(-5)), (F(0), F(0), -INF))):
        rec["position"][pick[k]] = p
    for k, t in enumerate((INF, NAN, F(0))):
        rec["t"][pick[7 + k]] = t
    c["n"][pick[10]] = 0
    c["n"][pick[11]] = 0xFFFFFFFF
    for k, v in enumerate((NAN, INF, -INF, F(1e-40), F(3e38))):
        c["rgb"][pick[12 + k]][k % 3] = v
    pplain = np.argwhere(c["prec"]["prim"] > CENTRES + 5)
    ppick = [tuple(p) for p in pplain[rng.choice(len(pplain), 60, replace=False)]]
    lens = (F(0), F(-0.0), F(-3), NAN, INF, F(1e-40))
    cols = (NAN, INF, -INF, F(1e-40), F(3e38), F(-1.5))
    for k, p in enumerate(ppick[:30]):
        c["prgbl"][p][3] = lens[k % len(lens)]
    for k, p in enumerate(ppick[30:]):
        c["prgbl"][p][k % 3] = cols[k % len(cols)]
    return c, names
