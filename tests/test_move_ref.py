"""CPU tests of the moved-sphere restatement (move_ref.py): with
equal sphere tables it is clamp_ref's resolve on bits, and on a synthetic view in
which one primitive moved together with its history the mapping is what lets
that primitive's pixels take history: neither vacuous nor total.  And the inputs of
tests/test_gpu_move_run.py (move_run_cases.py), by the restatement alone: the seam
takes history through the right table entry and through no other, the index edges
and the special values of the mapping do what their case says they do, and a
restatement with one mistake in it (a forgotten stride, an inverted k, a float
compare of the tables, values flushed to zero) gives other bits on them."""
import numpy as np
import pytest

import clamp_ref as CR
import move_ref as MR
import move_run_cases as MV
from test_gpu_history import PAIRS, SIZES, camera, inputs, view

F = np.float32
CLAMP = dict(gamma=1.0, radius=1)
TABLE = np.array([[0.0, 0.0, -5.0, 1.0], [1.5, 0.5, -5.0, 0.75], [-2.0, 1.0, -5.0, 2.0]], F)


def bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("w,h", SIZES)
def test_equal_tables_are_the_clamp_restatement(w, h, pair):
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = inputs(w, h, 7)
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    want, wbox = CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=CLAMP)
    for tab in (TABLE, None, TABLE[:1]):
        got, box = MR.resolve(rgb, n, rec, tab, tab, pcam, prgbl, prec, clamp=CLAMP)
        assert (bits(got) == bits(want)).all() and (bits(box) == bits(wbox)).all()
        assert MR.moved_positions(rec, tab, tab).tobytes() == rec["position"].tobytes()


def test_the_three_steps():
    """One record by hand: k = r0 / r1, e = P - c1, P' = c0 + e * k, each rounded once."""
    rec = np.zeros((1, 3), view(camera(), 1, 1).dtype)
    rec["prim"] = (2, 4, 0)
    rec["position"] = [(1.1, 0.7, -4.3), (1.0, 2.0, 3.0), (9.0, 9.0, 9.0)]
    prev = TABLE.copy()
    now = TABLE.copy()
    now[1] = (1.7, 0.4, -4.9, 0.3)
    got = MR.moved_positions(rec, prev, now)
    k = F(0.75) / F(0.3)
    for a in range(3):
        e = rec["position"][0, 0, a] - now[1, a]
        assert got[0, 0, a] == prev[1, a] + F(e * k)
    # a prim above the table (a triangle's) and the sky are untouched
    assert got[0, 1].tobytes() == rec["position"][0, 1].tobytes()
    assert got[0, 2].tobytes() == rec["position"][0, 2].tobytes()
    # r1 = 0: k is infinite, P' is not finite and no history is taken
    now[1, 3] = 0.0
    assert not np.isfinite(MR.moved_positions(rec, prev, now)[0, 0]).all()


# Measured here (the print below): with the mapping 0.958 of prim 2's 912 pixels take
# history, without it 0.000.  MIDPOINT is the midpoint between the two.
MIDPOINT = 0.479


def test_a_moved_primitive_takes_history_through_the_mapping():
    w, h = 70, 50
    cam, ccam = PAIRS["translated"]
    prec = view(cam, w, h)
    rgb, n, prgbl = inputs(w, h, 7)
    # prim 2 moved by `off` together with what it shows, and the camera moved too
    off = np.array([0.0, 0.0, -0.5], F)
    rec = view(ccam, w, h)
    moved = rec["prim"] == 2
    rec["position"][moved] = rec["position"][moved] + off
    prev = TABLE.copy()
    now = TABLE.copy()
    now[1, :3] = prev[1, :3] + off
    with_map, _ = MR.resolve(rgb, n, rec, prev, now, cam, prgbl, prec, clamp=CLAMP)
    without, _ = CR.resolve(rgb, n, rec, cam, prgbl, prec, clamp=CLAMP)
    nf = n.astype(F)
    a = float((with_map[..., 3] > nf)[moved].mean())
    b = float((without[..., 3] > nf)[moved].mean())
    print(f"moved prim: {int(moved.sum())} pixels, share taking history with the mapping {a:.3f}, without {b:.3f}")
    assert moved.sum() > 500
    assert a > MIDPOINT > b
    # the other prims are untouched by the table
    assert (bits(with_map[~moved]) == bits(without[~moved])).all()


# ---- the cases of tests/test_gpu_move_run.py: neither vacuous nor total, by the restatement alone ----

def run(c, s0, s1, rec=None, clamp=CLAMP, positions=None):
    """The restatement over a case of move_run_cases (positions: a mutant of moved_positions)."""
    rec = c["rec"] if rec is None else rec
    if positions is None:
        return MR.resolve(c["rgb"], c["n"], rec, s0, s1, c["pcam"], c["prgbl"], c["prec"], clamp=clamp)
    mapped = rec.copy()
    mapped["position"] = positions(rec, s0, s1)
    return CR.resolve(c["rgb"], c["n"], mapped, c["pcam"], c["prgbl"], c["prec"], clamp=clamp)


def share(c, out, rec=None):
    rec = c["rec"] if rec is None else rec
    return float(MV.took(out, c["n"])[rec["prim"] != 0].mean())


def mutant(kind):
    """moved_positions as a kernel with one mistake would compute them."""
    def positions(rec, s0, s1):
        s0, s1 = MR.table(s0), MR.table(s1)
        pos = rec["position"].astype(F)
        nsph = len(s1)
        prim = rec["prim"].astype(np.int64)
        on = (prim >= 1) & (prim <= nsph)
        i = np.where(on, prim - 1, 0)
        g0, g1 = s0[i], s1[i]
        if kind == "no stride":
            # spheres[sph] of a table with two float4 per sphere, the second one NaN
            padded = np.full((2 * nsph, 4), np.nan, F)
            padded[0::2] = s1
            g1 = padded[i]
        if kind == "float compare":
            differ = on & (g0 != g1).any(axis=-1)
        else:
            differ = on & (g0.view(np.uint32) != g1.view(np.uint32)).any(axis=-1)
        with np.errstate(all="ignore"):
            k = g1[..., 3] / g0[..., 3] if kind == "k inverted" else g0[..., 3] / g1[..., 3]
            e = pos - g1[..., :3]
            ek = e * k[..., None]
            if kind == "flush":
                tiny = np.finfo(F).tiny
                k = np.where(np.abs(k) < tiny, F(0), k)
                ek = e * k[..., None]
                ek = np.where(np.abs(ek) < tiny, F(0), ek)
            q = g0[..., :3] + ek
        return np.where(differ[..., None], q, pos)
    return positions


# Measured here (the print below), over all the parameters: with the right tables the
# share of the hit pixels that take history is 0.922 .. 1.000 (1.000 in every "mod" case
# and under the identity pair), with both tables rolled by one entry at most 0.028, with
# the tables swapped at most 0.167, with no mapping at most 0.278 (both at 9 x 9, 54 hit
# pixels).  SEAM_MIDPOINT is the midpoint between 0.922 and 0.278.
SEAM_MIDPOINT = 0.600
SEAMS = [("mod", "identity"), ("strips", "identity"), ("strips", "translated"), ("strips", "rotated")]


@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("w,h", [(9, 9), (24, 24), (70, 50)])
@pytest.mark.parametrize("layout,pair", SEAMS)
def test_seam_takes_history_through_the_right_entry_only(layout, pair, w, h, S):
    c = MV.seam(w, h, S, pair, layout)
    right, _ = run(c, c["s0"], c["s1"])
    shares = dict(right=share(c, right),
                  rolled=share(c, run(c, *MV.rolled(c))[0]),
                  swapped=share(c, run(c, c["s1"], c["s0"])[0]),
                  unmapped=share(c, CR.resolve(c["rgb"], c["n"], c["rec"], c["pcam"], c["prgbl"], c["prec"],
                                               clamp=CLAMP)[0]))
    print(f"seam {layout} {pair} {w}x{h} S={S}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares["right"] > SEAM_MIDPOINT
    assert max(shares["rolled"], shares["swapped"], shares["unmapped"]) < SEAM_MIDPOINT
    # the mistakes the construction is there to show change the result on bits
    for kind in ("no stride", "k inverted"):
        wrong, _ = run(c, c["s0"], c["s1"], positions=mutant(kind))
        assert share(c, wrong) < SEAM_MIDPOINT, kind
    # ... and the mutant-maker with no mistake is the restatement
    same, _ = run(c, c["s0"], c["s1"], positions=mutant(None))
    assert (bits(same) == bits(right)).all()
    # the plane test with the unmapped P: the projection finds the pixel, the taps fail
    if pair == "translated":
        mapped = c["rec"].copy()
        mapped["position"] = MR.moved_positions(c["rec"], c["s0"], c["s1"])
        from history_ref import project
        front, fx, fy = project(c["pcam"], mapped["position"], w, h)
        hit = c["rec"]["prim"] != 0
        off_plane = np.abs(c["rec"]["position"][..., 2] - F(-5.0)) > F(0.02) * c["rec"]["t"] + F(0.01)
        assert front[hit].all() and off_plane[hit].mean() > SEAM_MIDPOINT


@pytest.mark.parametrize("S", [37, 300])
def test_seam_with_an_identical_prefix(S):
    w, h = 70, 50
    c = MV.seam(w, h, S, "identity", "mod")
    s0, s1, rec, still = MV.half_identical(c)
    got, box = run(c, s0, s1, rec)
    want, wbox = CR.resolve(c["rgb"], c["n"], rec, c["pcam"], c["prgbl"], c["prec"], clamp=CLAMP)
    moving = (rec["prim"] != 0) & ~still
    assert still.sum() > 500 and moving.sum() > 500
    assert (bits(got[still]) == bits(want[still])).all() and (bits(box) == bits(wbox)).all()
    took, plain = MV.took(got, c["n"]), MV.took(want, c["n"])
    assert took[still].all() and took[moving].mean() > SEAM_MIDPOINT > plain[moving].mean()


@pytest.mark.parametrize("ns", [0, 1, 5])
def test_index_edges_take_history_where_the_contract_says(ns):
    """Every prim but the sky's takes history: spheres through the mapping, a triangle's
    id (ns + 1) and 0xFFFFFFFF with the position as it is.  A lane that takes prim
    ns + 1 for a sphere maps it through whatever lies behind the table."""
    w, h = 70, 50
    c = MV.index_edges(w, h, ns)
    got, _ = run(c, c["s0"], c["s1"])
    took = MV.took(got, c["n"])
    prim = c["rec"]["prim"]
    assert set(np.unique(prim)) == {0, 1, max(ns, 1), ns + 1, 0xFFFFFFFF}
    assert took[prim != 0].all() and not took[prim == 0].any()
    if ns:
        # one more entry in both tables (ns + 1 becomes a sphere that moved): those pixels lose their history
        g0 = np.concatenate([c["s0"], np.full((1, 4), np.nan, F)])
        g1 = np.concatenate([c["s1"], np.zeros((1, 4), F)])
        wrong, _ = run(c, g0, g1)
        assert not MV.took(wrong, c["n"])[prim == ns + 1].any()
    if ns > 1:
        rolled, _ = run(c, *MV.rolled(c))
        assert MV.took(rolled, c["n"])[(prim >= 1) & (prim <= ns)].mean() < SEAM_MIDPOINT
    # no prev: the means, len = n
    out, _ = MR.resolve(c["rgb"], c["n"], c["rec"], c["s0"], c["s1"], clamp=CLAMP)
    assert out[..., :3].tobytes() == c["rgb"].tobytes() and (out[..., 3] == c["n"].astype(F)).all()


# Measured here (the print below): 1400 of the 3500 pixels take history; the result holds 11
# NaN and 2 infinities; of the 75 pixels of the sphere whose centres differ in the sign of
# zero, 15 have a P' that differs from P on bits.
@pytest.mark.parametrize("gamma,radius", [(0.0, 1), (1.5, 3), (3.4028234663852886e38, 1)])
def test_special_values_of_the_mapping(gamma, radius):
    c, names = MV.special_move()
    clamp = dict(gamma=gamma, radius=radius)
    got, box = run(c, c["s0"], c["s1"], clamp=clamp)
    took = MV.took(got, c["n"])
    prim, pos = c["rec"]["prim"], c["rec"]["position"]
    print(f"special g{gamma} r{radius}: NaN {int(np.isnan(got).sum())}, inf {int(np.isinf(got).sum())}, "
          f"took {int(took.sum())} of {took.size}")
    assert np.isnan(got).any() and np.isinf(got).any() and took.sum() > 1000  # (the case cannot go blank)
    assert (c["n"] == 0).any() and (c["prgbl"][..., 3] == 0).any()
    q = MR.moved_positions(c["rec"], c["s0"], c["s1"])
    on_sphere = (prim >= 1) & (prim <= len(c["s0"]))
    with np.errstate(all="ignore"):
        k = (c["s0"][:, 3] / c["s1"][:, 3])[np.where(on_sphere, prim.astype(np.int64) - 1, 0)]
    # a non-finite k or P' takes no history: len = n
    dead = on_sphere & (~np.isfinite(k) | ~np.isfinite(q).all(axis=-1))
    assert dead.sum() > 500 and not took[dead].any()
    for i, name in enumerate(names):
        on = prim == i + 1
        assert name is None or on.sum() > 50, name
    # the sign of zero: differing bits, k = 1, and the ten operations do not give P back
    on = prim == MV.ZERO_SIGN + 1
    moved_bits = (q[on].view(np.uint32) != pos[on].view(np.uint32)).any(axis=-1)
    print(f"special: -0.0 against 0.0: {int(moved_bits.sum())} of {int(on.sum())} pixels have P' != P on bits")
    assert moved_bits.any() and took[on].any()
    wrong, _ = run(c, c["s0"], c["s1"], clamp=clamp, positions=mutant("float compare"))
    assert (bits(wrong[on]) != bits(got[on])).any(), "a float compare of the tables would pass"
    assert (bits(wrong[~on]) == bits(got[~on])).all()
    # subnormal k and subnormal e * k: these pixels take history, and flushed to zero they would not
    flushed, _ = run(c, c["s0"], c["s1"], clamp=clamp, positions=mutant("flush"))
    for i in (MV.TINY_K, MV.TINY_PRODUCT):
        on = prim == i + 1
        tiny = np.abs(q[on]) < np.finfo(F).tiny
        assert tiny.all() and (q[on] != 0).any(axis=-1).all(), names[i]
        assert took[on].mean() > 0.9 and not MV.took(flushed, c["n"])[on].any(), names[i]
