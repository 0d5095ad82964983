"""The moved-sphere resolve kernel on host arrays with two sphere tables
(rt_move_run), bit for bit against the numpy restatements of its
contract (move_ref.py; clamp_ref.py where the tables are equal).

Outputs are compared as raw f32 bits with one allowance: any NaN equals any NaN;
out_box first, then out_rgbl, so a moments mistake is told from a mapping or blend
mistake.  Nothing expected comes from the library.  The inputs are
move_run_cases.py's; that they are neither vacuous nor total (the right tables give
history, a wrong entry, swapped tables, a forgotten stride or mapping do not) is
asserted on the CPU, by the restatement alone, in test_move_ref.py.  Here only bits
are asserted.
"""
import numpy as np
import pytest

import clamp_ref as CR
import move_ref as MR
import move_run_cases as MV
import raytracer_amd as R
from test_gpu_clamp import GAMMAS, RADII
from test_gpu_history import PAIRS, SIZES, inputs, memo, same_bits, view

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = 3.4028234663852886e38


def run_both(c, s0, s1, clamp, what, rec=None, box=True, **opts):
    """rt_move_run against move_ref over a case of move_run_cases, the box first."""
    rec = c["rec"] if rec is None else rec
    want, wbox = MR.resolve(c["rgb"], c["n"], rec, s0, s1, c["pcam"], c["prgbl"], c["prec"],
                            **{"max_history": 32.0, "sigma_z": 0.02, **opts}, clamp=clamp)
    got, gbox = R.move_run(c["rgb"], c["n"], rec, s0, s1, c["pcam"], c["prgbl"], c["prec"], clamp=clamp, box=box, **opts)
    if box:
        same_bits(gbox, wbox, f"{what}: out_box")
    else:
        assert gbox is None
    same_bits(got, want, f"{what}: out_rgbl")
    return got


# ---- a. equal tables: the clamp restatement's bits ------------------------------------------------

TABLES = {"none": None, "one": MV.tables(1)[0], "300": MV.tables(300)[0]}


@pytest.mark.parametrize("tab", list(TABLES))
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("w,h", SIZES)
def test_equal_tables_are_the_clamp_restatement(w, h, pair, tab):
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = memo(("inputs", w, h), lambda: inputs(w, h, 7))
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    t = TABLES[tab]
    for radius in RADII:
        for gamma in GAMMAS:
            clamp = dict(gamma=gamma, radius=radius)
            what = f"{pair} {w}x{h} {tab} r{radius} g{gamma}"
            want, wbox = memo(("clamp", w, h, pair, radius, gamma),
                              lambda: CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=clamp))
            got, box = R.move_run(rgb, n, rec, t, t, pcam, prgbl, prec, clamp=clamp)
            same_bits(box, wbox, f"{what}: out_box")
            same_bits(got, want, f"{what}: out_rgbl")
    # out_box NULL: the same out_rgbl
    got, none = R.move_run(rgb, n, rec, t, t, pcam, prgbl, prec, clamp=clamp, box=False)
    assert none is None
    same_bits(got, want, f"{what}: no box")


# ---- b. the index seam ----------------------------------------------------------------------------

SEAMS = [("mod", "identity"), ("strips", "identity"), ("strips", "translated"), ("strips", "rotated")]


@pytest.mark.parametrize("S", [37, 300])
@pytest.mark.parametrize("w,h", [(9, 9), (24, 24), (70, 50)])
@pytest.mark.parametrize("layout,pair", SEAMS)
def test_seam_every_sphere_moved(layout, pair, w, h, S):
    c = MV.seam(w, h, S, pair, layout)
    what = f"seam {layout} {pair} {w}x{h} S={S}"
    run_both(c, c["s0"], c["s1"], dict(gamma=1.0, radius=1), what)
    # the tables the wrong way round and rolled by one entry are inputs like any other
    run_both(c, c["s1"], c["s0"], dict(gamma=1.0, radius=1), f"{what}, swapped")
    run_both(c, *MV.rolled(c), dict(gamma=1.5, radius=2), f"{what}, rolled", box=False)


@pytest.mark.parametrize("S", [37, 300])
def test_seam_with_an_identical_prefix(S):
    """The first half of the table equal on bits in prev_spheres and spheres: those pixels
    are the clamp restatement's, next to pixels that are mapped."""
    c = MV.seam(70, 50, S, "identity", "mod")
    s0, s1, rec, still = MV.half_identical(c)
    clamp = dict(gamma=1.0, radius=1)
    got = run_both(c, s0, s1, clamp, f"identical prefix S={S}", rec=rec)
    want, _ = CR.resolve(c["rgb"], c["n"], rec, c["pcam"], c["prgbl"], c["prec"], clamp=clamp)
    same_bits(got[still], want[still], f"identical prefix S={S}: the spheres that stayed")


# ---- c. the edges of the index ----------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(9, 9), (70, 50)])
@pytest.mark.parametrize("ns", [0, 1, 5, 300])
def test_edges_of_the_index(ns, w, h):
    """prim 0, 1, nspheres, nspheres + 1 (a triangle's) and 0xFFFFFFFF; nspheres 0 (NULL
    tables) and 1; and no prev under differing tables: the means with len = n."""
    c = MV.index_edges(w, h, ns)
    what = f"index edges ns={ns} {w}x{h}"
    for radius, gamma in ((1, 1.0), (3, 0.0)):
        run_both(c, c["s0"] if ns else None, c["s1"] if ns else None, dict(gamma=gamma, radius=radius), what)
    want, wbox = MR.resolve(c["rgb"], c["n"], c["rec"], c["s0"], c["s1"], clamp=dict(gamma=1.0, radius=2))
    got, box = R.move_run(c["rgb"], c["n"], c["rec"], c["s0"], c["s1"], clamp=dict(gamma=1.0, radius=2))
    same_bits(box, wbox, f"{what}, no prev: out_box")
    same_bits(got, want, f"{what}, no prev: out_rgbl")
    same_bits(got[..., :3], c["rgb"], f"{what}, no prev: the means")
    assert (got[..., 3] == c["n"].astype(F)).all()


# ---- d. special values of the mapping -------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("gamma", [0.0, 1.5, FLT_MAX])
def test_special_values_of_the_mapping(radius, gamma):
    """Zero, infinite, negative and subnormal radii, k and e * k that overflow or are
    subnormal, infinite, huge and NaN centres, centres that differ in the sign of zero,
    non-finite positions and t on sphere prims, n = 0, len = 0 (move_run_cases.special_move;
    what the restatement makes of them is asserted in test_move_ref.py)."""
    c, names = memo("special_move", MV.special_move)
    got = run_both(c, c["s0"], c["s1"], dict(gamma=gamma, radius=radius), f"special r{radius} g{gamma}")
    took = MV.took(got, c["n"])
    assert np.isnan(got).any() and np.isinf(got).any() and took.any()
    # a non-finite k or P' takes no history
    q = MR.moved_positions(c["rec"], c["s0"], c["s1"])
    prim = c["rec"]["prim"]
    on_sphere = (prim >= 1) & (prim <= len(c["s0"]))
    assert not took[on_sphere & ~np.isfinite(q).all(axis=-1)].any()
    got2 = run_both(c, c["s0"], c["s1"], dict(gamma=gamma, radius=radius), "special, other options",
                    max_history=3.0, sigma_z=1e-6, box=False)
    assert got2.tobytes() != got.tobytes()
