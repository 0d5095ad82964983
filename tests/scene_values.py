"""Scenes with unusual but legal values (a plain helper module, no tests).

The grammar takes a leading '-' and a literal of any length (60 nines parse to
+inf), and rt_world_set_*_material takes any float.  The reference renders
all of it in a defined way: a negative radius flips the normal (common.rs:95)
while the hit test sees r * r, refract has no total-internal-reflection branch
(materials.rs:94, maths.rs:31-36: ir 0.0 and -1.5 give infinite and NaN
directions from the second bounce on), fuzz and colours are not clamped.

Every case splices a few edge statements into a background that is large
enough for the trees: the 60-sphere field of test_gpu_corner_tree, or a
triangle soup with 40 spheres.  The edge primitives sit near z = -1.5, between
the camera (at the origin, looking down -z) and the background, so primary
rays see them.  case(name) is a Case; its src is the scene, its base the same
scene without the edge statements.

EDIT_CASES are the same material families applied through set_material to
the unchanged field (Case.edits: (sphere, kind, rgb, param), for both R.World
and O.Scene).

The shares next to each case are measured on the oracle alone
(tests/test_scene_values.py asserts the floors): the share of the 48 x 32 x 4
COUNTER samples, depth 8, whose colour differs from the base scene's."""
import numpy as np

import scenes as S
from test_gpu_corner_tree import _random_scene

NINES = "9" * 60 + ".0"  # parses to +inf
SOUP_SEED = 7
FRAME = (48, 32, 4, 8)  # the GPU cases' frame: w, h, spp, depth

DIFFUSE, METAL, DIELECTRIC = 0, 1, 2


def field():
    return _random_scene(seed=1, n=60, spread=3.0, radius=0.4, big=False)


def soup(n=300):
    return S.triangle_soup(SOUP_SEED, n, spheres=40)


def splice(src, materials=(), spheres=(), triangles=()):
    """src with statements added: materials after its materials, spheres after
    its spheres (they get the highest sphere indices), triangles at the end
    (the parser wants the three groups in that order)."""
    lines = src.strip("\n").split("\n")
    last = {k: max((i for i, ln in enumerate(lines) if ln.startswith(k)), default=None)
            for k in ("material", "sphere")}
    at_m = last["material"] + 1
    at_s = (last["sphere"] if last["sphere"] is not None else last["material"]) + 1
    out = lines[:at_m] + list(materials) + lines[at_m:at_s] + list(spheres) + lines[at_s:] + list(triangles)
    return "\n".join(out) + "\n"


def sphere(x, y, z, r, mat):
    """(x, y, z, r: floats printed with 6 places, or literal strings)"""
    f = [v if isinstance(v, str) else f"{v:.6f}" for v in (x, y, z, r)]
    return f"sphere center {f[0]} {f[1]} {f[2]} radius {f[3]} material {mat};"


def triangle(v0, v1, v2, mat):
    f = [" ".join(c if isinstance(c, str) else f"{c:.6f}" for c in v) for v in (v0, v1, v2)]
    return f"triangle v0 {f[0]} v1 {f[1]} v2 {f[2]} material {mat};"


def radii(src):
    """The f32 radii of src's spheres, in order."""
    return np.array([float(ln.split()[6]) for ln in src.split("\n") if ln.startswith("sphere")], np.float32)


class Case:
    def __init__(self, name, src, base, soup=False, edits=(), big_k=()):
        self.name, self.src, self.base, self.soup = name, src, base, soup
        self.edits = list(edits)  # (sphere index, kind, rgb, param), applied after parsing
        self.big_k = tuple(big_k)  # RT_AMD_BIG_K values the case is rerun with

    def apply_edits(self, *worlds):
        """set_material on every R.World / O.Scene given."""
        for w in worlds:
            for (i, kind, rgb, param) in self.edits:
                w.set_material(i, kind, rgb, param)


GLASS = "material EG : Dielectric ir 1.5;"
DIFF = "material ED : Diffuse color 0.8 0.3 0.3;"
MIRROR = "material EM : Metal color 0.9 0.9 0.9 fuzz 0.0;"

IR_VALUES = ("1.0", "0.5", "0.0", "-1.5", "3.0", "1000000.0")


def _sphere_case(name, materials, spheres, **kw):
    base = field()
    return Case(name, splice(base, materials, spheres), base, **kw)


def _hollow():
    # the hollow glass ball: a shell between r 0.5 and the flipped normals of r -0.45;
    # a diffuse ball whose normals point inwards
    return _sphere_case("hollow", [GLASS, DIFF], [
        sphere(-0.7, 0.0, -1.5, 0.5, "EG"), sphere(-0.7, 0.0, -1.5, -0.45, "EG"),
        sphere(0.8, 0.1, -1.5, -0.4, "ED")])


def _zero_r():
    # radius 0 makes the tree's 1 / rmin infinite, 0.000001 makes it huge; what a
    # frame shows of this case is the ordinary neighbour
    return _sphere_case("zero_r", [DIFF], [
        sphere(0.0, 0.3, -1.5, "0.0", "ED"), sphere(0.3, -0.2, -1.5, "0.000001", "ED"),
        sphere(-0.6, 0.0, -1.5, 0.3, "ED")])


def _ir():
    mats = [f"material EI{k} : Dielectric ir {v};" for k, v in enumerate(IR_VALUES)]
    sph = [sphere(-1.75 + 0.7 * k, 0.35 if k % 2 else -0.35, -1.5, 0.3, f"EI{k}") for k in range(6)]
    return _sphere_case("ir", mats, sph)


FUZZ_COL = (  # (kind, rgb, param)
    (METAL, (2.0, -0.5, 0.5), 1.5),
    (METAL, (-0.8, 0.2, 0.3), -0.7),  # (a negative luminance: pixels with a negative mean)
    (DIFFUSE, (3.0, 0.0, -1.0), 0.0),
    (METAL, (1.0, 1.0, 1.0), 100.0),
)


def _fuzz_col():
    mats = ["material EF0 : Metal color 2.0 -0.5 0.5 fuzz 1.5;",
            "material EF1 : Metal color -0.8 0.2 0.3 fuzz -0.7;",
            "material EF2 : Diffuse color 3.0 0.0 -1.0;",
            "material EF3 : Metal color 1.0 1.0 1.0 fuzz 100.0;"]
    sph = [sphere(-1.35 + 0.9 * k, 0.3 if k % 2 else -0.3, -1.5, 0.4, f"EF{k}") for k in range(4)]
    return _sphere_case("fuzz_col", mats, sph)


def _nonfinite():
    # an infinite centre, an infinite radius, a finite radius whose square
    # overflows: none can be hit, all stay in the brute-force list
    return _sphere_case("nonfinite", [DIFF, MIRROR], [
        sphere(NINES, 0.0, -1.5, 0.3, "ED"), sphere(0.5, 0.5, -1.5, NINES, "EM"),
        sphere(-0.5, -0.5, -1.5, "99999999999999999999.0", "ED"), sphere(0.0, 0.0, -1.5, 0.35, "EM")])


BIG_MIX_STEP = 0.0001


def big_mix_radii():
    """(below, above, median): the two added radii and the median radius of the
    case's 62 spheres.  Both added radii lie above the median, so the median
    is entry 31 of the field's sorted radii (bvh.cpp takes element n / 2)."""
    med = float(np.sort(radii(field()))[31])
    return 8.0 * med - BIG_MIX_STEP, 8.0 * med + BIG_MIX_STEP, med


def _big_mix():
    lo, hi, _ = big_mix_radii()
    return _sphere_case("big_mix", [DIFF, MIRROR], [
        sphere(-3.2, -0.6, -5.0, lo, "EM"), sphere(3.2, 0.6, -5.0, hi, "ED")], big_k=("2", "1e9"))


def _coincident():
    # same centre, same |r|: the diffuse ball has the lowest index and must win
    return _sphere_case("coincident", [DIFF, MIRROR, GLASS], [
        sphere(0.2, 0.1, -1.5, 0.4, "ED"), sphere(0.2, 0.1, -1.5, 0.4, "EM"),
        sphere(0.2, 0.1, -1.5, -0.4, "EG")])


def _cam_inside():
    # the camera inside a glass ball of radius 2 and exactly on the surface of a
    # diffuse one: origin = centre + (r, 0, 0)
    return _sphere_case("cam_inside", [GLASS, DIFF], [
        sphere(0.5, 0.3, -0.5, 2.0, "EG"), sphere(-0.75, 0.0, 0.0, 0.75, "ED")])


def _tri_degenerate(n=300):
    base = soup(n)
    tris = [
        triangle((0.5, 0.5, -1.5), (0.5, 0.5, -1.5), (0.5, 0.5, -1.5), "ED"),      # zero area
        triangle((-1.0, -1.0, -1.5), (0.0, 0.0, -1.5), (1.0, 1.0, -1.5), "ED"),    # collinear
        triangle((-1.0, 0.5, -1.5), (0.0, 0.5, -1.5), (NINES, 0.0, -1.5), "EM"),   # an infinite vertex
        # its plane holds the camera origin (the midpoint of v0 v1 and v2 are
        # opposite): n . o = 0 for primary rays, not for the later ones (common.rs:141)
        triangle((-2.0, -1.0, -3.0), (2.0, -1.0, -3.0), (0.0, 1.0, 3.0), "EM"),
        triangle((0.4, -0.9, -1.5), (1.6, -0.9, -1.5), (1.0, 0.1, -1.5), "ED"),    # an ordinary neighbour
    ]
    return Case("tri_degenerate", splice(base, [DIFF, MIRROR], (), tris), base, soup=True)


def _tri_tie(n=300):
    base = soup(n)
    a = ((-1.6, -1.0, -1.5), (-0.4, -1.0, -1.5), (-1.0, 0.2, -1.5))
    tris = [triangle(*a, "ED"), triangle(*a, "EM"),  # identical: the lower index wins
            # the plane z = -1.5 touches the ball's near pole: on the axis ray the
            # two hits have equal t and the triangle wins; the jittered rays of a
            # frame pass next to the axis, where the two t differ in the last bits
            triangle((-0.5, -0.5, -1.5), (0.5, -0.5, -1.5), (0.0, 0.6, -1.5), "EG")]
    return Case("tri_tie", splice(base, [DIFF, MIRROR, GLASS], [sphere(0.0, 0.0, -2.0, 0.5, "ED")], tris),
                base, soup=True)


def _visible(src, count):
    """The `count` spheres of src that cover most of the view from the origin
    (largest r / distance among those near the axis), by sphere index."""
    rows = [ln.split() for ln in src.split("\n") if ln.startswith("sphere")]
    c = np.array([[float(t) for t in r[2:5]] for r in rows])
    r = np.array([float(t[6]) for t in rows])
    dist = np.linalg.norm(c, axis=1)
    in_view = (np.abs(c[:, 0] / -c[:, 2]) < 1.2) & (np.abs(c[:, 1] / -c[:, 2]) < 0.8)
    order = np.argsort(-(r / dist) * in_view)
    return [int(i) for i in order[:count]]


def _edit_ir():
    src = field()
    edits = [(i, DIELECTRIC, (1.0, 1.0, 1.0), float(v)) for i, v in zip(_visible(src, 6), IR_VALUES)]
    return Case("edit_ir", src, src, edits=edits)


def _edit_fuzz_col():
    src = field()
    edits = [(i, kind, rgb, param) for i, (kind, rgb, param) in zip(_visible(src, 4), FUZZ_COL)]
    return Case("edit_fuzz_col", src, src, edits=edits)


_BUILDERS = {
    # name: builder                 # measured share of samples that differ from the base scene
    "hollow": _hollow,              # 11.4 %
    "zero_r": _zero_r,              # 2.2 % (the ordinary neighbour)
    "ir": _ir,                      # 14.1 %, NaN samples 2.2 %
    "fuzz_col": _fuzz_col,          # 18.8 %, negative 13.7 %, above 1 9.2 %
    "nonfinite": _nonfinite,        # 2.9 %
    "big_mix": _big_mix,            # 23.5 %
    "coincident": _coincident,      # 4.0 %
    "cam_inside": _cam_inside,      # 100 %
    "tri_degenerate": _tri_degenerate,  # 5.7 %
    "tri_tie": _tri_tie,            # 9.7 %
}
_EDIT_BUILDERS = {
    "edit_ir": _edit_ir,              # 3.8 %, NaN samples 1.1 %
    "edit_fuzz_col": _edit_fuzz_col,  # 3.0 %, negative 2.5 %, above 1 2.0 %
}

SPHERE_CASES = [k for k in _BUILDERS if not k.startswith("tri_")]
SOUP_CASES = [k for k in _BUILDERS if k.startswith("tri_")]
TABLE_CASES = SPHERE_CASES + SOUP_CASES
EDIT_CASES = list(_EDIT_BUILDERS)

_MEMO = {}


def case(name, soup_triangles=300):
    """The Case `name`; soup cases take the size of their soup (the numpy
    restatement renders 40 triangles at most in reasonable time)."""
    key = (name, soup_triangles if name in SOUP_CASES else None)
    if key not in _MEMO:
        if name in SOUP_CASES:
            _MEMO[key] = _BUILDERS[name](soup_triangles)
        else:
            _MEMO[key] = {**_BUILDERS, **_EDIT_BUILDERS}[name]()
    return _MEMO[key]
