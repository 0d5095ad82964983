"""Two scenes whose frames send some lanes of a wave through the fallbacks of
csrc/exactdiv.h while their neighbours stay inside the guards (a plain helper
module, no tests).  Built from tests/scene_values.py's field, splice and sphere.

Scene A: the 60-ball field in front of one diffuse sphere of radius 2^41
centred 1.5 * 2^41 behind the camera, so its near pole is 2^40 away and it
covers a disc of the view (tan of its angular radius: 0.894 of the half
height).  A hit on it divides (pos - c) by 2^41, outside the denominator guard
[2^-40, 2^40], and its roots come from a discriminant of the order 2^82.
Rays that pass it, or meet a ball of the field first, stay ordinary.  (Centred
2^41 + 2^20 behind the camera the sphere is a wall across the whole view and
takes 88.4 % of the primary rays: outside the band.)

Scene B: the camera at (2^-42, 2^-42, 2^-42) inside a unit glass ball centred
at the origin.  No ball of the field lies within one unit of the camera (the
glass takes every primary ray up to radius 2, and still 89.9 % at radius 6),
so 27 ordinary balls of radius 0.1 stand inside the glass, 0.7 from its
centre, in a 9 x 3 fan across the view: primary rays end on one of them or on
the glass.  The scene grammar builds the camera frame from an origin and an
aspect ratio (camera.rs:21-33), so the 2^-42 offsets are absorbed in llc and
no tiny vector reaches NVec3::new from this camera; tiny, huge, zero and
non-finite vectors in mixed waves are tools/guard_mix_check.hip's part.

edge_share(src) is the share of primary rays whose first hit is the scene's
last sphere, measured on the oracle: that sphere is made an emitter of colour
7 (no other first hit can give 7: sky colours are <= 1, and at depth 1 every
scattered path ends black), and the samples equal to 7 are counted."""
import numpy as np

import oracle as O
import scene_values as V

FRAME = (64, 8, 4, 4)  # w, h, spp, depth of the GPU frames
BAND = (0.20, 0.80)

R_A = 2.0 ** 41
Z_A = -1.5 * 2.0 ** 41
CAM_B = 2.0 ** -42
RADIUS_B = 1.0
EMISSION = 3


def scene_a():
    return V.splice(V.field(), [V.DIFF], [V.sphere(0.0, 0.0, Z_A, R_A, "ED")])


def fan_b():
    """27 ordinary balls inside the unit ball, towards the view plane's 9 x 3 grid."""
    out = []
    for j, y in enumerate((-0.66, 0.0, 0.66)):
        for i in range(9):
            d = np.array([-1.4 + 0.35 * i, y, -1.0])
            c = 0.7 * d / np.linalg.norm(d)
            out.append(V.sphere(c[0], c[1], c[2], 0.1, f"K{(i + j) % 2}"))  # (the field's diffuse and metal)
    return out


def scene_b(radius=RADIUS_B, fan=True):
    src = V.splice(V.field(), [V.GLASS], (fan_b() if fan else []) + [V.sphere(0.0, 0.0, 0.0, radius, "EG")])
    lines = src.split("\n")
    assert lines[0].startswith("camera origin 0.000000 0.000000 0.000000 ")
    c = f"{CAM_B:.30f}"
    lines[0] = f"camera origin {c} {c} {c} aspect 1.5;"
    return "\n".join(lines)


def edge_share(src):
    w, h, spp, _ = FRAME
    scene = O.Scene(src)
    scene.set_material(scene.num_spheres - 1, EMISSION, (7.0, 7.0, 7.0))
    _, _, _, smp = scene.render(w, h, spp, 1, mode=O.RNG_COUNTER, record_samples=True)
    return float(np.count_nonzero((smp[:, :3] == np.float32(7.0)).all(axis=1))) / (w * h * spp)
