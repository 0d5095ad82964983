"""Oriented cameras for the camera tests (a plain helper module, no tests).

Cameras are look_at(origin -> target, up, vertical fov in degrees) at aspect
1.5.  look_at() and with_vertical_fov() restate the reference's constructors
(camera.rs:34-69, maths.rs:88-137, 204-214) in numpy f32, one rounded
operation per step in its order; tan is the host libm's tanf through ctypes,
as Rust's f32::tan is the platform's."""
import ctypes as C
import ctypes.util

import numpy as np

f32 = np.float32
ASPECT = 1.5
Y = (0.0, 1.0, 0.0)
T = (0.0, 0.0, -5.0)  # the field's and the soup's centre of interest

# name: (origin, target, up, vfov degrees)
RTOW = {
    "book": ((13, 2, 3), (0, 0, 0), Y, 20),
    "back": ((0, 0, -3), (0, 0, 3), Y, 60),
    "down": ((0, 6, 0.5), (0, 0, 0), Y, 50),
    "roll": ((2, 1, 2), (0, 0.3, -1), (1, 1, 0), 70),
    "wide": ((0, 0.5, 1), (0.2, 0.4, -1), Y, 120),
    "inside": ((-2, 0.3, 0), (3, 0.3, 0.1), Y, 45),
}
FIELD = {
    "side": ((7, 1, -5), T, Y, 50),
    "behind": ((0, 0.5, -12), T, Y, 50),
    "high": ((0, 6, -1), T, Y, 60),
    "inside": ((0, 0, -5), (1, 0.2, -6), Y, 90),
    "roll": ((4, 3, 0), T, (1, 1, 0), 40),
    "tele": ((0, 0, 0), (0.3, 0.2, -5), Y, 10),
    "wide": ((0, 0, -1), T, Y, 120),
}
SOUP = FIELD  # the same seven cameras

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.restype = C.c_float
_libm.tanf.argtypes = [C.c_float]


def tanf(x):
    return f32(_libm.tanf(C.c_float(float(x))))


def radians(deg):
    """The f32 a caller passes for `deg` degrees."""
    return f32(np.radians(deg))


def _v(p):
    return np.array(p, dtype=f32)


def _cross(a, b):  # maths.rs:88-94 / 131-137: the middle component is the negated difference
    return np.array([a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0]], f32)


def _normalize(a):  # maths.rs:111-118
    length = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return np.array([a[0] / length, a[1] / length, a[2] / length], f32)


def new_at(origin, aspect):  # camera.rs:21-33
    o = _v(origin)
    vh = f32(2.0)
    vw = f32(aspect) * vh
    ll = o - np.array([vw / f32(2.0), vh / f32(2.0), f32(1.0)], f32)
    return np.concatenate([o, ll, [vw, 0, 0], [0, vh, 0]]).astype(f32)


def with_vertical_fov(origin, vfov, aspect=ASPECT):  # camera.rs:34-48
    o = _v(origin)
    h = tanf(f32(vfov) / f32(2.0))
    vh = f32(2.0) * h
    vw = f32(aspect) * vh
    ll = o - np.array([vw / f32(2.0), vh / f32(2.0), f32(1.0)], f32)
    return np.concatenate([o, ll, [vw, 0, 0], [0, vh, 0]]).astype(f32)


def look_at(origin, target, up=Y, vfov=radians(90), aspect=ASPECT):  # camera.rs:49-69
    """The 12 floats, or None where the reference asserts."""
    with np.errstate(all="ignore"):
        o, t = _v(origin), _v(target)
        d = o - t
        if np.all(np.abs(d) < f32(1e-8)):
            return None
        vh = f32(2.0) * tanf(f32(vfov) / f32(2.0))
        vw = vh * f32(aspect)
        w = _normalize(d)
        u = _cross(_normalize(_v(up)), w)
        v = _cross(w, u)
        if not np.abs(v[1]) > f32(1e-8):
            return None
        hor, ver = u * vw, v * vh
        ll = o - hor / f32(2.0) - ver / f32(2.0) - w
        return np.concatenate([o, ll, hor, ver]).astype(f32)


def translated(cam, x, y, z):  # rt_camera_translate
    c = np.array(cam, dtype=f32)
    d = np.array([x, y, z], f32)
    c[0:3] = c[0:3] + d
    c[3:6] = c[3:6] + d
    return c


def moved(cam, x, y, z):  # lib.rs:60-63: new_at(position + d, horizontal.x / vertical.y)
    c = np.array(cam, dtype=f32)
    with np.errstate(all="ignore"):
        return new_at(c[0:3] + np.array([x, y, z], f32), c[6] / c[10])


def camera(table, name):
    o, t, up, deg = table[name]
    return look_at(o, t, up, radians(deg))


def mirrored(cam):
    """cam seen in a mirror: horizontal reversed (the camera determinant changes sign)."""
    c = np.array(cam, dtype=f32)
    c[3:6] = c[3:6] + c[6:9]
    c[6:9] = -c[6:9]
    return c


def singular(cam):
    """cam with vertical parallel to horizontal: determinant 0."""
    c = np.array(cam, dtype=f32)
    c[9:12] = c[6:9]
    return c


def det(cam):
    c = np.array(cam, dtype=np.float64)
    return float(np.linalg.det(np.stack([c[6:9], c[9:12], c[3:6] - c[0:3]], axis=1)))


def spliced_soup():
    """The soup plus a triangle that spans the default camera's whole view (on
    every strip's list) and one that straddles its camera plane z = 0 (on the
    `always` list)."""
    import scene_values as V
    mat = "material EC : Diffuse color 0.3 0.8 0.3;"
    tris = [V.triangle((-40.0, -30.0, -9.0), (40.0, -30.0, -9.0), (0.0, 50.0, -9.0), "EC"),
            V.triangle((-0.5, -0.8, -2.0), (0.9, -0.8, -2.0), (0.2, -0.6, 1.5), "EC")]
    return V.splice(V.soup(), [mat], (), tris)


# Every soup triangle lies in z < -1: from the origin (where a record's phantom
# box is the triangle's own, padded), looking up +z, all are behind the camera
ALL_BEHIND = ((0.0, 0.0, 0.0), (0.0, 0.0, 5.0), Y, 60)


def apply(world, table, name):
    """world.look_at(...) for the named camera."""
    o, t, up, deg = table[name]
    world.look_at(o, t, up, float(radians(deg)), ASPECT)
