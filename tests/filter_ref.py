"""The edge-aware filter's contract (include/raytracer_amd.h)
restated in numpy f32, vectorised over the image with one shifted view per tap.

Every operation of the contract is one numpy float32 operation, written out:
no np.dot, no np.sum, no `**`, no float64.  A skipped tap leaves the sums as
they are (np.where), so the 25 accumulations keep the contract's order, j outer
and i inner.  Nothing here comes from the library.
"""
import numpy as np

F = np.float32
TAPS = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
SAME_PRIM = 1


def dot3(a, b):
    """((a.x*b.x) + (a.y*b.y)) + (a.z*b.z), each step rounded."""
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def level(c, rec, step, sl, sigma_z, normal_squarings, same_prim):
    h, w = c.shape[:2]
    prim, nrm, pos = rec["prim"], rec["normal"], rec["position"]
    lum = (c[..., 0] + c[..., 1]) + c[..., 2]
    zs = F(sigma_z) * rec["t"]
    num = np.zeros((h, w, 3), F)
    den = np.zeros((h, w), F)
    for j in range(5):
        dy = (j - 2) * step
        y0, y1 = max(0, -dy), min(h, h - dy)
        for i in range(5):
            dx = (i - 2) * step
            x0, x1 = max(0, -dx), min(w, w - dx)
            if y0 >= y1 or x0 >= x1:
                continue  # every such tap is outside the image
            P = (slice(y0, y1), slice(x0, x1))                      # the centres whose tap is inside
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))  # their taps
            hp, hq = prim[P] != 0, prim[Q] != 0
            keep = hp == hq
            if same_prim:
                keep = keep & (prim[P] == prim[Q])
            w0 = TAPS[j] * TAPS[i]
            d = dot3(nrm[P], nrm[Q])
            d = np.where(d > 0, d, F(0))
            for _ in range(normal_squarings):
                d = d * d
            v = pos[Q] - pos[P]
            e = np.abs(dot3(v, nrm[P])) / zs[P]
            wz = F(1) / (F(1) + e * e)
            wt = np.where(hp, (w0 * d) * wz, w0)
            el = np.abs(lum[Q] - lum[P]) / sl
            wl = F(1) / (F(1) + el * el)
            wt = wt * wl
            ok = keep & (wt > 0)  # (false for NaN)
            for k in range(3):
                num[P + (k,)] = np.where(ok, num[P + (k,)] + wt * c[Q + (k,)], num[P + (k,)])
            den[P] = np.where(ok, den[P] + wt, den[P])
    out = np.empty_like(c)
    for k in range(3):
        out[..., k] = np.where(den > 0, num[..., k] / den, c[..., k])
    assert out.dtype == F and wt.dtype == F and e.dtype == F and el.dtype == F
    return out


def rgba8(c):
    """sqrt(c_k) * 255.999 as u8 (saturating, NaN -> 0), alpha 255."""
    with np.errstate(all="ignore"):
        x = np.sqrt(np.asarray(c, F)) * F(255.999)
    assert x.dtype == F
    b = np.where(x > 0, np.where(x >= 255, F(255), x), F(0))  # (NaN fails x > 0)
    out = np.full(c.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = b.astype(np.uint8)  # (truncates)
    return out


def filter_image(rgb, rec, levels=3, sigma_l=0.5, sigma_z=0.02, normal_squarings=5, flags=0):
    """(rgb float32[h, w, 3], rgba uint8[h, w, 4]) of the contract."""
    c = np.array(rgb, F)
    assert c.ndim == 3 and c.shape[2] == 3 and rec.shape == c.shape[:2]
    with np.errstate(all="ignore"):
        for l in range(levels):
            sl = np.ldexp(F(sigma_l), -l)
            assert sl.dtype == F
            c = level(c, rec, 1 << l, sl, sigma_z, normal_squarings, bool(flags & SAME_PRIM))
    return c, rgba8(c)


def means(sums, n):
    """The accumulator's input colours: sum_k * inv, inv = 1.0f / (float)n_p (n a count or a plane of counts)."""
    n = np.asarray(n)
    with np.errstate(all="ignore"):
        inv = F(1) / n.astype(F)
        out = np.asarray(sums, F) * (inv[..., None] if inv.ndim else inv)
    assert out.dtype == F
    return out
