"""The temporal reprojection's contract (include/raytracer_amd.h rt_history_*,
DESIGN.md 5.10) restated in numpy f32, vectorised over the image.

Every operation of the contract is one numpy float32 operation, written out:
no np.dot, no np.cross, no np.sum, no float64.  A skipped tap leaves the sums as
they are (np.where), so the four accumulations keep the contract's order, j
outer and i inner.  A float becomes an index only where the range test passed.
History is the snapshot bookkeeping of a resolve (steps 2, 3 and 6).  Nothing
here comes from the library.
"""
import numpy as np

from filter_ref import means, rgba8

F = np.float32


def cross(a, b):
    """maths.rs:88-94: each product rounded, then the subtraction."""
    return (a[1] * b[2] - a[2] * b[1], -(a[0] * b[2] - a[2] * b[0]), a[0] * b[1] - a[1] * b[0])


def dot3(a, b):
    """((a.x*b.x) + (a.y*b.y)) + (a.z*b.z), each step rounded; a, b: three arrays or scalars each."""
    return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2])


def project(cam, pos, w, h):
    """Positions pos[..., 3] in the view of the camera's 12 floats at w x h ->
    (in front, fx, fy); fy counts rows from the bottom."""
    cam = np.asarray(cam).reshape(12)
    assert cam.dtype == F and pos.dtype == F
    with np.errstate(all="ignore"):
        O, L, H, V = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
        A = (L[0] - O[0], L[1] - O[1], L[2] - O[2])
        n0, n1, n2 = cross(H, V), cross(V, A), cross(A, H)
        det = dot3(A, n0)
        assert det.dtype == F and n1[1].dtype == F
        d = (pos[..., 0] - O[0], pos[..., 1] - O[1], pos[..., 2] - O[2])
        s, a, b = dot3(d, n0), dot3(d, n1), dot3(d, n2)
        front = ((s > 0) & (det > 0)) | ((s < 0) & (det < 0))
        u, v = a / s, b / s
        fx = u * F(w - 1) - F(0.5)
        fy = v * F(h - 1) - F(0.5)
        assert fx.dtype == F and fy.dtype == F and s.dtype == F
    return front, fx, fy


def resolve(rgb, n, rec, prev_cam=None, prev_rgbl=None, prev_rec=None, max_history=32.0, sigma_z=0.02):
    """Step 5: means rgb[h, w, 3], samples n (a count or a plane), the view's records
    rec, and prev (its 12 camera floats, {r, g, b, len}[h, w, 4] and records; prev_rgbl
    None: invalid) -> {out, len} float32[h, w, 4]."""
    m = np.asarray(rgb)
    assert m.dtype == F and m.ndim == 3 and m.shape[2] == 3 and rec.shape == m.shape[:2]
    vh, vw = m.shape[:2]
    nf = np.broadcast_to(np.asarray(n), (vh, vw)).astype(F)
    out = np.empty((vh, vw, 4), F)
    out[..., :3] = m
    out[..., 3] = nf
    if prev_rgbl is None:
        return out
    cam = np.asarray(prev_cam).reshape(12)
    prev = np.asarray(prev_rgbl)
    # (the frame's size is prev's: the view may be some whole rows of it, which a
    # test of a large frame uses -- nothing below depends on where a view pixel is)
    h, w = prev.shape[:2]
    assert cam.dtype == F and prev.dtype == F and prev.shape == (h, w, 4) and prev_rec.shape == (h, w) and vw == w
    mh, sz = F(max_history), F(sigma_z)
    with np.errstate(all="ignore"):
        prim, pos, nrm = rec["prim"], rec["position"], rec["normal"]
        P = (pos[..., 0], pos[..., 1], pos[..., 2])
        N = (nrm[..., 0], nrm[..., 1], nrm[..., 2])
        front, fx, fy = project(cam, pos, w, h)
        inside = (prim != 0) & front & (fx > -1) & (fx < F(w)) & (fy > -1) & (fy < F(h))  # (false for NaN)
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0f, fy - y0f
        x0 = np.where(inside, x0f, F(0)).astype(np.int64)
        y0 = np.where(inside, y0f, F(0)).astype(np.int64)
        zlim = sz * rec["t"]
        cs = [np.zeros((vh, vw), F) for _ in range(3)]
        ls, ws = np.zeros((vh, vw), F), np.zeros((vh, vw), F)
        pprim, ppos = prev_rec["prim"], prev_rec["position"]
        for j in (0, 1):
            wy = ty if j else F(1) - ty
            row = y0 + j  # from the bottom
            for i in (0, 1):
                wx = tx if i else F(1) - tx
                col = x0 + i
                ok = inside & (col >= 0) & (col < w) & (row >= 0) & (row < h)
                qy = np.where(ok, h - 1 - row, 0)
                qx = np.where(ok, col, 0)
                cq = prev[qy, qx]
                vq = ppos[qy, qx]
                e = np.abs(dot3((vq[..., 0] - P[0], vq[..., 1] - P[1], vq[..., 2] - P[2]), N))
                wt = wx * wy
                assert e.dtype == F and wt.dtype == F and zlim.dtype == F
                ok = ok & (cq[..., 3] > 0) & (pprim[qy, qx] == prim) & (e <= zlim) & (wt > 0)
                for k in range(3):
                    cs[k] = np.where(ok, cs[k] + wt * cq[..., k], cs[k])
                ls = np.where(ok, ls + wt * cq[..., 3], ls)
                ws = np.where(ok, ws + wt, ws)
        has = ws > 0
        hl = ls / ws
        cap = np.where(mh > nf, mh, nf)
        tl = hl + nf
        tl = np.where(tl > cap, cap, tl)
        alpha = nf / tl
        assert hl.dtype == F and tl.dtype == F and alpha.dtype == F and cap.dtype == F
        for k in range(3):
            hc = cs[k] / ws
            o = hc + (m[..., k] - hc) * alpha
            assert o.dtype == F
            out[..., k] = np.where(has, o, m[..., k])
        out[..., 3] = np.where(has, tl, nf)
    return out


class History:
    """An accumulator's two snapshots.  resolve(sums, n, rec, cam, edit): the
    accumulator's sums [h, w, 3], samples, current records, 12 camera floats and an
    integer that changes with every scene edit -> (rgb, rgba, len)."""

    def __init__(self, max_history=32.0, sigma_z=0.02):
        self.max_history, self.sigma_z = max_history, sigma_z
        self.cur = self.prev = None

    def reset(self):
        self.cur = self.prev = None

    def length(self, shape):
        return np.zeros(shape, F) if self.cur is None else self.cur["rgbl"][..., 3].copy()

    def resolve(self, sums, n, rec, cam, edit):
        cam = np.array(cam, F).reshape(12)
        if any(s is not None and s["edit"] != edit for s in (self.cur, self.prev)):
            self.reset()
        if self.cur is not None and self.cur["cam"].tobytes() != cam.tobytes():
            self.prev = self.cur  # (the old prev's place is what the new cur is written to)
        p = self.prev
        rgbl = resolve(means(sums, n), n, rec, *((p["cam"], p["rgbl"], p["rec"]) if p else (None, None, None)),
                       max_history=self.max_history, sigma_z=self.sigma_z)
        self.cur = dict(rgbl=rgbl, rec=rec.copy(), cam=cam, edit=edit)
        rgb = np.ascontiguousarray(rgbl[..., :3])
        return rgb, rgba8(rgb), rgbl[..., 3].copy()
