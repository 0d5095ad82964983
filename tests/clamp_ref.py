"""The clamped history resolve's contract (include/raytracer_amd.h rt_clamp_*,
DESIGN.md 5.10a) restated in numpy f32, vectorised over the image.

As history_ref: every operation of the contract is one numpy float32 operation,
written out; a skipped tap leaves the sums as they are (np.where), so the
moments keep the contract's order, j outer and i inner; a float becomes an index
only where the range test passed.  resolve() is history_ref.resolve with the
clamp step between hc = cs / ws and the blend; ClampHistory is the snapshot
bookkeeping with the keep-on-edit rule.  Nothing here comes from the library.
"""
import numpy as np

from filter_ref import means, rgba8
from history_ref import dot3, project

F = np.float32


def box(m, gamma, radius):
    """The neighbourhood box of every pixel of the means m[h, w, 3]:
    (lo, hi, mu) float32[h, w, 3] each.  Taps q = p + (i - r, j - r), top row
    first, j outer and i inner; a q outside the image is skipped."""
    m = np.asarray(m)
    assert m.dtype == F and m.ndim == 3 and m.shape[2] == 3
    h, w = m.shape[:2]
    r, g = int(radius), F(gamma)
    rows, cols = np.mgrid[0:h, 0:w]
    c = np.zeros((h, w), np.int64)
    s1 = np.zeros((h, w, 3), F)
    s2 = np.zeros((h, w, 3), F)
    with np.errstate(all="ignore"):
        for j in range(2 * r + 1):
            qy = rows + (j - r)
            for i in range(2 * r + 1):
                qx = cols + (i - r)
                ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                mq = m[np.where(ok, qy, rows), np.where(ok, qx, cols)]
                sq = mq * mq
                assert mq.dtype == F and sq.dtype == F
                c = np.where(ok, c + 1, c)
                s1 = np.where(ok[..., None], s1 + mq, s1)
                s2 = np.where(ok[..., None], s2 + sq, s2)
        ic = (F(1) / c.astype(F))[..., None]
        mu = s1 * ic
        var = s2 * ic - mu * mu
        var = np.where(var < 0, F(0), var)  # (NaN stays NaN)
        wd = g * np.sqrt(var)
        lo, hi = mu - wd, mu + wd
        assert ic.dtype == F and mu.dtype == F and var.dtype == F and wd.dtype == F and lo.dtype == F
    return lo, hi, mu


def resolve(rgb, n, rec, prev_cam=None, prev_rgbl=None, prev_rec=None, max_history=32.0, sigma_z=0.02, clamp=None):
    """Step 5 with the clamp: the arguments of history_ref.resolve and
    clamp = None | dict(gamma, radius) -> (rgbl float32[h, w, 4], box
    float32[h, w, 6] {lo.rgb, hi.rgb} of every pixel, None without a clamp).
    The view may be some whole rows of prev's frame; its box then takes the
    view's first and last rows for the image's, so a caller that checks a band
    hands in `radius` more rows on each side and drops them again."""
    m = np.asarray(rgb)
    assert m.dtype == F and m.ndim == 3 and m.shape[2] == 3 and rec.shape == m.shape[:2]
    vh, vw = m.shape[:2]
    nf = np.broadcast_to(np.asarray(n), (vh, vw)).astype(F)
    out = np.empty((vh, vw, 4), F)
    out[..., :3] = m
    out[..., 3] = nf
    bx = None
    if clamp is not None:
        lo, hi, _ = box(m, clamp["gamma"], clamp["radius"])
        bx = np.concatenate([lo, hi], axis=2)
    if prev_rgbl is None:
        return out, bx
    cam = np.asarray(prev_cam).reshape(12)
    prev = np.asarray(prev_rgbl)
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
            if clamp is not None:
                hc = np.where(hc < lo[..., k], lo[..., k], hc)  # (a NaN bound leaves hc alone)
                hc = np.where(hc > hi[..., k], hi[..., k], hc)
            o = hc + (m[..., k] - hc) * alpha
            assert o.dtype == F and hc.dtype == F
            out[..., k] = np.where(has, o, m[..., k])
        out[..., 3] = np.where(has, tl, nf)
    return out, bx


class ClampHistory:
    """An accumulator's two snapshots under a clamp setting.  clamp: None
    (disabled) or dict(gamma, radius[, keep_on_edit]); it may be changed between
    resolves, as rt_clamp_enable and rt_clamp_disable do, and no snapshot goes.
    resolve(sums, n, rec, cam, edit) -> (rgb, rgba, len)."""

    def __init__(self, max_history=32.0, sigma_z=0.02, clamp=None):
        self.max_history, self.sigma_z, self.clamp = max_history, sigma_z, clamp
        self.cur = self.prev = None

    def reset(self):
        self.cur = self.prev = None

    def length(self, shape):
        return np.zeros(shape, F) if self.cur is None else self.cur["rgbl"][..., 3].copy()

    def resolve(self, sums, n, rec, cam, edit):
        cam = np.array(cam, F).reshape(12)
        keep = self.clamp is not None and bool(self.clamp.get("keep_on_edit"))
        if not keep and any(s is not None and s["edit"] != edit for s in (self.cur, self.prev)):
            self.reset()
        if self.cur is not None and (self.cur["cam"].tobytes() != cam.tobytes() or (keep and self.cur["edit"] != edit)):
            self.prev = self.cur
        p = self.prev
        rgbl, _ = resolve(means(sums, n), n, rec, *((p["cam"], p["rgbl"], p["rec"]) if p else (None, None, None)),
                          max_history=self.max_history, sigma_z=self.sigma_z, clamp=self.clamp)
        self.cur = dict(rgbl=rgbl, rec=rec.copy(), cam=cam, edit=edit)
        rgb = np.ascontiguousarray(rgbl[..., :3])
        return rgb, rgba8(rgb), rgbl[..., 3].copy()
