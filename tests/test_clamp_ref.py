"""CPU tests of the clamp's restatement (clamp_ref.py): without a
clamp it is history_ref's resolve on bits; at 1 x 1 the box collapses onto the
pixel's mean; and on the synthetic views the GPU tests use, the clamp is neither
vacuous nor total."""
import numpy as np
import pytest

import clamp_ref as CR
import history_ref as HR
from test_gpu_history import PAIRS, SIZES, camera, inputs, view

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("w,h", SIZES)
def test_no_clamp_is_the_history_restatement(w, h, pair):
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = inputs(w, h, 7)
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    want = HR.resolve(rgb, n, rec, pcam, prgbl, prec)
    got, box = CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=None)
    assert box is None and (bits(got) == bits(want)).all()
    got, box = CR.resolve(rgb, n, rec, clamp=None)
    assert box is None and (bits(got) == bits(HR.resolve(rgb, n, rec))).all()


@pytest.mark.parametrize("gamma", [0.0, 1.0, 1.5, 3.4028234663852886e38])
@pytest.mark.parametrize("radius", [1, 2, 3])
def test_one_pixel_returns_its_mean(gamma, radius):
    """1 x 1: c = 1, mu = m, var = m * m - m * m = 0, so lo = hi = m, hc = m and
    out = m + (m - m) * alpha = m, with len = tl."""
    cam = camera()
    rec = view(cam, 1, 1)
    assert rec["prim"][0, 0] != 0
    rgb = np.array([[[0.3, 1.7, 0.02]]], F)
    n = np.array([[2]], np.uint32)
    prgbl = np.array([[[5.0, 0.0, 9.0, 7.0]]], F)
    got, box = CR.resolve(rgb, n, rec, cam, prgbl, rec, clamp=dict(gamma=gamma, radius=radius))
    assert (bits(got[..., :3]) == bits(rgb)).all()
    assert got[0, 0, 3] == 9.0  # tl = 7 + 2: the pixel had history
    assert (bits(box[..., :3]) == bits(rgb)).all() and (bits(box[..., 3:]) == bits(rgb)).all()
    plain = HR.resolve(rgb, n, rec, cam, prgbl, rec)
    assert plain[0, 0, 3] == 9.0 and (bits(plain[..., :3]) != bits(rgb)).any()


@pytest.mark.parametrize("pair", ["identity", "translated", "rotated"])
def test_the_clamp_binds_on_a_share_of_the_pixels(pair):
    """70 x 50, gamma = 1, radius = 1: among the pixels with history the clamp
    changes some channel of more than a tenth and fewer than nine tenths."""
    w, h = 70, 50
    pcam, ccam = PAIRS[pair]
    rgb, n, prgbl = inputs(w, h, 7)
    prec, rec = view(pcam, w, h), view(ccam, w, h)
    plain = HR.resolve(rgb, n, rec, pcam, prgbl, prec)
    got, box = CR.resolve(rgb, n, rec, pcam, prgbl, prec, clamp=dict(gamma=1.0, radius=1))
    has = plain[..., 3] > n.astype(F)
    assert has.sum() > 500
    assert (bits(got[..., 3]) == bits(plain[..., 3])).all()          # len is the parent's
    assert (bits(got[~has]) == bits(plain[~has])).all()              # no history: untouched
    changed = (bits(got[..., :3]) != bits(plain[..., :3])).any(axis=2)
    share = float(changed[has].mean())
    print(f"clamp share {pair}: {share:.3f} of {int(has.sum())} pixels with history")
    assert 0.1 < share < 0.9
    assert (box[..., :3] <= box[..., 3:]).all()
