"""Dense stereo without a GPU (include/erp_match.h "dense stereo on row-rectified views"): the
new symbols and defaults, and the numpy restatement's own known answers (tests/stereo_ref.py is
the oracle of tests/test_gpu_stereo.py, so it is checked here against facts that do not come
from it)."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_ref as SR  # noqa: E402


def shifted_pair(seed: int, rows: int, cols: int, d0: int):
    """left: iid uint8 noise; right: left shifted by d0, right[y, x - d0] = left[y, x], the
    columns shifted in filled with noise"""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    right = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    x = np.arange(cols)
    ok = (x - d0 >= 0) & (x - d0 < cols)
    right[:, x[ok] - d0] = left[:, x[ok]]
    return left, right


def shift_zone(cols: int, d0: int) -> np.ndarray:
    """the columns whose 9-wide census window lies inside both images, so that the true
    disparity has cost 0: 4 <= x - d0 and x <= cols - 5 for d0 >= 0, and the mirrored pair of
    conditions for d0 < 0"""
    x = np.arange(cols)
    return (x - d0 >= 4) & (x <= cols - 5) & (x >= 4) & (x - d0 <= cols - 5)


# (d0, d_min, n_disp): d0 positive from d_min = 0, the same through a negative d_min, and a
# negative d0, which only a negative d_min reaches
SHIFT_CASES = [(5, 0, 32), (3, -6, 16), (-3, -6, 16)]


def test_symbols_and_defaults():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    L = capi.load()
    for name in ("erp_stereo_params_default", "erp_stereo_rows_dev"):
        assert name in capi.EXPORTED and hasattr(L, name)
    p = capi.StereoParams(-1, -1, -1, -1, -5, -1, -1)
    L.erp_stereo_params_default(C.byref(p))
    assert (p.d_min, p.n_disp, p.p1, p.p2, p.lr_max, p.wrap_rows, p.channels) == \
        (0, 64, 8, 64, 1, 0, 3)
    assert C.sizeof(capi.StereoParams) == 28 and capi.STEREO_INVALID == SR.INVALID == -32768
    assert capi.OPTIONS["stereo_chunk_mb"] == 17
    assert L.erp_abi_version() == 2
    # the argument checks come before anything touches a device
    assert L.erp_stereo_rows_dev(None, None, None, 1, 4, 4, C.byref(p), None, None, None) == 1
    src = open(os.path.join(_build.ROOT, "include", "erp_match.h")).read()
    assert "#define ERP_STEREO_INVALID (-32768)" in src and "nobody has tuned" in src


@pytest.mark.parametrize("d0,d_min,D", SHIFT_CASES)
@pytest.mark.parametrize("wrap", [0, 1])
def test_constant_shift_known_answer(d0, d_min, D, wrap):
    """in the zone the true d costs 0 on every path while every other d costs a Binomial(62,
    1/2) draw per pixel, so d* = d0, the left-right check passes and, by rule 5, the parabola
    offset stays within half a pixel.  (S itself need not be 0 at the zone's first pixels: a
    path that enters the zone carries L(q, d0) - m over from the border pixel before it.)"""
    rows, cols = 24, 96
    left, right = shifted_pair(11 + d0, rows, cols, d0)
    disp16, depth, parts = SR.disparity(left, right, d_min=d_min, n_disp=D, wrap_rows=wrap,
                                        parts=True)
    zone = shift_zone(cols, d0)
    assert zone.sum() >= cols - 8 - abs(d0) - 1
    assert (parts["dstar"][:, zone] == d0 - d_min).all()
    assert (disp16[:, zone] != SR.INVALID).all()
    assert (np.abs(disp16[:, zone].astype(np.int32) - 16 * d0) <= 8).all()
    # the carried L(q, d0) - m shrinks by the smallest other L at every step inside the zone (at
    # least the smallest other cost, about 12 of 62 bits on noise) and starts below 63 + p2 = 127:
    # 8 columns inside the zone it is gone on both horizontal paths, and S is 0 at the true d only
    zx = np.nonzero(zone)[0]
    inner = np.zeros(cols, bool)
    inner[zx[8]:zx[-8]] = True
    S = parts["S"][:, inner]
    assert (S[:, :, d0 - d_min] == 0).all()
    assert (np.delete(S, d0 - d_min, axis=2) > 0).all()
    assert np.isnan(depth[disp16 == SR.INVALID]).all()


def test_restatement_edges():
    """rows below the census height wrap correctly; the floor division floors; uint16 holds S"""
    g = np.arange(15, dtype=np.int32).reshape(3, 5) * 7 % 11
    w = SR.census(g, 1)
    # bit 0 is the neighbour (dy, dx) = (-3, -4): row (y - 3) % 3 = y, column clamped
    for y in range(3):
        for x in range(5):
            assert int(w[y, x]) & 1 == int(g[y, max(x - 4, 0)] < g[y, x])
    c = SR.census(g, 0)
    assert int(c[0, 0]) & 1 == 0  # clamped onto the pixel itself: never smaller
    S = np.array([[[9, 4, 5, 9], [7, 7, 7, 7], [9, 5, 4, 4]]], np.uint16)
    ds, disp = SR.winner(S, -2)
    assert ds.tolist() == [[1, 0, 2]]
    # a = 9, b = 5, c = 4: den = 6, off = floor((64 + 6) / 12) = 5; flat: 0; a = 5, b = 4, c = 4:
    # den = 1, off = floor((16 + 1) / 2) = 8
    assert disp.tolist() == [[16 * (-2 + 1) + 5, 16 * -2, 16 * (-2 + 2) + 8]]
    ds, disp = SR.winner(np.array([[[9, 4, 9, 3, 8]]], np.uint16), 0)
    # a = 9, b = 8, c = 3: floor((16 + 11) / 22) = 1
    assert disp.tolist() == [[16 * 3 + 1]]
    # a = 5, b = 9, c = 3: den = 8, floor((-64 + 8) / 16) = floor(-3.5) = -4, not -3
    ds, disp = SR.winner(np.array([[[9, 5, 3, 9, 9]]], np.uint16), 0)
    assert disp.tolist() == [[32 - 4]]
    rng = np.random.default_rng(0)
    cst = rng.integers(0, 64, (5, 6, 16)).astype(np.int32)
    assert SR.aggregate(cst, 255, 255).max() <= 4 * (63 + 255)


def test_depth_rule_against_triangulation():
    """rule 7 against a direct intersection of the two rays in a pole-to-pole frame: the left
    centre at the origin, the right centre one baseline along the pole axis, on the side the
    disparity's sign implies; angles are measured from the x = 0 pole"""
    cols = 180
    x = np.arange(1, cols)[None, :].repeat(6, 0)
    disp16 = np.array([-40, -7, 3, 16, 50, 200])[:, None].repeat(cols - 1, 1)
    full = np.zeros((6, cols), np.int16)
    full[:, 1:] = disp16
    z = SR.depth_of(full)[:, 1:]
    thL = np.pi * x / cols
    thR = np.pi * (x - disp16 / 16.0) / cols
    ok = (thR > 1e-3) & (thR < np.pi - 1e-3)
    assert ok.sum() > 900
    s = np.where(thR > thL, 1.0, -1.0)  # the right centre: (s, 0) in (axis, perpendicular)
    # rho (cos thL, sin thL) = (s, 0) + mu (cos thR, sin thR)
    rho = np.empty_like(thL)
    for idx in zip(*np.nonzero(ok)):
        A = np.array([[np.cos(thL[idx]), -np.cos(thR[idx])], [np.sin(thL[idx]), -np.sin(thR[idx])]])
        rho[idx], mu = np.linalg.solve(A, np.array([s[idx], 0.0]))
        assert mu > 0 and rho[idx] > 0
    assert np.allclose(z[ok], rho[ok], rtol=1e-9, atol=0)
    # disp16 == 0: +inf; invalid: NaN
    e = SR.depth_of(np.array([[0, SR.INVALID, 16]], np.int16))
    assert np.isposinf(e[0, 0]) and np.isnan(e[0, 1]) and np.isfinite(e[0, 2])
