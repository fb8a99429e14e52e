"""Eight-path SGM and the uniqueness test without a GPU (include/erp_match.h rules 4b and 6b):
the extended struct's defaults, and the numpy restatement's own known answers
(tests/stereo8_ref.py is the oracle of tests/test_gpu_stereo8.py, so it is checked here against
facts that do not come from it)."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo8_ref as S8  # noqa: E402
import stereo_ref as SR  # noqa: E402
from test_stereo_host import shift_zone, shifted_pair  # noqa: E402


def test_symbols_and_defaults():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    L = capi.load()
    for name in ("erp_stereo_params_ex_default", "erp_stereo_rows_ex_dev"):
        assert name in capi.EXPORTED and hasattr(L, name)
    p = capi.StereoParamsEx(capi.StereoParams(-1, -1, -1, -1, -5, -1, -1), -1, -1, (7, 7))
    L.erp_stereo_params_ex_default(C.byref(p))
    b = p.base
    assert (b.d_min, b.n_disp, b.p1, b.p2, b.lr_max, b.wrap_rows, b.channels) == \
        (0, 64, 8, 64, 1, 0, 3)
    assert (p.n_paths, p.uniqueness, tuple(p.reserved)) == (4, 0, (0, 0))
    # additive: the old struct keeps its bytes, the extension starts with it; the ABI stays 2
    assert C.sizeof(capi.StereoParams) == 28 and C.sizeof(capi.StereoParamsEx) == 44
    assert capi.StereoParamsEx.base.offset == 0 and capi.StereoParamsEx.n_paths.offset == 28
    assert L.erp_abi_version() == 2
    L.erp_stereo_params_ex_default(None)
    # the argument checks come before anything touches a device
    assert L.erp_stereo_rows_ex_dev(None, None, None, 1, 4, 4, C.byref(p), None, None, None) == 1
    assert "stereo_ex" in _build.DRIVERS
    src = open(os.path.join(_build.ROOT, "include", "erp_match.h")).read()
    assert "4b. The diagonal paths" in src and "6b. Uniqueness" in src


@pytest.mark.parametrize("wrap", [0, 1])
def test_constant_shift_known_answer(wrap):
    """test_stereo_host's known answer with eight paths, 24 x 96, D = 32, d0 = 5: in the zone the
    true d costs 0 on every path, the diagonals included (the right image is the left one
    shifted along its rows, so the census words agree in every row, wrapped or clamped), hence
    d* = d0, the pixel is valid and the parabola offset stays within half a pixel.  The zone's
    pixels are also unique at 5, 15 and 30 %: away from the zone's first columns S(d0) is 0 and
    rule 6b compares 0 with something positive; at those columns the carried L is small against
    the eight-path sums of the other d."""
    rows, cols, D, d0 = 24, 96, 32, 5
    left, right = shifted_pair(11 + d0, rows, cols, d0)
    disp16, depth, parts = S8.disparity(left, right, n_disp=D, wrap_rows=wrap, n_paths=8,
                                        parts=True)
    zone = shift_zone(cols, d0)
    assert zone.sum() >= cols - 8 - d0 - 1
    assert (parts["dstar"][:, zone] == d0).all()
    assert (disp16[:, zone] != SR.INVALID).all()
    dev = np.abs(disp16[:, zone].astype(np.int32) - 16 * d0)
    print(f"wrap {wrap}: max |disp16 - 16 d0| in the zone = {dev.max()}")
    assert (dev <= 8).all()
    assert parts["S"].max() <= 8 * (63 + 64)
    # eight paths are not four: the sums differ
    S4 = SR.aggregate(SR.cost(SR.census(SR.gray(left), wrap), SR.census(SR.gray(right), wrap), 0, D),
                      8, 64)
    assert (parts["S"] != S4).mean() > 0.5
    for u in (5, 15, 30):
        du, _ = S8.disparity(left, right, n_disp=D, wrap_rows=wrap, n_paths=8, uniqueness=u)
        assert (du[:, zone] != SR.INVALID).all(), u
        # the rule only ever rejects, and what it keeps is unchanged
        assert ((du == disp16) | (du == SR.INVALID)).all()
    # on noise outside the zone a strict ratio does reject something
    d99, _ = S8.disparity(left, right, n_disp=D, wrap_rows=wrap, n_paths=8, uniqueness=99)
    assert (d99 == SR.INVALID).sum() > (disp16 == SR.INVALID).sum()


def test_one_row_wrapped_diagonals_are_the_row_paths():
    """rows = 1, wrap_rows = 1: every diagonal's previous pixel is (0, x -+ 1), the row path's, so
    S = the four-path S plus twice the two row paths' sum"""
    rng = np.random.default_rng(3)
    c = rng.integers(0, 64, (1, 37, 16)).astype(np.int32)
    S8_ = S8.aggregate(c, 8, 64, 1).astype(np.int32)
    S4 = SR.aggregate(c, 8, 64).astype(np.int32)
    ch = c.transpose(1, 0, 2)
    H = (SR._path(ch, 8, 64) + SR._path(ch[::-1], 8, 64)[::-1]).transpose(1, 0, 2)
    assert (S8_ == S4 + 2 * H).all()
    # without the wrap every pixel of the one row is a first pixel: L = c on all four diagonals
    assert (S8.aggregate(c, 8, 64, 0).astype(np.int32) == S4 + 4 * c).all()


# D = 2, p1 = 1, p2 = 10, c(., 0) = 0 and c(., 1) = V: L_r(., 0) stays 0 (m = 0), and rule 4 becomes
# L_r(p, 1) = V(p) + min(L_r(q, 1), 1): V(p) on a first pixel, V(p) + 1 behind a pixel with
# L_r >= 1, V(p) behind one with L_r = 0.  The expected L_r(., 1) below are worked out by hand from
# that, path by path; the entries that the wrap changes lie on the seam (row 0 or row 2).
V = [[0, 2, 0],
     [3, 0, 0],
     [0, 0, 5]]
HAND = {  # (dy, dx): (wrap_rows = 0, wrap_rows = 1)
    (1, 1): ([[0, 2, 0], [3, 0, 1], [0, 1, 5]],    # first: column 0, and row 0 without the wrap
             [[0, 2, 1], [3, 0, 1], [0, 1, 5]]),   # (0,2) <- (2,1) = 1 across the seam
    (-1, -1): ([[1, 2, 0], [3, 1, 0], [0, 0, 5]],  # first: column 2, and row 2
               [[1, 2, 0], [3, 1, 0], [1, 0, 5]]),  # (2,0) <- (0,1) = 2
    (1, -1): ([[0, 2, 0], [4, 0, 0], [0, 0, 5]],   # first: column 2, and row 0
              [[0, 3, 0], [4, 0, 0], [0, 0, 5]]),  # (0,1) <- (2,2) = 5
    (-1, 1): ([[0, 3, 0], [3, 0, 0], [0, 0, 5]],   # first: column 0, and row 2
              [[0, 3, 0], [3, 0, 0], [0, 0, 6]]),  # (2,2) <- (0,1) = 3
}


@pytest.mark.parametrize("step", list(HAND))
def test_diagonals_by_hand(step):
    c = np.zeros((3, 3, 2), np.int32)
    c[:, :, 1] = V
    for wrap in (0, 1):
        L = S8.diag_path(c, 1, 10, step[0], step[1], wrap)
        assert (L[:, :, 0] == 0).all()
        assert L[:, :, 1].tolist() == HAND[step][wrap], (step, wrap)
    assert S8.DIAGONALS == list(HAND)


def _literal_path(c, p1, p2, dy, dx, wrap):
    """rule 4b pixel by pixel, as the header words it (no vectorisation, no column order)"""
    rows, cols, D = c.shape
    memo = {}

    def L(y, x):
        if (y, x) in memo:
            return memo[(y, x)]
        qy, qx = y - dy, x - dx
        first = qx < 0 or qx >= cols
        if qy < 0 or qy >= rows:
            if wrap:
                qy %= rows
            else:
                first = True
        if first:
            out = [int(v) for v in c[y, x]]
        else:
            q = L(qy, qx)
            m = min(q)
            out = []
            for d in range(D):
                cand = [q[d], m + p2]
                if d > 0:
                    cand.append(q[d - 1] + p1)
                if d < D - 1:
                    cand.append(q[d + 1] + p1)
                out.append(int(c[y, x, d]) + min(cand) - m)
        memo[(y, x)] = out
        return out
    return np.array([[L(y, x) for x in range(cols)] for y in range(rows)], np.int32)


@pytest.mark.parametrize("rows,cols", [(3, 3), (1, 5), (2, 7), (7, 2), (5, 4)])
def test_diagonals_against_the_literal_rule(rows, cols):
    """rows < cols: a wrapped line crosses the seam more than once"""
    rng = np.random.default_rng(rows * 10 + cols)
    c = rng.integers(0, 64, (rows, cols, 5)).astype(np.int32)
    for dy, dx in S8.DIAGONALS:
        for wrap in (0, 1):
            assert (S8.diag_path(c, 3, 20, dy, dx, wrap) ==
                    _literal_path(c, 3, 20, dy, dx, wrap)).all(), (dy, dx, wrap)
    assert S8.aggregate(c, 255, 255, 1).max() <= 8 * (63 + 255)


def test_uniqueness_by_hand():
    """rule 6b at 20 %: a pixel falls when some d more than 1 away has S(d) * 80 < S(d*) * 100"""
    cases = [
        # (S over d, d*, unique at 20 %)
        ([100, 50, 40, 45, 100, 100], 2, True),   # 50 and 45 are d* - 1 and d* + 1: left out
        ([49, 100, 40, 100, 100, 100], 2, False),  # 49 * 80 = 3920 < 4000
        ([50, 100, 40, 100, 100, 100], 2, True),   # 50 * 80 = 4000: not below
        ([40, 100, 100, 40, 100, 100], 0, False),  # a tie: the first argmin wins, the other one rejects it
        ([0, 9, 9, 0, 9, 9], 0, True),             # a tie at 0: 0 < 0 is false
        ([40, 41, 100, 100, 100, 100], 0, True),   # d* = 0: only d = 1 is close, and it is left out
        ([40, 100, 41, 100, 100, 100], 0, False),  # d* = 0: d = 2 counts
        ([100, 100, 100, 100, 41, 40], 5, True),   # d* = D - 1: d = D - 2 is left out
        ([100, 100, 100, 41, 100, 40], 5, False),  # d* = D - 1: d = D - 3 counts
    ]
    S = np.array([[c[0] for c in cases]], np.uint16)
    ds, _ = SR.winner(S, 0)
    assert ds[0].tolist() == [c[1] for c in cases]
    assert S8.unique(S, ds, 20)[0].tolist() == [c[2] for c in cases]
    # 99 %: S(d) * 1 < S(d*) * 100; 199 < 200 rejects, 200 does not
    S = np.array([[[2, 300, 199, 300], [2, 300, 200, 300], [2, 150, 300, 300]]], np.uint16)
    ds, _ = SR.winner(S, 0)
    assert S8.unique(S, ds, 99)[0].tolist() == [False, True, True]
    # the largest sums fit the products: 2544 * 100
    S = np.full((1, 1, 16), 2544, np.uint16)
    assert not S8.unique(S, SR.winner(S, 0)[0], 1)[0, 0]


def test_defaults_are_the_four_path_restatement():
    left, right = shifted_pair(2, 9, 40, 3)
    for wrap in (0, 1):
        a = SR.disparity(left, right, n_disp=16, wrap_rows=wrap)[0]
        b = S8.disparity(left, right, n_disp=16, wrap_rows=wrap)[0]
        assert a.tobytes() == b.tobytes()
