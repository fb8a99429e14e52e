"""numpy restatement of the dense-stereo rules 4b (the diagonal paths) and 6b (uniqueness) on
top of tests/stereo_ref.py (include/erp_match.h "dense stereo on row-rectified views"), the
oracle of tests/test_stereo8_host.py and tests/test_gpu_stereo8.py.  A diagonal path is a loop
over the columns, vectorised over rows and d: the previous pixels of a column are the column
before it, shifted by one row."""
from __future__ import annotations

import numpy as np

import stereo_ref as SR

INVALID, BIG = SR.INVALID, SR.BIG
DIAGONALS = [(1, 1), (-1, -1), (1, -1), (-1, 1)]  # (dy, dx), the header's order


def diag_path(c: np.ndarray, p1: int, p2: int, dy: int, dx: int, wrap_rows: int) -> np.ndarray:
    """rule 4b: L_r of the path with the step (dy, dx) on c [rows, cols, D] -> [rows, cols, D]"""
    rows, cols, D = c.shape
    L = np.empty_like(c)
    xs = range(cols) if dx > 0 else range(cols - 1, -1, -1)
    pad = np.full((rows, 1), BIG, np.int32)
    y = np.arange(rows)
    for i, x in enumerate(xs):
        if i == 0:  # q's column is outside the image
            L[:, x] = c[:, x]
            continue
        yq = y - dy  # q = (y - dy, x - dx)
        first = (yq < 0) | (yq >= rows)
        q = L[yq % rows, x - dx]
        m = q.min(-1, keepdims=True)
        lo = np.concatenate([pad, q[:, :-1]], -1) + p1
        hi = np.concatenate([q[:, 1:], pad], -1) + p1
        n = c[:, x] + np.minimum(np.minimum(q, lo), np.minimum(hi, m + p2)) - m
        if not wrap_rows:
            n[first] = c[first, x]
        L[:, x] = n
    return L


def aggregate(c: np.ndarray, p1: int, p2: int, wrap_rows: int, n_paths: int = 8) -> np.ndarray:
    """rules 4 and 4b -> S uint16 [rows, cols, D]"""
    S = SR.aggregate(c, p1, p2).astype(np.int32)
    if n_paths == 8:
        for dy, dx in DIAGONALS:
            S += diag_path(c, p1, p2, dy, dx, wrap_rows)
        assert S.max() <= 8 * (63 + p2)
    else:
        assert n_paths == 4
    return S.astype(np.uint16)


def unique(S: np.ndarray, ds: np.ndarray, uniqueness: int) -> np.ndarray:
    """rule 6b -> bool [rows, cols], False where the rule rejects the pixel"""
    Si = S.astype(np.int64)
    far = np.abs(np.arange(S.shape[2])[None, None, :] - ds[..., None]) > 1
    best = np.take_along_axis(Si, ds[..., None].astype(np.int64), -1)
    return ~(far & (Si * (100 - uniqueness) < best * 100)).any(-1)


def disparity(left: np.ndarray, right: np.ndarray, *, d_min: int = 0, n_disp: int = 64,
              p1: int = 8, p2: int = 64, lr_max: int = 1, wrap_rows: int = 0, n_paths: int = 4,
              uniqueness: int = 0, parts: bool = False):
    """stereo_ref.disparity with the two new parameters"""
    D = n_disp
    cl, cr = SR.census(SR.gray(left), wrap_rows), SR.census(SR.gray(right), wrap_rows)
    S = aggregate(SR.cost(cl, cr, d_min, D), p1, p2, wrap_rows, n_paths)
    ds, disp = SR.winner(S, d_min)
    dr = SR.right_disparity(S, d_min)
    cols = ds.shape[1]
    xr = np.arange(cols)[None, :] - d_min - ds
    valid = (xr >= 0) & (xr < cols)
    if lr_max >= 0:
        back = np.take_along_axis(dr, np.clip(xr, 0, cols - 1), 1)
        valid &= np.abs(ds - back) <= lr_max
    if uniqueness > 0:
        valid &= unique(S, ds, uniqueness)
    disp16 = np.where(valid, disp, INVALID).astype(np.int16)
    out = (disp16, SR.depth_of(disp16))
    return out + ({"S": S, "dstar": ds, "dright": dr},) if parts else out
