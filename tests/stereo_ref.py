"""numpy restatement of the dense-stereo rules 1-7 (include/erp_match.h "dense stereo on
row-rectified views"), the oracle of tests/test_stereo_host.py and tests/test_gpu_stereo.py.
Integer arithmetic throughout except the depth; vectorised over rows and d, so the test shapes
take milliseconds."""
from __future__ import annotations

import numpy as np

INVALID = -32768
BIG = 1 << 20  # stands for a neighbour d-1 / d+1 outside [0, D): never the minimum


def gray(im: np.ndarray) -> np.ndarray:
    """rule 1: [rows, cols] or [rows, cols, 1] bytes as they are, [rows, cols, 3] (b, g, r)"""
    if im.ndim == 2:
        return im.astype(np.int32)
    if im.shape[2] == 1:
        return im[:, :, 0].astype(np.int32)
    b, g, r = (im[:, :, k].astype(np.int32) for k in range(3))
    return (b * 1868 + g * 9617 + r * 4899 + 8192) >> 14


def census(g: np.ndarray, wrap_rows: int) -> np.ndarray:
    """rule 2 -> uint64 [rows, cols]"""
    rows, cols = g.shape
    ys, xs = np.arange(rows), np.arange(cols)
    out = np.zeros((rows, cols), np.uint64)
    k = 0
    for dy in range(-3, 4):
        yy = (ys + dy) % rows if wrap_rows else np.clip(ys + dy, 0, rows - 1)
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            xx = np.clip(xs + dx, 0, cols - 1)
            out |= (g[yy][:, xx] < g).astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == 62
    return out


def _popcount(v: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(v).view(np.uint8).reshape(v.shape + (8,)),
                         axis=-1).sum(-1).astype(np.int32)


def cost(cen_l: np.ndarray, cen_r: np.ndarray, d_min: int, D: int) -> np.ndarray:
    """rule 3 -> int32 [rows, cols, D]"""
    rows, cols = cen_l.shape
    c = np.full((rows, cols, D), 63, np.int32)
    x = np.arange(cols)
    for d in range(D):
        xr = x - d_min - d
        ok = (xr >= 0) & (xr < cols)
        if ok.any():
            c[:, ok, d] = _popcount(cen_l[:, ok] ^ cen_r[:, xr[ok]])
    return c


def _path(c: np.ndarray, p1: int, p2: int) -> np.ndarray:
    """rule 4 along axis 0 of c [len, lines, D], forwards"""
    L = np.empty_like(c)
    L[0] = c[0]
    pad = np.full(c.shape[1:2] + (1,), BIG, np.int32)
    for i in range(1, c.shape[0]):
        q = L[i - 1]
        m = q.min(-1, keepdims=True)
        lo = np.concatenate([pad, q[:, :-1]], -1) + p1
        hi = np.concatenate([q[:, 1:], pad], -1) + p1
        L[i] = c[i] + np.minimum(np.minimum(q, lo), np.minimum(hi, m + p2)) - m
    return L


def aggregate(c: np.ndarray, p1: int, p2: int) -> np.ndarray:
    """rule 4 -> S uint16 [rows, cols, D]"""
    ch = c.transpose(1, 0, 2)  # [cols, rows, D]: a step along x
    S = _path(ch, p1, p2) + _path(ch[::-1], p1, p2)[::-1]
    S = S.transpose(1, 0, 2) + _path(c, p1, p2) + _path(c[::-1], p1, p2)[::-1]
    assert S.max() <= 4 * (63 + p2)
    return S.astype(np.uint16)


def winner(S: np.ndarray, d_min: int):
    """rule 5 -> (d* int32 [rows, cols], raw disp16 int32 [rows, cols])"""
    D = S.shape[2]
    Si = S.astype(np.int64)
    ds = Si.argmin(-1)  # the first minimum
    c = np.take_along_axis(Si, ds[..., None], -1)[..., 0]
    a = np.take_along_axis(Si, np.clip(ds - 1, 0, D - 1)[..., None], -1)[..., 0]
    b = np.take_along_axis(Si, np.clip(ds + 1, 0, D - 1)[..., None], -1)[..., 0]
    den = a + b - 2 * c
    use = (ds > 0) & (ds < D - 1) & (den > 0)
    off = np.where(use, ((a - b) * 16 + den) // np.where(use, 2 * den, 1), 0)  # // floors
    return ds.astype(np.int32), (16 * (d_min + ds) + off).astype(np.int32)


def right_disparity(S: np.ndarray, d_min: int) -> np.ndarray:
    """rule 6's dR -> int32 [rows, cols], -1 where no d has its column in range"""
    rows, cols, D = S.shape
    xr = np.arange(cols)[:, None]
    d = np.arange(D)[None, :]
    col = xr + d_min + d
    ok = (col >= 0) & (col < cols)
    v = np.where(ok[None], S[:, np.clip(col, 0, cols - 1), d].astype(np.int64), 1 << 30)
    return np.where(ok.any(-1)[None], v.argmin(-1), -1).astype(np.int32)


def depth_of(disp16: np.ndarray) -> np.ndarray:
    """rule 7 -> float64 [rows, cols] before the rounding to float (disp16 after the check)"""
    rows, cols = disp16.shape
    x = np.broadcast_to(np.arange(cols, dtype=np.float64), (rows, cols))
    d = disp16.astype(np.float64)
    thL = np.pi * x / cols
    thR = np.pi * (x - d / 16.0) / cols
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.sin(thR) / np.abs(np.sin(thL - thR))
    z = np.where(disp16 == 0, np.inf, z)
    return np.where(disp16 == INVALID, np.nan, z)


def disparity(left: np.ndarray, right: np.ndarray, *, d_min: int = 0, n_disp: int = 64,
              p1: int = 8, p2: int = 64, lr_max: int = 1, wrap_rows: int = 0, parts: bool = False):
    """one pair -> (disp16 int16 [rows, cols], depth float64 [rows, cols]); with ``parts`` also
    a dict of the intermediate S, d*, dR"""
    D = n_disp
    cl, cr = census(gray(left), wrap_rows), census(gray(right), wrap_rows)
    S = aggregate(cost(cl, cr, d_min, D), p1, p2)
    ds, disp = winner(S, d_min)
    dr = right_disparity(S, d_min)
    rows, cols = ds.shape
    xr = np.arange(cols)[None, :] - d_min - ds
    valid = (xr >= 0) & (xr < cols)
    if lr_max >= 0:
        back = np.take_along_axis(dr, np.clip(xr, 0, cols - 1), 1)
        valid &= np.abs(ds - back) <= lr_max
    disp16 = np.where(valid, disp, INVALID).astype(np.int16)
    out = (disp16, depth_of(disp16))
    return out + ({"S": S, "dstar": ds, "dright": dr},) if parts else out
