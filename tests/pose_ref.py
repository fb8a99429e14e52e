"""The reference chain of the pose selection (include/erp_match.h "pose selection") in numpy:
the candidates from numpy.linalg.svd of oracle.rank2(e) with decompose_e's det fixes and W, the
bearings from oracle.pixel_to_bearing, the rules as the header states them (fp64, products and
sums left to right).  Shared by tests/test_pose_host.py and tests/test_gpu_pose.py; nothing here
is modified after it is computed.

The model: E' = [t]x R with the residual l^T E' r, so  d_l * l = d_r * (Rc r) + tc.  A scene
built as synth does (r ~ R_gt^T (d_l l) + t_gt) therefore has Rc = R_gt and tc = -R_gt t_gt."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polish_ref as PR  # noqa: E402

from erp_match_eightpoint_test_amd import synth  # noqa: E402

EPS = 2.0 ** -53
DEPTH_K = 256.0        # |dd| <= DEPTH_K * EPS * (1 + |d|) / det  (the derived bound)
DET_BAND = 64.0 * EPS  # a det this near min_sin2 (or 0) would make the voter test ambiguous
CAND_TOL = 1e-9        # two SVD routines on one 3x3: the candidates as a set
W_REF, H_REF = 5376, 2688
# (euler_gt, M, seed): the known-answer scenes
SCENES = [((0.1, 0.2, 0.05), 9, 1), ((0.1, -0.2, 0.05), 64, 2), ((0.2, 0.1, 2.0), 65, 3),
          ((-2.5, 0.3, 1.0), 257, 4), ((0.0, 0.0, 0.0), 63, 6)]
_scenes: dict = {}


def candidates(oracle, e):
    """(E' as 9 doubles, R1, R2, t) of a solved 9-vector: cv::decomposeEssentialMat's steps on
    numpy's SVD of E'"""
    Ec = oracle.rank2(e)
    U, _, Vt = np.linalg.svd(Ec.reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    Wm = np.array([[0.0, 1, 0], [-1, 0, 0], [0, 0, 1]])
    return Ec, U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, 2].copy()


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def depths(bl, br, Rc, t):
    """(d_l, d_r, det) of every match under (Rc, +t): rule 2, left to right"""
    Rc = np.asarray(Rc, np.float64).reshape(3, 3)
    q = np.stack([Rc[i, 0] * br[:, 0] + Rc[i, 1] * br[:, 1] + Rc[i, 2] * br[:, 2]
                  for i in range(3)], 1)
    tt = np.broadcast_to(np.asarray(t, np.float64), bl.shape)
    a, b, c, lt, qt = _dot(bl, bl), _dot(bl, q), _dot(q, q), _dot(bl, tt), _dot(q, tt)
    det = a * c - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c * lt - b * qt) / det, (b * lt - a * qt) / det, det


def select(oracle, bl, br, Ec, R1, R2, t, mask=None, thr: float = 0.0, min_sin2: float = 0.0,
           slack=(0.0, 0.0)):
    """rules 3 - 6 on given candidates -> dict(votes [4], n_voters, which, t_sign (+1 / -1; 0
    without voters), Rm, t, depth [M, 2], front [M] uint8, ambiguous: the matches whose vote or
    voter test is within rounding of a boundary).  slack[w]: how far rotation w's entries may be
    from the ones the code under test used (a record carries only the selected matrix; the other
    one is then the chain's own, up to CAND_TOL away): it widens that rotation's ambiguity bands
    (d and det move by at most 8 x slack x (1 + |d|) / det and 8 x slack)."""
    M = len(bl)
    ok = np.ones(M, bool) if mask is None else np.asarray(mask[:M]) != 0
    amb = np.zeros(M, bool)
    if thr > 0:
        cnt = np.array([oracle.inlier_count(bl[i:i + 1], br[i:i + 1], Ec, PR.thr64(thr),
                                            PR.AMBIGUOUS) for i in range(M)]).reshape(M, 2)
        amb |= ok & (cnt[:, 1] != 0)
        ok &= cnt[:, 0] == 1
    votes, per = np.zeros(4, np.int64), []
    voter_any = np.zeros(M, bool)
    for w, Rc in enumerate((R1, R2)):
        dl, dr, det = depths(bl, br, Rc, t)
        par = ok & (det > 0) & (det >= min_sin2)
        band = DET_BAND + 8 * slack[w]
        amb |= ok & ((np.abs(det - min_sin2) <= band) | (np.abs(det) <= band))
        with np.errstate(invalid="ignore"):
            bound = ((DEPTH_K * EPS + 8 * slack[w])
                     * (1 + np.maximum(np.abs(dl), np.abs(dr))) / det)
            amb |= par & ((np.abs(dl) <= bound) | (np.abs(dr) <= bound))
        plus, minus = par & (dl > 0) & (dr > 0), par & (dl < 0) & (dr < 0)
        votes[2 * w], votes[2 * w + 1] = plus.sum(), minus.sum()
        voter_any |= par
        per.append((dl, dr, det, par, plus, minus))
    out = {"votes": votes, "n_voters": int(voter_any.sum()), "ambiguous": int(amb.sum())}
    if out["n_voters"] == 0:
        out.update(which=0, t_sign=0, Rm=np.zeros((3, 3)), t=np.zeros(3),
                   depth=np.zeros((M, 2)), front=np.zeros(M, np.uint8), det=np.zeros(M))
        return out
    k = int(np.argmax(votes))  # (argmax: the first of equal counts, the lowest k)
    which, s = k >> 1, k & 1
    dl, dr, det, par, plus, minus = per[which]
    sg = -1.0 if s else 1.0
    depth = np.zeros((M, 2))
    depth[par, 0], depth[par, 1] = sg * dl[par], sg * dr[par]
    out.update(which=which, t_sign=-1 if s else 1, Rm=np.asarray((R1, R2)[which], np.float64),
               t=sg * np.asarray(t, np.float64), depth=depth,
               front=(minus if s else plus).astype(np.uint8), det=np.where(par, det, 0.0))
    return out


def flags(oracle, sel, res_R, res_T):
    """(R float, T float, rot_agrees, t_flipped) of a selection against a result record's R, T"""
    R = oracle.rot2eular(sel["Rm"]).astype(np.float32)
    T = sel["t"].astype(np.float32)
    res_R, res_T = np.asarray(res_R, np.float32), np.asarray(res_T, np.float32)
    dot = float(T[0]) * float(res_T[0])
    dot = dot + float(T[1]) * float(res_T[1])
    dot = dot + float(T[2]) * float(res_T[2])
    return R, T, int(R.tobytes() == res_R.tobytes()), int(dot < 0)


def reference_valid(oracle, Rm, valid_abs: float = 1.57) -> bool:
    """the reference's validity rule (src/eight_point.cpp:70-84): every float Euler angle of the
    rotation under valid_abs in magnitude"""
    return bool(np.abs(oracle.rot2eular(Rm).astype(np.float32)).max() < valid_abs)


def scene(oracle, euler, M: int, seed: int) -> dict:
    """a clean scene as synth builds them (left bearings uniform, depths U[2, 10], unit t_gt,
    fractional pixels) with e from oracle.eight_point_estimation on all matches"""
    key = (tuple(euler), M, seed)
    if key in _scenes:
        return _scenes[key]
    rng = np.random.default_rng(seed)
    R = synth.eular2rot(euler)
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    l = rng.standard_normal((M, 3))
    l /= np.linalg.norm(l, axis=1, keepdims=True)
    d_l = rng.uniform(2.0, 10.0, M)
    Xr = (l * d_l[:, None]) @ R + t
    kl = synth.bearing_to_pixel(l, W_REF, H_REF).astype(np.float32)
    kr = synth.bearing_to_pixel(Xr, W_REF, H_REF).astype(np.float32)
    bl = oracle.pixel_to_bearing(W_REF, H_REF, kl)
    br = oracle.pixel_to_bearing(W_REF, H_REF, kr)
    est = oracle.eight_point_estimation(bl, br)
    out = {"R_gt": R, "t_gt": t, "tc_gt": -R @ t, "d_l": d_l, "d_r": np.linalg.norm(Xr, axis=1),
           "kl": kl, "kr": kr, "bl": bl, "br": br, "W": W_REF, "H": H_REF, "M": M,
           "e": np.asarray(est["E"], np.float64).copy(), "est": est}
    _scenes[key] = out
    return out
