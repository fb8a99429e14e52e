"""The reference chain of guided matching (include/erp_match.h "guided matching"), built only
from the oracle's pixel_to_bearing, rank2, inlier_count, l2sq / match_two_image and numpy.
Shared by tests/test_guided_host.py and tests/test_gpu_guided.py; results are cached per case
and never modified.

The gate |l^T E' r| < thr is evaluated in numpy (a plain matrix product, within a few 1e-16 of
the fixed-order residual); any (i, j) within polish_ref.AMBIGUOUS of thr is decided by
oracle.inlier_count -- the fixed order itself -- and counted as ambiguous.  thr, ratio and
max_dist are the floats the C ABI takes; thr is widened to double as the library does."""
from __future__ import annotations

import numpy as np

import polish_ref as PR
from erp_match_eightpoint_test_amd import synth
from erp_match_eightpoint_test_amd.capi import DMATCH_DTYPE

AMBIGUOUS = PR.AMBIGUOUS
INF = np.float32(np.inf)
_cache: dict = {}


def fit_e(oracle, p) -> np.ndarray:
    """the solved 9-vector of eight_point_estimation on the ground-truth partners of a
    synth.make_pair pair"""
    gi = np.where(p["gt_partner"] >= 0)[0]
    bl = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_l"][gi])
    br = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_r"][p["gt_partner"][gi]])
    return np.asarray(oracle.eight_point_estimation(bl, br)["E"], np.float64).copy()


def gate(oracle, bl, br, Ec, thr: float):
    """(bool [nq, nt]: |l_i^T Ec r_j| < thr, the (i, j) within AMBIGUOUS of thr); a NaN residual
    is not gated"""
    t = PR.thr64(thr)
    nq, nt = len(bl), len(br)
    if nq == 0 or nt == 0:
        return np.zeros((nq, nt), bool), 0
    with np.errstate(invalid="ignore"):
        res = np.abs(bl @ np.asarray(Ec, np.float64).reshape(3, 3) @ br.T)
        g = res < t
        near = np.argwhere(np.abs(res - t) < AMBIGUOUS)
    for i, j in near:
        n, _ = oracle.inlier_count(bl[i:i + 1], br[j:j + 1], Ec, t, 0.0)
        g[i, j] = n == 1
    return g, len(near)


def top2(oracle, q, t, cols):
    """(j0, e0, e1) of query row q over the train rows `cols` (ascending): the smallest squared
    distance in the flann::L2 order, the lowest j among equal ones, and the second smallest
    (+inf when there is one row only)"""
    if len(cols) == 1:
        return int(cols[0]), np.float32(oracle.l2sq(q, t[cols[0]])), INF
    _, best, d0, d1 = oracle.match_two_image(q[None, :], np.ascontiguousarray(t[cols]), 0.3, 1)
    return int(cols[best[0]]), np.float32(d0[0]), np.float32(d1[0])


def prepare(oracle, desc_l, desc_r, kp_l, kp_r, W: int, H: int, e, thr: float) -> dict:
    """rules 1-3 for one pair (the expensive part, shared by every ratio / max_dist / unique
    setting) -> dict(top: per query (j0, e0, e1) or None, gated: sum |G_i|, ambiguous: the
    (i, j) within AMBIGUOUS of thr, kp_l, kp_r)"""
    desc_l = np.ascontiguousarray(desc_l, np.float32).reshape(-1, 64)
    desc_r = np.ascontiguousarray(desc_r, np.float32).reshape(-1, 64)
    kp_l = np.ascontiguousarray(kp_l, np.float32).reshape(-1, 2)
    kp_r = np.ascontiguousarray(kp_r, np.float32).reshape(-1, 2)
    bl = oracle.pixel_to_bearing(W, H, kp_l)
    br = oracle.pixel_to_bearing(W, H, kp_r)
    g, amb = gate(oracle, bl, br, oracle.rank2(e), thr)
    top = [top2(oracle, desc_l[i], desc_r, np.flatnonzero(g[i])) if g[i].any() else None
           for i in range(len(desc_l))]
    return {"top": top, "gated": int(g.sum()), "ambiguous": amb, "kp_l": kp_l, "kp_r": kp_r}


def select(prep: dict, ratio: float = 0.8, max_dist: float = 0.0, unique: bool = True) -> dict:
    """rules 4-6 on prepare()'s dict -> dict(matches: DMATCH records in ascending queryIdx,
    key_left, key_right: their keypoints, count, gated, ambiguous)"""
    ratio32, md32 = np.float32(ratio), np.float32(max_dist)
    acc = []
    for i, tp in enumerate(prep["top"]):
        if tp is None:
            continue
        j0, e0, e1 = tp
        d0, d1 = np.sqrt(e0), np.sqrt(e1)
        with np.errstate(invalid="ignore"):
            ok = d0 < np.float32(ratio32 * d1) and (not md32 > 0 or d0 < md32)
        if ok:
            acc.append((i, j0, d0))
    if unique:
        best = {}
        for i, j0, d0 in acc:  # ascending i: a later query needs a strictly smaller d0
            if j0 not in best or d0 < best[j0][2]:
                best[j0] = (i, j0, d0)
        acc = sorted(best.values())
    m = np.zeros(len(acc), DMATCH_DTYPE)
    for k, (i, j0, d0) in enumerate(acc):
        m[k] = (i, j0, 0, d0)
    return {"matches": m, "count": len(acc), "gated": prep["gated"],
            "ambiguous": prep["ambiguous"], "key_left": prep["kp_l"][m["queryIdx"]],
            "key_right": prep["kp_r"][m["trainIdx"]]}


def guided(oracle, desc_l, desc_r, kp_l, kp_r, W: int, H: int, e, thr: float, ratio: float = 0.8,
           max_dist: float = 0.0, unique: bool = True) -> dict:
    return select(prepare(oracle, desc_l, desc_r, kp_l, kp_r, W, H, e, thr), ratio, max_dist,
                  unique)


def prepared(oracle, seed: int, n: int, sigma: float, thr: float) -> dict:
    """prepare() of pair_e(seed, n, sigma) at thr, cached"""
    k = ("g", seed, n, sigma, thr)
    if k not in _cache:
        p, e = pair_e(oracle, seed, n, sigma)
        _cache[k] = prepare(oracle, p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"],
                            p["H"], e, thr)
    return _cache[k]


def pair(seed: int, n: int, sigma: float) -> dict:
    """synth.make_pair(seed, n, sigma=sigma), cached"""
    k = ("p", seed, n, sigma)
    if k not in _cache:
        _cache[k] = synth.make_pair(seed, n_kpts=n, sigma=sigma)
    return _cache[k]


def pair_e(oracle, seed: int, n: int, sigma: float):
    """(the pair, E fitted on its ground-truth partners), cached"""
    k = ("e", seed, n, sigma)
    if k not in _cache:
        _cache[k] = fit_e(oracle, pair(seed, n, sigma))
    return pair(seed, n, sigma), _cache[k]


def n_partners(p) -> int:
    return int((p["gt_partner"] >= 0).sum())


def n_correct(p, m) -> int:
    """matches of m at the true partner"""
    return int((p["gt_partner"][m["queryIdx"]] == m["trainIdx"]).sum())


# ---- the cases of the two test files (every one is checked for ambiguity by the host tests) ----
THRS = (0.003, 0.01)
RAGGED = [(1, 1), (1, 2), (63, 65), (65, 63), (64, 64), (130, 200), (257, 129), (40, 0), (0, 40)]
RAGGED_MAX_NQ, RAGGED_MAX_NT = 260, 203   # above every nq / nt


def ragged_pairs(oracle) -> list:
    """one pair per RAGGED shape: the first nq left and nt right rows of synth.make_pair(20 + k,
    max(nq, nt, 16)), E fitted on the whole pair's ground-truth partners; cached"""
    if "ragged" not in _cache:
        out = []
        for k, (nq, nt) in enumerate(RAGGED):
            p, e = pair_e(oracle, 20 + k, max(nq, nt, 16), 0.03)
            out.append({"desc_l": np.ascontiguousarray(p["desc_l"][:nq]),
                        "desc_r": np.ascontiguousarray(p["desc_r"][:nt]),
                        "kp_l": np.ascontiguousarray(p["kp_l"][:nq]),
                        "kp_r": np.ascontiguousarray(p["kp_r"][:nt]), "W": p["W"], "H": p["H"],
                        "e": e})
        _cache["ragged"] = out
    return _cache["ragged"]


def ragged_prepared(oracle, thr: float) -> list:
    """prepare() of every ragged pair at thr, cached"""
    k = ("ragged", thr)
    if k not in _cache:
        _cache[k] = [prepare(oracle, p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"],
                             p["H"], p["e"], thr) for p in ragged_pairs(oracle)]
    return _cache[k]
