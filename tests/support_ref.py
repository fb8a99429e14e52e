"""The support stage's rules (include/erp_match.h "support-scored winner") restated on the oracle:
oracle.find(detail=True) with inlier_thr for the per-iteration records and counts, oracle.rank2
and oracle.inlier_count for a count from a given E, and the selection written out in plain Python.
Shared by tests/test_support_host.py and tests/test_gpu_support.py."""
from __future__ import annotations

import numpy as np

AMBIGUOUS = 1e-12   # a residual this close to thr may fall either way (test_inlier_count_vs_oracle)


def thr64(thr: float) -> float:
    """the threshold as the library sees it: a C float widened to double"""
    return float(np.float32(thr))


def rdist(a, b) -> np.float32:
    """the consensus' distance (src/eight_point.cpp:138-139): sqrtf of float squared differences"""
    d = np.asarray(a, np.float32) - np.asarray(b, np.float32)
    s = np.float32(d[0] * d[0]) + np.float32(d[1] * d[1])
    s = np.float32(s) + np.float32(d[2] * d[2])
    return np.sqrt(np.float32(s))


def counts_of(oracle, bl, br, hyp, thr: float, band: float = AMBIGUOUS):
    """rule 2 from the records' E: (count_h [iters], the matches within `band` of thr per
    iteration [iters])"""
    t = thr64(thr)
    n = np.zeros(len(hyp), np.int64)
    near = np.zeros(len(hyp), np.int64)
    for h in range(len(hyp)):
        n[h], near[h] = oracle.inlier_count(bl, br, oracle.rank2(hyp[h]["E"]), t, band)
    return n, near


def consensus_iter(hyp, min_idx: int) -> int:
    """rule 5: the iteration that pushed row min_idx (R1 then R2 per iteration)"""
    flags = np.stack([hyp["R1_valid"] != 0, hyp["R2_valid"] != 0], 1).reshape(-1)
    rows = np.nonzero(flags)[0]
    assert 0 <= min_idx < len(rows), (min_idx, len(rows))
    return int(rows[min_idx] // 2)


def select(hyp, counts, res_R, min_idx: int):
    """rules 3 - 5 -> dict(iter, which, inliers, scored, consensus_iter, consensus_inliers, row),
    or None when no iteration is scored (K = 0)"""
    v1, v2 = hyp["R1_valid"] != 0, hyp["R2_valid"] != 0
    scored = np.nonzero(v1 | v2)[0]
    if len(scored) == 0:
        return None
    best = int(scored[np.argmax(np.asarray(counts)[scored])])  # (argmax: the first maximum)
    if v1[best] and v2[best]:
        which = 0 if rdist(hyp[best]["R1"], res_R) <= rdist(hyp[best]["R2"], res_R) else 1
    else:
        which = 0 if v1[best] else 1
    row = int(v1[:best].sum() + v2[:best].sum()) + (1 if which == 1 and v1[best] else 0)
    ci = consensus_iter(hyp, min_idx)
    return {"iter": best, "which": which, "inliers": int(counts[best]), "scored": len(scored),
            "consensus_iter": ci, "consensus_inliers": int(counts[ci]), "row": row}


def from_find(oracle, W, H, kl, kr, thr: float, **cfg):
    """oracle.find(detail=True) with inlier_thr = thr and the selection on its records -> (find's
    dict, select()'s dict or None)"""
    r = oracle.find(W, H, kl, kr, oracle.make_cfg(inlier_thr=thr64(thr), **cfg), detail=True)
    if r["status"] != 0:
        return r, None
    return r, select(r["hyp"], r["hyp"]["inliers"], r["R"], int(r["min_idx"]))


def rotation_error_deg(oracle, R, euler_gt) -> float:
    """the angle between eular2rot(R) and the ground truth, the smaller of R and R^T (the
    estimator's rotation maps right to left or left to right by convention)"""
    Rh = oracle.eular2rot(np.asarray(R, np.float64))
    Rg = oracle.eular2rot(np.asarray(euler_gt, np.float64))

    def ang(A):
        return float(np.degrees(np.arccos(np.clip((np.trace(A @ Rg.T) - 1.0) / 2.0, -1.0, 1.0))))
    return min(ang(Rh), ang(Rh.T))
