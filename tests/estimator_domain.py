"""Inputs at the edges of the estimator's domain, shared by test_estimator_domain_host.py (the
oracle-only pins of their properties) and test_gpu_estimator_domain.py (the GPU against the
oracle on them).  Everything is regenerated from synth seeds; nothing here touches the GPU.

Scenes: A = 120 matches with a fifth outliers on a 2048 x 1024 image, B = 40 matches, C = 400
matches on 5376 x 2688.
"""
from __future__ import annotations

import functools

import numpy as np

from erp_match_eightpoint_test_amd import synth

SCENES = {"A": (11, dict(m=120, outlier_frac=0.2, W=2048, H=1024)),
          "B": (7, dict(m=40, W=2048, H=1024)),
          "C": (3, dict(m=400, W=5376, H=2688))}
ITERS = 300          # the iteration count of the single-pair cases
VALID_ALL = 4.0      # valid_abs > pi: every rotation is valid, K = 2 iters
GAP_MIN = 2e-5       # 20x the R bar (1e-6): a GPU rotation within the bar cannot change sides
SMALL_KS = (1, 2, 3, 5)

# left x right bearing scales of section C; "rows" = a factor per row and side from [0.5, 2]
SCALES = [(1.0, 1.0), (2.0, 2.0), (3.0, 1.0), (2.0 ** 10, 2.0 ** -10), (2.0 ** -20, 2.0 ** -20),
          (1e-4, 1e-4), (1e3, 1e3), (2.0 ** 40, 2.0 ** 40), "rows"]
SCALE_IDS = ["1x1", "2x2", "3x1", "2^10x2^-10", "2^-20x2^-20", "1e-4x1e-4", "1e3x1e3",
             "2^40x2^40", "rows_0.5_2"]


@functools.lru_cache(maxsize=None)
def scene(name: str) -> dict:
    seed, kw = SCENES[name]
    return synth.make_correspondences(seed, **kw)


@functools.lru_cache(maxsize=None)
def euler_maxabs(name: str, iters: int = ITERS) -> np.ndarray:
    """sorted max |Euler angle| of the 2 iters rotations the oracle's find makes on a scene
    (R1 and R2 of every iteration, as stored: float32 widened)"""
    import oracle
    c = scene(name)
    o = oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"],
                    oracle.make_cfg(iters=iters, valid_abs=VALID_ALL), detail=True)
    assert o["K"] == 2 * iters, (name, o["K"])
    a = np.concatenate([np.abs(o["hyp"]["R1"]).max(axis=1), np.abs(o["hyp"]["R2"]).max(axis=1)])
    return np.sort(a.astype(np.float64))


def valid_abs_for_k(name: str, k: int, iters: int = ITERS) -> float:
    """the valid_abs that keeps exactly the k rotations with the smallest angles: the midpoint
    between the k-th and the (k+1)-th sorted value"""
    a = euler_maxabs(name, iters)
    return float(0.5 * (a[k - 1] + a[k]))


def edge_keypoints(name: str = "A"):
    """section B1: the scene with six keypoints at and beyond the image -- the two poles, a
    negative column, a column and row far outside, the bottom row and half a pixel past the
    right border (the last two on the right side) -> (kl, kr) copies"""
    c = scene(name)
    W, H = c["W"], c["H"]
    kl, kr = c["kp_l"].copy(), c["kp_r"].copy()
    kl[0] = (W, 0)
    kl[1] = (0, H)
    kl[2] = (-300, H / 2)
    kl[3] = (4000, -200)
    kr[4] = (W / 2, H)
    kr[5] = (W + 0.5, 1500)
    return kl, kr


def scaled_bearings(bl, br, scale, lo: float = 0.5, hi: float = 2.0, seed: int = 20240):
    """section C: (bl, br) times a (left, right) scale pair, or -- scale == "rows" -- times a
    factor per row and side drawn log-uniformly from [lo, hi]"""
    if scale == "rows":
        rng = np.random.default_rng(seed)
        f = np.exp(rng.uniform(np.log(lo), np.log(hi), size=(2, len(bl), 1)))
        return bl * f[0], br * f[1]
    return bl * scale[0], br * scale[1]


def pair_from_keys(seed: int, kl, kr, W: int, H: int, extra: int = 40) -> dict:
    """a batch pair whose ratio test keeps exactly the len(kl) given keypoint pairs, in order
    (query i matches train i: its train descriptor is a copy; `extra` more rows a side are
    random and match nothing) -- the construction of test_gpu_gram_pipeline._pair_with_matches
    around given keypoints, so find sees (kl, kr) as they are"""
    rng = np.random.default_rng(seed)
    M = len(kl)
    dl = synth.random_descriptors(rng, M + extra)
    dr = synth.random_descriptors(rng, M + extra)
    dr[:M] = dl[:M]
    px = lambda k: (rng.random((k, 2)) * [W, H]).astype(np.float32)  # noqa: E731
    return {"desc_l": dl, "desc_r": dr,
            "kp_l": np.concatenate([np.asarray(kl, np.float32), px(extra)]),
            "kp_r": np.concatenate([np.asarray(kr, np.float32), px(extra)]), "W": W, "H": H}


def scene_pair(name: str) -> dict:
    c = scene(name)
    return pair_from_keys(SCENES[name][0] + 500, c["kp_l"], c["kp_r"], c["W"], c["H"])


def nonfinite_cases(name: str = "A") -> dict:
    """section B2: one NaN coordinate on the left, one +Inf on the right, every keypoint NaN"""
    c = scene(name)
    out = {}
    kl, kr = c["kp_l"].copy(), c["kp_r"].copy()
    kl[5, 0] = np.nan
    out["nan_left"] = (kl, kr)
    kl, kr = c["kp_l"].copy(), c["kp_r"].copy()
    kr[7, 1] = np.inf
    out["inf_right"] = (kl, kr)
    out["all_nan"] = (np.full_like(c["kp_l"], np.nan), np.full_like(c["kp_r"], np.nan))
    return out
