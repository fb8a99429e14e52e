"""Oracle-only pins of the inputs test_gpu_estimator_domain.py relies on (tests/estimator_domain.py):
what the oracle -- and with it the reference -- does at the edges of the estimator's input domain.
A change of a synth seed or of the oracle that moves one of these fails here, loudly, instead of
silently emptying a GPU case.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimator_domain as D  # noqa: E402


@pytest.mark.parametrize("name", "ABC")
def test_valid_abs_above_pi_keeps_every_rotation(oracle, name):
    """valid_abs = 4 > pi: K = 2 iters exactly, the capacity edge of the consensus rows; the
    angles reach pi"""
    a = D.euler_maxabs(name)
    assert len(a) == 2 * D.ITERS and np.isfinite(a).all()
    assert 3.1 < a[-1] <= np.float32(np.pi)


@pytest.mark.parametrize("name", "ABC")
@pytest.mark.parametrize("valid_abs", [0.0, -1.0, float("nan")], ids=["0", "-1", "nan"])
def test_valid_abs_not_positive_gives_no_valid_hypothesis(oracle, name, valid_abs):
    c = D.scene(name)
    o = oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"],
                    oracle.make_cfg(iters=D.ITERS, valid_abs=valid_abs), detail=True)
    assert o["K"] == 0 and o["status"] == -3 and o["min_idx"] == -1
    assert not o["R"].any() and not o["T"].any() and o["min_dist"] == 0
    assert o["sample_n"] == len(c["kp_l"]) // 4
    assert not o["hyp"]["R1_valid"].any() and not o["hyp"]["R2_valid"].any()
    assert np.isfinite(o["hyp"]["E"]).all()  # the records are still written


@pytest.mark.parametrize("name", "ABC")
def test_smallest_angles_are_separated(oracle, name):
    """the 8 gaps between the 9 smallest max |Euler angle| values are all above 20x the R bar,
    so valid_abs at a midpoint selects the same k rotations on the GPU as in the oracle"""
    a = D.euler_maxabs(name)
    gaps = np.diff(a[:9])
    print(name, "smallest gaps:", gaps)
    assert (gaps > D.GAP_MIN).all(), gaps


@pytest.mark.parametrize("name", "ABC")
@pytest.mark.parametrize("k", D.SMALL_KS)
def test_midpoint_valid_abs_gives_k(oracle, name, k):
    c = D.scene(name)
    va = D.valid_abs_for_k(name, k)
    o = oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"],
                    oracle.make_cfg(iters=D.ITERS, valid_abs=va), detail=True)
    assert o["K"] == k and o["status"] == 0
    if k <= 2:  # the trimmed window [0.2 K, 0.8 K) is empty: every mean is NaN, row 0 wins
        assert o["min_idx"] == 0


def test_edge_keypoints_are_unit_bearings(oracle):
    """B1: poles, negative and far-outside pixels still give unit bearings, status 0, K = 299"""
    c = D.scene("A")
    kl, kr = D.edge_keypoints()
    for k in (kl, kr):
        b = oracle.pixel_to_bearing(c["W"], c["H"], k)
        assert np.isfinite(b).all()
        assert np.abs(np.linalg.norm(b, axis=1) - 1).max() <= 4e-16
        assert np.abs(b).max() <= 1.0
    o = oracle.find(c["W"], c["H"], kl, kr, oracle.make_cfg(iters=D.ITERS))
    assert o["status"] == 0 and o["K"] == 299


def test_nonfinite_keypoints_drop_iterations_in_the_oracle(oracle):
    """B2: the oracle (as the reference) silently loses every iteration that sampled the row"""
    c = D.scene("A")
    cfg = oracle.make_cfg(iters=D.ITERS)
    assert oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"], cfg)["K"] == 300
    cases = D.nonfinite_cases()
    b = oracle.pixel_to_bearing(c["W"], c["H"], cases["nan_left"][0])
    assert np.isnan(b[5]).any() and np.isfinite(np.delete(b, 5, axis=0)).all()
    b = oracle.pixel_to_bearing(c["W"], c["H"], cases["inf_right"][1])
    assert not np.isfinite(b[7]).all()
    o = oracle.find(c["W"], c["H"], *cases["nan_left"], cfg)
    assert o["status"] == 0 and o["K"] == 205
    o = oracle.find(c["W"], c["H"], *cases["inf_right"], cfg)
    assert o["status"] == 0 and 0 < o["K"] < 300
    o = oracle.find(c["W"], c["H"], *cases["all_nan"], cfg)
    assert o["status"] == -3 and o["K"] == 0


@pytest.mark.parametrize("iters,frac", [(80, 0.25), (1, 0.25), (1, 1.0)])
def test_oracle_is_scale_invariant(oracle, iters, frac):
    """C: uniform bearing scales leave the oracle's initial_guess unchanged, exactly"""
    c = D.scene("A")
    bl = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_l"])
    br = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_r"])
    cfg = oracle.make_cfg(iters=iters, sample_frac=frac)
    base = oracle.initial_guess(bl, br, cfg)
    assert base["status"] == 0 and base["K"] >= 1
    for s in D.SCALES + [(1e3, 1e-3)]:
        o = oracle.initial_guess(*D.scaled_bearings(bl, br, s), cfg)
        assert o["status"] == 0, s
        if s != "rows":
            assert o["K"] == base["K"], s
            assert np.array_equal(o["R"], base["R"]) and np.array_equal(o["T"], base["T"]), s
