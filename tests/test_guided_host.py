"""Guided matching on the host (include/erp_match.h "guided matching"): properties of the numpy
chain alone (tests/guided_ref.py), with E fitted on the ground-truth partners.  No GPU."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_ref as GR  # noqa: E402

SEEDS = (7, 8, 9)


@pytest.mark.parametrize("seed", SEEDS)
def test_thr_one_equals_the_plain_list(oracle, seed):
    """|l^T E' r| <= 0.7072 < 1: everything is gated, and with ratio 0.3, unique off and max_dist
    off the chain is match_two_image"""
    p, _ = GR.pair_e(oracle, seed, 512, 0.03)
    prep = GR.prepared(oracle, seed, 512, 0.03, 1.0)
    assert prep["gated"] == 512 * 512
    g = GR.select(prep, ratio=0.3, max_dist=0.0, unique=False)
    ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
    assert len(ref) > 0 and g["matches"].tobytes() == ref.tobytes()


@pytest.mark.parametrize("seed", SEEDS)
def test_max_dist_removes_the_lone_gated_outliers(oracle, seed):
    p, _ = GR.pair_e(oracle, seed, 512, 0.03)
    prep = GR.prepared(oracle, seed, 512, 0.03, 0.003)
    loose = GR.select(prep, ratio=0.8, max_dist=0.0, unique=False)
    tight = GR.select(prep, ratio=0.8, max_dist=0.8, unique=False)
    n_true = GR.n_partners(p)
    print(f"seed {seed}: partners {n_true}, without max_dist {loose['count']} "
          f"({GR.n_correct(p, loose['matches'])} correct), with 0.8 {tight['count']} "
          f"({GR.n_correct(p, tight['matches'])} correct)")
    # without max_dist a query whose band holds one wrong row is accepted against +inf
    assert loose["count"] > n_true and GR.n_correct(p, loose["matches"]) == n_true
    assert tight["count"] == n_true and GR.n_correct(p, tight["matches"]) == n_true
    # unique changes nothing once every match is at its true partner
    assert GR.select(prep, 0.8, 0.8, True)["matches"].tobytes() == tight["matches"].tobytes()


def test_strict_list_is_empty_where_the_guided_list_is_not(oracle):
    p, _ = GR.pair_e(oracle, 7, 512, 0.08)
    ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
    assert len(ref) == 0
    g = GR.select(GR.prepared(oracle, 7, 512, 0.08, 0.003), ratio=0.8, max_dist=0.8, unique=True)
    n_true = GR.n_partners(p)
    assert n_true > 400 and GR.n_correct(p, g["matches"]) == n_true


def test_no_case_of_either_test_file_is_ambiguous(oracle):
    """no (i, j) of any case lies within AMBIGUOUS of its threshold: the GPU tests compare every
    case exactly and leave nothing out.  (A case that ever fails here is replaced, not skipped.)"""
    amb = {}
    for seed in SEEDS:
        for thr in (1.0, 0.003):
            amb[(seed, 512, 0.03, thr)] = GR.prepared(oracle, seed, 512, 0.03, thr)["ambiguous"]
    amb[(7, 512, 0.08, 0.003)] = GR.prepared(oracle, 7, 512, 0.08, 0.003)["ambiguous"]
    for thr in GR.THRS + (1.0,):
        for k, prep in enumerate(GR.ragged_prepared(oracle, thr)):
            amb[("ragged", GR.RAGGED[k], thr)] = prep["ambiguous"]
    assert not any(amb.values()), {k: v for k, v in amb.items() if v}


def test_ragged_cases_exercise_the_rules(oracle):
    """the ragged batch is not vacuous: matches exist, unique and max_dist each remove some"""
    tot = {}
    for thr in GR.THRS:
        for unique in (False, True):
            for md in (0.0, 0.8):
                tot[(thr, unique, md)] = sum(GR.select(p, 0.8, md, unique)["count"]
                                             for p in GR.ragged_prepared(oracle, thr))
    print(tot)
    assert all(v > 100 for v in tot.values())
    assert tot[(0.01, True, 0.0)] < tot[(0.01, False, 0.0)]
    assert tot[(0.01, False, 0.8)] < tot[(0.01, False, 0.0)]
