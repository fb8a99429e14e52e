"""The pose selection's rules (include/erp_match.h "pose selection") against ground truth, on the
CPU: tests/pose_ref.py's chain on clean scenes built here from synth.eular2rot and
synth.bearing_to_pixel with fractional pixels, e from oracle.eight_point_estimation on all
matches.  The vote must be unanimous, the selected pose the scene's (Rc = R_gt, tc = -R_gt t_gt),
the depths the scene's; in the two large-rotation scenes the reference's validity rule rejects
both rotations, so find could not have returned the pose at all."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_ref as PO  # noqa: E402

R_TOL = 1e-5      # |Rm - R_gt|, |tc + R_gt t_gt| (measured: 1e-6)
D_TOL = 1e-4      # relative depth error (measured: 2e-5; the pixels are float)


@pytest.mark.parametrize("euler,M,seed", PO.SCENES)
def test_vote_selects_ground_truth(oracle, euler, M, seed):
    s = PO.scene(oracle, euler, M, seed)
    Ec, R1, R2, t = PO.candidates(oracle, s["e"])
    sel = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t)
    k = 2 * sel["which"] + (sel["t_sign"] < 0)
    dR = np.abs(sel["Rm"] - s["R_gt"]).max()
    dt = np.abs(sel["t"] - s["tc_gt"]).max()
    dd = max(np.abs(sel["depth"][:, 0] / s["d_l"] - 1).max(),
             np.abs(sel["depth"][:, 1] / s["d_r"] - 1).max())
    print(f"euler {euler} M {M}: votes {sel['votes'].tolist()} k {k} |dR|={dR:.2e} |dt|={dt:.2e} "
          f"depth rel {dd:.2e} min det {sel['det'].min():.2e} "
          f"min |d| {np.abs(sel['depth']).min():.2f}")
    # unanimous
    assert sel["n_voters"] == M and sel["votes"][k] == M and sel["votes"].sum() == M
    assert sel["front"].all() and sel["ambiguous"] == 0
    assert dR < R_TOL and dt < R_TOL and dd < D_TOL
    # the margins the GPU test's ambiguity condition relies on
    assert sel["det"].min() >= 1e-4 and np.abs(sel["depth"]).min() > 1.0


@pytest.mark.parametrize("euler,M,seed", [c for c in PO.SCENES if max(map(abs, c[0])) > 1.57])
def test_reference_rule_rejects_both_rotations(oracle, euler, M, seed):
    """what find cannot return: both candidates fail `every Euler angle under 1.57 rad`, in the
    oracle's own estimate and in the chain's candidates"""
    s = PO.scene(oracle, euler, M, seed)
    assert not s["est"]["R1_valid"] and not s["est"]["R2_valid"]
    _, R1, R2, _ = PO.candidates(oracle, s["e"])
    assert not PO.reference_valid(oracle, R1) and not PO.reference_valid(oracle, R2)


def test_candidates_are_the_oracles(oracle):
    """numpy's SVD gives the oracle's {R1, R2} and +-T (as a set: which is called R1 is noise)"""
    for euler, M, seed in PO.SCENES:
        s = PO.scene(oracle, euler, M, seed)
        _, R1, R2, t = PO.candidates(oracle, s["e"])
        mine = [oracle.rot2eular(R1), oracle.rot2eular(R2)]
        ref = [s["est"]["R1"], s["est"]["R2"]]
        d = min(max(np.abs(mine[0] - ref[0]).max(), np.abs(mine[1] - ref[1]).max()),
                max(np.abs(mine[0] - ref[1]).max(), np.abs(mine[1] - ref[0]).max()))
        dt = min(np.abs(t - s["est"]["T"]).max(), np.abs(t + s["est"]["T"]).max())
        assert d < 1e-6 and dt < 1e-6, (euler, d, dt)


def test_the_winning_label_varies_with_the_scene(oracle):
    """which of the four labels the true pose carries is the SVD's sign noise: over seven seeds
    of one geometry more than one label wins (three do here), so no label can be hard-wired"""
    ks = set()
    for seed in range(7):
        s = PO.scene(oracle, (0.1, 0.2, 0.05), 33, 100 + seed)
        Ec, R1, R2, t = PO.candidates(oracle, s["e"])
        sel = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t)
        ks.add(2 * sel["which"] + (sel["t_sign"] < 0))
    print("candidates seen:", sorted(ks))
    assert len(ks) >= 2


def test_mask_threshold_and_parallax_rules(oracle):
    s = PO.scene(oracle, *PO.SCENES[1])
    Ec, R1, R2, t = PO.candidates(oracle, s["e"])
    M = s["M"]
    full = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t)
    mask = np.zeros(M, np.uint8)
    mask[::3] = 1
    part = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t, mask=mask)
    assert part["n_voters"] == int(mask.sum()) and part["which"] == full["which"]
    assert np.array_equal(part["front"], mask) and not part["depth"][mask == 0].any()
    none = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t, mask=np.zeros(M, np.uint8))
    assert none["n_voters"] == 0 and not none["votes"].any()
    far = PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t, min_sin2=2.0)
    assert far["n_voters"] == 0
    # a clean scene's residuals are ~1e-7: every match passes 1e-3, none passes 1e-12
    assert PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t, thr=1e-3)["n_voters"] == M
    assert PO.select(oracle, s["bl"], s["br"], Ec, R1, R2, t, thr=1e-12)["n_voters"] == 0
