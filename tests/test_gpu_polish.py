"""The polish stage on the GPU (include/erp_match.h "polish"): the winner's inlier set and the
iterated inlier refit, checked round by round against the oracle ON THE GPU'S OWN RECORDS -- the
set under the GPU's E of round r-1 is computed by oracle.rank2 + inlier_count and must give the
GPU's counts of round r; the refit on that set by oracle.eight_point_estimation (with the
nearest-rotation and T-sign rules applied on the oracle's side) must give the GPU's E, R, T
within the project's bars (1e-6).  Cases and chain: tests/polish_ref.py.
One batched call per threshold; several ragged pairs share the 0.01 call."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polish_ref as PR  # noqa: E402

from erp_match_eightpoint_test_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-6        # E (sign-aligned), R (rad), T against the oracle's refit
BAND = 1e-12      # a match this near the threshold under the GPU's own E would be undecidable
TINY = "tiny"     # the 4-keypoint pair in the middle of the 0.01 batch: ERP_TOO_FEW_POINTS
GROUPS = {0.01: [PR.CASES[0], PR.CASES[1], PR.CASES[2], TINY, PR.CASES[3], PR.CASES[5],
                 PR.CASES[7]],
          0.005: [PR.CASES[4]], 0.02: [PR.CASES[6]], 0.002: [PR.CASES[8]]}


def _pair(oracle, c):
    return synth.make_pair(99, n_kpts=4) if c == TINY else PR.case(oracle, c)["pair"]


def _batch(pairs):
    import torch
    cat = lambda k: np.concatenate([p[k] for p in pairs])  # noqa: E731
    ol = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    orr = np.concatenate([[0], np.cumsum([len(p["desc_r"]) for p in pairs])]).astype(np.int64)
    W = np.array([p["W"] for p in pairs], np.int32)
    H = np.array([p["H"] for p in pairs], np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return (t(cat("desc_l")), t(cat("desc_r")), t(cat("kp_l")), t(cat("kp_r")), t(ol), t(orr), t(W),
            t(H), int(np.diff(ol).max()), int(np.diff(orr).max()))


@pytest.fixture(scope="module")
def runs(gpu_lib, oracle):
    """per threshold: one erp_pair_batch_run with records (cfg.inlier_thr = thr, so the records
    carry the count kernel's inliers), one polish with 3 rounds and one with 0 -- device tensors
    and host copies, computed once and never modified"""
    import torch
    from erp_match_eightpoint_test_amd import (PairBatchRunner, hyps_to_numpy, polish_rounds_to_numpy,
                                               polish_to_numpy, results_to_numpy)
    out = {}
    for thr, cases in GROUPS.items():
        b = _batch([_pair(oracle, c) for c in cases])
        run = PairBatchRunner(iters=PR.ITERS, inlier_thr=PR.thr64(thr))
        outs = run.run(*b, want=("hyps", "key_left", "key_right"))
        pol = run.polish(outs, b[6], b[7], thr, rounds=PR.ROUNDS, want_rounds=True)
        pol0 = run.polish(outs, b[6], b[7], thr, rounds=0)
        torch.cuda.synchronize()
        out[thr] = {"cases": cases, "run": run, "outs": outs, "W": b[6], "H": b[7], "dev": pol,
                    "results": results_to_numpy(outs["results"]), "hyps": hyps_to_numpy(outs["hyps"]),
                    "kl": outs["key_left"].cpu().numpy(), "kr": outs["key_right"].cpu().numpy(),
                    "polish": polish_to_numpy(pol["polish"]),
                    "rounds": polish_rounds_to_numpy(pol["rounds"]),
                    "mask": pol["mask"].cpu().numpy(), "polish0": polish_to_numpy(pol0["polish"]),
                    "mask0": pol0["mask"].cpu().numpy()}
    return out


def _slot(runs, c):
    thr = c[3]
    return runs[thr], runs[thr]["cases"].index(c)


def _bytes(rec, fields=("R", "T", "E")):
    return b"".join(np.ascontiguousarray(rec[f]).tobytes() for f in fields)


def _gpu_set(oracle, k, E, thr):
    S, near = PR.mask_of(oracle, k["bl"], k["br"], oracle.rank2(E), thr, BAND)
    assert near == 0, "a match within 1e-12 of the threshold under the GPU's E"
    return S


@pytest.mark.parametrize("c", PR.CASES)
def test_chain_parity_round_by_round(runs, oracle, c):
    g, i = _slot(runs, c)
    k = PR.case(oracle, c)
    res, hyps, pol, rounds = g["results"][i], g["hyps"][i], g["polish"][i], g["rounds"][i]
    M, thr = k["M"], c[3]
    assert res["status"] == 0 and res["M"] == M and pol["status"] == 0
    # the gathered keypoints are the oracle's (the matcher is bit-exact): its bearings apply
    assert np.array_equal(g["kl"][i, :M], k["kl"]) and np.array_equal(g["kr"][i, :M], k["kr"])
    # the winner by the rule on the GPU's own records; the iteration is the oracle's too.  (Which
    # of R1 / R2 a rotation is called is NOT comparable across implementations: a joint sign
    # flip of a singular pair of E' swaps the two, and the sign of the null vector -- a column
    # of norm ~1e-17 -- comes out of rounding noise.  Existing parity tests compare {R1, R2} as a
    # set for the same reason.  So `which` is checked against the GPU's records here and through
    # the chosen R below.)
    w, which = PR.winner_of(hyps, int(res["min_idx"]))
    assert (pol["winner_iter"], pol["winner_which"]) == (w, which)
    assert w == k["winner_iter"]
    assert np.array_equal(hyps[w]["R2" if which else "R1"], res["R"])
    ref = k["chain"]
    assert pol["rounds_done"] == len(ref["rounds"])
    E_prev, R_prev, T_prev = hyps[w]["E"], res["R"], res["T"]
    S_prev = _gpu_set(oracle, k, E_prev, thr)
    assert pol["n_inliers_winner"] == int(S_prev.sum())
    last = None
    for r in range(int(pol["rounds_done"])):
        rd = rounds[r]
        assert rd["n_fit"] == int(S_prev.sum()) >= PR.MIN_FIT
        f = PR.refit(oracle, k["bl"], k["br"], S_prev, R_prev, T_prev)
        assert f is not None and rd["which"] in (0, 1)  # (f["R"]: the oracle's nearer candidate)
        sign = 1.0 if float(np.dot(rd["E"], f["e"])) >= 0 else -1.0
        dE = np.abs(sign * rd["E"] - f["e"]).max()
        dR, dT = np.abs(rd["R"] - f["R"]).max(), np.abs(rd["T"] - f["T"]).max()
        S = _gpu_set(oracle, k, rd["E"], thr)
        print(f"{c} round {r + 1}: fit {rd['n_fit']} -> {rd['n_inliers']} which {rd['which']} "
              f"|dE|={dE:.2e} |dR|={dR:.2e} |dT|={dT:.2e}")
        assert dE <= TOL and dR <= TOL and dT <= TOL
        assert rd["n_inliers"] == int(S.sum()) >= int(S_prev.sum()) and rd["reserved"] == 0
        S_prev, E_prev, R_prev, T_prev, last = S, rd["E"], rd["R"], rd["T"], rd
    # records past rounds_done are zero
    assert not rounds[int(pol["rounds_done"]):].tobytes().strip(b"\0")
    # the output state is the last accepted one, byte for byte
    if last is not None:
        assert _bytes(pol) == _bytes(last)
    else:
        assert _bytes(pol) == res["R"].tobytes() + res["T"].tobytes() + hyps[w]["E"].tobytes()
    assert pol["n_inliers"] == int(S_prev.sum())
    # the final mask is the oracle's under the GPU's final E; bytes past M are 0
    assert g["mask"].shape[1] > M
    assert np.array_equal(g["mask"][i, :M], S_prev.astype(np.uint8))
    assert not g["mask"][i, M:].any()
    print(f"{c}: euler error {PR.euler_err(res['R'], k['pair']):.5f} -> "
          f"{PR.euler_err(pol['R'], k['pair']):.5f} rad")


@pytest.mark.parametrize("c", PR.CASES)
def test_rounds_0_is_the_winner(runs, oracle, c):
    g, i = _slot(runs, c)
    k = PR.case(oracle, c)
    res, hyps, p0 = g["results"][i], g["hyps"][i], g["polish0"][i]
    w = int(p0["winner_iter"])
    assert p0["status"] == 0 and p0["rounds_done"] == 0 and w == k["winner_iter"]
    assert _bytes(p0) == res["R"].tobytes() + res["T"].tobytes() + hyps[w]["E"].tobytes()
    # the new stage against the existing count kernel (the run had cfg.inlier_thr = thr)
    assert p0["n_inliers"] == p0["n_inliers_winner"] == hyps[w]["inliers"]
    S0 = _gpu_set(oracle, k, hyps[w]["E"], c[3])
    assert np.array_equal(g["mask0"][i, :k["M"]], S0.astype(np.uint8))
    assert not g["mask0"][i, k["M"]:].any()
    assert g["polish"][i]["n_inliers_winner"] == p0["n_inliers"]


@pytest.mark.parametrize("c", [PR.CASES[5], PR.CASES[6]])
def test_fewer_than_nine_inliers_stop(runs, oracle, c):
    g, i = _slot(runs, c)
    pol, p0 = g["polish"][i], g["polish0"][i]
    assert pol["rounds_done"] == 0 and pol["n_inliers"] < PR.MIN_FIT
    assert pol.tobytes() == p0.tobytes()
    assert np.array_equal(g["mask"][i], g["mask0"][i]) and g["mask"][i].sum() == pol["n_inliers"]


def test_batch_equals_single_pairs_and_a_second_run(runs):
    """the 0.01 batch: 6 cases and the 4-keypoint pair in the middle"""
    import torch
    from erp_match_eightpoint_test_amd import polish_to_numpy
    g = runs[0.01]
    run, outs, n = g["run"], g["outs"], len(g["cases"])
    again = run.polish(outs, g["W"], g["H"], 0.01, rounds=PR.ROUNDS, want_rounds=True)
    torch.cuda.synchronize()
    for f in ("polish", "rounds", "mask"):
        assert torch.equal(again[f], g["dev"][f]), f
    t = g["cases"].index(TINY)
    assert 0 < t < n - 1
    for i in range(n):
        one = {f: outs[f][i:i + 1].contiguous() for f in ("results", "hyps", "key_left", "key_right")}
        s = run.polish(one, g["W"][i:i + 1].contiguous(), g["H"][i:i + 1].contiguous(), 0.01,
                       rounds=PR.ROUNDS, want_rounds=True)
        for f in ("polish", "rounds", "mask"):
            assert torch.equal(s[f][0], g["dev"][f][i]), (i, f)
    # the pair the find rejected: its status and zeros
    assert g["results"][t]["status"] == 2
    rec = g["polish"][t].copy()
    assert rec["status"] == 2
    rec["status"] = 0
    assert not rec.tobytes().strip(b"\0") and not g["rounds"][t].tobytes().strip(b"\0")
    assert not g["mask"][t].any()
    assert polish_to_numpy(g["dev"]["polish"])[t]["status"] == 2


def _find_dev_then_polish(ctx, k, thr, rounds, cfg):
    """erp_eight_point_find_dev with records, then erp_polish_dev on the same keys"""
    import torch
    from erp_match_eightpoint_test_amd import capi
    dkl, dkr = torch.from_numpy(k["kl"]).cuda(), torch.from_numpy(k["kr"]).cuda()
    res = torch.zeros((1, capi.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    hyps = torch.zeros((1, cfg.iters, capi.HYP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    p = k["pair"]
    st = ctx.L.erp_eight_point_find_dev(ctx.h, p["W"], p["H"], dkl.data_ptr(), dkr.data_ptr(),
                                        k["M"], C.byref(cfg), res.data_ptr(), hyps.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    assert st == 0
    wh = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")  # noqa: E731
    pol = ctx.polish(res, hyps, dkl[None].contiguous(), dkr[None].contiguous(), wh(p["W"]),
                     wh(p["H"]), thr, rounds=rounds, valid_abs=cfg.valid_abs)
    torch.cuda.synchronize()
    return (res.cpu().numpy().view(capi.RESULT_DTYPE)[0],
            pol["polish"].cpu().numpy().view(capi.POLISH_DTYPE)[0], pol["mask"].cpu().numpy()[0])


def test_find_polished_is_find_then_polish(gpu_lib, oracle):
    from erp_match_eightpoint_test_amd import Context, eight_point
    c = PR.CASES[2]
    k = PR.case(oracle, c)
    ep = eight_point(iters=PR.ITERS)
    R, T, mask = ep.find_polished(k["pair"]["W"], k["pair"]["H"], k["kl"], k["kr"], c[3], PR.ROUNDS)
    res, pol, m2 = _find_dev_then_polish(Context(), k, c[3], PR.ROUNDS, ep.cfg)
    assert ep.last_polish.tobytes() == pol.tobytes() and pol["rounds_done"] == 3
    assert ep.last_result["min_idx"] == res["min_idx"] and _bytes(ep.last_result, ("R", "T")) == \
        _bytes(res, ("R", "T"))
    assert np.array_equal(mask, m2.astype(bool)) and mask.sum() == pol["n_inliers"]
    assert R.tobytes() == pol["R"].tobytes() and T.tobytes() == pol["T"].tobytes()
    # and it is the batched run's answer for the same pair (the chain is the same arithmetic)
    assert PR.euler_err(R, k["pair"]) < PR.euler_err(ep.last_result["R"], k["pair"]) / 10


def test_find_polished_consumes_the_stream_as_find_does(gpu_lib, oracle):
    from erp_match_eightpoint_test_amd import RandStream, eight_point
    c = PR.CASES[3]
    k = PR.case(oracle, c)
    p = k["pair"]
    a, b = RandStream(1, 0), RandStream(1, 0)
    ea, eb = eight_point(stream=a, iters=PR.ITERS), eight_point(stream=b, iters=PR.ITERS)
    for n in (1, 2):  # the second call goes on where the first stopped, as find's does
        ea.find(p["W"], p["H"], k["kl"], k["kr"])
        eb.find_polished(p["W"], p["H"], k["kl"], k["kr"], c[3], PR.ROUNDS)
        assert a.draws == b.draws == n * PR.ITERS * (k["M"] - 1)
        fields = ("R", "T", "status", "M", "K", "min_idx", "sample_n", "min_dist")
        assert _bytes(ea.last_result, fields) == _bytes(eb.last_result, fields)
    # a call that fails on the polish's arguments consumes nothing
    with pytest.raises(Exception):
        eb.find_polished(p["W"], p["H"], k["kl"], k["kr"], 0.0, PR.ROUNDS)
    assert b.draws == a.draws


def test_cpp_find_polished_driver(gpu_lib, oracle, tmp_path):
    """erp::eight_point::find_polished as a reference maintainer links it (g++ against the
    library, no Python in the process) equals the Python wrapper's call"""
    from erp_match_eightpoint_test_amd import _build, capi, eight_point
    driver = _build.build_polish_driver()
    c = PR.CASES[0]
    k = PR.case(oracle, c)
    p = k["pair"]
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    outd.mkdir()
    np.array([p["W"], p["H"], PR.ITERS, k["M"], PR.ROUNDS], np.int32).tofile(ind / "meta.i32")
    np.array([c[3]], np.float32).tofile(ind / "thr.f32")
    k["kl"].tofile(ind / "kl.f32")
    k["kr"].tofile(ind / "kr.f32")
    r = subprocess.run([driver, str(ind), str(outd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(outd / "polished.bin", np.uint8)
    res = raw[24:24 + 64].view(capi.RESULT_DTYPE)[0]
    pol = raw[24 + 64:].view(capi.POLISH_DTYPE)[0]
    mask = np.fromfile(outd / "mask.u8", np.uint8)
    ep = eight_point(iters=PR.ITERS)
    R, T, m2 = ep.find_polished(p["W"], p["H"], k["kl"], k["kr"], c[3], PR.ROUNDS)
    assert pol.tobytes() == ep.last_polish.tobytes() and pol["rounds_done"] == 2
    assert _bytes(res, ("R", "T")) == _bytes(ep.last_result, ("R", "T"))
    assert raw[:12].tobytes() == R.tobytes() and raw[12:24].tobytes() == T.tobytes()
    assert np.array_equal(mask.astype(bool), m2) and len(mask) == k["M"]
    assert int(mask.sum()) == pol["n_inliers"] == 155
