"""Guided matching on the GPU (include/erp_match.h "guided matching")
against tests/guided_ref.py's chain, exactly: counts, indices, the distance bits, gathered keys,
gated, and the bytes of results_out and winners_out.  No tolerance anywhere: the gate is the
fixed-order fp64 residual, the distances are the matcher's, and tests/test_guided_host.py asserts
that no (i, j) of any case used here lies within polish_ref.AMBIGUOUS of its threshold (the
cases whose E comes out of a GPU run assert it themselves)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guided_ref as GR  # noqa: E402
import polish_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_NQ, MAX_NT = GR.RAGGED_MAX_NQ, GR.RAGGED_MAX_NT
SETTINGS = [(thr, unique, md) for thr in GR.THRS for unique in (False, True) for md in (0.0, 0.8)]
CHAIN_SEEDS = (7, 8, 9, 10)
CHAIN_THR = 0.01
CHAIN_RUN_RATIO = 0.5
ERP_INVALID_ARG, ERP_TOO_FEW_POINTS, ERP_INTERNAL = 1, 2, 7


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(pairs, max_nq=None, max_nt=None):
    """the packed batch of `pairs` (dicts with desc_l, desc_r, kp_l, kp_r, W, H) as run() and
    guided_match() take it"""
    cat = lambda k, w: np.concatenate([np.asarray(p[k], np.float32).reshape(-1, w)  # noqa: E731
                                       for p in pairs])
    ol = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    orr = np.concatenate([[0], np.cumsum([len(p["desc_r"]) for p in pairs])]).astype(np.int64)
    W = np.array([p["W"] for p in pairs], np.int32)
    H = np.array([p["H"] for p in pairs], np.int32)
    # (one spare row: an empty side still has a valid pointer)
    pad = lambda a, w: np.concatenate([a, np.zeros((1, w), np.float32)])  # noqa: E731
    return (_t(pad(cat("desc_l", 64), 64)), _t(pad(cat("desc_r", 64), 64)),
            _t(pad(cat("kp_l", 2), 2)), _t(pad(cat("kp_r", 2), 2)), _t(ol), _t(orr), _t(W), _t(H),
            int(np.diff(ol).max()) if max_nq is None else max_nq,
            int(np.diff(orr).max()) if max_nt is None else max_nt)


def _records(pairs, res_status=None, win_status=None):
    """result records as a find could have left them (distinct bytes everywhere, so a copy is
    checkable) and winner records that carry each pair's E"""
    from erp_match_eightpoint_test_amd import capi
    n = len(pairs)
    res = np.frombuffer(np.random.default_rng(3).bytes(64 * n), capi.RESULT_DTYPE).copy()
    win = np.zeros(n, capi.WINNER_DTYPE)
    res["status"] = 0 if res_status is None else res_status
    win["status"] = 0 if win_status is None else win_status
    for i, p in enumerate(pairs):
        win[i]["E"] = p["e"]
        win[i]["iter"], win[i]["which"], win[i]["sample_n"] = 5 + i, 1, 77
    return res, win


def _call(ctx, pairs, thr, ratio=0.8, max_dist=0.0, unique=True, res=None, win=None,
          max_nq=None, max_nt=None, results=True):
    """Context.guided_match on host pairs (winner records as the source) -> host copies"""
    import torch
    from erp_match_eightpoint_test_amd import capi
    n = len(pairs)
    if res is None:
        res, win = _records(pairs)
    b = _batch(pairs, max_nq, max_nt)
    want = [k for k in ctx.GUIDED_WANT if results or k != "results"]
    o = ctx.guided_match(*b, _t(win.view(np.uint8).reshape(n, 88)), 16, 0,
                         results=_t(res.view(np.uint8).reshape(n, 64)) if results else None,
                         thr=thr, ratio=ratio, max_dist=max_dist, unique=unique, want=want)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    out["matches"] = out["matches"].view(capi.DMATCH_DTYPE).reshape(n, -1)
    out["winners"] = out["winners"].view(capi.WINNER_DTYPE).reshape(-1)
    if results:
        out["results"] = out["results"].view(capi.RESULT_DTYPE).reshape(-1)
    out["res_in"], out["win_in"] = res, win
    return out


def _equals_chain(tag, out, i, ref):
    """pair i of a call against the chain's dict, exactly; zeros from the count up"""
    m = int(out["count"][i])
    assert m == ref["count"], (tag, m, ref["count"])
    assert out["matches"][i, :m].tobytes() == ref["matches"].tobytes(), tag
    assert out["key_left"][i, :m].tobytes() == ref["key_left"].tobytes(), tag
    assert out["key_right"][i, :m].tobytes() == ref["key_right"].tobytes(), tag
    assert int(out["gated"][i]) == ref["gated"], (tag, int(out["gated"][i]), ref["gated"])
    assert not out["matches"][i, m:].tobytes().strip(b"\0"), tag
    assert not out["key_left"][i, m:].any() and not out["key_right"][i, m:].any(), tag
    if "results" in out:
        want = out["res_in"][i].copy()
        want["M"] = m
        assert out["results"][i].tobytes() == want.tobytes(), tag
    w, wi = out["winners"][i], out["win_in"][i]
    assert (w["status"], w["iter"], w["which"], w["sample_n"]) == (0, -1, 0, 0), (tag, w)
    assert w["E"].tobytes() == wi["E"].tobytes(), tag


def _zero_pair(tag, out, i, status):
    """a pair with a status: count 0, zeros, M = 0, a winner record with the status only"""
    assert out["count"][i] == 0 and out["gated"][i] == 0, tag
    assert not out["matches"][i].tobytes().strip(b"\0"), tag
    assert not out["key_left"][i].any() and not out["key_right"][i].any(), tag
    want = out["res_in"][i].copy()
    want["M"] = 0
    assert out["results"][i].tobytes() == want.tobytes(), tag
    w = out["winners"][i].copy()
    assert w["status"] == status, (tag, w)
    w["status"] = 0
    assert not w.tobytes().strip(b"\0"), tag


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from erp_match_eightpoint_test_amd import Context
    return Context(0)


# ------------------------------------------------------------- 1. the ragged batch
@pytest.fixture(scope="module")
def ragged(ctx, oracle):
    """the ragged batch under every setting, one call each; computed once and never modified"""
    pairs = GR.ragged_pairs(oracle)
    return {s: _call(ctx, pairs, s[0], 0.8, s[2], s[1], max_nq=MAX_NQ, max_nt=MAX_NT)
            for s in SETTINGS}


@pytest.mark.parametrize("thr,unique,max_dist", SETTINGS)
def test_ragged_batch_equals_the_chain(ragged, oracle, thr, unique, max_dist):
    out = ragged[(thr, unique, max_dist)]
    preps = GR.ragged_prepared(oracle, thr)
    assert out["matches"].shape[1] == MAX_NQ > max(nq for nq, _ in GR.RAGGED)
    total = 0
    for i, prep in enumerate(preps):
        ref = GR.select(prep, 0.8, max_dist, unique)
        assert ref["ambiguous"] == 0
        _equals_chain(f"pair {GR.RAGGED[i]} thr {thr} unique {unique} max_dist {max_dist}", out, i,
                      ref)
        total += ref["count"]
    assert total > 100   # (the host test shows what the settings change)
    for i, (nq, nt) in enumerate(GR.RAGGED):
        if nq == 0 or nt == 0:
            assert out["count"][i] == 0 and out["winners"][i]["status"] == 0


def test_thr_one_equals_knn2_ratio(ctx, oracle):
    """thr = 1 gates everything (|l^T E' r| <= 0.7072): with unique and max_dist off the list is
    erp_match_knn2_ratio's at the same ratio, bit for bit -- every tile here overflows any item
    list, so this is the per-lane loop of the gate kernel"""
    from erp_match_eightpoint_test_amd import capi, feature_matcher
    pairs = GR.ragged_pairs(oracle)
    fm = feature_matcher(ctx=ctx)
    seen = 0
    for ratio in (0.3, 0.8):
        out = _call(ctx, pairs, 1.0, ratio, 0.0, False, max_nq=MAX_NQ, max_nt=MAX_NT)
        for i, (nq, nt) in enumerate(GR.RAGGED):
            if nq == 0 or nt < 2:
                continue
            p = pairs[i]
            assert int(out["gated"][i]) == nq * nt
            plain = fm._match_device(_t(p["desc_l"]), _t(p["desc_r"]), ratio).cpu().numpy()
            plain = np.ascontiguousarray(plain).view(capi.DMATCH_DTYPE).reshape(-1)
            m = int(out["count"][i])
            assert m == len(plain) and out["matches"][i, :m].tobytes() == plain.tobytes()
            seen += m
    assert seen > 100


# ------------------------------------------------------------- 2. ties and rules
@pytest.fixture(scope="module")
def tie_base(oracle):
    """a 64 x 64 pair, a query i whose true partner j is gated at thr 0.01 with at least one
    other gated row, and a train row `far` that is not gated for i"""
    p, e = GR.pair_e(oracle, 31, 64, 0.03)
    prep = GR.prepare(oracle, p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"], p["H"], e,
                      0.01)
    bl = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_l"])
    br = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_r"])
    g, amb = GR.gate(oracle, bl, br, oracle.rank2(e), 0.01)
    assert amb == 0
    for i in range(64):
        j = int(p["gt_partner"][i])
        if j >= 0 and g[i, j] and g[i].sum() >= 2 and prep["top"][i][0] == j and not g[i].all():
            far = int(np.flatnonzero(~g[i])[0])
            return {"p": p, "e": e, "i": i, "j": j, "far": far}
    raise AssertionError("no query with a gated partner and a second gated row")


def _variant(tb, desc_r=None, kp_r=None, desc_l=None, kp_l=None):
    p = tb["p"]
    return {"desc_l": p["desc_l"] if desc_l is None else desc_l,
            "desc_r": p["desc_r"] if desc_r is None else desc_r,
            "kp_l": p["kp_l"] if kp_l is None else kp_l,
            "kp_r": p["kp_r"] if kp_r is None else kp_r, "W": p["W"], "H": p["H"], "e": tb["e"]}


def _chain_of(oracle, v, thr, ratio, max_dist, unique):
    ref = GR.guided(oracle, v["desc_l"], v["desc_r"], v["kp_l"], v["kp_r"], v["W"], v["H"], v["e"],
                    thr, ratio, max_dist, unique)
    assert ref["ambiguous"] == 0
    return ref


def test_duplicate_train_row_inside_and_outside_the_gate(ctx, oracle, tie_base):
    p, i, j, far = tie_base["p"], tie_base["i"], tie_base["j"], tie_base["far"]
    dup_d = np.concatenate([p["desc_r"], p["desc_r"][j:j + 1]])
    inside = _variant(tie_base, dup_d, np.concatenate([p["kp_r"], p["kp_r"][j:j + 1]]))
    outside = _variant(tie_base, dup_d, np.concatenate([p["kp_r"], p["kp_r"][far:far + 1]]))
    got = {}
    for name, v in (("inside", inside), ("outside", outside)):
        for ratio in (1.0, 2.0):
            out = _call(ctx, [v], 0.01, ratio, 0.0, False)
            _equals_chain(f"duplicate {name} ratio {ratio}", out, 0,
                          _chain_of(oracle, v, 0.01, ratio, 0.0, False))
            m = out["matches"][0, :out["count"][0]]
            got[(name, ratio)] = m[m["queryIdx"] == i]
    # both copies gated: d0 = d1, rejected at ratio 1; accepted at ratio 2 with the LOWER index
    assert len(got[("inside", 1.0)]) == 0
    assert got[("inside", 2.0)]["trainIdx"].tolist() == [j]
    # one copy outside the gate: d1 is another row's, the query is accepted at ratio 1
    assert got[("outside", 1.0)]["trainIdx"].tolist() == [j]
    # equal e takes the lowest j also when the copy comes first
    first_d = np.concatenate([p["desc_r"][j:j + 1], p["desc_r"]])
    first = _variant(tie_base, first_d, np.concatenate([p["kp_r"][j:j + 1], p["kp_r"]]))
    out = _call(ctx, [first], 0.01, 2.0, 0.0, False)
    _equals_chain("copy first", out, 0, _chain_of(oracle, first, 0.01, 2.0, 0.0, False))
    m = out["matches"][0, :out["count"][0]]
    assert m[m["queryIdx"] == i + 0]["trainIdx"].tolist() == [0]


def test_two_identical_queries_claim_one_row_lowest_i_wins(ctx, oracle, tie_base):
    p, i, j = tie_base["p"], tie_base["i"], tie_base["j"]
    v = _variant(tie_base, desc_l=np.concatenate([p["desc_l"], p["desc_l"][i:i + 1]]),
                 kp_l=np.concatenate([p["kp_l"], p["kp_l"][i:i + 1]]))
    both = _call(ctx, [v], 0.01, 0.8, 0.0, False)
    _equals_chain("twins, unique off", both, 0, _chain_of(oracle, v, 0.01, 0.8, 0.0, False))
    m = both["matches"][0, :both["count"][0]]
    twins = m[m["trainIdx"] == j]
    assert twins["queryIdx"].tolist() == [i, 64]
    assert twins["distance"][0].tobytes() == twins["distance"][1].tobytes()
    one = _call(ctx, [v], 0.01, 0.8, 0.0, True)
    _equals_chain("twins, unique on", one, 0, _chain_of(oracle, v, 0.01, 0.8, 0.0, True))
    m = one["matches"][0, :one["count"][0]]
    assert m[m["trainIdx"] == j]["queryIdx"].tolist() == [i]


def test_nan_keypoints_are_never_gated_and_change_no_status(ctx, oracle, tie_base):
    p, i, j = tie_base["p"], tie_base["i"], tie_base["j"]
    kp_l, kp_r = p["kp_l"].copy(), p["kp_r"].copy()
    other = (i + 1) % 64
    kp_l[other] = (np.nan, 100.0)
    kp_r[j] = (200.0, np.nan)
    v = _variant(tie_base, kp_l=kp_l, kp_r=kp_r)
    for thr in (0.01, 1.0):
        out = _call(ctx, [v], thr, 0.8, 0.0, True)
        _equals_chain(f"NaN keypoints thr {thr}", out, 0, _chain_of(oracle, v, thr, 0.8, 0.0, True))
        m = out["matches"][0, :out["count"][0]]
        assert other not in m["queryIdx"] and j not in m["trainIdx"]
        assert out["winners"][0]["status"] == 0 and out["results"][0]["status"] == 0
    assert int(out["gated"][0]) == 63 * 63   # thr 1: every finite (i, j)


# ------------------------------------------------------------- 3. status rules
def test_status_pairs_give_zeros_and_leave_their_neighbours_alone(ctx, oracle, ragged):
    pairs = GR.ragged_pairs(oracle)
    rs, ws = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
    rs[3], ws[5], rs[6], ws[6] = ERP_TOO_FEW_POINTS, ERP_INTERNAL, ERP_TOO_FEW_POINTS, ERP_INTERNAL
    res, win = _records(pairs, rs, ws)
    s = (0.01, True, 0.0)
    out = _call(ctx, pairs, s[0], 0.8, s[2], s[1], res=res, win=win, max_nq=MAX_NQ, max_nt=MAX_NT)
    base = ragged[s]
    _zero_pair("result status", out, 3, ERP_TOO_FEW_POINTS)
    _zero_pair("winner status", out, 5, ERP_INTERNAL)
    _zero_pair("both: the result's comes first", out, 6, ERP_TOO_FEW_POINTS)
    for i in (0, 1, 2, 4, 7, 8):
        for k in ("count", "matches", "key_left", "key_right", "gated", "results", "winners"):
            assert out[k][i].tobytes() == base[k][i].tobytes(), (i, k)
    assert base["count"][3] > 0 and base["count"][5] > 0 and base["count"][6] > 0


# ------------------------------------------------------------- 4. independence and determinism
def test_each_pair_alone_gives_the_batch_bytes_and_runs_repeat(ctx, oracle, ragged):
    pairs = GR.ragged_pairs(oracle)
    s = (0.003, True, 0.8)
    base = ragged[s]
    again = _call(ctx, pairs, s[0], 0.8, s[2], s[1], max_nq=MAX_NQ, max_nt=MAX_NT)
    for k in ("count", "matches", "key_left", "key_right", "gated", "results", "winners"):
        assert again[k].tobytes() == base[k].tobytes(), k
    for i, p in enumerate(pairs):
        res, win = _records(pairs)
        one = _call(ctx, [p], s[0], 0.8, s[2], s[1], res=res[i:i + 1], win=win[i:i + 1],
                    max_nq=MAX_NQ, max_nt=MAX_NT)
        for k in ("count", "matches", "key_left", "key_right", "gated", "results", "winners"):
            assert one[k][0].tobytes() == base[k][i].tobytes(), (GR.RAGGED[i], k)


def test_scratch_canaries_are_intact(gpu_lib, oracle, ragged):
    """a fresh context allocates every buffer of the stage with canary bytes behind it; none is
    touched.  The pad goes back to 0 (after the context is gone: its buffers are on record)."""
    from erp_match_eightpoint_test_amd import Context, feature_matcher
    pairs = GR.ragged_pairs(oracle)
    gpu_lib.erp_debug_set_alloc_pad(256)
    try:
        c = Context(0)
        for s in ((0.01, True, 0.8), (1.0, False, 0.0)):
            out = _call(c, pairs, s[0], 0.8, s[2], s[1], max_nq=MAX_NQ, max_nt=MAX_NT)
            if s in ragged:
                assert out["matches"].tobytes() == ragged[s]["matches"].tobytes()
        p = pairs[5]
        feature_matcher(ctx=c).match_guided(p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"],
                                            p["H"], p["e"], thr=0.01)
        assert gpu_lib.erp_debug_check_pads() == 0
        c.close()
    finally:
        gpu_lib.erp_debug_set_alloc_pad(0)


# ------------------------------------------------------------- 5. the chain behind find
@pytest.fixture(scope="module")
def chain(gpu_lib, oracle):
    """run(winners) -> polish -> guided_match(source="polish") -> polish -> select_pose for four
    300-keypoint pairs with descriptor noise 0.05; computed once.  The feeding run matches at
    ratio 0.5: at the reference's 0.3 these pairs keep 0 to 3 matches and find returns
    ERP_TOO_FEW_POINTS (the oracle's matcher says so too), so there would be no E to guide
    with; at 0.5 the list has 233 to 239 of the 240 true partners and the guided list all 240."""
    import torch
    from erp_match_eightpoint_test_amd import (PairBatchRunner, polish_rounds_to_numpy,
                                               polish_to_numpy, pose_to_numpy, results_to_numpy,
                                               winners_to_numpy)
    from erp_match_eightpoint_test_amd.capi import DMATCH_DTYPE
    pairs = [GR.pair(s, 300, 0.05) for s in CHAIN_SEEDS]
    b = _batch(pairs)
    run = PairBatchRunner(iters=PR.ITERS)
    outs = run.run(*b, ratio=CHAIN_RUN_RATIO, want=("winners", "key_left", "key_right"))
    pol = run.polish(outs, b[6], b[7], CHAIN_THR, rounds=PR.ROUNDS)
    g = run.guided_match(outs, *b, source="polish", polish=pol, thr=CHAIN_THR, ratio=0.8,
                         max_dist=0.8, unique=True)
    pol2 = run.polish(g, b[6], b[7], CHAIN_THR, rounds=PR.ROUNDS, want_rounds=True)
    pose = run.select_pose(g, b[6], b[7], source="polish", polish=pol2)
    torch.cuda.synchronize()
    return {"pairs": pairs, "run": run, "W": b[6], "H": b[7], "max_nq": b[8],
            "res": results_to_numpy(outs["results"]).copy(),
            "polish": polish_to_numpy(pol["polish"]).copy(),
            "g": {"count": g["count"].cpu().numpy(), "gated": g["gated"].cpu().numpy(),
                  "matches": g["matches"].cpu().numpy().view(DMATCH_DTYPE).reshape(len(pairs), -1),
                  "key_left": g["key_left"].cpu().numpy(), "key_right": g["key_right"].cpu().numpy(),
                  "results": results_to_numpy(g["results"]).copy(),
                  "winners": winners_to_numpy(g["winners"]).copy()},
            "polish2": polish_to_numpy(pol2["polish"]).copy(),
            "rounds2": polish_rounds_to_numpy(pol2["rounds"]).copy(),
            "mask2": pol2["mask"].cpu().numpy(), "pose": pose_to_numpy(pose["pose"]).copy(),
            "depth": pose["depth"].cpu().numpy(), "front": pose["front"].cpu().numpy(),
            "pose_results": pose["results"]}


@pytest.mark.parametrize("k", range(len(CHAIN_SEEDS)))
def test_chain_guided_list_then_polish_then_pose(chain, oracle, k):
    from test_gpu_pose import _against_chain
    p, g = chain["pairs"][k], chain["g"]
    res, pol = chain["res"][k], chain["polish"][k]
    assert res["status"] == 0 and pol["status"] == 0
    # the guided list: the chain fed the GPU's own polished E
    ref = GR.guided(oracle, p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"], p["H"],
                    pol["E"], CHAIN_THR, 0.8, 0.8, True)
    assert ref["ambiguous"] == 0, "an (i, j) within 1e-9 of the threshold under the GPU's E"
    out = dict(g, res_in=chain["res"], win_in=chain["polish"])
    _equals_chain(f"chain seed {CHAIN_SEEDS[k]}", out, k, ref)
    M = ref["count"]
    print(f"seed {CHAIN_SEEDS[k]}: plain list {res['M']}, guided {M}, at the true partner "
          f"{GR.n_correct(p, ref['matches'])} of {GR.n_partners(p)}")
    assert M == GR.n_partners(p) > res["M"] > 200 and GR.n_correct(p, ref["matches"]) == M
    # the polish on the guided dict, round by round against the oracle on the GPU's own records
    # (tests/test_gpu_polish.py's check)
    bl = oracle.pixel_to_bearing(p["W"], p["H"], g["key_left"][k, :M])
    br = oracle.pixel_to_bearing(p["W"], p["H"], g["key_right"][k, :M])
    p2, rounds = chain["polish2"][k], chain["rounds2"][k]

    def gpu_set(E):
        S, near = PR.mask_of(oracle, bl, br, oracle.rank2(E), CHAIN_THR, 1e-12)
        assert near == 0
        return S
    assert p2["status"] == 0 and (p2["winner_iter"], p2["winner_which"]) == (-1, 0)
    S_prev, R_prev, T_prev = gpu_set(pol["E"]), g["results"][k]["R"], g["results"][k]["T"]
    assert p2["n_inliers_winner"] == int(S_prev.sum()) == M   # (guided matches ARE inliers)
    for r in range(int(p2["rounds_done"])):
        rd = rounds[r]
        f = PR.refit(oracle, bl, br, S_prev, R_prev, T_prev)
        assert f is not None and rd["n_fit"] == int(S_prev.sum())
        sign = 1.0 if float(np.dot(rd["E"], f["e"])) >= 0 else -1.0
        assert np.abs(sign * rd["E"] - f["e"]).max() <= 1e-6
        assert np.abs(rd["R"] - f["R"]).max() <= 1e-6 and np.abs(rd["T"] - f["T"]).max() <= 1e-6
        S = gpu_set(rd["E"])
        assert rd["n_inliers"] == int(S.sum()) >= int(S_prev.sum())
        S_prev, R_prev, T_prev = S, rd["R"], rd["T"]
    assert p2["n_inliers"] == int(S_prev.sum())
    assert np.array_equal(chain["mask2"][k, :M], S_prev.astype(np.uint8))
    assert not chain["mask2"][k, M:].any()
    # the pose selection on the guided dict against tests/pose_ref.py's chain
    sel = _against_chain(oracle, f"chain seed {CHAIN_SEEDS[k]}", chain["pose"][k],
                         chain["depth"][k], chain["front"][k], bl, br, p2["E"], g["results"][k],
                         mask=chain["mask2"][k], thr=0.0)
    assert sel["n_voters"] == p2["n_inliers"]
    assert PR.euler_err(chain["pose"][k]["R"], p) < 0.01


def test_chain_results_feed_rectify_batch(chain):
    import torch
    from erp_match_eightpoint_test_amd import erp_rotation
    n = len(CHAIN_SEEDS)
    rng = np.random.default_rng(5)
    left, right = (_t(rng.integers(0, 256, (n, 32, 64, 3), dtype=np.uint8)) for _ in range(2))
    got = erp_rotation(ctx=chain["run"].ctx).rectify_batch(left, right,
                                                           results=chain["pose_results"],
                                                           vertical=False, fill=7)
    torch.cuda.synchronize()
    assert got["done"].cpu().numpy().tolist() == [1] * n


# ------------------------------------------------------------- 6. invalid arguments
def test_invalid_arguments_are_refused_before_any_gpu_work(ctx, oracle):
    import ctypes as C
    import torch
    from erp_match_eightpoint_test_amd import capi
    pairs = GR.ragged_pairs(oracle)[2:4]
    b = _batch(pairs)
    _, win = _records(pairs)
    src = _t(win.view(np.uint8).reshape(2, 88))
    count = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    matches = torch.full((2, b[8], 4), -7, dtype=torch.int32, device="cuda")

    def call(thr=0.01, ratio=0.8, max_dist=0.0, dim=64, e_off=16, max_nq=b[8]):
        batch = capi.PairBatch(2, dim, max_nq, b[9], *[t.data_ptr() for t in b[:8]])
        inp = capi.GuidedInputs(batch, None, src.data_ptr() + e_off, 88, src.data_ptr(), 88)
        out = capi.GuidedOutputs(count.data_ptr(), matches.data_ptr())
        cfg = capi.GuidedCfg(thr, ratio, max_dist, 1)
        return ctx.L.erp_match_guided_dev(ctx.h, C.byref(inp), C.byref(cfg), C.byref(out),
                                          torch.cuda.current_stream().cuda_stream)
    nan = float("nan")
    bad = [dict(thr=0.0), dict(thr=-1.0), dict(thr=nan), dict(ratio=0.0), dict(ratio=-0.5),
           dict(ratio=nan), dict(max_dist=nan), dict(dim=128), dict(e_off=12),
           dict(max_nq=65536)]
    for kw in bad:
        assert call(**kw) == ERP_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert (count == -7).all() and (matches == -7).all()   # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert (count >= 0).all()


# ------------------------------------------------------------- 7. host entry point, C++ driver
def test_host_entry_point_and_cpp_driver_give_the_device_list(ctx, oracle, ragged, tmp_path):
    from erp_match_eightpoint_test_amd import _build, capi, feature_matcher
    i = 5   # (130, 200)
    p = GR.ragged_pairs(oracle)[i]
    fm = feature_matcher(ctx=ctx)
    driver = _build.build_guided_driver()
    for s in ((0.01, True, 0.8), (0.003, False, 0.0)):
        base = ragged[s]
        dev = base["matches"][i, :base["count"][i]]
        assert len(dev) > 20
        host = fm.match_guided(p["desc_l"], p["desc_r"], p["kp_l"], p["kp_r"], p["W"], p["H"],
                               p["e"], thr=s[0], ratio=0.8, max_dist=s[2], unique=s[1])
        assert host.tobytes() == dev.tobytes()
        ind, outd = tmp_path / f"in{s[0]}", tmp_path / f"out{s[0]}"
        ind.mkdir()
        outd.mkdir()
        np.array([p["W"], p["H"], len(p["desc_l"]), len(p["desc_r"]), int(s[1])],
                 np.int32).tofile(ind / "meta.i32")
        np.array([s[0], 0.8, s[2]], np.float32).tofile(ind / "cfg.f32")
        np.asarray(p["e"], np.float64).tofile(ind / "e.f64")
        for name, a in (("d1", p["desc_l"]), ("d2", p["desc_r"]), ("k1", p["kp_l"]),
                        ("k2", p["kp_r"])):
            np.ascontiguousarray(a, np.float32).tofile(ind / f"{name}.f32")
        r = subprocess.run([driver, str(ind), str(outd)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(outd / "matches.bin", capi.DMATCH_DTYPE)
        assert got.tobytes() == dev.tobytes()
    # an empty side and a lone train row
    assert len(fm.match_guided(p["desc_l"][:0], p["desc_r"], p["kp_l"][:0], p["kp_r"], p["W"],
                               p["H"], p["e"], thr=0.01)) == 0
    assert len(fm.match_guided(p["desc_l"], p["desc_r"][:0], p["kp_l"], p["kp_r"][:0], p["W"],
                               p["H"], p["e"], thr=0.01)) == 0


# ------------------------------------------------------------- 8. the shared host staging slot
def test_host_entry_points_share_one_staging_slot(gpu_lib, oracle):
    """erp_match_guided, erp_eight_point_find_posed and erp_eight_point_find_polished stage
    through one scratch slot of the context.  Back to back on ONE context, with sizes that grow
    the slot and then use less of it -- match_guided (40, 40), find_posed m = 700, find_polished
    m = 9, match_guided (40, 40) again --, every output equals, byte for byte, the same call on a
    fresh context: a wrong size or a stale pointer in the shared slot would show here.  80
    iterations, the default seed / offset, no rand stream."""
    from erp_match_eightpoint_test_amd import (Context, ErpError, eight_point, feature_matcher,
                                               synth)
    g, e = GR.pair_e(oracle, 28, 40, 0.03)
    assert len(g["desc_l"]) == 40 and len(g["desc_r"]) == 40
    p = synth.make_pair(41, n_kpts=1024)
    idx = np.flatnonzero(p["gt_partner"] >= 0)[:700]
    assert len(idx) == 700
    kl, kr = p["kp_l"][idx], p["kp_r"][p["gt_partner"][idx]]
    thr = 0.01

    def guided(c):
        m = feature_matcher(ctx=c).match_guided(g["desc_l"], g["desc_r"], g["kp_l"], g["kp_r"],
                                                g["W"], g["H"], e, thr=thr)
        return [m.tobytes()]

    def posed(c):
        ep = eight_point(ctx=c, iters=80)
        ret = ep.find_posed(p["W"], p["H"], kl, kr, thr, 3)
        assert ep.last_pose["status"] == 0
        return [a.tobytes() for a in (*ret, ep.last_result, ep.last_polish, ep.last_pose)]

    def polished(c):
        ep = eight_point(ctx=c, iters=80)
        try:   # (nine matches: whatever find makes of them, the records are compared)
            ret = ep.find_polished(p["W"], p["H"], kl[:9], kr[:9], thr, 3)
        except ErpError as err:
            ret = (np.int32(err.status),)
        return [a.tobytes() for a in (*ret, ep.last_result, ep.last_polish)]

    calls = (guided, posed, polished, guided)
    shared = Context(0)
    got = [f(shared) for f in calls]
    assert len(np.frombuffer(got[0][0], np.uint8)) > 0   # (the guided list is not empty)
    for k, f in enumerate(calls):
        fresh = Context(0)
        assert f(fresh) == got[k], f.__name__
        fresh.close()
    assert got[3] == got[0]
    shared.close()
