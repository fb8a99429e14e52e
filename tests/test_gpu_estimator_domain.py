"""The estimator at the edges of its input domain (tests/estimator_domain.py builds the inputs,
test_estimator_domain_host.py pins what the oracle does on them):

A. valid_abs through every route: K = 0 (valid_abs 0, -1, NaN -> ERP_NO_VALID_HYPOTHESIS and the
   stages behind a status-3 record), K = 2 iters (valid_abs 4: the capacity edge of the consensus
   rows, angles up to pi) and K = 1, 2, 3, 5 arriving through the validity compaction.
B. keypoints at and beyond the image (finite: parity; non-finite: ERP_INVALID_ARG for the pair,
   the other pairs of a batch untouched).
C. the scale of caller bearings through erp_initial_guess (the fixed-point Gram) against the
   exactly scale-invariant oracle, and against erp_eight_point_estimation (the fp64 Gram).

Bars: R, T within TOL_RT = 1e-6 of the oracle, E within 1e-6 up to sign; K, statuses, sample
sets and integer fields exact.  Both consensus routes (ERP_OPT_SMALL_BATCH 0 / 1000000).
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimator_domain as D  # noqa: E402
from parity_log import record  # noqa: E402
from test_gpu_parity import TOL_RT, _batch, _check_batch_vs_oracle, _check_hyps  # noqa: E402

pytestmark = pytest.mark.gpu

ROUTES = {"prune": 0, "all_rows": 1000000}
NO_VALID = {"0": 0.0, "-1": -1.0, "nan": float("nan")}
THR = 0.01  # the polish's inlier threshold


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from erp_match_eightpoint_test_amd import Context
    return Context(0)


@pytest.fixture(params=list(ROUTES))
def route(request, ctx):
    ctx.set_option("small_batch", ROUTES[request.param])
    yield request.param
    ctx.set_option("small_batch", -1)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _oracle_find(name: str, iters: int, va_key):
    """the oracle's find on a scene; va_key: a float or a key of NO_VALID"""
    import oracle
    c = D.scene(name)
    va = NO_VALID[va_key] if isinstance(va_key, str) else va_key
    return oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"],
                       oracle.make_cfg(iters=iters, valid_abs=va), detail=True)


def _find(ctx, kl, kr, W, H, cfg, with_hyps=True):
    """erp_eight_point_find_winner_dev on host keypoints, with records or on the lite route ->
    host copies (res, win, hyps) and the device tensors shaped for the stages behind"""
    import torch
    from erp_match_eightpoint_test_amd import capi
    m = len(kl)
    d = {"kl": _t(np.asarray(kl, np.float32)).reshape(1, m, 2),
         "kr": _t(np.asarray(kr, np.float32)).reshape(1, m, 2),
         "W": _t(np.array([W], np.int32)), "H": _t(np.array([H], np.int32)),
         "res": torch.zeros((1, capi.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda"),
         "win": torch.full((1, capi.WINNER_DTYPE.itemsize), 0xAB, dtype=torch.uint8, device="cuda"),
         "hyps": torch.zeros((1, cfg.iters, capi.HYP_DTYPE.itemsize), dtype=torch.uint8,
                             device="cuda") if with_hyps else None}
    st = ctx.L.erp_eight_point_find_winner_dev(
        ctx.h, W, H, d["kl"].data_ptr(), d["kr"].data_ptr(), m, C.byref(cfg), d["res"].data_ptr(),
        d["hyps"].data_ptr() if with_hyps else None, d["win"].data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    # erp_eight_point_find_dev is the same call without the winner stage: the same record
    plain = torch.zeros_like(d["res"])
    st = ctx.L.erp_eight_point_find_dev(
        ctx.h, W, H, d["kl"].data_ptr(), d["kr"].data_ptr(), m, C.byref(cfg), plain.data_ptr(),
        None, torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    assert torch.equal(plain, d["res"])
    return {"res": d["res"].cpu().numpy().view(capi.RESULT_DTYPE).reshape(-1)[0],
            "win": d["win"].cpu().numpy().view(capi.WINNER_DTYPE).reshape(-1)[0],
            "hyps": d["hyps"].cpu().numpy().view(capi.HYP_DTYPE).reshape(-1) if with_hyps else None,
            "dev": d}


def _behind(ctx, res, hyps, win, kl, kr, W, H, valid_abs):
    """the stages behind the result records: the polish from the records (where given) and from
    the winners, the pose selection on the winners and on the polish -> host copies"""
    import torch
    from erp_match_eightpoint_test_amd import polish_to_numpy, pose_to_numpy, results_to_numpy
    out = {}
    pols = {"pol_win": ctx.polish(res, None, kl, kr, W, H, THR, rounds=3, valid_abs=valid_abs,
                                  winners=win)}
    if hyps is not None:
        pols["pol_rec"] = ctx.polish(res, hyps, kl, kr, W, H, THR, rounds=3, valid_abs=valid_abs)
    poses = {"pose_win": ctx.select_pose(res, kl, kr, W, H, win, 16, 0),
             "pose_pol": ctx.select_pose(res, kl, kr, W, H, pols["pol_win"]["polish"], 48, 24,
                                         mask=pols["pol_win"]["mask"])}
    torch.cuda.synchronize()
    for k, v in pols.items():
        out[k] = {"rec": polish_to_numpy(v["polish"]), "mask": v["mask"].cpu().numpy()}
    for k, v in poses.items():
        out[k] = {"rec": pose_to_numpy(v["pose"]), "depth": v["depth"].cpu().numpy(),
                  "front": v["front"].cpu().numpy(),
                  "results": results_to_numpy(v["results"]), "results_dev": v["results"]}
    return out


def _zero_but_status(rec):
    r = rec.copy()
    r["status"] = 0
    return not r.tobytes().strip(b"\0")


def _winner_of(hyps, min_idx):
    """(iteration, which) of the record that pushed row min_idx: R1 then R2 per record"""
    flags = np.stack([hyps["R1_valid"] != 0, hyps["R2_valid"] != 0], 1).reshape(-1)
    rows = np.nonzero(flags)[0]
    assert 0 <= min_idx < len(rows), (min_idx, len(rows))
    return int(rows[min_idx] // 2), int(rows[min_idx] % 2)


def _assert_status_record(r, status, M, o):
    """a result record of a pair without an answer: the status, zeros, M and sample_n"""
    assert r["status"] == status, r
    assert r["min_idx"] == -1 and not r["R"].any() and not r["T"].any() and r["min_dist"] == 0, r
    assert r["M"] == M and r["sample_n"] == o["sample_n"], (r, o["sample_n"])


def _assert_behind_carry(b, p, status, res_in):
    """pair p of every stage behind: the status and zeros; mask, depth and front zero;
    results_out byte-equal to the input record"""
    for k, v in b.items():
        assert v["rec"][p]["status"] == status and _zero_but_status(v["rec"][p]), (k, v["rec"][p])
        if "mask" in v:
            assert not v["mask"][p].any(), k
        else:
            assert not v["depth"][p].any() and not v["front"][p].any(), k
            assert v["results"][p].tobytes() == res_in[p].tobytes(), k


def _assert_against_oracle(tag, r, o):
    dr, dt = np.abs(r["R"] - o["R"]).max(), np.abs(r["T"] - o["T"]).max()
    record(tag, R=dr, T=dt)
    print(f"{tag}: |dR| {dr:.3g} |dT| {dt:.3g}")
    assert r["status"] == 0 and r["K"] == o["K"] and r["sample_n"] == o["sample_n"], (r, o["K"])
    assert dr <= TOL_RT and dt <= TOL_RT, (tag, dr, dt)


# ------------------------------------------------------------------ A1: K = 0, status 3
@pytest.mark.parametrize("va", list(NO_VALID))
def test_no_valid_hypothesis_find_dev(ctx, route, va):
    """records route and lite route of the single-pair call, and the stages behind the record"""
    from erp_match_eightpoint_test_amd import default_cfg
    c, o = D.scene("A"), _oracle_find("A", D.ITERS, va)
    cfg = default_cfg(iters=D.ITERS, valid_abs=NO_VALID[va])
    rec = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=True)
    lite = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=False)
    for run in (rec, lite):
        r = run["res"]
        assert r["K"] == 0 == o["K"]
        _assert_status_record(r, 3, len(c["kp_l"]), o)
        assert run["win"]["status"] == 3 and _zero_but_status(run["win"]), run["win"]
    assert lite["res"].tobytes() == rec["res"].tobytes()
    # the hypothesis records are still written, every flag 0
    _check_hyps(rec["hyps"], o["hyp"], fixture=f"domain K=0 (valid_abs {va})")
    assert not rec["hyps"]["R1_valid"].any() and not rec["hyps"]["R2_valid"].any()
    d = rec["dev"]
    b = _behind(ctx, d["res"], d["hyps"], d["win"], d["kl"], d["kr"], d["W"], d["H"], NO_VALID[va])
    _assert_behind_carry(b, 0, 3, np.asarray(rec["res"]).reshape(1))


@pytest.mark.parametrize("va", list(NO_VALID))
def test_no_valid_hypothesis_host_calls(ctx, route, va):
    """erp_eight_point_find and the Python wrappers: ErpError with status 3, zero records"""
    from erp_match_eightpoint_test_amd import ErpError, eight_point
    c, o = D.scene("A"), _oracle_find("A", D.ITERS, va)
    ep = eight_point(ctx=ctx, iters=D.ITERS, valid_abs=NO_VALID[va])
    for call in (lambda: ep.find(c["W"], c["H"], c["kp_l"], c["kp_r"]),
                 lambda: ep.find_winner(c["W"], c["H"], c["kp_l"], c["kp_r"]),
                 lambda: ep.find_posed(c["W"], c["H"], c["kp_l"], c["kp_r"], THR)):
        with pytest.raises(ErpError) as ei:
            call()
        assert ei.value.status == 3
        assert ep.last_result["K"] == 0
        _assert_status_record(ep.last_result, 3, len(c["kp_l"]), o)
    assert ep.last_winner["status"] == 3 and _zero_but_status(ep.last_winner)
    assert ep.last_polish["status"] == 3 and _zero_but_status(ep.last_polish)
    assert ep.last_pose["status"] == 3 and _zero_but_status(ep.last_pose)


@pytest.mark.parametrize("records", [True, False], ids=["records", "lite"])
@pytest.mark.parametrize("va", list(NO_VALID))
def test_no_valid_hypothesis_batch(ctx, route, oracle, va, records):
    """PairBatchRunner.run on 3 ragged pairs (120, 40 and 400 matches), the stages behind its
    records and the rectification from them"""
    import torch
    from erp_match_eightpoint_test_amd import (PairBatchRunner, erp_rotation, hyps_to_numpy,
                                               results_to_numpy, winners_to_numpy)
    names = "ABC"
    args = _batch([D.scene_pair(n) for n in names])
    run = PairBatchRunner(ctx=ctx, iters=D.ITERS, valid_abs=NO_VALID[va])
    want = ("samples", "key_left", "key_right", "winners") + (("hyps",) if records else ())
    out = run.run(*args, want=want)
    torch.cuda.synchronize()
    res, win = results_to_numpy(out["results"]), winners_to_numpy(out["winners"])
    for p, n in enumerate(names):
        c, o = D.scene(n), _oracle_find(n, D.ITERS, va)
        assert res[p]["K"] == 0 == o["K"]
        _assert_status_record(res[p], 3, len(c["kp_l"]), o)
        s = o["sample_n"]
        assert np.array_equal(np.sort(out["samples"][p, :, :s].cpu().numpy(), axis=1),
                              np.sort(o["samples"], axis=1))
        assert win[p]["status"] == 3 and _zero_but_status(win[p])
        if records:
            h = hyps_to_numpy(out["hyps"])[p]
            _check_hyps(h, o["hyp"])
            assert not h["R1_valid"].any() and not h["R2_valid"].any()
    W, H = args[6], args[7]
    b = _behind(ctx, out["results"], out.get("hyps"), out["winners"], out["key_left"],
                out["key_right"], W, H, NO_VALID[va])
    for p in range(3):
        _assert_behind_carry(b, p, 3, res)
    # the rectification leaves such a pair out, from find's records and from the pose's
    rng = np.random.default_rng(5)
    left, right = (_t(rng.integers(0, 256, (3, 32, 64, 3), dtype=np.uint8)) for _ in range(2))
    er = erp_rotation(ctx=ctx)
    for recs in (out["results"], b["pose_win"]["results_dev"]):
        got = er.rectify_batch(left, right, results=recs.contiguous(), vertical=False, fill=7)
        torch.cuda.synchronize()
        assert got["done"].cpu().numpy().tolist() == [0, 0, 0]
        assert (got["left_rectified"] == 7).all() and (got["right_rectified"] == 7).all()


@pytest.mark.parametrize("world", [1, 3])
def test_no_valid_hypothesis_sharded(ctx, world):
    """the hypothesis-block path with the row-sharded consensus: K = 0 in every shard"""
    import torch
    from erp_match_eightpoint_test_amd import dist, hyps_to_numpy, results_to_numpy
    c, o = D.scene("A"), _oracle_find("A", D.ITERS, "0")
    m = len(c["kp_l"])
    res, merged = dist.find_hypothesis_sharded_dev(
        ctx, c["W"], c["H"], _t(c["kp_l"]), _t(c["kp_r"]), m, D.ITERS,
        cfg_kwargs={"valid_abs": 0.0}, emulate_world=world)
    torch.cuda.synchronize()
    r = results_to_numpy(res.view(1, -1))[0]
    assert r["K"] == 0
    _assert_status_record(r, 3, m, o)
    h = hyps_to_numpy(merged.unsqueeze(0))[0]
    _check_hyps(h[:D.ITERS], o["hyp"])
    assert not h["R1_valid"].any() and not h["R2_valid"].any()


# ------------------------------------------------------------ A2: K = 2 iters, every row valid
@pytest.mark.parametrize("iters", [300, 100, 130])
def test_every_rotation_valid_single_pair(ctx, route, oracle, iters):
    """valid_abs = 4: K == 2 iters == the oracle's; the winner record's E is the records' E at
    the located iteration, and the lite route (wave counts of 64 x 2, at 100 and 130 iterations
    with a partial last wave) gives the same bytes"""
    from erp_match_eightpoint_test_amd import default_cfg
    from erp_match_eightpoint_test_amd.dist import min_idx_agrees
    c, o = D.scene("A"), _oracle_find("A", iters, D.VALID_ALL)
    cfg = default_cfg(iters=iters, valid_abs=D.VALID_ALL)
    rec = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=True)
    lite = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=False)
    r, w, h = rec["res"], rec["win"], rec["hyps"]
    assert r["K"] == 2 * iters == o["K"]
    _assert_against_oracle(f"domain K=2 iters ({iters} iterations): result", r, o)
    _check_hyps(h, o["hyp"], fixture=f"domain K=2 iters ({iters} iterations)")
    assert h["R1_valid"].all() and h["R2_valid"].all()
    # every iteration pushes both rotations, and their order within an iteration follows the
    # sign of a noise-level singular vector: the winner is the oracle's row, or
    # its twin of the same iteration; on the GPU's own list it is the oracle's consensus exactly
    ok, _ = min_idx_agrees(r["min_idx"], o["min_idx"], o["hyp"]["R1_valid"], o["hyp"]["R2_valid"])
    assert ok, (r["min_idx"], o["min_idx"])
    rv = np.stack([h["R1"], h["R2"]], 1).reshape(-1, 3)
    assert oracle.consensus(rv)[1] == r["min_idx"]
    assert w["status"] == 0 and (w["iter"], w["which"]) == _winner_of(h, int(r["min_idx"]))
    assert (w["iter"], w["which"]) == (r["min_idx"] // 2, r["min_idx"] % 2)
    assert w["E"].tobytes() == h[w["iter"]]["E"].tobytes()
    assert lite["res"].tobytes() == r.tobytes() and lite["win"].tobytes() == w.tobytes()


def _full_k_child():
    """body of test_every_rotation_valid_batch_canaries (a process of its own: the pad must be
    set before the process's first allocation), modelled on test_gpu_parity._canary_child: the
    same sizes and option set at 600 iterations with valid_abs = 4, so K = 1200 = the row
    buffers' stride and >= kLipMinK"""
    import oracle
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, capi, hyps_to_numpy,
                                               synth, winners_to_numpy)
    oracle.build()
    L = capi.load()
    L.erp_debug_set_alloc_pad(256)
    c = Context(0)
    for name, v in (("small_batch", 0), ("lip2", 1), ("lipg", 3), ("flat_refs", 25),
                    ("refine_hint", 1), ("zoom_levels", 2)):
        c.set_option(name, v)
    iters = 600
    sizes = [300, 310, 290, 305, 320, 295, 300, 315, 285]
    pairs = [synth.make_pair(5200 + i, n_kpts=n) for i, n in enumerate(sizes)]
    outs = PairBatchRunner(ctx=c, iters=iters, valid_abs=D.VALID_ALL).run(
        *_batch(pairs), want=("matches", "hyps", "samples", "rvec", "dist", "winners"))
    torch.cuda.synchronize()
    assert L.erp_debug_check_pads() == 0
    res = _check_batch_vs_oracle(oracle, pairs, outs, iters,
                                 cfg=oracle.make_cfg(iters=iters, valid_abs=D.VALID_ALL))
    assert np.all(res["status"] == 0)
    assert np.all(res["K"] == 2 * iters), res["K"]
    hyps, win = hyps_to_numpy(outs["hyps"]), winners_to_numpy(outs["winners"])
    for p in range(len(pairs)):
        w = win[p]
        assert w["status"] == 0, (p, w)
        assert (w["iter"], w["which"]) == (res[p]["min_idx"] // 2, res[p]["min_idx"] % 2), (p, w)
        assert w["E"].tobytes() == hyps[p][w["iter"]]["E"].tobytes(), p
    print("full K child ok")


def test_every_rotation_valid_batch_canaries(gpu_lib, oracle):
    """9 pairs whose every rotation is valid (K = 1200 = 2 iters) through every pre-pruning
    route with 256 canary bytes behind every context buffer: no canary touched, all statuses OK,
    every stage equal to the oracle's at the same valid_abs, the winners' E the records'"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_estimator_domain as t; "
            "t._full_k_child()" % (here, os.path.dirname(here)))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "full K child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# --------------------------------------------------- A3: K = 1, 2, 3, 5 through the compaction
@pytest.mark.parametrize("k", D.SMALL_KS)
@pytest.mark.parametrize("name", "ABC")
def test_small_k_through_validity_compaction(ctx, route, name, k):
    """valid_abs between the k-th and the (k+1)-th smallest angle of the oracle's run: K == k
    arrives through the compaction, the lite estimates and the winner stage"""
    from erp_match_eightpoint_test_amd import default_cfg
    va = D.valid_abs_for_k(name, k)
    c, o = D.scene(name), _oracle_find(name, D.ITERS, va)
    assert o["K"] == k
    cfg = default_cfg(iters=D.ITERS, valid_abs=va)
    rec = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=True)
    lite = _find(ctx, c["kp_l"], c["kp_r"], c["W"], c["H"], cfg, with_hyps=False)
    r, w, h = rec["res"], rec["win"], rec["hyps"]
    assert r["K"] == k
    _assert_against_oracle(f"domain K={k} scene {name}: result", r, o)
    assert r["min_idx"] == o["min_idx"]
    if k <= 2:
        assert r["min_idx"] == 0  # the trimmed window is empty: row 0
    assert int(h["R1_valid"].sum() + h["R2_valid"].sum()) == k
    assert w["status"] == 0 and (w["iter"], w["which"]) == _winner_of(h, int(r["min_idx"]))
    assert w["E"].tobytes() == h[w["iter"]]["E"].tobytes()
    assert lite["res"].tobytes() == r.tobytes() and lite["win"].tobytes() == w.tobytes()
    d = rec["dev"]
    b = _behind(ctx, d["res"], d["hyps"], d["win"], d["kl"], d["kr"], d["W"], d["H"], va)
    for key, v in b.items():
        assert v["rec"][0]["status"] == 0, (key, v["rec"][0])
    assert b["pol_rec"]["rec"].tobytes() == b["pol_win"]["rec"].tobytes()
    assert (b["pol_rec"]["rec"][0]["winner_iter"], b["pol_rec"]["rec"][0]["winner_which"]) == \
        (w["iter"], w["which"])


# ------------------------------------------------------ B1: finite keypoints beyond the image
def test_edge_keypoints_vs_oracle(ctx, oracle):
    """poles, a negative column, far outside, the bottom row, half a pixel past the border:
    sample sets exact, every hypothesis and the result within the bars, K exact"""
    import torch
    from erp_match_eightpoint_test_amd import (PairBatchRunner, default_cfg, hyps_to_numpy,
                                               results_to_numpy)
    c = D.scene("A")
    kl, kr = D.edge_keypoints()
    o = oracle.find(c["W"], c["H"], kl, kr, oracle.make_cfg(iters=D.ITERS), detail=True)
    assert o["status"] == 0 and o["K"] == 299
    rec = _find(ctx, kl, kr, c["W"], c["H"], default_cfg(iters=D.ITERS), with_hyps=True)
    _check_hyps(rec["hyps"], o["hyp"], fixture="domain edge keypoints")
    _assert_against_oracle("domain edge keypoints: result", rec["res"], o)
    assert rec["res"]["min_idx"] == o["min_idx"] and rec["win"]["status"] == 0
    # the sample sets leave the library through the batch call only: the same pair as a batch
    out = PairBatchRunner(ctx=ctx, iters=D.ITERS).run(
        *_batch([D.pair_from_keys(31, kl, kr, c["W"], c["H"])]), want=("hyps", "samples"))
    torch.cuda.synchronize()
    s = o["sample_n"]
    assert np.array_equal(np.sort(out["samples"][0, :, :s].cpu().numpy(), axis=1),
                          np.sort(o["samples"], axis=1))
    rb = results_to_numpy(out["results"])[0]
    assert rb["M"] == len(kl) and rb["R"].tobytes() == rec["res"]["R"].tobytes()
    _check_hyps(hyps_to_numpy(out["hyps"])[0], o["hyp"])


# -------------------------------------------------------------- B2: non-finite keypoints
@pytest.mark.parametrize("case", ["nan_left", "inf_right", "all_nan"])
def test_nonfinite_keypoint_is_invalid_arg(ctx, route, case):
    """a pair with a non-finite matched keypoint: ERP_INVALID_ARG and zeros, never ERP_OK with
    some K (the oracle, as the reference, silently drops the iterations that sampled the row)"""
    from erp_match_eightpoint_test_amd import ErpError, default_cfg, eight_point
    c = D.scene("A")
    kl, kr = D.nonfinite_cases()[case]
    cfg = default_cfg(iters=D.ITERS)
    rec = _find(ctx, kl, kr, c["W"], c["H"], cfg, with_hyps=True)
    lite = _find(ctx, kl, kr, c["W"], c["H"], cfg, with_hyps=False)
    o = {"sample_n": len(kl) // 4}
    for run in (rec, lite):
        _assert_status_record(run["res"], 1, len(kl), o)
        assert run["win"]["status"] == 1 and _zero_but_status(run["win"]), run["win"]
    d = rec["dev"]
    b = _behind(ctx, d["res"], d["hyps"], d["win"], d["kl"], d["kr"], d["W"], d["H"], 1.57)
    _assert_behind_carry(b, 0, 1, np.asarray(rec["res"]).reshape(1))
    ep = eight_point(ctx=ctx, iters=D.ITERS)
    for call in (lambda: ep.find(c["W"], c["H"], kl, kr),
                 lambda: ep.find_winner(c["W"], c["H"], kl, kr),
                 lambda: ep.find_posed(c["W"], c["H"], kl, kr, THR)):
        with pytest.raises(ErpError) as ei:
            call()
        assert ei.value.status == 1
        _assert_status_record(ep.last_result, 1, len(kl), o)
    assert ep.last_winner["status"] == 1 and _zero_but_status(ep.last_winner)
    assert ep.last_polish["status"] == 1 and _zero_but_status(ep.last_polish)
    assert ep.last_pose["status"] == 1 and _zero_but_status(ep.last_pose)


@pytest.mark.parametrize("share", [0, 1])
def test_nonfinite_keypoint_in_a_batch_touches_no_other_pair(ctx, route, share):
    """4 pairs with known matches (120, 40, 100, 100), a NaN in a matched keypoint of pair 2 --
    with shared replays the representative of match count 100: pair 2 gets ERP_INVALID_ARG, the
    records, hypothesis records and sample sets of pairs 0, 1, 3 are byte-identical to the run
    with the keypoint restored"""
    import torch
    from erp_match_eightpoint_test_amd import (PairBatchRunner, results_to_numpy, synth,
                                               winners_to_numpy)
    cs = [D.scene("A"), D.scene("B"), synth.make_correspondences(21, m=100),
          synth.make_correspondences(22, m=100)]
    pairs = [D.pair_from_keys(40 + i, c["kp_l"], c["kp_r"], c["W"], c["H"])
             for i, c in enumerate(cs)]
    ctx.set_option("sampler_share", share)
    try:
        runs = []
        for poison in (False, True):
            ps = [dict(p) for p in pairs]
            if poison:
                ps[2]["kp_l"] = ps[2]["kp_l"].copy()
                ps[2]["kp_l"][5, 0] = np.nan
            out = PairBatchRunner(ctx=ctx, iters=D.ITERS).run(
                *_batch(ps), want=("hyps", "samples", "winners"))
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy() for k, v in out.items()})
    finally:
        ctx.set_option("sampler_share", -1)
    clean, bad = runs
    rc, rb = (results_to_numpy(torch.from_numpy(r["results"])) for r in runs)
    assert [int(x) for x in rc["M"]] == [120, 40, 100, 100] == [int(x) for x in rb["M"]]
    assert (rc["status"] == 0).all() and (rc["K"] > 0).all()
    _assert_status_record(rb[2], 1, 100, {"sample_n": 25})
    wb = winners_to_numpy(torch.from_numpy(bad["winners"]))
    assert wb[2]["status"] == 1 and _zero_but_status(wb[2])
    for p in (0, 1, 3):
        for k in ("results", "hyps", "samples", "winners"):
            assert clean[k][p].tobytes() == bad[k][p].tobytes(), (p, k)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_bearing_is_invalid_arg(ctx, oracle, bad):
    """erp_initial_guess and erp_eight_point_estimation refuse a non-finite bearing on the host"""
    from erp_match_eightpoint_test_amd import ErpError, eight_point
    c = D.scene("A")
    bl = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_l"])
    br = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_r"])
    ep = eight_point(ctx=ctx)
    for side in (0, 1):
        a, b = bl.copy(), br.copy()
        (a, b)[side][17, 2] = bad
        for call in (ep.initial_guess, ep.eight_point_estimation):
            with pytest.raises(ErpError) as ei:
                call(c["W"], c["H"], a, b)
            assert ei.value.status == 1


# ------------------------------------------------- C: bearing scale through erp_initial_guess
@functools.lru_cache(maxsize=None)
def _bearings():
    import oracle
    c = D.scene("A")
    return (oracle.pixel_to_bearing(c["W"], c["H"], c["kp_l"]),
            oracle.pixel_to_bearing(c["W"], c["H"], c["kp_r"]))


@pytest.mark.parametrize("iters,frac", [(80, 0.25), (1, 0.25), (1, 1.0)])
@pytest.mark.parametrize("scale", D.SCALES, ids=D.SCALE_IDS)
def test_initial_guess_bearing_scale(ctx, oracle, scale, iters, frac):
    """status 0, the oracle's K, R and T within the bar of the oracle's initial_guess on the same
    scaled bearings (exactly scale-invariant for the uniform scales: test_estimator_domain_host).
    With one iteration over every row the answer is also erp_eight_point_estimation's: the
    fixed-point Gram next to the fp64 one"""
    from erp_match_eightpoint_test_amd import eight_point
    c = D.scene("A")
    bl, br = D.scaled_bearings(*_bearings(), scale)
    o = oracle.initial_guess(bl, br, oracle.make_cfg(iters=iters, sample_frac=frac))
    assert o["status"] == 0
    ep = eight_point(ctx=ctx, iters=iters, sample_frac=frac)
    R, T = ep.initial_guess(c["W"], c["H"], bl, br)
    r = ep.last_result
    tag = f"domain bearing scale {D.SCALE_IDS[D.SCALES.index(scale)]}"
    _assert_against_oracle(f"{tag}: iters {iters} frac {frac}", r, o)
    assert np.array_equal(R, r["R"]) and np.array_equal(T, r["T"])
    if frac == 1.0:
        R1, R2, Te, v1, v2, _ = ep.eight_point_estimation(c["W"], c["H"], bl, br)
        assert v1 or v2
        Re = R1 if v1 else R2
        dr, dt = np.abs(R - Re).max(), np.abs(T - Te).max()
        record(f"{tag}: initial_guess against eight_point_estimation", R=dr, T=dt)
        print(f"{tag}: against eight_point_estimation |dR| {dr:.3g} |dT| {dt:.3g}")
        assert dr <= TOL_RT and dt <= TOL_RT, (dr, dt)


def test_initial_guess_wide_row_factors_measured(ctx, oracle):
    """a factor per row and side over [1e-3, 1e3]: measured and recorded, not asserted -- the
    fixed point keeps 44 bits below the largest row's products, so rows a million times smaller
    lose most of their digits (include/erp_match.h erp_initial_guess)"""
    from erp_match_eightpoint_test_amd import ErpError, eight_point
    c = D.scene("A")
    bl, br = D.scaled_bearings(*_bearings(), "rows", 1e-3, 1e3)
    o = oracle.initial_guess(bl, br, oracle.make_cfg(iters=80))
    ep = eight_point(ctx=ctx, iters=80)
    try:
        R, T = ep.initial_guess(c["W"], c["H"], bl, br)
    except ErpError as e:
        print("domain bearing row factors 1e-3..1e3: status", e.status)
        return
    dr, dt = np.abs(R - o["R"]).max(), np.abs(T - o["T"]).max()
    record("domain bearing row factors 1e-3..1e3 (not asserted)", R=dr, T=dt)
    print(f"domain bearing row factors 1e-3..1e3: K {ep.last_result['K']} (oracle {o['K']}) "
          f"|dR| {dr:.3g} |dT| {dt:.3g}")
