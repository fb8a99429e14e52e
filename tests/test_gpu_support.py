"""The support stage on the GPU (include/erp_match.h "support-scored winner", DESIGN.md section
3.19) against tests/support_ref.py on the run's own records.  Every comparison is byte or integer
equality, with one allowance: a count may differ from the oracle's by the matches the oracle
reports within 1e-12 of thr (test_inlier_count_vs_oracle's bar, through inlier_count's `band`),
and a test fails when more than 1 % of its (pair, iteration) cells needed it.

One ragged batch serves most cases: pair k has exactly MS[k] matches (estimator_domain's
pair_from_keys around synth.make_correspondences, 30 % outliers), run at eight iteration counts
with records and lite.  Both forms of the count kernel (Context option support_count) run.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import estimator_domain as ED  # noqa: E402
import polish_ref as PR  # noqa: E402
import support_ref as SR  # noqa: E402

from erp_match_eightpoint_test_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

# s = 2 (thin), 8 / 9 (the thin / full boundary), the tile edges 31 / 32 / 33 and 63 / 65, one
# LDS stage + 1, four stages with a tail, then no match at all and too few
MS = (8, 35, 36, 31, 32, 33, 63, 65, 257, 1000, 0, 3)
ITERS = (1, 31, 32, 33, 64, 65, 80, 200)
THR = 0.01
SUP = ("support", "support_counts")


@functools.lru_cache(maxsize=None)
def _scene(k, seed0=7300, outliers=0.3):
    m = MS[k]
    c = synth.make_correspondences(seed0 + k, max(m, 8), outliers, integer=False)
    return {**c, "kp_l": c["kp_l"][:m], "kp_r": c["kp_r"][:m]}


@functools.lru_cache(maxsize=None)
def _pair(k):
    c = _scene(k)
    return ED.pair_from_keys(8800 + k, c["kp_l"], c["kp_r"], c["W"], c["H"])


def _tensors(pairs):
    import torch
    cat = lambda k: np.concatenate([p[k] for p in pairs])  # noqa: E731
    off = lambda k: np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]).astype(np.int64)  # noqa: E731
    ol, orr = off("desc_l"), off("desc_r")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    return (t(cat("desc_l")), t(cat("desc_r")), t(cat("kp_l")), t(cat("kp_r")), t(ol), t(orr),
            t(np.array([p["W"] for p in pairs], np.int32)),
            t(np.array([p["H"] for p in pairs], np.int32)), int(np.diff(ol).max()),
            int(np.diff(orr).max()))


def _host(o):
    from erp_match_eightpoint_test_amd import (hyps_to_numpy, results_to_numpy, support_to_numpy,
                                               winners_to_numpy)
    h = {"results": results_to_numpy(o["results"]).copy()}
    if "support" in o:
        h["support"] = support_to_numpy(o["support"]).copy()
        h["support_winners"] = winners_to_numpy(o["support_winners"]).copy()
        h["support_results"] = results_to_numpy(o["support_results"]).copy()
    if "support_counts" in o:
        h["support_counts"] = o["support_counts"].cpu().numpy().copy()
    if "hyps" in o:
        h["hyps"] = hyps_to_numpy(o["hyps"]).copy()
    for k in ("key_left", "key_right"):
        if k in o:
            h[k] = o[k].cpu().numpy().copy()
    return h


def _run(tensors, want=(), iters=80, opts=None, stream=None, runner=None, thr=THR, support=True,
         **cfg):
    """one PairBatchRunner.run -> (runner, device outputs, host copies)"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner
    if runner is None:
        c = Context(0)
        for k, v in (opts or {}).items():
            c.set_option(k, v)
        runner = PairBatchRunner(ctx=c, iters=iters, stream=stream, **cfg)
    want = tuple(want) + (SUP if support else ())
    o = runner.run(*tensors, want=want, support_thr=thr if support else None)
    torch.cuda.synchronize()
    return runner, o, _host(o)


def _support_bytes(h):
    return b"".join(h[k].tobytes() for k in ("support", "support_winners", "support_results",
                                             "support_counts"))


def _core(res):
    """a result record without its diagnostics (near_ties, survivors, binned_rows depend on the
    consensus route a launch takes, include/erp_match.h)"""
    return b"".join(np.ascontiguousarray(res[f]).tobytes()
                    for f in ("R", "T", "status", "M", "K", "min_idx", "sample_n", "min_dist"))


def _zero_but_status(rec):
    r = rec.copy()
    r["status"] = 0
    return not r.tobytes().strip(b"\0")


@pytest.fixture(scope="module")
def batch(gpu_lib):
    """the ragged batch at every iteration count: with records and lite, and the records of the
    cfg.inlier_thr route; computed once and never modified"""
    tensors = _tensors([_pair(k) for k in range(len(MS))])
    out = {"tensors": tensors}
    for it in ITERS:
        out[it] = {"rec": _run(tensors, ("hyps", "key_left", "key_right"), iters=it),
                   "lite": _run(tensors, ("key_left", "key_right"), iters=it),
                   "thr": _run(tensors, ("hyps",), iters=it, support=False,
                               inlier_thr=SR.thr64(THR))}
    return out


@functools.lru_cache(maxsize=None)
def _bearings(k):
    import oracle
    c = _scene(k)
    return (oracle.pixel_to_bearing(c["W"], c["H"], c["kp_l"]),
            oracle.pixel_to_bearing(c["W"], c["H"], c["kp_r"]))


def _check_pair(oracle, tag, bl, br, res, hyps, sup, win, sres, counts, thr):
    """one OK pair's outputs against support_ref on its own records -> cells that needed the
    1e-12 allowance"""
    ref_n, near = SR.counts_of(oracle, bl, br, hyps, thr)
    diff = np.abs(counts.astype(np.int64) - ref_n)
    assert (diff <= near).all(), (tag, np.nonzero(diff > near)[0][:8], counts[:8], ref_n[:8])
    sel = SR.select(hyps, counts, res["R"], int(res["min_idx"]))
    assert sel is not None and sup["status"] == 0, (tag, sup)
    for f, v in sel.items():
        assert sup[f] == v, (tag, f, sup, sel)
    it, which = sel["iter"], sel["which"]
    assert (win["status"], win["iter"], win["which"], win["sample_n"]) == \
        (0, it, which, res["sample_n"]), (tag, win)
    assert win["E"].tobytes() == hyps[it]["E"].tobytes(), tag
    want = res.copy()
    want["R"], want["T"], want["min_idx"] = hyps[it]["R2" if which else "R1"], hyps[it]["T"], sel["row"]
    assert sres.tobytes() == want.tobytes(), (tag, sres, want)
    return int((near > 0).sum())


# ----------------------------------------------------------------- the ragged batch
@pytest.mark.parametrize("iters", ITERS)
def test_counts_and_selection_against_the_reference(batch, oracle, iters):
    _, _, h = batch[iters]["rec"]
    allowed = cells = 0
    for k, m in enumerate(MS):
        res = h["results"][k]
        assert res["M"] == m, (k, res)
        if res["status"] != 0:
            assert h["support"][k]["status"] == res["status"], (k, h["support"][k])
            continue
        assert np.array_equal(h["key_left"][k, :m], _scene(k)["kp_l"])
        bl, br = _bearings(k)
        allowed += _check_pair(oracle, (iters, k), bl, br, res, h["hyps"][k], h["support"][k],
                               h["support_winners"][k], h["support_results"][k],
                               h["support_counts"][k], THR)
        cells += iters
    # (a single iteration may leave most pairs without a valid rotation)
    assert (iters < 31 or cells >= 8 * iters) and allowed <= 0.01 * cells, (allowed, cells)


@pytest.mark.parametrize("iters", ITERS)
def test_counts_equal_the_inlier_thr_route(batch, iters):
    """support_counts == hyps[].inliers of a run with cfg.inlier_thr = thr, for every iteration
    (the invalid ones too) of every ERP_OK pair; the pairs that do not run have rows of zeros"""
    _, _, h = batch[iters]["rec"]
    _, _, t = batch[iters]["thr"]
    assert t["results"].tobytes() == h["results"].tobytes()
    assert h["support_counts"].dtype == np.int32 and h["support_counts"].shape == (len(MS), iters)
    ok = h["results"]["status"] == 0
    inl = np.ascontiguousarray(t["hyps"]["inliers"])
    assert h["support_counts"][ok].tobytes() == inl[ok].tobytes()
    assert not h["support_counts"][~ok].any()   # (a pair that is not ERP_OK: a row of zeros)
    invalid = (t["hyps"]["R1_valid"] == 0) & (t["hyps"]["R2_valid"] == 0)
    print("iterations without a valid rotation:", int(invalid[ok].sum()), "of them counted > 0:",
          int((invalid[ok] & (h["support_counts"][ok] > 0)).sum()))


@pytest.mark.parametrize("iters", ITERS)
def test_lite_equals_records(batch, iters):
    _, o, lite = batch[iters]["lite"]
    _, _, rec = batch[iters]["rec"]
    assert "hyps" not in o
    assert lite["results"].tobytes() == rec["results"].tobytes()
    for f in ("support", "support_winners", "support_results", "support_counts"):
        assert lite[f].tobytes() == rec[f].tobytes(), f
    for k in np.nonzero(rec["results"]["status"] == 0)[0]:
        w = lite["support_winners"][k]
        assert w["E"].tobytes() == rec["hyps"][k][w["iter"]]["E"].tobytes(), k


def test_shapes_of_the_batch(batch):
    """what the batch is meant to hit, on the GPU's own records"""
    _, _, h = batch[200]["rec"]
    res, sup = h["results"], h["support"]
    assert [int(res[k]["sample_n"]) for k in (0, 1, 2)] == [2, 8, 9]
    for k, m in enumerate(MS):
        if m < 4:
            assert res[k]["status"] == 2 and sup[k]["status"] == 2, (k, res[k], sup[k])
            assert _zero_but_status(sup[k]) and _zero_but_status(h["support_winners"][k])
            assert h["support_results"][k].tobytes() == res[k].tobytes()
            assert not h["support_counts"][k].any()
    ok = res["status"] == 0
    assert ok.sum() >= 8
    print("iter:", sup["iter"][ok].tolist(), "which:", sup["which"][ok].tolist(),
          "inliers:", sup["inliers"][ok].tolist(), "consensus:", sup["consensus_iter"][ok].tolist(),
          sup["consensus_inliers"][ok].tolist())
    assert (sup["inliers"][ok] >= sup["consensus_inliers"][ok]).all()
    assert (sup["scored"][ok] <= 200).all() and (sup["row"][ok] < res["K"][ok]).all()


@pytest.mark.parametrize("arm", [0, 1], ids=["valu", "mfma"])
@pytest.mark.parametrize("iters", [33, 200])
def test_both_count_kernels_give_the_same_bytes(batch, arm, iters):
    """ERP_OPT_SUPPORT_COUNT 0 / 1 against the default (automatic) run, on both routes"""
    t = batch["tensors"]
    for route, want in (("lite", ()), ("rec", ("hyps",))):
        _, _, h = _run(t, want, iters=iters, opts={"support_count": arm})
        assert _support_bytes(h) == _support_bytes(batch[iters][route][2]), (arm, route)


def test_sampler_share_off_and_on(batch):
    t = batch["tensors"]
    for share in (0, 1):
        _, _, h = _run(t, (), opts={"sampler_share": share})
        assert _support_bytes(h) == _support_bytes(batch[80]["lite"][2]), share


def test_philox(batch, oracle):
    t = batch["tensors"]
    _, _, rec = _run(t, ("hyps",), sampler=1)
    _, _, lite = _run(t, (), sampler=1)
    assert _support_bytes(lite) == _support_bytes(rec)
    assert _support_bytes(lite) != _support_bytes(batch[80]["lite"][2])
    for k in (2, 8):
        assert rec["results"][k]["status"] == 0
        _check_pair(oracle, ("philox", k), *_bearings(k), rec["results"][k], rec["hyps"][k],
                    rec["support"][k], rec["support_winners"][k], rec["support_results"][k],
                    rec["support_counts"][k], THR)


def test_rand_stream_two_successive_calls(batch, oracle):
    """on a rand stream the stage consumes nothing of its own: the second call's result records are
    the oracle's on the continued stream, lite on one stream equals records on another at the same
    position, and the support records follow the rules on the call's own records"""
    from erp_match_eightpoint_test_amd import RandStream
    t = batch["tensors"]
    a, b = RandStream(1, 0), RandStream(1, 0)
    ra, _, la1 = _run(t, (), stream=a)
    rb, _, rb1 = _run(t, ("hyps",), stream=b)
    _, _, la2 = _run(t, (), runner=ra)
    _, _, rb2 = _run(t, ("hyps",), runner=rb)
    per_call = 80 * sum(m - 1 for m in MS if m >= 4)
    assert a.draws == b.draws == 2 * per_call
    for lite, rec in ((la1, rb1), (la2, rb2)):
        assert lite["results"].tobytes() == rec["results"].tobytes()
        assert _support_bytes(lite) == _support_bytes(rec)
    assert _support_bytes(la1) != _support_bytes(la2)
    offset = per_call
    for k, m in enumerate(MS):
        if m < 4:
            continue
        if k in (2, 7):
            c = _scene(k)
            o = oracle.find(c["W"], c["H"], c["kp_l"], c["kp_r"],
                            oracle.make_cfg(iters=80, offset=offset), detail=True)
            res = rb2["results"][k]
            assert (res["status"], res["K"], res["min_idx"]) == (o["status"], o["K"], o["min_idx"])
            assert np.abs(res["R"] - o["R"]).max() <= 1e-5  # (DESIGN.md section 4's bar)
            _check_pair(oracle, ("stream", k), *_bearings(k), res, rb2["hyps"][k],
                        rb2["support"][k], rb2["support_winners"][k], rb2["support_results"][k],
                        rb2["support_counts"][k], THR)
        offset += 80 * (m - 1)


# ----------------------------------------------------------------- single pairs
def _find_support_dev(kl, kr, W, H, cfg, with_hyps, thr=THR, ctx=None, counts=True):
    """erp_eight_point_find_support_dev on host keypoint arrays -> host copies"""
    import torch
    from erp_match_eightpoint_test_amd import Context, capi
    ctx = ctx or Context(0)
    m = len(kl)
    u8 = lambda n: torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda")  # noqa: E731
    dkl = torch.from_numpy(np.ascontiguousarray(kl, np.float32)).cuda()
    dkr = torch.from_numpy(np.ascontiguousarray(kr, np.float32)).cuda()
    res, sup, win, sres = u8(64), u8(32), u8(88), u8(64)
    cnt = torch.full((cfg.iters,), -1, dtype=torch.int32, device="cuda")
    hyps = torch.zeros((cfg.iters, capi.HYP_DTYPE.itemsize), dtype=torch.uint8, device="cuda") \
        if with_hyps else None
    so = capi.SupportOutputs(sup.data_ptr(), win.data_ptr(), sres.data_ptr(),
                             cnt.data_ptr() if counts else None)
    st = ctx.L.erp_eight_point_find_support_dev(
        ctx.h, W, H, dkl.data_ptr(), dkr.data_ptr(), m, C.byref(cfg), res.data_ptr(),
        hyps.data_ptr() if with_hyps else None, thr, C.byref(so),
        torch.cuda.current_stream().cuda_stream)
    assert st == 0, st
    torch.cuda.synchronize()
    return {"results": res.cpu().numpy().view(capi.RESULT_DTYPE)[0],
            "support": sup.cpu().numpy().view(capi.SUPPORT_DTYPE)[0],
            "support_winners": win.cpu().numpy().view(capi.WINNER_DTYPE)[0],
            "support_results": sres.cpu().numpy().view(capi.RESULT_DTYPE)[0],
            "support_counts": cnt.cpu().numpy(),
            "hyps": hyps.cpu().numpy().view(capi.HYP_DTYPE).reshape(-1) if with_hyps else None}


@pytest.mark.parametrize("k", [0, 1, 2, 8])
@pytest.mark.parametrize("with_hyps", [False, True], ids=["lite", "records"])
def test_single_pairs_through_find_support_dev(batch, k, with_hyps):
    """one pair alone (on the lite route the estimate's REST instantiation): the batch's records"""
    from erp_match_eightpoint_test_amd import default_cfg
    c = _scene(k)
    got = _find_support_dev(c["kp_l"], c["kp_r"], c["W"], c["H"], default_cfg(), with_hyps)
    want = batch[80]["rec"][2]
    for f in ("support", "support_winners", "support_counts"):
        assert got[f].tobytes() == want[f][k].tobytes(), (k, f, got[f], want[f][k])
    assert _core(got["support_results"]) == _core(want["support_results"][k])


def test_degenerate_pair(gpu_lib):
    """40 matches that repeat 4 distinct correspondences, aimed at the Jacobi fallback as
    test_gpu_winners.py builds it: records route and lite route agree byte for byte"""
    from erp_match_eightpoint_test_amd import default_cfg
    p = synth.make_pair(9500, n_kpts=4, inlier_frac=1.0, sigma=0.005)
    kl = np.tile(p["kp_l"][:4], (10, 1))
    kr = np.tile(p["kp_r"][p["gt_partner"][:4]], (10, 1))
    cfg = default_cfg()
    r = _find_support_dev(kl, kr, p["W"], p["H"], cfg, True)
    l = _find_support_dev(kl, kr, p["W"], p["H"], cfg, False)
    print("degenerate pair: status", r["results"]["status"], "support", r["support"])
    assert r["results"]["sample_n"] == 10
    assert l["results"].tobytes() == r["results"].tobytes()
    assert _support_bytes(l) == _support_bytes(r)
    assert r["support"]["status"] == r["results"]["status"]
    if r["support"]["status"] == 0:
        it = r["support"]["iter"]
        assert r["support_winners"]["E"].tobytes() == r["hyps"][it]["E"].tobytes()
        assert r["support"]["inliers"] == r["support_counts"][it] == 40  # (every match repeats)
    else:
        assert _zero_but_status(r["support"])


@functools.lru_cache(maxsize=None)
def _big_pair(k):
    m = (33, 40, 47, 52, 57, 60, 62, 63, 64)[k]
    c = synth.make_correspondences(7500 + k, m, 0.3, integer=False)
    return c, ED.pair_from_keys(8900 + k, c["kp_l"], c["kp_r"], c["W"], c["H"])


def test_a_batch_above_1024_waves(gpu_lib, oracle):
    """9 pairs x 10 000 iterations (1413 waves): estimate_lite_kernel<false> and eigen_rest_kernel
    run, so evec holds every e"""
    t = _tensors([_big_pair(k)[1] for k in range(9)])
    _, _, rec = _run(t, ("hyps",), iters=10000)
    _, _, lite = _run(t, (), iters=10000)
    _, _, thr = _run(t, ("hyps",), iters=10000, support=False, inlier_thr=SR.thr64(THR))
    assert (rec["results"]["status"] == 0).all()
    assert lite["results"].tobytes() == rec["results"].tobytes()
    assert _support_bytes(lite) == _support_bytes(rec)
    assert rec["support_counts"].tobytes() == np.ascontiguousarray(thr["hyps"]["inliers"]).tobytes()
    for k in range(9):
        hy, sup = rec["hyps"][k], rec["support"][k]
        sel = SR.select(hy, rec["support_counts"][k], rec["results"][k]["R"],
                        int(rec["results"][k]["min_idx"]))
        assert all(sup[f] == v for f, v in sel.items()), (k, sup, sel)
    c = _big_pair(4)[0]
    bl = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_l"])
    br = oracle.pixel_to_bearing(c["W"], c["H"], c["kp_r"])
    near = _check_pair(oracle, "big 4", bl, br, rec["results"][4], rec["hyps"][4], rec["support"][4],
                       rec["support_winners"][4], rec["support_results"][4],
                       rec["support_counts"][4], THR)
    assert near <= 100


# ----------------------------------------------------------------- the band
def test_threshold_next_to_a_residual(batch, oracle):
    """thr = the floats just above and just below an actual residual: the fast evaluation cannot
    decide that match, the fp64 recheck must, and the counts stay exact"""
    k = 8
    _, _, h = batch[80]["rec"]
    hyps = h["hyps"][k]
    bl, br = _bearings(k)
    it = int(h["support"][k]["iter"])
    Ec = oracle.rank2(hyps[it]["E"])
    r = np.abs([np.dot(Ec, np.outer(bl[i], br[i]).reshape(9)) for i in range(len(bl))])
    r0 = np.float32(np.sort(r)[len(r) // 3])  # (some match's residual, as a float)
    c = _scene(k)
    from erp_match_eightpoint_test_amd import default_cfg
    for thr in (np.nextafter(r0, np.float32(1)), np.nextafter(r0, np.float32(0)), r0):
        for arm in (0, 1):
            from erp_match_eightpoint_test_amd import Context
            ctx = Context(0)
            ctx.set_option("support_count", arm)
            g = _find_support_dev(c["kp_l"], c["kp_r"], c["W"], c["H"], default_cfg(), True,
                                  thr=float(thr), ctx=ctx)
            assert g["hyps"]["E"].tobytes() == hyps["E"].tobytes()
            near = _check_pair(oracle, ("band", float(thr), arm), bl, br, g["results"], g["hyps"],
                               g["support"], g["support_winners"], g["support_results"],
                               g["support_counts"], float(thr))
            assert near <= 1


@pytest.mark.parametrize("arm", [0, 1], ids=["valu", "mfma"])
def test_thr_1_counts_every_match_and_a_tiny_thr_none(batch, arm):
    from erp_match_eightpoint_test_amd import Context, default_cfg
    _, _, h = batch[80]["rec"]
    for k in (3, 8):
        c = _scene(k)
        hyps = h["hyps"][k]
        first = int(np.nonzero((hyps["R1_valid"] != 0) | (hyps["R2_valid"] != 0))[0][0])
        for thr, count in ((1.0, MS[k]), (1e-12, 0)):
            ctx = Context(0)
            ctx.set_option("support_count", arm)
            g = _find_support_dev(c["kp_l"], c["kp_r"], c["W"], c["H"], default_cfg(), False,
                                  thr=thr, ctx=ctx)
            assert (g["support_counts"] == count).all(), (k, thr, g["support_counts"])
            assert (g["support"]["status"], g["support"]["iter"], g["support"]["inliers"]) == \
                (0, first, count), (k, thr, g["support"])


# ----------------------------------------------------------------- statuses
def test_no_valid_hypothesis(batch):
    """valid_abs = 0: K = 0, the result status is ERP_NO_VALID_HYPOTHESIS and so is the stage's"""
    for want in ((), ("hyps",)):
        _, _, h = _run(batch["tensors"], want, valid_abs=0.0)
        assert (h["results"]["K"] == 0).all()
        for k, m in enumerate(MS):
            st = 3 if m >= 4 else 2
            assert h["results"][k]["status"] == st == h["support"][k]["status"], (k, h["results"][k])
            assert _zero_but_status(h["support"][k]) and _zero_but_status(h["support_winners"][k])
            assert h["support_winners"][k]["status"] == st
            assert h["support_results"][k].tobytes() == h["results"][k].tobytes()
        assert not h["support_counts"].any()


def test_a_nan_keypoint_pair_beside_good_pairs(batch):
    """the pair gets its status and zeros; its neighbours' records are those of the batch"""
    ks = (2, 5, 8)
    bad = dict(_pair(5))
    bad["kp_l"] = bad["kp_l"].copy()
    bad["kp_l"][7, 0] = np.nan
    _, _, h = _run(_tensors([_pair(2), bad, _pair(8)]), ())
    want = batch[80]["lite"][2]
    assert h["results"][1]["status"] not in (0,) and h["support"][1]["status"] == h["results"][1]["status"]
    assert _zero_but_status(h["support"][1]) and _zero_but_status(h["support_winners"][1])
    assert h["support_results"][1].tobytes() == h["results"][1].tobytes()
    assert not h["support_counts"][1].any()
    for i in (0, 2):
        for f in ("support", "support_winners", "support_counts"):
            assert h[f][i].tobytes() == want[f][ks[i]].tobytes(), (i, f)
        assert _core(h["support_results"][i]) == _core(want["support_results"][ks[i]]), i


def test_argument_rules_on_the_device(batch):
    """a partial ERP_OPT_DEBUG_STAGES mask and thr <= 0 are ERP_INVALID_ARG"""
    import torch
    from erp_match_eightpoint_test_amd import Context, ErpError, capi, default_cfg
    with pytest.raises(ErpError) as e:
        _run(batch["tensors"], (), opts={"debug_stages": 63})
    assert e.value.status == 1
    ctx = Context(0)
    c = _scene(2)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    kl, kr = d(c["kp_l"]), d(c["kp_r"])
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    so = capi.SupportOutputs(buf.data_ptr(), None, None, None)
    cfg = default_cfg()
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert ctx.L.erp_eight_point_find_support_dev(
            ctx.h, c["W"], c["H"], kl.data_ptr(), kr.data_ptr(), MS[2], C.byref(cfg),
            buf[64:].data_ptr(), None, thr, C.byref(so), None) == 1, thr
    ctx.set_option("debug_stages", 31)
    assert ctx.L.erp_eight_point_find_support_dev(
        ctx.h, c["W"], c["H"], kl.data_ptr(), kr.data_ptr(), MS[2], C.byref(cfg),
        buf[64:].data_ptr(), None, 0.01, C.byref(so), None) == 1


def test_only_the_required_output(batch):
    """winners, results and counts are optional: the support records alone are the batch's"""
    c = _scene(8)
    from erp_match_eightpoint_test_amd import default_cfg
    import torch
    from erp_match_eightpoint_test_amd import Context, capi
    ctx = Context(0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    kl, kr = d(c["kp_l"]), d(c["kp_r"])
    res = torch.zeros(64, dtype=torch.uint8, device="cuda")
    sup = torch.zeros(32, dtype=torch.uint8, device="cuda")
    so = capi.SupportOutputs(sup.data_ptr(), None, None, None)
    cfg = default_cfg()
    assert ctx.L.erp_eight_point_find_support_dev(
        ctx.h, c["W"], c["H"], kl.data_ptr(), kr.data_ptr(), MS[8], C.byref(cfg), res.data_ptr(),
        None, THR, C.byref(so), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert sup.cpu().numpy().tobytes() == batch[80]["rec"][2]["support"][8].tobytes()


# ----------------------------------------------------------------- the chain behind it
def test_plain_results_are_unchanged(batch):
    t = batch["tensors"]
    _, o, h = _run(t, ("hyps",), support=False)
    assert "support" not in o
    want = batch[80]["rec"][2]
    assert h["results"].tobytes() == want["results"].tobytes()
    assert h["hyps"].tobytes() == want["hyps"].tobytes()


def test_polish_and_pose_on_the_support_view(batch, oracle):
    """polish() and select_pose() take support_view(out) as they take run()'s dict: the polish
    against polish_ref's chain started from the support winner's state (its bar: 1e-6), the pose
    selection against pose_ref through test_gpu_pose's comparison"""
    import torch
    from test_gpu_pose import _against_chain
    from erp_match_eightpoint_test_amd import PairBatchRunner, polish_to_numpy, pose_to_numpy
    t = batch["tensors"]
    run, o, h = batch[80]["lite"]
    view = PairBatchRunner.support_view(o)
    assert view["results"] is o["support_results"] and view["winners"] is o["support_winners"]
    pol = run.polish(view, t[6], t[7], THR, rounds=PR.ROUNDS)
    pose = run.select_pose(view, t[6], t[7], source="winners", thr=THR)
    torch.cuda.synchronize()
    pr, mask = polish_to_numpy(pol["polish"]), pol["mask"].cpu().numpy()
    po = pose_to_numpy(pose["pose"])
    depth, front = pose["depth"].cpu().numpy(), pose["front"].cpu().numpy()
    for k in (2, 7, 8, 9):
        m = MS[k]
        sup, win, sres = h["support"][k], h["support_winners"][k], h["support_results"][k]
        assert sup["status"] == 0
        bl, br = _bearings(k)
        ref = PR.chain(oracle, bl, br, win["E"], sres["R"], sres["T"], THR)
        assert ref["near"] == 0, k
        p = pr[k]
        assert (p["status"], p["winner_iter"], p["winner_which"]) == (0, sup["iter"], sup["which"])
        assert p["n_inliers_winner"] == int(ref["sets"][0].sum()) == sup["inliers"], (k, p, sup)
        assert p["rounds_done"] == len(ref["rounds"]) and p["n_inliers"] == int(ref["sets"][-1].sum())
        sign = 1.0 if float(np.dot(p["E"], ref["e"])) >= 0 else -1.0
        assert np.abs(sign * p["E"] - ref["e"]).max() <= 1e-6
        assert np.abs(p["R"] - ref["R"]).max() <= 1e-6 and np.abs(p["T"] - ref["T"]).max() <= 1e-6
        assert np.array_equal(mask[k, :m], ref["sets"][-1].astype(np.uint8)) and not mask[k, m:].any()
        _against_chain(oracle, ("support view", k), po[k], depth[k], front[k], bl, br, win["E"],
                       sres, thr=THR)


# ----------------------------------------------------------------- bindings
@pytest.mark.parametrize("k", [1, 8])
def test_host_and_python_find_support(batch, k):
    from erp_match_eightpoint_test_amd import eight_point
    c = _scene(k)
    ep = eight_point()
    R, T, E = ep.find_support(c["W"], c["H"], c["kp_l"], c["kp_r"], THR, want_counts=True)
    want = batch[80]["rec"][2]
    assert ep.last_support.tobytes() == want["support"][k].tobytes()
    assert ep.last_winner.tobytes() == want["support_winners"][k].tobytes()
    assert _core(ep.last_support_result) == _core(want["support_results"][k])
    assert _core(ep.last_result) == _core(want["results"][k])
    assert ep.last_counts.tobytes() == want["support_counts"][k].tobytes()
    assert E.tobytes() == want["support_winners"][k]["E"].tobytes()
    assert R.tobytes() == want["support_results"][k]["R"].tobytes()
    assert T.tobytes() == want["support_results"][k]["T"].tobytes()


def test_find_support_raises_on_too_few_points(batch):
    from erp_match_eightpoint_test_amd import ErpError, eight_point
    c = _scene(11)
    ep = eight_point()
    with pytest.raises(ErpError) as e:
        ep.find_support(c["W"], c["H"], c["kp_l"], c["kp_r"], THR)
    assert e.value.status == 2 and ep.last_support["status"] == 2
    assert _zero_but_status(ep.last_support)


def test_cpp_find_support_driver(batch, tmp_path):
    """erp::eight_point::find_support as a reference maintainer links it (g++ against the library,
    no Python in the process) against the batch's records"""
    from erp_match_eightpoint_test_amd import _build, capi
    driver = _build.build_support_driver()
    k = 8
    c = _scene(k)
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    outd.mkdir()
    np.array([c["W"], c["H"], 80, MS[k]], np.int32).tofile(ind / "meta.i32")
    np.array([0.25, THR], np.float64).tofile(ind / "cfg.f64")
    c["kp_l"].tofile(ind / "kl.f32")
    c["kp_r"].tofile(ind / "kr.f32")
    r = subprocess.run([driver, str(ind), str(outd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(outd / "support.bin", np.uint8)
    want = batch[80]["rec"][2]
    res = raw[24:88].view(capi.RESULT_DTYPE)[0]
    sup = raw[88:120].view(capi.SUPPORT_DTYPE)[0]
    win = raw[120:208].view(capi.WINNER_DTYPE)[0]
    counts = raw[208:].view(np.int32)
    assert _core(res) == _core(want["results"][k])
    assert sup.tobytes() == want["support"][k].tobytes()
    assert win.tobytes() == want["support_winners"][k].tobytes()
    assert counts.tobytes() == want["support_counts"][k].tobytes()
    assert raw[:12].tobytes() == want["support_results"][k]["R"].tobytes()
    assert raw[12:24].tobytes() == want["support_results"][k]["T"].tobytes()


def test_graphs_on_enqueues_plainly(batch):
    """with erp_ctx_set_graphs on the support call still runs (kernel by kernel), twice"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner
    c = Context(0)
    c.set_graphs(True)
    run = PairBatchRunner(ctx=c, iters=80, reuse_outputs=True)
    want = batch[80]["lite"][2]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(2):
            _, _, h = _run(batch["tensors"], (), runner=run)
            assert h["results"].tobytes() == want["results"].tobytes()
            assert _support_bytes(h) == _support_bytes(want)


# ----------------------------------------------------------------- what it is worth
def test_support_winner_recovers_the_pose_with_minimal_samples(gpu_lib, oracle):
    """the host test's value check on the GPU: 400 matches, 40 % outliers, 500 iterations of
    s = 10, thr 0.005, seeds 0..11 as one batch"""
    scenes = [synth.make_correspondences(s, 400, 0.4, integer=False) for s in range(12)]
    t = _tensors([ED.pair_from_keys(9900 + s, c["kp_l"], c["kp_r"], c["W"], c["H"])
                  for s, c in enumerate(scenes)])
    _, _, h = _run(t, (), iters=500, thr=0.005, sample_frac=0.025)
    assert (h["results"]["status"] == 0).all() and (h["support"]["status"] == 0).all()
    assert (h["results"]["sample_n"] == 10).all()
    cons = [SR.rotation_error_deg(oracle, h["results"][s]["R"], c["euler_gt"])
            for s, c in enumerate(scenes)]
    sup = [SR.rotation_error_deg(oracle, h["support_results"][s]["R"], c["euler_gt"])
           for s, c in enumerate(scenes)]
    print("consensus error (deg):", np.round(cons, 3).tolist())
    print("support error (deg):", sup)
    assert max(sup) < 0.01, sup
    assert np.median(cons) > 1.0, cons
