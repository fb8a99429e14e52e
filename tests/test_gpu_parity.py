"""GPU parity: the HIP path (through the C ABI) against the CPU oracle and the golden fixtures.

Bars (DESIGN.md "Parity"):
* matches: (queryIdx, trainIdx, distance bits) bit-exact;
* sampler: every iteration's sampled index set identical (glibc replay is integer work);
* per-iteration E within 1e-6 (after sign alignment; north_star allows 1e-4; typical 1e-12,
  thin-SVD samples with a small s-th singular value reach ~2e-8), {R1,R2} equal as a set within
  TOL_RT rad, T within TOL_RT;
* final R, T: equal to the oracle's within TOL_RT (same consensus winner up to identical values).
The largest deviation each fixture shows is recorded (tests/parity_log.py, ERP_PARITY_OUT).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from erp_match_eightpoint_test_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, os.path.dirname(__file__))
from parity_log import record  # noqa: E402  (the measured deviations, ERP_PARITY_OUT)


@pytest.fixture(scope="module")
def ctx(gpu_lib):
    from erp_match_eightpoint_test_amd import Context
    return Context(0)


def _npz(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


# ------------------------------------------------------------------------------ matcher
# every matcher test runs on both exact-k=2 methods: the bf16-MFMA filter + exact rescoring
# (default) and the LDS-tiled packed-FP32 sweep (configs[3]'s scalar path)
@pytest.fixture(scope="module", params=["mfma_filter", "valu_exact"])
def mctx(gpu_lib, request):
    from erp_match_eightpoint_test_amd import Context, capi
    c = Context(0)
    c.set_matcher(capi.MATCHER_MFMA_FILTER if request.param == "mfma_filter"
                  else capi.MATCHER_VALU_EXACT)
    return c

def test_match_golden_fixture(mctx):
    from erp_match_eightpoint_test_amd import feature_matcher
    g = _npz("match_384.npz")
    fm = feature_matcher(ctx=mctx)
    mt = fm.match_two_image(g["desc_l"], g["desc_r"])
    assert np.array_equal(mt["queryIdx"], g["query"])
    assert np.array_equal(mt["trainIdx"], g["train"])
    assert np.array_equal(mt["distance"].view(np.uint32), g["dist_bits"])
    assert np.all(mt["imgIdx"] == 0)


@pytest.mark.parametrize("nq,nt", [(1, 2), (2, 2), (63, 65), (300, 4097), (2048, 2048),
                                   (4096, 4096), (5000, 1000)])
def test_match_vs_oracle_sizes(mctx, oracle, nq, nt):
    from erp_match_eightpoint_test_amd import feature_matcher
    p = synth.make_pair(nq * 7 + nt, n_kpts=nq, n_train=nt)
    ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
    mt = feature_matcher(ctx=mctx).match_two_image(p["desc_l"], p["desc_r"])
    assert len(mt) == len(ref)
    assert np.array_equal(mt.view(np.uint32), ref.view(np.uint32))


def test_match_ties_and_ratio_boundary(mctx, oracle):
    from erp_match_eightpoint_test_amd import feature_matcher
    rng = np.random.default_rng(5)
    t = synth.random_descriptors(rng, 700)
    t[500:520] = t[10:30]                        # duplicates across chunks
    q = np.concatenate([t[5:40], synth.random_descriptors(rng, 60)])
    q[40] = q[41]
    ref, _, _, _ = oracle.match_two_image(q, t)
    mt = feature_matcher(ctx=mctx).match_two_image(q, t)
    assert np.array_equal(mt.view(np.uint32), ref.view(np.uint32))


def _all_queries_vs_oracle(mctx, oracle, q, t):
    """every query's exact k=2 through the matcher: ratio 1e30 keeps every query (checks
    trainIdx = j0 and distance = sqrtf(d0) bit-exactly), ratio 1.0 drops exactly the queries
    whose two nearest distances tie (checks d1 == d0 detection), ratio 0.3 = the reference."""
    from erp_match_eightpoint_test_amd import feature_matcher
    fm = feature_matcher(ctx=mctx)
    for ratio in (1e30, 1.0, 0.3):
        ref, _, _, _ = oracle.match_two_image(q, t, ratio=ratio)
        mt = fm.match_two_image(q, t, ratio=ratio)
        assert len(mt) == len(ref), ratio
        assert np.array_equal(mt.view(np.uint32), ref.view(np.uint32)), ratio


def test_match_filter_candidate_overflow(mctx, oracle):
    """>32 train rows inside the filter's error window of one query (near-duplicates differing
    in the last bits): the candidate list overflows and the exact sweep path must decide."""
    rng = np.random.default_rng(11)
    t = synth.random_descriptors(rng, 1200)
    base = t[7].copy()
    for k in range(300):
        v = base.copy()
        v[k % 64] = np.nextafter(v[k % 64], np.float32(2.0) if k % 2 else np.float32(-2.0))
        t[100 + k] = v
    q = np.concatenate([base[None, :], t[50:90], synth.random_descriptors(rng, 100)])
    _all_queries_vs_oracle(mctx, oracle, q, t)


def test_match_filter_near_ties_unnormalised(mctx, oracle):
    """distances equal up to rounding, unnormalised magnitudes (1e-3 .. 1e2) and zero rows: the
    filter's error bound scales with |q|^2 + |t|^2 and must never drop a true neighbour."""
    rng = np.random.default_rng(12)
    t = synth.random_descriptors(rng, 900).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), size=(900, 1))).astype(np.float32)
    t = (t * scale).astype(np.float32)
    t[3] = 0.0
    t[4] = 0.0
    q = t[rng.integers(0, 900, 200)] + rng.normal(0, 1e-6, (200, 64)).astype(np.float32)
    q[0] = 0.0
    # two train rows at the same distance from a query but on different sides
    q[1] = t[10]
    d = rng.normal(0, 1e-3, 64).astype(np.float32)
    t[11] = t[10] + d
    t[12] = t[10] - d
    _all_queries_vs_oracle(mctx, oracle, q.astype(np.float32), t)


@pytest.mark.parametrize("nq,nt", [(300, 4097), (4096, 4096)])
def test_match_all_queries_vs_oracle(mctx, oracle, nq, nt):
    p = synth.make_pair(nq * 3 + nt, n_kpts=nq, n_train=nt)
    _all_queries_vs_oracle(mctx, oracle, p["desc_l"], p["desc_r"])


def test_match_edge_counts(mctx):
    from erp_match_eightpoint_test_amd import ErpError, feature_matcher
    fm = feature_matcher(ctx=mctx)
    assert len(fm.match_two_image(np.zeros((0, 64), np.float32), np.zeros((5, 64), np.float32))) == 0
    with pytest.raises(ErpError):
        fm.match_two_image(np.ones((3, 64), np.float32), np.ones((1, 64), np.float32))


def test_match_device_path(mctx, oracle):
    import torch
    from erp_match_eightpoint_test_amd import feature_matcher
    p = synth.make_pair(99, n_kpts=1500)
    ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
    q = torch.from_numpy(p["desc_l"]).cuda()
    t = torch.from_numpy(p["desc_r"]).cuda()
    out = feature_matcher(ctx=mctx).match_two_image(q, t).cpu().numpy()
    assert np.array_equal(out.view(np.uint32).reshape(-1), ref.view(np.uint32).reshape(-1))


# --------------------------------------------------------------------------- estimator
TOL_RT = 1e-6  # R (rad) / T against the oracle (1e-6); measured: parity_log


def _check_hyps(gh, oh, tol=TOL_RT, fixture=None):
    for a, b in zip(gh, oh):
        assert a["R1_valid"] + a["R2_valid"] == b["R1_valid"] + b["R2_valid"]
        same = max(np.abs(a["R1"] - b["R1"]).max(), np.abs(a["R2"] - b["R2"]).max())
        swap = max(np.abs(a["R1"] - b["R2"]).max(), np.abs(a["R2"] - b["R1"]).max())
        e = min(np.abs(a["E"] - b["E"]).max(), np.abs(a["E"] + b["E"]).max())
        if fixture:
            record(fixture + ": every iteration", R=min(same, swap),
                   T=np.abs(a["T"] - b["T"]).max(), E=e)
        assert min(same, swap) <= tol
        assert np.abs(a["T"] - b["T"]).max() <= tol
        assert e <= 1e-6


def _run_find_dev(ctx, kl, kr, W, H, iters):
    import ctypes as C
    import torch
    from erp_match_eightpoint_test_amd import capi, hyps_to_numpy
    cfg = capi.default_cfg(iters=iters)
    m = kl.shape[0]
    dkl = torch.from_numpy(np.ascontiguousarray(kl, np.float32)).cuda()
    dkr = torch.from_numpy(np.ascontiguousarray(kr, np.float32)).cuda()
    res = torch.zeros(capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    hyp = torch.zeros((iters, capi.HYP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    st = ctx.L.erp_eight_point_find_dev(ctx.h, W, H, dkl.data_ptr(), dkr.data_ptr(), m,
                                        C.byref(cfg), res.data_ptr(), hyp.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(capi.RESULT_DTYPE)[0]
    return st, r, hyps_to_numpy(hyp.unsqueeze(0))[0]


def test_find_golden_fixture(ctx):
    g = _npz("find_400_it80.npz")
    st, r, hyps = _run_find_dev(ctx, g["kl"], g["kr"], int(g["W"]), int(g["H"]), 80)
    assert st == 0 and r["status"] == 0
    _check_hyps(hyps, g["hyp"], fixture="find_400_it80")
    assert r["K"] == int(g["K"])
    record("find_400_it80: result", R=np.abs(r["R"] - g["R"]).max(), T=np.abs(r["T"] - g["T"]).max())
    assert np.abs(r["R"] - g["R"]).max() <= TOL_RT
    assert np.abs(r["T"] - g["T"]).max() <= TOL_RT
    # KAT: the recovered rotation is the synthetic ground truth (two_synthesis_image_test)
    assert np.degrees(np.abs(r["R"] - g["euler_gt"])).mean() < 1.0


def test_find_host_api_matches_dev(ctx):
    from erp_match_eightpoint_test_amd import eight_point
    g = _npz("find_400_it80.npz")
    ep = eight_point(ctx=ctx)
    R, T = ep.find(int(g["W"]), int(g["H"]), g["kl"], g["kr"], len(g["kl"]))
    assert np.abs(R - g["R"]).max() <= TOL_RT and np.abs(T - g["T"]).max() <= TOL_RT


def test_find_manual_regime_fixture(ctx):
    g = _npz("find_manual_100_it500.npz")
    st, r, hyps = _run_find_dev(ctx, g["kl"], g["kr"], int(g["W"]), int(g["H"]), 500)
    assert st == 0 and r["status"] == 0
    _check_hyps(hyps, g["hyp"], fixture="find_manual_100_it500")
    assert r["K"] == int(g["K"])
    record("find_manual_100_it500: result", R=np.abs(r["R"] - g["R"]).max(),
           T=np.abs(r["T"] - g["T"]).max())
    assert np.abs(r["R"] - g["R"]).max() <= TOL_RT
    assert np.abs(r["T"] - g["T"]).max() <= TOL_RT


@pytest.mark.parametrize("m", [4, 8, 20, 35, 36])
def test_find_thin_svd_edges(ctx, m):
    g = _npz("find_edges.npz")
    st, r, hyps = _run_find_dev(ctx, g[f"m{m}_kl"], g[f"m{m}_kr"], 5376, 2688, 80)
    assert st == int(g[f"m{m}_status"]) == 0
    if m >= 8:  # sample_n = 1 (m = 4) is rank-1: the rank-2 fix / decomposition is
        # ill-posed there (documented), so only the sampled sets and E are compared
        _check_hyps(hyps, g[f"m{m}_hyp"], fixture=f"find_edges m={m}")
        record(f"find_edges m={m}: result", R=np.abs(r["R"] - g[f"m{m}_R"]).max())
        assert np.abs(r["R"] - g[f"m{m}_R"]).max() <= TOL_RT
    else:
        for a, b in zip(hyps, g[f"m{m}_hyp"]):
            assert min(np.abs(a["E"] - b["E"]).max(), np.abs(a["E"] + b["E"]).max()) <= 1e-6


def test_host_call_after_side_stream_call(gpu_lib, oracle):
    """a host-pointer call (initial_guess, eight_point_estimation) right after an
    async *_dev call on a non-blocking side stream, on ONE context, must not overwrite the
    scratch the side stream is still reading: both results equal their standalone runs"""
    import ctypes as C
    import torch
    from erp_match_eightpoint_test_amd import Context, capi, eight_point
    g = _npz("find_400_it80.npz")
    W, H, iters = int(g["W"]), int(g["H"]), 20000
    ctx = Context(0)
    solo_st, solo, _ = _run_find_dev(ctx, g["kl"], g["kr"], W, H, iters)
    c2 = synth.make_correspondences(11, m=120, outlier_frac=0.2, W=2048, H=1024)
    bl = oracle.pixel_to_bearing(2048, 1024, c2["kp_l"])
    br = oracle.pixel_to_bearing(2048, 1024, c2["kp_r"])
    ep = eight_point(ctx=ctx, iters=80)
    R_solo, T_solo = ep.initial_guess(2048, 1024, bl, br)
    est_solo = ep.eight_point_estimation(2048, 1024, bl, br)
    side = torch.cuda.Stream()
    cfg = capi.default_cfg(iters=iters)
    dkl = torch.from_numpy(np.ascontiguousarray(g["kl"], np.float32)).cuda()
    dkr = torch.from_numpy(np.ascontiguousarray(g["kr"], np.float32)).cuda()
    res = torch.zeros(capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        res.zero_()
        torch.cuda.synchronize()
        assert ctx.L.erp_eight_point_find_dev(ctx.h, W, H, dkl.data_ptr(), dkr.data_ptr(),
                                              len(g["kl"]), C.byref(cfg), res.data_ptr(), None,
                                              side.cuda_stream) == 0
        R, T = ep.initial_guess(2048, 1024, bl, br)  # no sync in between
        est = ep.eight_point_estimation(2048, 1024, bl, br)
        side.synchronize()
        r = res.cpu().numpy().view(capi.RESULT_DTYPE)[0]
        assert r["status"] == solo["status"] == 0 and r["K"] == solo["K"]
        assert np.array_equal(r["R"], solo["R"]) and np.array_equal(r["T"], solo["T"])
        assert np.array_equal(R, R_solo) and np.array_equal(T, T_solo)
        assert all(np.array_equal(a, b) for a, b in zip(est, est_solo))


def test_find_too_few_points(ctx):
    from erp_match_eightpoint_test_amd import ErpError, eight_point
    ep = eight_point(ctx=ctx)
    with pytest.raises(ErpError) as ei:
        ep.find(5376, 2688, np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32), 3)
    assert ei.value.status == 2


def test_eight_point_estimation_api(ctx, oracle):
    from erp_match_eightpoint_test_amd import eight_point
    c = synth.make_correspondences(7, m=40, outlier_frac=0.0, W=2048, H=1024)
    bl = oracle.pixel_to_bearing(2048, 1024, c["kp_l"])
    br = oracle.pixel_to_bearing(2048, 1024, c["kp_r"])
    ho = oracle.eight_point_estimation(bl, br)
    R1, R2, T, v1, v2, E = eight_point(ctx=ctx).eight_point_estimation(2048, 1024, bl, br)
    same = max(np.abs(R1 - ho["R1"]).max(), np.abs(R2 - ho["R2"]).max())
    swap = max(np.abs(R1 - ho["R2"]).max(), np.abs(R2 - ho["R1"]).max())
    assert min(same, swap) <= TOL_RT
    assert np.abs(T - ho["T"]).max() <= TOL_RT
    assert min(np.abs(E - ho["E"]).max(), np.abs(E + ho["E"]).max()) <= 1e-8


# ---------------------------------------------------------------------- batch pipeline
SMALL_BATCH = {"prune": 0, "all_rows": 1000000}


@pytest.fixture(params=["prune", "all_rows"])
def consensus_path(request, ctx):
    """both consensus routes: the Lipschitz / gradient / second-stage pre-pruning that batches
    of more than ERP_OPT_SMALL_BATCH pairs take, and the every-row bounds pass of small batches
    (the single-pair call, capi.hip run_consensus) -- set on the module's context (tests that
    make their own contexts apply SMALL_BATCH[consensus_path] to them)"""
    ctx.set_option("small_batch", SMALL_BATCH[request.param])
    yield request.param
    ctx.set_option("small_batch", -1)


def _batch(pairs, device="cuda"):
    import torch
    dl = np.concatenate([p["desc_l"] for p in pairs])
    dr = np.concatenate([p["desc_r"] for p in pairs])
    kl = np.concatenate([p["kp_l"] for p in pairs])
    kr = np.concatenate([p["kp_r"] for p in pairs])
    ol = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    orr = np.concatenate([[0], np.cumsum([len(p["desc_r"]) for p in pairs])]).astype(np.int64)
    W = np.array([p["W"] for p in pairs], np.int32)
    H = np.array([p["H"] for p in pairs], np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return (t(dl), t(dr), t(kl), t(kr), t(ol), t(orr), t(W), t(H),
            int(np.diff(ol).max()), int(np.diff(orr).max()))


def _check_batch_vs_oracle(oracle, pairs, outs, iters, cfg=None):
    """outs = PairBatchRunner.run(..., want=("matches", "hyps", "samples", "rvec", "dist")) of
    pairs, synchronised: every stage against the oracle (cfg: the oracle's, for a run with
    other constants than the reference's; its iters = iters)"""
    from erp_match_eightpoint_test_amd import hyps_to_numpy, results_to_numpy
    res = results_to_numpy(outs["results"])
    hyps = hyps_to_numpy(outs["hyps"])
    for i, p in enumerate(pairs):
        ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
        M = len(ref)
        assert res[i]["M"] == M
        got = outs["matches"][i, :M].cpu().numpy()
        assert np.array_equal(got.view(np.uint32).reshape(-1), ref.view(np.uint32).reshape(-1))
        kl = p["kp_l"][ref["queryIdx"]]
        kr = p["kp_r"][ref["trainIdx"]]
        o = oracle.find(p["W"], p["H"], kl, kr, cfg or oracle.make_cfg(iters=iters), detail=True)
        s = o["sample_n"]
        got_s = np.sort(outs["samples"][i, :, :s].cpu().numpy(), axis=1)
        assert np.array_equal(got_s, np.sort(o["samples"], axis=1))
        _check_hyps(hyps[i], o["hyp"])
        assert res[i]["K"] == o["K"]
        assert np.abs(res[i]["R"] - o["R"]).max() <= TOL_RT
        assert np.abs(res[i]["T"] - o["T"]).max() <= TOL_RT
        # consensus: the oracle's trimmed means on the GPU's own R list pick the same winner
        K = o["K"]
        rv = outs["rvec"][i, :K].cpu().numpy()
        _, mi, dref = oracle.consensus(rv)
        assert mi == res[i]["min_idx"]  # std::min_element: the FIRST minimum, strictly
        d = outs["dist"][i, :K].cpu().numpy()
        live = np.isfinite(d)
        assert live.sum() >= 1 and np.all(dref[~live] >= dref.min())
        assert np.allclose(d[live], dref[live], rtol=1e-12, atol=0)
    return res


def test_batch_pipeline_vs_oracle(ctx, oracle):
    from erp_match_eightpoint_test_amd import PairBatchRunner
    import torch
    pairs = [synth.make_pair(1000 + i, n_kpts=n) for i, n in enumerate([512, 700, 300, 1024])]
    args = _batch(pairs)
    run = PairBatchRunner(ctx=ctx, iters=200)
    outs = run.run(*args, want=("matches", "hyps", "samples", "rvec", "dist"))
    torch.cuda.synchronize()
    _check_batch_vs_oracle(oracle, pairs, outs, 200)


def _canary_child():
    """body of test_consensus_scratch_canaries (a process of its own: the pad must be set before
    the process's first allocation and never changed)"""
    import oracle
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, capi
    oracle.build()
    L = capi.load()
    L.erp_debug_set_alloc_pad(256)
    c = Context(0)
    for name, v in (("small_batch", 0), ("lip2", 1), ("lipg", 3), ("flat_refs", 25),
                    ("refine_hint", 1), ("zoom_levels", 2)):
        c.set_option(name, v)
    iters = 1100
    sizes = [300, 310, 290, 305, 320, 295, 300, 315, 285]
    pairs = [synth.make_pair(5200 + i, n_kpts=n) for i, n in enumerate(sizes)]
    outs = PairBatchRunner(ctx=c, iters=iters).run(
        *_batch(pairs), want=("matches", "hyps", "samples", "rvec", "dist"))
    torch.cuda.synchronize()
    # one single pair on the small-batch route (automatic: 1 pair x (2 iters)^2 <= 2e9)
    c.set_option("small_batch", -1)
    p = pairs[0]
    mt, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
    st, r, _ = _run_find_dev(c, p["kp_l"][mt["queryIdx"]], p["kp_r"][mt["trainIdx"]], p["W"],
                             p["H"], iters)
    assert L.erp_debug_check_pads() == 0
    assert st == 0 and r["status"] == 0
    res = _check_batch_vs_oracle(oracle, pairs, outs, iters)
    assert np.all(res["status"] == 0)
    assert res["K"].min() >= 1024  # every pair above the no-pre-pruning floor (kLipMinK)
    # the single-pair route picks the batch's winner for that pair
    assert r["K"] == res[0]["K"] and r["min_idx"] == res[0]["min_idx"]
    assert np.abs(r["R"] - res[0]["R"]).max() <= TOL_RT
    assert np.abs(r["T"] - res[0]["T"]).max() <= TOL_RT
    print("canary child ok")


def test_consensus_scratch_canaries(gpu_lib, oracle):
    """every consensus route (second pre-pruning stage, gradient references of both stages, flat
    route, refine hint, two zoom levels: both strides of the row lists in sortbuf) on 9 pairs
    with 256 canary bytes behind every context buffer, then a single pair on the small-batch
    route: no canary touched (erp_consensus_ws.hpp sizes every part the kernels write), all
    statuses OK and the results equal to the oracle's as in test_batch_pipeline_vs_oracle"""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_parity as t; t._canary_child()"
            % (here, os.path.dirname(here)))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "canary child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_batch_pipeline_hip_graph_replay(gpu_lib):
    """erp_ctx_set_graphs: the first call captures the pipeline into a HIP graph, the next calls
    with the same buffers replay it; other buffers or a grown scratch capture anew.  Every
    result (and match list) equals the plain launch sequence's, byte for byte."""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner
    pairs = [synth.make_pair(3100 + i, n_kpts=n) for i, n in enumerate([600, 900, 300])]
    args = _batch(pairs)
    ref = PairBatchRunner(ctx=Context(0), iters=300).run(*args, want=("matches",))
    cg = Context(0)
    cg.set_graphs(True)
    run = PairBatchRunner(ctx=cg, iters=300, reuse_outputs=True)
    st = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(st):
        for _ in range(3):  # capture, replay, replay (same output buffers: reuse one dict)
            o = run.run(*args, want=("matches",), stream=st.cuda_stream)
            outs.append({k: v.clone() for k, v in o.items()})
        st.synchronize()
    for o in outs:
        assert torch.equal(o["results"], ref["results"])
        assert torch.equal(o["matches"], ref["matches"])
    # a larger batch on the same context (grown scratch, new buffers): a new capture, correct
    pairs2 = [synth.make_pair(3200 + i, n_kpts=1500) for i in range(4)]
    args2 = _batch(pairs2)
    ref2 = PairBatchRunner(ctx=Context(0), iters=300).run(*args2)
    with torch.cuda.stream(st):
        o2 = run.run(*args2, stream=st.cuda_stream)
        st.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(o2["results"], ref2["results"])


def test_graph_replay_with_new_contents_equals_fresh_run(gpu_lib):
    """reuse_outputs + graphs: the SAME input buffers refilled with other pairs of the same shape
    replay the captured graph; every output (results, match lists, R_vec_arr) equals a fresh
    plain run of those pairs byte for byte, including the entries past each pair's M / K (the
    pipeline zeroes the optional outputs inside the graph: ADVICE r04)"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner
    sizes = [600, 900, 300]
    args = _batch([synth.make_pair(3300 + i, n_kpts=n) for i, n in enumerate(sizes)])
    args_b = _batch([synth.make_pair(3400 + i, n_kpts=n, inlier_frac=0.5) for i, n in enumerate(sizes)])
    want = ("matches", "rvec", "tvec")
    cg = Context(0)
    cg.set_graphs(True)
    run = PairBatchRunner(ctx=cg, iters=300, reuse_outputs=True)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        run.run(*args, want=want, stream=st.cuda_stream)  # capture (pairs A)
        st.synchronize()
        for a, b in zip(args, args_b):  # refill the same buffers with pairs B
            if isinstance(a, torch.Tensor):
                a.copy_(b)
        o = run.run(*args, want=want, stream=st.cuda_stream)  # replay
        st.synchronize()
        got = {k: v.clone() for k, v in o.items()}
    ref = PairBatchRunner(ctx=Context(0), iters=300).run(*args_b, want=want)
    torch.cuda.synchronize()
    for k in ("results",) + want:
        assert torch.equal(got[k], ref[k]), k


def test_batch_pipeline_valu_matcher_equals_mfma(gpu_lib):
    """the whole batch pipeline with the packed-FP32 exact sweep as the matcher: matches and
    results identical to the MFMA-filter pipeline (ragged pair sizes, several train chunks)"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, capi, results_to_numpy
    sizes = [(700, 650), (1300, 1290), (257, 1031), (2048, 2048)]
    pairs = [synth.make_pair(400 + i, n_kpts=nq, n_train=nt) for i, (nq, nt) in enumerate(sizes)]
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    ol = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    orr = np.concatenate([[0], np.cumsum([len(p["desc_r"]) for p in pairs])]).astype(np.int64)
    args = (t(np.concatenate([p["desc_l"] for p in pairs])),
            t(np.concatenate([p["desc_r"] for p in pairs])),
            t(np.concatenate([p["kp_l"] for p in pairs])),
            t(np.concatenate([p["kp_r"] for p in pairs])), t(ol), t(orr),
            t(np.array([p["W"] for p in pairs], np.int32)),
            t(np.array([p["H"] for p in pairs], np.int32)),
            int(np.diff(ol).max()), int(np.diff(orr).max()))
    outs = {}
    for name, method in (("mfma", capi.MATCHER_MFMA_FILTER), ("valu", capi.MATCHER_VALU_EXACT)):
        c = Context(0)
        c.set_matcher(method)
        o = PairBatchRunner(ctx=c, iters=300).run(*args, want=("matches",))
        torch.cuda.synchronize()
        outs[name] = (results_to_numpy(o["results"]), o["matches"].cpu().numpy())
    ra, ma = outs["mfma"]
    rb, mb = outs["valu"]
    assert np.array_equal(ra.view(np.uint8), rb.view(np.uint8))
    for i in range(len(pairs)):
        M = int(ra[i]["M"])
        assert M > 0 and np.array_equal(ma[i, :M], mb[i, :M])


@pytest.mark.parametrize("sizes,iters", [([4096], 2000), ([512, 700, 300, 1024], 300),
                                         ([9000], 200), ([60000], 70)])
def test_sampler_kernels_identical(gpu_lib, sizes, iters):
    """every glibc-replay sampler kernel gives the same sample sets and records: the throughput
    blocks (sampler_kernel<0>, ERP_OPT_SAMPLER_LAT = 0), the latency blocks step by step (<2>)
    and positions first (<3>), and the split replay (sampler_split_kernel: segments replayed from
    their start bitmaps, ERP_OPT_SAMPLER_SPLIT = 1 -- skipped by the launcher where its bitmaps
    do not fit the LDS, M = 60000); ragged sizes, partial waves, the d < 256 blocks, the
    straddling and last blocks"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    pairs = [synth.make_pair(4300 + i, n_kpts=n) for i, n in enumerate(sizes)]
    args = _batch(pairs)
    outs = {}
    for name, opts in (("lat0", {"sampler_lat": 0, "sampler_split": 0}),
                       ("lat1", {"sampler_lat": 1, "sampler_split": 0}),
                       ("lat2", {"sampler_lat": 2, "sampler_split": 0}),
                       ("split", {"sampler_split": 1})):
        c = Context(0)
        for k, v in opts.items():
            c.set_option(k, v)
        o = PairBatchRunner(ctx=c, iters=iters).run(*args, want=("samples",))
        torch.cuda.synchronize()
        r = results_to_numpy(o["results"])
        assert np.all(r["status"] == 0), name
        outs[name] = (r.view(np.uint8).copy(), o["samples"].cpu().numpy())
    ra, sa = outs["lat0"]
    for name in ("lat1", "lat2", "split"):
        rb, sb = outs[name]
        assert np.array_equal(sa, sb), name
        assert np.array_equal(ra, rb), name


def test_batch_full_size_properties(ctx, oracle):
    """configs[1] shape: 4096 x 4096 keypoints, 10k iterations.  Size-independent checks:
    matches bit-exact vs the oracle, sampled sets of a spread of iterations vs the oracle's
    glibc replay (jump-ahead across 10k * (M-1) draws), KAT on the recovered rotation."""
    import torch
    from erp_match_eightpoint_test_amd import PairBatchRunner, results_to_numpy
    p = synth.make_pair(20200423, n_kpts=4096)
    args = _batch([p])
    run = PairBatchRunner(ctx=ctx, iters=10000)
    outs = run.run(*args, want=("matches", "samples"))
    torch.cuda.synchronize()
    r = results_to_numpy(outs["results"])[0]
    ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"], nthreads=8)
    M = len(ref)
    assert r["status"] == 0 and r["M"] == M
    got = outs["matches"][0, :M].cpu().numpy()
    assert np.array_equal(got.view(np.uint32).reshape(-1), ref.view(np.uint32).reshape(-1))
    s = int(M * 0.25)
    g = oracle.GlibcRand(1)
    samples = outs["samples"][0].cpu().numpy()
    check = {0, 1, 63, 64, 65, 127, 4095, 9999}
    for it in range(10000):
        a = g.random_array(M)
        if it in check:
            assert np.array_equal(np.sort(samples[it, :s]), np.sort(a[:s])), it
    assert np.degrees(np.abs(r["R"] - p["euler_gt"])).mean() < 1.0


def test_sampler_large_match_count(ctx, oracle):
    """M ~ 27k matches: the sampler's i >= s draws land on bitmap words far beyond the
    workgroup's LDS allocation (positions up to M-1: byte offsets up to ~220 KB, past the CU's
    160 KB of LDS),
    which must read as taken and write nothing (kernels.hip replay_block_draws); the sampled sets
    of the first iterations and of a wave boundary equal the oracle's glibc replay."""
    import torch
    from erp_match_eightpoint_test_amd import PairBatchRunner, results_to_numpy
    p = synth.make_pair(4242, n_kpts=60000)
    args = _batch([p])
    outs = PairBatchRunner(ctx=ctx, iters=130).run(*args, want=("samples",))
    torch.cuda.synchronize()
    r = results_to_numpy(outs["results"])[0]
    M = int(r["M"])
    assert r["status"] == 0 and M > 25000
    s = int(M * 0.25)
    g = oracle.GlibcRand(1)
    samples = outs["samples"][0].cpu().numpy()
    for it in range(130):
        a = g.random_array(M)
        if it in (0, 1, 2, 63, 64, 129):
            assert np.array_equal(np.sort(samples[it, :s]), np.sort(a[:s])), it


@pytest.mark.parametrize("sizes,iters", [([512, 700, 300, 1024], 300), ([9000], 200),
                                         ([60000], 70)])
def test_philox_sampler_vs_oracle(gpu_lib, oracle, sizes, iters):
    """sampler = ERP_SAMPLER_PHILOX: every iteration's sampled set equals the
    oracle's Floyd-on-Philox set (erp_oracle.c erpo_philox_sample, Random123 KAT-pinned), the
    hypotheses and the result equal the oracle's find() run with the same sampler; a pair with
    M ~ 27k matches (an 864-word bitmap per lane, past one CU's LDS) gets ERP_INVALID_ARG"""
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, capi, hyps_to_numpy,
                                               results_to_numpy)
    pairs = [synth.make_pair(5100 + i, n_kpts=n) for i, n in enumerate(sizes)]
    args = _batch(pairs)
    c = Context(0)
    outs = PairBatchRunner(ctx=c, iters=iters, sampler=1).run(*args, want=("hyps", "samples"))
    torch.cuda.synchronize()
    res = results_to_numpy(outs["results"])
    hyps = hyps_to_numpy(outs["hyps"])
    for i, p in enumerate(pairs):
        M = int(res[i]["M"])
        if M > 20480:  # beyond one CU's LDS for the per-lane bitmap: a loud status, no result
            assert res[i]["status"] == capi.ERP_INVALID_ARG
            continue
        assert res[i]["status"] == 0
        s = int(M * 0.25)
        got = np.sort(outs["samples"][i, :, :s].cpu().numpy(), axis=1)
        for it in range(iters):
            assert np.array_equal(got[it], oracle.philox_sample(M, s, it)), it
        ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"], nthreads=8)
        assert len(ref) == M
        kl = p["kp_l"][ref["queryIdx"]]
        kr = p["kp_r"][ref["trainIdx"]]
        o = oracle.find(p["W"], p["H"], kl, kr, oracle.make_cfg(iters=iters, sampler=1),
                        detail=True)
        _check_hyps(hyps[i], o["hyp"])
        assert res[i]["K"] == o["K"]
        assert np.abs(res[i]["R"] - o["R"]).max() <= TOL_RT
        assert np.abs(res[i]["T"] - o["T"]).max() <= TOL_RT


def test_philox_hypothesis_blocks_by_offset(ctx, oracle):
    """Philox iteration blocks [a, b) at offset stream_offset(0, a, M, sampler=1) = a reproduce
    one run's records (the counter-based configs[4] partition)"""
    from erp_match_eightpoint_test_amd import dist as D
    import torch
    g = _npz("find_manual_100_it500.npz")
    kl = torch.from_numpy(np.ascontiguousarray(g["kl"])).cuda()
    kr = torch.from_numpy(np.ascontiguousarray(g["kr"])).cuda()
    m = kl.shape[0]
    fn = D.gpu_hypotheses(ctx, int(g["W"]), int(g["H"]), kl, kr, m, {"sampler": 1})
    full = fn(500, 0)
    parts = [fn(b - a, D.stream_offset(0, a, m, 1))
             for a, b in [D.block_range(500, 3, r) for r in range(3)]]
    merged = np.concatenate(parts)
    for f in ("R1", "R2", "T", "R1_valid", "R2_valid", "E"):
        assert np.array_equal(merged[f], full[f]), f
    o = oracle.find(int(g["W"]), int(g["H"]), g["kl"], g["kr"],
                    oracle.make_cfg(iters=500, sampler=1), detail=True)
    _check_hyps(full, o["hyp"])


@pytest.mark.parametrize("m", [20480, 20481, 30000])
def test_philox_match_cap_is_invalid_arg(ctx, m):
    """the Philox sampler's per-lane bitmap holds M <= 20480: every host-m entry point refuses a
    larger pair with ERP_INVALID_ARG up front (hypotheses_dev, find_dev, initial_guess) instead of
    returning hypotheses built from empty samples; M = 20480 itself runs"""
    import ctypes as C

    import torch
    from erp_match_eightpoint_test_amd import HYP_DTYPE, capi
    rng = np.random.default_rng(m)
    kl = torch.from_numpy(rng.uniform(0, 2000, (m, 2)).astype(np.float32)).cuda()
    kr = torch.from_numpy(rng.uniform(0, 2000, (m, 2)).astype(np.float32)).cuda()
    cfg = capi.default_cfg(iters=2, sampler=1)
    hyps = torch.zeros((2, HYP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    res = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    want = capi.ERP_OK if m <= 20480 else capi.ERP_INVALID_ARG
    assert ctx.L.erp_eight_point_hypotheses_dev(ctx.h, 2048, 1024, kl.data_ptr(), kr.data_ptr(),
                                                m, C.byref(cfg), hyps.data_ptr(), st) == want
    assert ctx.L.erp_eight_point_find_dev(ctx.h, 2048, 1024, kl.data_ptr(), kr.data_ptr(), m,
                                          C.byref(cfg), res.data_ptr(), None, st) == want
    torch.cuda.synchronize()
    if m > 20480:
        bl = np.zeros((m, 3))
        bl[:, 2] = 1.0
        out = capi.PairResult()
        assert ctx.L.erp_initial_guess(ctx.h, bl.ctypes.data, bl.ctypes.data, m, C.byref(cfg),
                                       None, None, C.byref(out)) == capi.ERP_INVALID_ARG


# ------------------------------------------------- opt-in inlier count (cfg.inlier_thr > 0)
@pytest.mark.parametrize("sizes,iters,thr,sampler", [([512, 700, 300], 80, 1e-3, 0),
                                                     ([512, 700, 300], 80, 2e-2, 0),
                                                     ([4096], 10000, 5e-3, 0),
                                                     ([1024, 900], 500, 5e-3, 1)])
def test_inlier_count_vs_oracle(gpu_lib, oracle, sizes, iters, thr, sampler):
    """erp_ransac_cfg.inlier_thr > 0 (no reference counterpart): every iteration's
    count of |l^T E' r| < thr over ALL M matches equals the oracle's fp64 count evaluated on the
    GPU record's own E (erpo_rank2 + erpo_inlier_count: exact, up to the matches within 1e-12 of
    the threshold), and the oracle find's own count within the matches a 1e-9 change of E' could
    flip (80 / 500 iterations); the result records equal the run with the count off, whose
    records carry 0 (the default path is unchanged)."""
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, hyps_to_numpy,
                                               results_to_numpy)
    pairs = [synth.make_pair(7300 + i, n_kpts=n) for i, n in enumerate(sizes)]
    args = _batch(pairs)
    c = Context(0)
    on = PairBatchRunner(ctx=c, iters=iters, sampler=sampler, inlier_thr=thr).run(
        *args, want=("matches", "hyps"))
    off = PairBatchRunner(ctx=c, iters=iters, sampler=sampler).run(*args, want=("hyps",))
    torch.cuda.synchronize()
    r_on, r_off = results_to_numpy(on["results"]), results_to_numpy(off["results"])
    assert np.array_equal(r_on.view(np.uint8), r_off.view(np.uint8))
    h_on, h_off = hyps_to_numpy(on["hyps"]), hyps_to_numpy(off["hyps"])
    assert (h_off["inliers"] == 0).all()
    for f in ("R1", "R2", "T", "R1_valid", "R2_valid", "E"):
        assert np.array_equal(h_on[f], h_off[f]), f
    for i, p in enumerate(pairs):
        assert r_on[i]["status"] == 0
        M = int(r_on[i]["M"])
        mt = on["matches"][i, :M].cpu().numpy()
        bl = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_l"][mt[:, 0]])
        br = oracle.pixel_to_bearing(p["W"], p["H"], p["kp_r"][mt[:, 1]])
        got = h_on[i]["inliers"]
        assert got.max() > 0 and (got <= M).all()
        for it in range(iters):
            n, nb = oracle.inlier_count(bl, br, oracle.rank2(h_on[i][it]["E"]), thr, 1e-12)
            assert abs(int(got[it]) - n) <= nb, (i, it, int(got[it]), n, nb)
        if iters <= 500:
            o = oracle.find(p["W"], p["H"], p["kp_l"][mt[:, 0]], p["kp_r"][mt[:, 1]],
                            oracle.make_cfg(iters=iters, sampler=sampler, inlier_thr=thr),
                            detail=True)
            for it in range(iters):
                _, nb = oracle.inlier_count(bl, br, o["hyp"][it]["E_corr"], thr, 1e-9)
                assert abs(int(got[it]) - int(o["hyp"][it]["inliers"])) <= nb, (i, it)
            # the consensus winner's count: the iteration that pushed row min_idx
            v = h_on[i]["R1_valid"].astype(int) + h_on[i]["R2_valid"].astype(int)
            w_it = int(np.searchsorted(np.cumsum(v), int(r_on[i]["min_idx"]), side="right"))
            print(f"pair {i}: winner iteration {w_it} inliers {got[w_it]} of M {M} "
                  f"(median {np.median(got)}, max {got.max()})")
            assert got[w_it] > 0


# ---------------------------------------------------------- sharding entry points (GPU)
def test_hypothesis_blocks_by_offset_match_full_run(ctx, oracle):
    """erp_eight_point_hypotheses_dev on iteration blocks [0,a) and [a,I) with the glibc offset
    a*(M-1) reproduces the records of one I-iteration run (configs[4] sharding on one GPU)."""
    import torch
    from erp_match_eightpoint_test_amd import dist as D
    g = _npz("find_manual_100_it500.npz")
    kl = torch.from_numpy(np.ascontiguousarray(g["kl"])).cuda()
    kr = torch.from_numpy(np.ascontiguousarray(g["kr"])).cuda()
    m = kl.shape[0]
    fn = D.gpu_hypotheses(ctx, int(g["W"]), int(g["H"]), kl, kr, m, {})
    full = fn(500, 0)
    parts = [fn(b - a, a * (m - 1)) for a, b in [D.block_range(500, 3, r) for r in range(3)]]
    merged = np.concatenate(parts)
    for f in ("R1", "R2", "T", "R1_valid", "R2_valid", "E"):
        bad = np.nonzero(np.any((merged[f] != full[f]).reshape(len(full), -1), axis=1))[0]
        assert len(bad) == 0, (f, bad[:10], merged[f][bad[:3]], full[f][bad[:3]])
    _check_hyps(full, g["hyp"])
    rvec, tvec = D.valid_list(merged)
    res = D.gpu_consensus(ctx, "cuda")(rvec, tvec)
    assert res["status"] == 0 and res["K"] == int(g["K"])
    assert np.abs(res["R"] - g["R"]).max() <= TOL_RT and np.abs(res["T"] - g["T"]).max() <= TOL_RT


@pytest.mark.parametrize("world", [1, 3, 8])
def test_hypothesis_sharded_dev_padded_blocks(ctx, world):
    """the device-resident configs[4] partition: zero-padded blocks of B = ceil(I / world)
    records per rank (emulated in one process, concatenated in rank order as the RCCL
    all-gather would) -> erp_consensus_hyps_dev gives the unsharded find's result; world 1 goes
    through dist.find_hypothesis_sharded_dev itself."""
    import ctypes as C

    import torch
    from erp_match_eightpoint_test_amd import HYP_DTYPE, capi, eight_point, results_to_numpy
    from erp_match_eightpoint_test_amd import dist as D
    g = _npz("find_manual_100_it500.npz")
    W, H = int(g["W"]), int(g["H"])
    kl = torch.from_numpy(np.ascontiguousarray(g["kl"])).cuda()
    kr = torch.from_numpy(np.ascontiguousarray(g["kr"])).cuda()
    m, iters = kl.shape[0], 500
    if world == 1:
        res, _ = D.find_hypothesis_sharded_dev(ctx, W, H, kl, kr, m, iters)
    else:
        blocks = []
        for r in range(world):
            blk, a, b = D.padded_block(iters, world, r)
            loc = torch.zeros((blk, HYP_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
            if b > a:
                cfg = capi.default_cfg(iters=b - a, offset=a * (m - 1))
                capi.check(ctx.L.erp_eight_point_hypotheses_dev(
                    ctx.h, W, H, kl.data_ptr(), kr.data_ptr(), m, C.byref(cfg), loc.data_ptr(),
                    torch.cuda.current_stream().cuda_stream), "hypotheses")
            blocks.append(loc)
        merged = torch.cat(blocks)
        res = torch.zeros(64, dtype=torch.uint8, device="cuda")
        cfg = capi.default_cfg(iters=iters)
        capi.check(ctx.L.erp_consensus_hyps_dev(ctx.h, m, merged.data_ptr(), merged.shape[0],
                                                C.byref(cfg), res.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream),
                   "consensus_hyps")
    torch.cuda.synchronize()
    r = results_to_numpy(res.view(1, -1))[0]
    ep = eight_point(ctx=ctx, iters=iters)
    R, T = ep.find(W, H, g["kl"], g["kr"])
    assert r["status"] == 0 and r["K"] == int(g["K"]) == ep.last_result["K"]
    assert r["min_idx"] == ep.last_result["min_idx"]
    assert np.array_equal(r["R"], R) and np.array_equal(r["T"], T)


@pytest.mark.parametrize("world,iters", [(2, 500), (3, 500), (8, 500), (5, 4000), (2, 100000),
                                         (8, 100000)])
def test_consensus_row_shards_equal_unsharded(ctx, world, iters, consensus_path):
    """configs[4]'s sharded consensus: the K^2 bounds pass split into `world` row shards
    (erp_consensus_hyps_shard_dev per shard: reference rows, Lipschitz pre-pruning against the
    shard's own references, the kept rows; summed as the RCCL all_reduce would) then
    erp_consensus_hyps_finish_dev gives the unsharded find's result, field for field -- up to
    configs[4]'s 100k iterations (K ~ 89k rows)."""
    import torch
    from erp_match_eightpoint_test_amd import eight_point, results_to_numpy
    from erp_match_eightpoint_test_amd import dist as D
    g = _npz("find_manual_100_it500.npz")
    W, H = int(g["W"]), int(g["H"])
    kl = torch.from_numpy(np.ascontiguousarray(g["kl"])).cuda()
    kr = torch.from_numpy(np.ascontiguousarray(g["kr"])).cuda()
    m = kl.shape[0]
    res, _ = D.find_hypothesis_sharded_dev(ctx, W, H, kl, kr, m, iters, emulate_world=world)
    torch.cuda.synchronize()
    r = results_to_numpy(res.view(1, -1))[0]
    ep = eight_point(ctx=ctx, iters=iters)
    R, T = ep.find(W, H, g["kl"], g["kr"])
    ref = ep.last_result
    for f in ("status", "K", "min_idx", "near_ties"):
        assert r[f] == ref[f], (f, r[f], ref[f])
    # (how many rows survive the selections depends on which references each shard prunes
    # with -- a diagnostic, not part of the result; include/erp_match.h says so).  Bounded:
    # a survivor is a binned row (pruned rows get LB > every UB), so 1 <= survivors <= binned
    # rows <= K (the row-sharded path reports binned_rows = K: not combined over the shards)
    assert 1 <= ref["survivors"] <= ref["binned_rows"] <= ref["K"]
    assert 1 <= r["survivors"] <= r["binned_rows"] == r["K"]
    assert np.array_equal(r["R"], R) and np.array_equal(r["T"], T)
    assert r["min_dist"] == ref["min_dist"]


@pytest.mark.parametrize("K", [1, 2, 3, 5, 40, 1000])
def test_consensus_dev_vs_oracle(ctx, oracle, K, consensus_path):
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng(K)
    rv = (rng.standard_normal((K, 3)) * 0.01).astype(np.float32)
    if K >= 5:
        rv[K // 2] = rv[1]           # exact duplicate rows (tie -> first index)
    tv = rng.standard_normal((K, 3)).astype(np.float32)
    rc, mi, d = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, tv)
    assert res["status"] == 0 and res["K"] == K
    assert res["min_idx"] == mi
    assert np.array_equal(res["R"], rv[mi]) and np.array_equal(res["T"], tv[mi])


def test_consensus_bimodal_many_survivors(ctx, oracle, consensus_path):
    """two far clusters (R1 and R2 both valid): the bounds prune little; still exact."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng(9)
    a = rng.standard_normal((600, 3)) * 6e-5 + np.array([0.1, 0.2, 0.3])
    b = rng.standard_normal((600, 3)) * 6e-5 + np.array([-1.2, 0.9, 0.4])
    rv = np.concatenate([a, b]).astype(np.float32)[rng.permutation(1200)]
    tv = np.zeros_like(rv)
    rc, mi, d = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, tv)
    assert res["min_idx"] == mi


def test_consensus_heavy_duplicates(ctx, oracle, consensus_path):
    """few distinct R vectors repeated many times: zero distances put the window ranks in the
    underflow bin, which takes the radix fallback of consensus_rows."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng(21)
    base = (rng.standard_normal((5, 3)) * 0.01).astype(np.float32)
    rv = base[rng.integers(0, 5, 1500)]
    tv = rng.standard_normal((1500, 3)).astype(np.float32)
    rc, mi, d = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, tv)
    assert res["status"] == 0
    assert res["min_idx"] == mi


def test_consensus_survivor_means_bimodal_pair(ctx, oracle, consensus_path):
    """a full-size synthetic pair whose R1 and R2 are both valid in every iteration (K = 2I):
    thousands of consensus survivors; their trimmed means must match the oracle's."""
    from erp_match_eightpoint_test_amd import PairBatchRunner, results_to_numpy
    import torch
    p = synth.make_pair(20200423 + 8, n_kpts=4096)
    run = PairBatchRunner(ctx=ctx, iters=1500)
    outs = run.run(*_batch([p]), want=("rvec", "dist"))
    torch.cuda.synchronize()
    res = results_to_numpy(outs["results"])[0]
    K = int(res["K"])
    assert K == 3000   # R1 and R2 valid in every iteration: the two-cluster regime (the
    #                    coarse bounds keep most rows; the refine pass and the exact pass decide)
    rv = outs["rvec"][0, :K].cpu().numpy()
    _, mi, dref = oracle.consensus(rv)
    assert mi == res["min_idx"]
    d = outs["dist"][0, :K].cpu().numpy()
    live = np.isfinite(d)
    assert live.sum() == res["survivors"]
    assert np.all(dref[~live] >= dref.min())
    assert np.allclose(d[live], dref[live], rtol=1e-12, atol=0)


def test_consensus_nonfinite_input_is_invalid_arg(ctx):
    """a NaN / inf rotation vector handed to the consensus-only entry is rejected
    (ERP_INVALID_ARG) instead of being binned."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng(5)
    for bad in (np.nan, np.inf, -np.inf):
        rv = (rng.standard_normal((300, 3)) * 0.01).astype(np.float32)
        rv[137, 1] = bad
        res = D.gpu_consensus(ctx, "cuda")(rv, np.zeros_like(rv))
        assert res["status"] == 1, res
    rv = (rng.standard_normal((300, 3)) * 0.01).astype(np.float32)  # the context recovers
    assert D.gpu_consensus(ctx, "cuda")(rv, np.zeros_like(rv))["status"] == 0


@pytest.mark.parametrize("case", ["wide_range", "dup_block", "tiny_cluster"])
def test_consensus_bounds_wide_dynamic_range(ctx, oracle, case, consensus_path):
    """binned-distance bounds when the window's ranks sit in the lowest binades of the
    40-binade range (tight cluster + rotations near the validity limit, many exact duplicates):
    the winner and every survivor's mean stay exact."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng({"wide_range": 1, "dup_block": 2, "tiny_cluster": 3}[case])
    K = 2500
    if case == "wide_range":
        rv = rng.standard_normal((K, 3)) * 1e-5 + 0.3
        far = rng.choice(K, 40, replace=False)
        rv[far] = rng.uniform(-1.56, 1.56, (40, 3))
    elif case == "dup_block":
        rv = rng.standard_normal((K, 3)) * 2e-3
        rv[rng.choice(K, 900, replace=False)] = rv[7]
        rv[rng.choice(K, 30, replace=False)] = rng.uniform(-1.5, 1.5, (30, 3))
    else:
        rv = rng.standard_normal((K, 3)) * 1e-7 + np.array([1.0, -0.5, 0.25])
    rv = rv.astype(np.float32)
    tv = rng.standard_normal((K, 3)).astype(np.float32)
    _, mi, dref = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, tv)
    assert res["status"] == 0 and res["K"] == K
    # the first minimum strictly, and ITS T (tv is random: another duplicate's T differs)
    assert res["min_idx"] == mi
    assert np.array_equal(res["R"], rv[mi]) and np.array_equal(res["T"], tv[mi])
    assert abs(res["min_dist"] - dref[mi]) <= 1e-12 * abs(dref[mi])


@pytest.mark.parametrize("case", ["cluster", "cluster_outliers", "shell", "uniform_cube",
                                  "two_clusters"])
def test_consensus_lipschitz_prepruning(ctx, oracle, case, consensus_path):
    """K >= 1024: the bounds pass first bins every 32nd row, rows provably beaten through the
    1-Lipschitz bound T(i) >= T(c) - d(i, c) skip the histogram pass.  The winner and its mean
    stay exact; on a single cluster most rows are pruned (binned_rows well below K); on a shell
    (every mean nearly equal) little is pruned and the result is still exact."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng({"cluster": 11, "cluster_outliers": 12, "shell": 13,
                                 "uniform_cube": 14, "two_clusters": 15}[case])
    K = 6000
    if case == "cluster":
        rv = rng.standard_normal((K, 3)) * 6e-5 + np.array([0.09, 0.24, 0.26])
    elif case == "cluster_outliers":
        rv = rng.standard_normal((K, 3)) * 6e-5 + np.array([0.09, 0.24, 0.26])
        far = rng.choice(K, 300, replace=False)
        rv[far] = rng.uniform(-1.5, 1.5, (300, 3))
    elif case == "shell":
        v = rng.standard_normal((K, 3))
        rv = 0.01 * v / np.linalg.norm(v, axis=1, keepdims=True) + 0.2
    elif case == "uniform_cube":
        rv = rng.uniform(-1.0, 1.0, (K, 3))
    else:
        a = rng.standard_normal((K // 2, 3)) * 6e-5 + np.array([0.1, 0.2, 0.3])
        b = rng.standard_normal((K - K // 2, 3)) * 6e-5 + np.array([-1.2, 0.9, 0.4])
        rv = np.concatenate([a, b])[rng.permutation(K)]
    rv = rv.astype(np.float32)
    tv = rng.standard_normal((K, 3)).astype(np.float32)
    _, mi, dref = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, tv)
    assert res["status"] == 0 and res["K"] == K
    # the first minimum strictly, and ITS T (tv is random: another duplicate's T differs)
    assert res["min_idx"] == mi
    assert np.array_equal(res["R"], rv[mi]) and np.array_equal(res["T"], tv[mi])
    assert abs(res["min_dist"] - dref[mi]) <= 1e-12 * abs(dref[mi])
    assert (K + 47) // 48 <= res["binned_rows"] <= K  # (the reference rows: every 48th)
    if case in ("cluster", "cluster_outliers", "uniform_cube") and consensus_path == "prune":
        assert res["binned_rows"] < K // 2, res["binned_rows"]


@pytest.mark.parametrize("case", ["cluster", "cluster_outliers", "shell", "two_clusters",
                                  "bench_pairs"])
def test_consensus_grad_pruning_exact(gpu_lib, oracle, case, consensus_path):
    """the convexity-augmented pruning (central references' distance gradient G, ERP_OPT_LIPG) keeps
    every result field the Lipschitz-only run gives (status, K, min_idx, R, T, min_dist,
    near_ties), is deterministic run to run (every byte, binned_rows included), and bins no more
    rows than Lipschitz alone -- on synthetic clouds against the oracle and on configs[1]-shaped
    pairs through the batch pipeline"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    from erp_match_eightpoint_test_amd import dist as D

    def ctx_with(v):
        c = Context(0)
        c.set_option("lipg", int(v))
        c.set_option("small_batch", SMALL_BATCH[consensus_path])
        return c

    if case == "bench_pairs":
        pairs = [synth.make_pair(20200423 + i, n_kpts=2048) for i in range(6)]
        args = _batch(pairs)
        recs = {}
        for v in ("0", "1", "1", "3", "3"):
            out = PairBatchRunner(ctx=ctx_with(v), iters=10000).run(*args)
            torch.cuda.synchronize()
            recs.setdefault(v, []).append(results_to_numpy(out["results"]))
        a = recs["0"][0]
        for v in ("1", "3"):
            b = recs[v][0]
            assert np.array_equal(recs[v][0].view(np.uint8), recs[v][1].view(np.uint8))
            for f in ("status", "M", "K", "min_idx", "R", "T", "min_dist", "near_ties"):
                assert np.array_equal(a[f], b[f]), (v, f)
            # (a second-stage reference the gradient prunes no longer prunes for stage 2: a few
            # rows may move to the coarse list, so the bound is on the total, not per row)
            assert b["binned_rows"].sum() <= a["binned_rows"].sum(), v
            print(f"binned rows lipschitz {a['binned_rows'].tolist()} -> lipg={v} "
                  f"{b['binned_rows'].tolist()}")
        return
    rng = np.random.default_rng({"cluster": 21, "cluster_outliers": 22, "shell": 23,
                                 "two_clusters": 25}[case])
    K = 8000
    if case == "cluster":
        rv = rng.standard_normal((K, 3)) * 6e-5 + np.array([0.09, 0.24, 0.26])
    elif case == "cluster_outliers":
        rv = rng.standard_normal((K, 3)) * 6e-5 + np.array([0.09, 0.24, 0.26])
        far = rng.choice(K, 400, replace=False)
        rv[far] = rng.uniform(-1.5, 1.5, (400, 3))
    elif case == "shell":
        v = rng.standard_normal((K, 3))
        rv = 0.01 * v / np.linalg.norm(v, axis=1, keepdims=True) + 0.2
    else:
        a = rng.standard_normal((K // 2, 3)) * 6e-5 + np.array([0.1, 0.2, 0.3])
        b = rng.standard_normal((K - K // 2, 3)) * 6e-5 + np.array([-1.2, 0.9, 0.4])
        rv = np.concatenate([a, b])[rng.permutation(K)]
    rv = rv.astype(np.float32)
    tv = rng.standard_normal((K, 3)).astype(np.float32)
    _, mi, dref = oracle.consensus(rv)
    r0 = D.gpu_consensus(ctx_with("0"), "cuda")(rv, tv)
    r1 = D.gpu_consensus(ctx_with("1"), "cuda")(rv, tv)
    r2 = D.gpu_consensus(ctx_with("1"), "cuda")(rv, tv)
    r3 = D.gpu_consensus(ctx_with("3"), "cuda")(rv, tv)
    assert r1.tobytes() == r2.tobytes()
    assert r3.tobytes() == D.gpu_consensus(ctx_with("3"), "cuda")(rv, tv).tobytes()
    assert r3["binned_rows"] <= r0["binned_rows"] + 64, (r3["binned_rows"], r0["binned_rows"])
    for r in (r0, r1, r3):
        assert r["status"] == 0 and r["min_idx"] == mi
        assert abs(r["min_dist"] - dref[mi]) <= 1e-12 * abs(dref[mi])
    assert r1["binned_rows"] <= r0["binned_rows"] + 64, (r1["binned_rows"], r0["binned_rows"])


@pytest.mark.parametrize("case", ["two_clusters", "twin_pairs", "bench_pairs"])
def test_consensus_refine_hint_and_flat_exact(gpu_lib, oracle, case, consensus_path):
    """the refine pass's hinted sub-bin windows (ERP_OPT_REFINE_HINT; kernels.hip
    consensus_hint_kernel / refine_windows) and the flat-pair route (ERP_OPT_FLAT_REFS: the
    first-stage references refined, the first stage re-run against them) keep every result
    field of the run without them, are deterministic run to run, and leave no more survivors
    for the exact pass -- on a synthetic two-cluster set against the oracle, on two-cluster
    configs[1]-shaped pairs (the bench's worst-case seeds, R1 and R2 valid in every iteration;
    the first against the oracle's consensus on its own rotation vectors) and on the default
    bench pairs through the batch pipeline"""
    import json
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    from erp_match_eightpoint_test_amd import dist as D

    def ctx_with(hint, flat):
        c = Context(0)
        c.set_option("refine_hint", int(hint))
        c.set_option("flat_refs", int(flat))
        c.set_option("small_batch", SMALL_BATCH[consensus_path])
        return c

    variants = (("0", "0"), ("1", "0"), ("1", "25"), ("1", "25"))
    fields = ("status", "M", "K", "min_idx", "R", "T", "min_dist", "near_ties")
    if case in ("twin_pairs", "bench_pairs"):
        if case == "twin_pairs":
            seeds = json.load(open(os.path.join(os.path.dirname(__file__), "..", "scripts",
                                                "twin_seeds.json")))["seeds"]
            pairs = [synth.make_pair(seeds[i], n_kpts=4096, inlier_frac=0.98)
                     for i in (0, 3, 4, 5)]
        else:
            pairs = [synth.make_pair(20200423 + i, n_kpts=4096) for i in range(8)]
        args = _batch(pairs)
        recs = []
        for v in variants:
            out = PairBatchRunner(ctx=ctx_with(*v), iters=10000).run(*args, want=("rvec",))
            torch.cuda.synchronize()
            recs.append((results_to_numpy(out["results"]), out["rvec"][0].cpu().numpy()))
        a, rv0 = recs[0]
        assert np.array_equal(recs[2][0].view(np.uint8), recs[3][0].view(np.uint8))
        for b, _ in recs[1:]:
            for f in fields:
                assert np.array_equal(a[f], b[f]), f
        # hinted windows: never more survivors; the flat route: never more binned rows
        assert np.all(recs[1][0]["survivors"] <= a["survivors"])
        assert np.all(recs[2][0]["binned_rows"] <= recs[1][0]["binned_rows"])
        for name, (r, _) in zip(("none", "hint", "hint+flat"), recs[:3]):
            print(f"{case} {name}: survivors {r['survivors'].tolist()} "
                  f"binned_rows {r['binned_rows'].tolist()}")
        if case == "twin_pairs":
            assert a["K"][0] == 20000  # the two-cluster regime
            if consensus_path == "prune":
                assert recs[2][0]["binned_rows"][0] < a["binned_rows"][0] // 4
            _, mi, _ = oracle.consensus(rv0[:int(a["K"][0])])
            assert int(recs[2][0]["min_idx"][0]) == mi
        return
    rng = np.random.default_rng(26)
    K = 8000
    a_ = rng.standard_normal((K // 2, 3)) * 6e-5 + np.array([0.1, 0.2, 0.3])
    b_ = rng.standard_normal((K - K // 2, 3)) * 6e-5 + np.array([-1.2, 0.9, 0.4])
    rv = np.concatenate([a_, b_])[rng.permutation(K)].astype(np.float32)
    tv = rng.standard_normal((K, 3)).astype(np.float32)
    _, mi, dref = oracle.consensus(rv)
    res = [D.gpu_consensus(ctx_with(*v), "cuda")(rv, tv) for v in variants]
    assert res[2].tobytes() == res[3].tobytes()
    for r in res:
        assert r["status"] == 0 and r["min_idx"] == mi
        assert abs(r["min_dist"] - dref[mi]) <= 1e-12 * abs(dref[mi])
    assert res[1]["survivors"] <= res[0]["survivors"]
    assert res[2]["binned_rows"] <= res[1]["binned_rows"]
    print(f"survivors {[int(r['survivors']) for r in res[:3]]} "
          f"binned_rows {[int(r['binned_rows']) for r in res[:3]]}")


def test_consensus_small_set_bins_every_row(ctx, oracle, consensus_path):
    """below 1024 rows there is no pre-pruning: every row is binned."""
    from erp_match_eightpoint_test_amd import dist as D
    rng = np.random.default_rng(31)
    rv = (rng.standard_normal((900, 3)) * 0.01).astype(np.float32)
    _, mi, _ = oracle.consensus(rv)
    res = D.gpu_consensus(ctx, "cuda")(rv, np.zeros_like(rv))
    assert res["min_idx"] == mi and res["binned_rows"] == 900
