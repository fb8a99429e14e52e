"""The rand stream on the GPU: finds and batched pairs that continue the glibc rand() stream as
the reference's process-global rand() does (include/erp_match.h "rand stream").

Consumption rule under test: a pair consumes iters (M - 1) draws when the sampler runs it
((int)(M sample_frac) >= 1 and M >= 2), 0 otherwise; pairs of a batch consume in pair order,
calls in the order they take the stream.  Every expectation is the CPU oracle's find at the
offset the rule gives.  Bars: R, T within 1e-6 of the oracle, integer fields exact, sample sets
exact as sets."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest

from erp_match_eightpoint_test_amd import synth

pytestmark = pytest.mark.gpu
TOL_RT = 1e-6
ITERS = 80
FRAC = 0.25
WORK_COUNTERS = ("survivors", "binned_rows")  # diagnostics of the route, not of the result


def _draws(M, iters=ITERS):
    return iters * (M - 1) if (int(M * FRAC) >= 1 and M >= 2) else 0


@pytest.fixture(scope="module")
def pairs(oracle):
    """5 ragged pairs, the third from unrelated descriptors (no match survives the ratio test:
    the sampler does not run it), each with the oracle's matches and gathered keypoints --
    computed once, never modified"""
    out = []
    for i, n in enumerate([50, 70, 60, 64, 90]):
        p = synth.make_pair(9100 + i, n_kpts=n)
        if i == 2:
            p["desc_r"] = synth.random_descriptors(np.random.default_rng(77), n)
        ref, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
        p["M"] = len(ref)
        p["kl"] = np.ascontiguousarray(p["kp_l"][ref["queryIdx"]])
        p["kr"] = np.ascontiguousarray(p["kp_r"][ref["trainIdx"]])
        out.append(p)
    Ms = [p["M"] for p in out]
    assert Ms[2] < 4 and _draws(Ms[2]) == 0, Ms
    assert len(set(Ms)) == 5 and all(M >= 30 for k, M in enumerate(Ms) if k != 2), Ms
    return out


def _batch(pairs, device="cuda"):
    import torch
    cat = lambda k: np.concatenate([p[k] for p in pairs])  # noqa: E731
    ol = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    orr = np.concatenate([[0], np.cumsum([len(p["desc_r"]) for p in pairs])]).astype(np.int64)
    W = np.array([p["W"] for p in pairs], np.int32)
    H = np.array([p["H"] for p in pairs], np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return (t(cat("desc_l")), t(cat("desc_r")), t(cat("kp_l")), t(cat("kp_r")), t(ol), t(orr), t(W),
            t(H), int(np.diff(ol).max()), int(np.diff(orr).max()))


def _ofind(oracle, p, offset, detail=False, iters=ITERS):
    return oracle.find(p["W"], p["H"], p["kl"], p["kr"], oracle.make_cfg(iters=iters, offset=offset),
                       detail=detail)


def _check_result(r, o, M):
    """an erp_pair_result record (or eight_point.last_result) against the oracle's find"""
    assert r["status"] == 0 and r["M"] == M
    assert r["K"] == o["K"] and r["min_idx"] == o["min_idx"] and r["sample_n"] == o["sample_n"]
    dR, dT = np.abs(r["R"] - o["R"]).max(), np.abs(r["T"] - o["T"]).max()
    print(f"M={M} K={r['K']} |dR|={dR:.2e} |dT|={dT:.2e}")
    assert dR <= TOL_RT and dT <= TOL_RT


def _check_hyps(gh, oh):
    for a, b in zip(gh, oh):
        assert a["R1_valid"] + a["R2_valid"] == b["R1_valid"] + b["R2_valid"]
        same = max(np.abs(a["R1"] - b["R1"]).max(), np.abs(a["R2"] - b["R2"]).max())
        swap = max(np.abs(a["R1"] - b["R2"]).max(), np.abs(a["R2"] - b["R1"]).max())
        assert min(same, swap) <= TOL_RT
        assert np.abs(a["T"] - b["T"]).max() <= TOL_RT


def _check_batch(oracle, pairs, outs, base):
    """every pair of a run that started `base` draws into the stream; returns the draws the run
    consumed, derived from the returned M's"""
    from erp_match_eightpoint_test_amd import hyps_to_numpy, results_to_numpy
    res = results_to_numpy(outs["results"])
    hyps = hyps_to_numpy(outs["hyps"])
    off = base
    for i, p in enumerate(pairs):
        M = int(res[i]["M"])
        assert M == p["M"]
        if _draws(M) == 0:  # the sampler skipped it: nothing drawn, the next pair starts here too
            assert res[i]["status"] == 2 and i == 2
            continue
        o = _ofind(oracle, p, off, detail=True)
        s = o["sample_n"]
        got = np.sort(outs["samples"][i, :, :s].cpu().numpy(), axis=1)
        assert np.array_equal(got, np.sort(o["samples"], axis=1)), (i, off)
        _check_hyps(hyps[i], o["hyp"])
        _check_result(res[i], o, M)
        off += _draws(M)
    return off - base


def _same_records(a, b):
    """erp_pair_result records byte-identical apart from the work counters"""
    a, b = a.copy(), b.copy()
    for f in WORK_COUNTERS:
        a[f] = 0
        b[f] = 0
    return a.tobytes() == b.tobytes()


def _find_dev(ctx, p, iters=ITERS):
    import torch
    from erp_match_eightpoint_test_amd import capi
    cfg = capi.default_cfg(iters=iters)
    dkl = torch.from_numpy(p["kl"]).cuda()
    dkr = torch.from_numpy(p["kr"]).cuda()
    res = torch.zeros(capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    st = ctx.L.erp_eight_point_find_dev(ctx.h, p["W"], p["H"], dkl.data_ptr(), dkr.data_ptr(),
                                        p["M"], C.byref(cfg), res.data_ptr(), None,
                                        torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return res.cpu().numpy().view(capi.RESULT_DTYPE)[0]


def test_two_finds_on_two_objects_share_the_stream(gpu_lib, oracle, pairs):
    """the red-before-green test: the second find continues where the first stopped"""
    from erp_match_eightpoint_test_amd import RandStream, eight_point
    a, b = pairs[0], pairs[1]  # M = 40 and 54
    assert a["M"] != b["M"]
    rs = RandStream(1, 0)
    for p, off in ((a, 0), (b, ITERS * (a["M"] - 1))):
        ep = eight_point(stream=rs, iters=ITERS)  # a fresh object per find, as the reference
        assert rs.get() == (1, off)
        ep.find(p["W"], p["H"], p["kl"], p["kr"])
        _check_result(ep.last_result, _ofind(oracle, p, off), p["M"])
    assert rs.get() == (1, ITERS * (a["M"] - 1) + ITERS * (b["M"] - 1))
    # without a stream every find starts at offset 0, as it always did
    for p in (a, b):
        ep = eight_point(iters=ITERS)
        ep.find(p["W"], p["H"], p["kl"], p["kr"])
        _check_result(ep.last_result, _ofind(oracle, p, 0), p["M"])


def test_cpp_driver_on_the_process_stream(gpu_lib, oracle, pairs, tmp_path):
    """tests/cpp/rand_stream_driver.cpp: g++-linked, erp::rand_stream::process() on two
    successive erp::eight_point objects"""
    from erp_match_eightpoint_test_amd import _build
    from erp_match_eightpoint_test_amd.capi import RESULT_DTYPE
    driver = _build.build_stream_driver()
    sets = [pairs[0], pairs[1]]
    ind, outd = tmp_path / "in", tmp_path / "out"
    ind.mkdir()
    outd.mkdir()
    np.array([sets[0]["W"], sets[0]["H"], ITERS, len(sets)] + [p["M"] for p in sets],
             np.int32).tofile(ind / "meta.i32")
    for i, p in enumerate(sets):
        p["kl"].tofile(ind / f"kl{i}.f32")
        p["kr"].tofile(ind / f"kr{i}.f32")
    r = subprocess.run([driver, str(ind), str(outd)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    offs = [0, _draws(sets[0]["M"]), _draws(sets[0]["M"]) + _draws(sets[1]["M"])]
    assert np.fromfile(outd / "draws.u64", np.uint64).tolist() == offs
    for i, p in enumerate(sets):
        raw = np.fromfile(outd / f"find{i}.bin", np.uint8)
        res = raw[24:].view(RESULT_DTYPE)[0]
        o = _ofind(oracle, p, offs[i])
        _check_result(res, o, p["M"])
        assert np.abs(raw[:12].view(np.float32) - o["R"]).max() <= TOL_RT
        assert np.abs(raw[12:24].view(np.float32) - o["T"]).max() <= TOL_RT


@pytest.fixture(scope="module")
def ragged(gpu_lib, oracle, pairs):
    """the 5-pair batch run twice on one runner and one stream; (records of run 1, records of
    run 2, draws per run)"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, RandStream, results_to_numpy
    rs = RandStream(1, 0)
    run = PairBatchRunner(ctx=Context(0), iters=ITERS, stream=rs)
    args = _batch(pairs)
    outs1 = run.run(*args, want=("samples", "hyps"))
    torch.cuda.synchronize()
    total = _check_batch(oracle, pairs, outs1, 0)
    assert total == sum(_draws(p["M"]) for p in pairs) and rs.get() == (1, total)
    outs2 = run.run(*args, want=("samples", "hyps"))
    torch.cuda.synchronize()
    assert _check_batch(oracle, pairs, outs2, total) == total
    assert rs.get() == (1, 2 * total)
    return results_to_numpy(outs1["results"]), results_to_numpy(outs2["results"]), total


def test_ragged_batch_consumes_in_pair_order(ragged, pairs):
    """(the checks are in the fixture) every pair at the offset derived from the returned M's, the
    ineligible pair leaves the next pair's offset unchanged, the second run continues"""
    r1, r2, total = ragged
    assert total > 0 and not _same_records(r1, r2)
    assert r1[2]["M"] < 4 and r1[2]["status"] == 2


def test_batch_equals_sequential_finds(ragged, gpu_lib, pairs):
    from erp_match_eightpoint_test_amd import Context, RandStream
    r1, _, total = ragged
    rs = RandStream(1, 0)
    ctx = Context(0)
    ctx.set_rand_stream(rs)
    for i, p in enumerate(pairs):
        r = _find_dev(ctx, p)
        assert _same_records(np.array([r]), r1[i:i + 1]), (i, r, r1[i])
    assert rs.get() == (1, total)


def _batch_records(pairs, stream, opts=(), ctx=None, torch_stream=None):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    ctx = ctx or Context(0)
    for k, v in opts:
        ctx.set_option(k, v)
    run = PairBatchRunner(ctx=ctx, iters=ITERS, stream=stream)
    outs = run.run(*_batch(pairs), stream=torch_stream)
    torch.cuda.synchronize()
    return results_to_numpy(outs["results"])


@pytest.mark.parametrize("opts", [(("sampler_lat", 0),), (("sampler_lat", 1),),
                                  (("sampler_lat", 2),), (("sampler_split", 0),),
                                  (("sampler_split", 1),),
                                  (("sampler_lat", 0), ("sampler_split", 0), ("sampler_tiers", 1)),
                                  (("sampler_lat", 0), ("sampler_split", 0), ("sampler_tiers", 3))])
def test_sampler_routes_read_the_per_pair_windows(ragged, gpu_lib, pairs, opts):
    """the latency, split and tiered sampler variants all start from sampler_window_kernel's
    windows: identical records on every route"""
    from erp_match_eightpoint_test_amd import RandStream
    r1, _, _ = ragged
    got = _batch_records(pairs, RandStream(1, 0), opts)
    assert got.tobytes() == r1.tobytes()


def test_two_contexts_share_one_stream(gpu_lib, pairs):
    """two contexts on two HIP streams, 3 pairs each, one rand stream: the records equal the
    serial ones in call order"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, RandStream, results_to_numpy
    A, B = [pairs[0], pairs[1], pairs[2]], [pairs[3], pairs[4], pairs[0]]
    rs = RandStream(1, 0)
    serial = [_batch_records(A, rs), _batch_records(B, rs)]
    rs2 = RandStream(1, 0)
    runs = [PairBatchRunner(ctx=Context(0), iters=ITERS, stream=rs2) for _ in range(2)]
    sts = [torch.cuda.Stream(), torch.cuda.Stream()]
    args = [_batch(A), _batch(B)]
    torch.cuda.synchronize()
    outs = [runs[k].run(*args[k], stream=sts[k].cuda_stream) for k in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        assert results_to_numpy(outs[k]["results"]).tobytes() == serial[k].tobytes(), k
    assert rs2.get() == rs.get()


def test_graph_replay_continues_the_stream(gpu_lib, oracle, pairs):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, RandStream, results_to_numpy
    p = pairs[1]
    rs = RandStream(1, 0)
    ctx = Context(0)
    ctx.set_graphs(True)
    run = PairBatchRunner(ctx=ctx, iters=ITERS, reuse_outputs=True, stream=rs)
    args = _batch([p])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    with torch.cuda.stream(st):
        for _ in range(3):  # capture, replay, replay: identical buffers
            o = run.run(*args, stream=st.cuda_stream)
            got.append(o["results"].clone())
        st.synchronize()
    for k in range(3):
        _check_result(results_to_numpy(got[k])[0], _ofind(oracle, p, k * _draws(p["M"])), p["M"])
    assert rs.get() == (1, 3 * _draws(p["M"]))


def test_set_and_advance_after_device_use(gpu_lib, oracle, pairs):
    from erp_match_eightpoint_test_amd import Context, RandStream
    p = pairs[4]
    rs = RandStream(1, 0)
    ctx = Context(0)
    ctx.set_rand_stream(rs)
    _find_dev(ctx, pairs[0])  # first device use: the state lives on the device from here on
    rs.set(1, 2 ** 40 + 12345)
    a = _find_dev(ctx, p)
    assert rs.get() == (1, 2 ** 40 + 12345 + _draws(p["M"]))
    rs.set(1, 2 ** 40)
    rs.advance(12345)
    assert rs.get() == (1, 2 ** 40 + 12345)
    b = _find_dev(ctx, p)
    assert a.tobytes() == b.tobytes() and a["status"] == 0
    # the same place reached on the host by a stream no GPU call has touched
    ctx.set_rand_stream(RandStream(1, 2 ** 40 + 12345))
    assert _find_dev(ctx, p).tobytes() == a.tobytes()
    # a device set, against the oracle's stepped stream
    ctx.set_rand_stream(rs)
    rs.set(1, 3 * 10 ** 8)
    _check_result(_find_dev(ctx, p), _ofind(oracle, p, 3 * 10 ** 8), p["M"])
    ctx.set_rand_stream(None)


def test_other_entry_points(gpu_lib, oracle, pairs):
    import torch
    from erp_match_eightpoint_test_amd import (Context, ErpError, PairBatchRunner, RandStream,
                                               eight_point, epipolar_tool)
    p, q = pairs[0], pairs[1]
    rs = RandStream(1, 0)
    ctx = Context(0)
    ep = eight_point(ctx=ctx, stream=rs, iters=ITERS)
    ep.find(p["W"], p["H"], p["kl"], p["kr"])
    off = _draws(p["M"])
    # epipolar_tool shuffles on the stream where the find left it (epipolar_tool.cpp:15)
    tool = epipolar_tool(q["kl"], q["kr"], q["W"], q["H"], 256, 128, 5, ctx=ctx, stream=rs)
    want = oracle.GlibcRand(1, off).random_array(q["M"])[:5]
    assert np.array_equal(tool.random_idx, want)
    off += q["M"] - 1
    assert rs.get() == (1, off)
    E = np.array([0, -0.3, 0.2, 0.3, 0, -0.9, -0.2, 0.9, 0], np.float64)
    img = tool.draw_epipole(E)  # repeats the constructor's choice, consumes nothing
    ref_tool = epipolar_tool(q["kl"], q["kr"], q["W"], q["H"], 256, 128, 5, seed=1,
                             offset=off - (q["M"] - 1), ctx=Context(0))
    assert torch.equal(img, ref_tool.draw_epipole(E)) and rs.get() == (1, off)
    # erp_epipolar_draw_dev itself on a context with a stream draws from it and advances it
    idx = np.zeros(5, np.int32)
    out = torch.empty((128, 256, 3), dtype=torch.uint8, device="cuda")
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert ctx.L.erp_epipolar_draw_dev(ctx.h, ptr(q["kl"]), ptr(q["kr"]), q["M"], q["W"], q["H"],
                                       256, 128, 5, 99, 424242, ptr(E), out.data_ptr(), ptr(idx),
                                       torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx, oracle.GlibcRand(1, off).random_array(q["M"])[:5])
    off += q["M"] - 1
    # initial_guess consumes like find
    bl = oracle.pixel_to_bearing(p["W"], p["H"], p["kl"])
    br = oracle.pixel_to_bearing(p["W"], p["H"], p["kr"])
    ep.initial_guess(p["W"], p["H"], bl, br)
    g = oracle.initial_guess(bl, br, oracle.make_cfg(iters=ITERS, offset=off))
    _check_result(ep.last_result, g, p["M"])
    off += _draws(p["M"])
    assert rs.get() == (1, off)
    # Philox on a context with a stream: invalid
    ph = eight_point(ctx=ctx, iters=ITERS, sampler=1)
    with pytest.raises(ErpError) as ei:
        ph.find(p["W"], p["H"], p["kl"], p["kr"])
    assert ei.value.status == 1
    with pytest.raises(ErpError) as ei:
        PairBatchRunner(ctx=ctx, iters=ITERS, sampler=1).run(*_batch([p]))
    assert ei.value.status == 1 and rs.get() == (1, off)
    # detached again: today's results, the stream untouched
    ctx.set_rand_stream(None)
    ep.find(p["W"], p["H"], p["kl"], p["kr"])
    _check_result(ep.last_result, _ofind(oracle, p, 0), p["M"])
    assert rs.get() == (1, off)
