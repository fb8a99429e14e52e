"""The polish stage without a GPU (include/erp_match.h "polish"): the properties of the reference
chain (tests/polish_ref.py) that the GPU test's expectations stand on, the argument checks of
erp_polish_dev / erp_eight_point_find_polished, and the Python wrappers' input checks."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polish_ref as PR  # noqa: E402

# what the issue's table states per case: (M, winner_iter, the inlier counts |S_0|, |S_1|, ..)
EXPECT = {(1, 256, 0.2, 0.01): (197, 60, [16, 155, 155]),
          (2, 256, 0.2, 0.01): (196, 37, None),
          (3, 256, 0.2, 0.01): (193, 18, [42, 82, 125, 158]),
          (23, 128, 0.1, 0.01): (99, None, None),
          (13, 1024, 0.3, 0.005): (733, None, None),
          (11, 64, 0.3, 0.01): (51, None, [5]),
          (12, 48, 0.3, 0.02): (38, None, [6]),
          (12, 48, 0.0, 0.01): (None, None, [38, 38]),
          (5, 300, 0.0, 0.002): (None, None, [230, 230])}


@pytest.mark.parametrize("c", PR.CASES)
def test_chain_properties(oracle, c):
    k = PR.case(oracle, c)
    o = k["find"]
    assert o["status"] == 0
    ch = k["chain"]
    counts = [int(s.sum()) for s in ch["sets"]]
    print(f"{c}: M={k['M']} winner=({k['winner_iter']}, {k['winner_which']}) inliers={counts} "
          f"which={[r['which'] for r in ch['rounds']]} near={ch['near']}")
    # the condition under which the chain is unambiguous: no match within 1e-9 of the threshold
    assert ch["near"] == 0
    assert all(b >= a for a, b in zip(counts, counts[1:]))
    # |S_0| is the count the find itself gives the winner's record at inlier_thr = thr
    assert counts[0] == o["hyp"]["inliers"][k["winner_iter"]]
    assert len(ch["rounds"]) == len(counts) - 1 <= PR.ROUNDS
    for r, rd in enumerate(ch["rounds"]):
        assert rd["n_fit"] == counts[r] >= PR.MIN_FIT and rd["n_inliers"] == counts[r + 1]
    M, win, want = EXPECT[c]
    assert M is None or k["M"] == M
    assert win is None or k["winner_iter"] == win
    # (a fixed point shows as one more accepted round that repeats the count)
    assert want is None or counts == want


def test_case_2_takes_r2_in_round_2(oracle):
    ch = PR.case(oracle, PR.CASES[1])["chain"]
    counts = [int(s.sum()) for s in ch["sets"]]
    assert counts[0] == 50 and counts[-1] == 160
    assert ch["rounds"][1]["which"] == 1


@pytest.mark.parametrize("c", [PR.CASES[0], PR.CASES[1], PR.CASES[3]])
def test_chain_beats_the_winner_tenfold(oracle, c):
    """the chain's final error is below one tenth of the winner's (measured 1/141, 1/122 and
    1/100: the bar leaves a factor of ~10)"""
    k = PR.case(oracle, c)
    before = PR.euler_err(k["find"]["R"], k["pair"])
    after = PR.euler_err(k["chain"]["R"], k["pair"])
    print(f"{c}: {before:.5f} -> {after:.5f} rad (1/{before / after:.0f})")
    assert after < before / 10


@pytest.mark.parametrize("c", [PR.CASES[5], PR.CASES[6]])
def test_fewer_than_nine_inliers_stop_the_chain(oracle, c):
    ch = PR.case(oracle, c)["chain"]
    assert len(ch["rounds"]) == 0 and int(ch["sets"][0].sum()) < PR.MIN_FIT


@pytest.fixture(scope="module")
def lib():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    return capi.load()


def test_polish_dev_rejects_bad_arguments_without_a_device(lib):
    from erp_match_eightpoint_test_amd import capi
    inp = capi.PolishInputs(1, 80, 16, 8, 8, 8, 8, 8, 8)  # (never dereferenced)
    bad = C.c_void_p(8)
    assert lib.erp_polish_dev(None, C.byref(inp), 1.57, 0.01, 3, bad, None, None, None) == 1
    # a context is checked first, so the argument checks are exercised through a fake handle only
    # as far as they come before any use of it: thr, rounds, iters, key_stride
    fake = C.c_void_p(8)
    assert lib.erp_polish_dev(fake, None, 1.57, 0.01, 3, bad, None, None, None) == 1
    for thr, rounds in ((0.0, 3), (-1.0, 3), (float("nan"), 3), (0.01, -1), (0.01, 9)):
        assert lib.erp_polish_dev(fake, C.byref(inp), 1.57, thr, rounds, bad, None, None,
                                  None) == 1, (thr, rounds)
    for field, v in (("iters", 0), ("key_stride", -1), ("n_pairs", -1)):
        i2 = capi.PolishInputs(1, 80, 16, 8, 8, 8, 8, 8, 8)
        setattr(i2, field, v)
        assert lib.erp_polish_dev(fake, C.byref(i2), 1.57, 0.01, 3, bad, None, None, None) == 1, field
    # n_pairs == 0: ERP_OK, nothing is touched
    i0 = capi.PolishInputs(0, 80, 16, None, None, None, None, None, None)
    assert lib.erp_polish_dev(fake, C.byref(i0), 1.57, 0.01, 3, None, None, None, None) == 0
    # missing pointers
    for k in ("results", "hyps", "width", "height", "key_left", "key_right"):
        i3 = capi.PolishInputs(1, 80, 16, 8, 8, 8, 8, 8, 8)
        setattr(i3, k, None)
        assert lib.erp_polish_dev(fake, C.byref(i3), 1.57, 0.01, 3, bad, None, None, None) == 1, k
    assert lib.erp_polish_dev(fake, C.byref(inp), 1.57, 0.01, 3, None, None, None, None) == 1


def test_find_polished_rejects_bad_arguments_without_a_device(lib):
    from erp_match_eightpoint_test_amd import capi
    cfg = capi.RansacCfg()
    lib.erp_ransac_cfg_default(C.byref(cfg))
    fake, kp = C.c_void_p(8), C.c_void_p(8)
    f = lib.erp_eight_point_find_polished
    assert f(None, 64, 32, kp, kp, 10, C.byref(cfg), 0.01, 3, None, None, None) == 1
    assert f(fake, 64, 32, kp, kp, 10, None, 0.01, 3, None, None, None) == 1
    assert f(fake, 64, 32, kp, kp, -1, C.byref(cfg), 0.01, 3, None, None, None) == 1
    assert f(fake, 64, 32, None, kp, 10, C.byref(cfg), 0.01, 3, None, None, None) == 1
    assert f(fake, 64, 32, kp, kp, 10, C.byref(cfg), 0.0, 3, None, None, None) == 1
    assert f(fake, 64, 32, kp, kp, 10, C.byref(cfg), 0.01, 9, None, None, None) == 1
    assert f(fake, 64, 32, kp, kp, 70000, C.byref(cfg), 0.01, 3, None, None, None) == 1


def test_structs_match_the_header():
    from erp_match_eightpoint_test_amd import capi
    assert C.sizeof(capi.PolishRound) == capi.POLISH_ROUND_DTYPE.itemsize == 112
    assert C.sizeof(capi.PolishResult) == capi.POLISH_DTYPE.itemsize == 120
    assert C.sizeof(capi.PolishInputs) == 64
    for st, dt in ((capi.PolishRound, capi.POLISH_ROUND_DTYPE), (capi.PolishResult, capi.POLISH_DTYPE)):
        for name, _ in st._fields_:
            assert getattr(st, name).offset == dt.fields[name][1], name
    assert {"erp_polish_dev", "erp_eight_point_find_polished"} <= set(capi.EXPORTED)


class _NoCtx:
    """stands in for a Context where the wrapper must fail before it reaches the library"""
    def polish(self, *a, **k):
        raise AssertionError("reached the library")


def test_runner_polish_rejects_missing_outputs():
    from erp_match_eightpoint_test_amd import PairBatchRunner
    run = PairBatchRunner.__new__(PairBatchRunner)  # (no device: the check comes first)
    run.ctx = _NoCtx()
    for have in ((), ("results",), ("results", "hyps"), ("results", "hyps", "key_left"),
                 ("results", "key_left", "key_right")):
        with pytest.raises(ValueError, match="polish needs"):
            run.polish({k: None for k in have}, None, None, 0.01)


def test_context_polish_rejects_host_arrays():
    from erp_match_eightpoint_test_amd import Context
    ctx = Context.__new__(Context)
    a = np.zeros((1, 64), np.uint8)
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):
        ctx.polish(a, a, a, a, a, a, 0.01)
