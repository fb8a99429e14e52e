"""Winner records without a GPU (include/erp_match.h "winner records"): the record's layout, the
argument checks that come before any use of the context, the exported symbols, and the Python
wrappers' choice between hypothesis records and winner records."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

NAMES = {"erp_pair_batch_run_winners", "erp_eight_point_find_winner_dev",
         "erp_eight_point_find_winner", "erp_polish_winners_dev"}


@pytest.fixture(scope="module")
def lib():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    return capi.load()


def test_record_layout():
    from erp_match_eightpoint_test_amd import capi
    assert C.sizeof(capi.Winner) == capi.WINNER_DTYPE.itemsize == 88
    for name, _ in capi.Winner._fields_:
        assert getattr(capi.Winner, name).offset == capi.WINNER_DTYPE.fields[name][1], name
    assert capi.Winner.E.offset == 16 and capi.WINNER_DTYPE["E"].shape == (9,)
    # additive: the ABI version and the existing records keep their sizes
    assert C.sizeof(capi.Hypothesis) == 120 and C.sizeof(capi.PairResult) == 64
    assert C.sizeof(capi.PolishInputs) == 64 and C.sizeof(capi.BatchOutputs) == 72


def test_symbols_are_exported(lib):
    from erp_match_eightpoint_test_amd import capi
    assert NAMES <= set(capi.EXPORTED)
    for n in NAMES:
        assert getattr(lib, n) is not None
    assert lib.erp_abi_version() == 2


def _batch_args():
    from erp_match_eightpoint_test_amd import capi
    b = capi.PairBatch(1, 64, 16, 16, 8, 8, 8, 8, 8, 8, 8, 8)  # (never dereferenced)
    o = capi.BatchOutputs(8, None, None, None, None, None, None, None, None)
    cfg = capi.RansacCfg()
    capi.load().erp_ransac_cfg_default(C.byref(cfg))
    return b, o, cfg


def test_batch_run_winners_rejects_bad_arguments_without_a_device(lib):
    b, o, cfg = _batch_args()
    f = lib.erp_pair_batch_run_winners
    fake, w = C.c_void_p(8), C.c_void_p(8)
    assert f(fake, C.byref(b), 0.3, C.byref(cfg), C.byref(o), None, None) == 1  # NULL winners
    assert f(None, C.byref(b), 0.3, C.byref(cfg), C.byref(o), w, None) == 1     # NULL context
    assert f(fake, C.byref(b), 0.3, None, C.byref(o), w, None) == 1
    for field, v in (("iters", 0), ("sampler", 2), ("sample_frac", 0.0), ("trim_lo", 0.9)):
        _, _, bad = _batch_args()
        setattr(bad, field, v)
        assert f(fake, C.byref(b), 0.3, C.byref(bad), C.byref(o), w, None) == 1, field
    assert f(fake, None, 0.3, C.byref(cfg), C.byref(o), w, None) == 1
    assert f(fake, C.byref(b), 0.3, C.byref(cfg), None, w, None) == 1


def test_find_winner_rejects_bad_arguments_without_a_device(lib):
    _, _, cfg = _batch_args()
    fake, p = C.c_void_p(8), C.c_void_p(8)
    bad = type(cfg).from_buffer_copy(cfg)
    bad.iters = 0
    d, h = lib.erp_eight_point_find_winner_dev, lib.erp_eight_point_find_winner
    assert d(fake, 64, 32, p, p, 10, C.byref(cfg), p, None, None, None) == 1  # NULL winner
    assert d(None, 64, 32, p, p, 10, C.byref(cfg), p, None, p, None) == 1     # NULL context
    assert d(fake, 64, 32, p, p, 10, C.byref(bad), p, None, p, None) == 1     # bad cfg
    assert d(fake, 64, 32, p, p, 10, None, p, None, p, None) == 1
    assert d(fake, 64, 32, p, p, 70000, C.byref(cfg), p, None, p, None) == 1
    assert d(fake, 64, 32, p, p, 10, C.byref(cfg), None, None, p, None) == 1  # NULL result
    assert h(fake, 64, 32, p, p, 10, C.byref(cfg), None, None, None, None) == 1
    assert h(None, 64, 32, p, p, 10, C.byref(cfg), None, None, None, p) == 1
    assert h(fake, 64, 32, p, p, 10, C.byref(bad), None, None, None, p) == 1
    assert h(fake, 64, 32, p, p, 10, None, None, None, None, p) == 1


def test_polish_winners_rejects_bad_arguments_without_a_device(lib):
    from erp_match_eightpoint_test_amd import capi
    f = lib.erp_polish_winners_dev
    fake, p = C.c_void_p(8), C.c_void_p(8)
    # hyps NULL and iters 0: neither is read on this entry point
    inp = capi.PolishInputs(1, 0, 16, 8, 8, 8, 8, 8, None)
    assert f(None, C.byref(inp), p, 1.57, 0.01, 3, p, None, None, None) == 1
    assert f(fake, C.byref(inp), None, 1.57, 0.01, 3, p, None, None, None) == 1  # NULL winners
    assert f(fake, C.byref(inp), p, 1.57, 0.01, 3, None, None, None, None) == 1
    for thr, rounds in ((0.0, 3), (float("nan"), 3), (0.01, -1), (0.01, 9)):
        assert f(fake, C.byref(inp), p, 1.57, thr, rounds, p, None, None, None) == 1
    for k in ("results", "width", "height", "key_left", "key_right"):
        i2 = capi.PolishInputs(1, 0, 16, 8, 8, 8, 8, 8, None)
        setattr(i2, k, None)
        assert f(fake, C.byref(i2), p, 1.57, 0.01, 3, p, None, None, None) == 1, k
    i0 = capi.PolishInputs(0, 0, 16, None, None, None, None, None, None)
    assert f(fake, C.byref(i0), None, 1.57, 0.01, 3, None, None, None, None) == 0  # no pairs
    # erp_polish_dev still needs its records
    assert lib.erp_polish_dev(fake, C.byref(inp), 1.57, 0.01, 3, p, None, None, None) == 1


class _RecCtx:
    """stands in for a Context: records what the runner hands to Context.polish"""
    def polish(self, results, hyps, *a, **k):
        self.got = (results, hyps, k.get("winners"))
        return {}


def _runner():
    from erp_match_eightpoint_test_amd import PairBatchRunner, capi
    run = PairBatchRunner.__new__(PairBatchRunner)  # (no device)
    run.ctx = _RecCtx()
    run.cfg = capi.RansacCfg(valid_abs=1.57)
    return run


def test_runner_polish_prefers_hyps_when_both_are_present():
    run = _runner()
    out = {"results": "r", "hyps": "h", "winners": "w", "key_left": "kl", "key_right": "kr"}
    run.polish(out, None, None, 0.01)
    assert run.ctx.got == ("r", "h", None)
    del out["hyps"]
    run.polish(out, None, None, 0.01)
    assert run.ctx.got == ("r", None, "w")
    del out["winners"]
    with pytest.raises(ValueError, match="polish needs"):
        run.polish(out, None, None, 0.01)


def test_context_polish_checks_the_winner_tensor():
    from erp_match_eightpoint_test_amd import Context
    ctx = Context.__new__(Context)
    a = np.zeros((1, 64), np.uint8)
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):
        ctx.polish(a, None, a, a, a, a, 0.01, winners=a)
    with pytest.raises(ValueError, match="contiguous CUDA tensors"):
        ctx.polish(a, None, a, a, a, a, 0.01)  # neither records nor winners


def test_winners_to_numpy_views_the_records():
    import torch
    from erp_match_eightpoint_test_amd import WINNER_DTYPE, winners_to_numpy
    rec = np.zeros(3, WINNER_DTYPE)
    rec["iter"] = [5, 6, 7]
    rec["E"][1] = np.arange(9)
    t = torch.from_numpy(rec.view(np.uint8).reshape(3, 88).copy())
    got = winners_to_numpy(t)
    assert got.shape == (3,) and got.tobytes() == rec.tobytes()
