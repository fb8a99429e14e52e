"""The host side of the rotation sweep (no GPU): sweep_relative_rotation against the oracle's
3x3 geometry, and the ctypes signatures of the three sweep entry points."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    return capi.load()


def test_sweep_relative_rotation_against_oracle(lib, oracle):
    """two_real_image_test/main.cpp:215-219: rot2eular(eular2rot((double)R) * initial.inv())"""
    from erp_match_eightpoint_test_amd import RESULT_DTYPE, sweep_relative_rotation
    rng = np.random.default_rng(5)
    R = rng.uniform(-0.6, 0.6, (5, 3)).astype(np.float32)
    initial = oracle.eular2rot(rng.uniform(-0.4, 0.4, 3))
    inv = oracle.inv3(initial)
    want = np.stack([oracle.rot2eular(oracle.eular2rot(r.astype(np.float64)) @ inv) for r in R])
    got = sweep_relative_rotation(R, initial)
    assert got.shape == (5, 3) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12
    recs = np.zeros(5, RESULT_DTYPE)
    recs["R"] = R
    assert sweep_relative_rotation(recs, initial).tobytes() == got.tobytes()
    # the identity start gives the estimate back (to rot2eular(eular2rot(.))'s rounding)
    assert np.abs(sweep_relative_rotation(R, np.eye(3)) - R).max() <= 1e-12
    from erp_match_eightpoint_test_amd import ErpError
    with pytest.raises(ErpError):
        sweep_relative_rotation(R, np.zeros((3, 3)))


class _NoCalls:
    """stands in for the library: any entry point looked up is a test failure"""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the inputs were checked")


class _StubCtx:
    L = _NoCalls()
    h = None
    device = 0
    rand_stream = None


def test_wrappers_reject_host_inputs_before_any_call():
    import torch
    from erp_match_eightpoint_test_amd import PairBatchRunner, erp_rotation, spherical_surf
    ss, er = spherical_surf(ctx=_StubCtx()), erp_rotation(ctx=_StubCtx())
    run = PairBatchRunner.__new__(PairBatchRunner)
    run.ctx = _StubCtx()
    im = torch.zeros((8, 16, 3), dtype=torch.uint8)            # a host tensor: not CUDA
    mats = np.stack([np.eye(3)] * 3)
    for a, b, m in [(im, im, mats), (im.numpy(), im, mats), (im[None], im[None], mats)]:
        with pytest.raises(ValueError):
            ss.do_all_sweep(a, b, m)
        with pytest.raises(ValueError):
            run.run_sweep(a, b, m)
    keys = torch.zeros((3, 4, 2))
    with pytest.raises(ValueError):
        er.match_error(keys, keys, torch.zeros(3, dtype=torch.int32), mats, 16, 8)
    with pytest.raises(ValueError):
        er.match_error(keys, keys, torch.zeros(3, dtype=torch.int32), mats[:, :2], 16, 8)


def test_sweep_entry_points_reject_null_context(lib):
    from erp_match_eightpoint_test_amd import capi
    prm, pk, info = capi.SurfParams(), capi.PackedPairs(), capi.ImageBatchInfo()
    lib.erp_surf_params_default(C.byref(prm))
    cfg, out = capi.default_cfg(), capi.BatchOutputs()
    m = np.eye(3).reshape(1, 9).copy()
    assert lib.erp_image_sweep_features_dev(None, None, None, 1, m.ctypes.data, 672, 336,
                                            C.byref(prm), 512, 0, 0, C.byref(pk), C.byref(info),
                                            None) == 1
    assert lib.erp_image_sweep_run(None, None, None, 1, m.ctypes.data, 672, 336, C.byref(prm),
                                   512, 0, 0, C.byref(pk), 0.3, C.byref(cfg), C.byref(out), None,
                                   C.byref(info), None) == 1
    assert lib.erp_match_error_dev(None, None, None, 1024, None, 1, 1, m.ctypes.data, 672, 336,
                                   None, None) == 1
