"""Batched do_all, the parts that need no GPU: the three new C entry points reject NULL
arguments before touching anything, and the Python wrappers reject malformed inputs before any
library call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    return capi.load()


def _structs():
    from erp_match_eightpoint_test_amd import capi
    prm = capi.SurfParams()
    cfg = capi.RansacCfg()
    return prm, cfg, capi.PackedPairs(), capi.BatchOutputs(), capi.ImageBatchInfo()


def test_null_context_rejected(lib):
    from erp_match_eightpoint_test_amd import capi
    prm, cfg, pk, bo, info = _structs()
    lib.erp_surf_params_default(C.byref(prm))
    lib.erp_ransac_cfg_default(C.byref(cfg))
    assert lib.erp_pack_band_features_dev(None, None, None, None, 0, 16, 672, 336, C.byref(pk),
                                          None) == capi.ERP_INVALID_ARG
    assert lib.erp_image_pairs_features_dev(None, None, None, 0, 672, 336, C.byref(prm), 16, 0, 0,
                                            C.byref(pk), C.byref(info),
                                            None) == capi.ERP_INVALID_ARG
    assert lib.erp_image_pairs_run(None, None, None, 0, 672, 336, C.byref(prm), 16, 0, 0,
                                   C.byref(pk), 0.3, C.byref(cfg), C.byref(bo), C.byref(info),
                                   None) == capi.ERP_INVALID_ARG


def test_null_info_rejected(lib):
    """info is checked together with the context, before the context is looked at: a dummy
    non-NULL context pointer is enough here"""
    from erp_match_eightpoint_test_amd import capi
    prm, cfg, pk, bo, _ = _structs()
    lib.erp_surf_params_default(C.byref(prm))
    lib.erp_ransac_cfg_default(C.byref(cfg))
    dummy = C.create_string_buffer(64)
    res = C.create_string_buffer(64)
    bo.results = C.addressof(res)
    ctx = C.c_void_p(C.addressof(dummy))
    assert lib.erp_image_pairs_features_dev(ctx, None, None, 0, 672, 336, C.byref(prm), 16, 0, 0,
                                            C.byref(pk), None, None) == capi.ERP_INVALID_ARG
    assert lib.erp_image_pairs_run(ctx, None, None, 0, 672, 336, C.byref(prm), 16, 0, 0,
                                   C.byref(pk), 0.3, C.byref(cfg), C.byref(bo), None,
                                   None) == capi.ERP_INVALID_ARG


def test_struct_layouts_match_header():
    """erp_packed_pairs / erp_image_batch_info as the header lays them out (LP64)"""
    from erp_match_eightpoint_test_amd import capi
    assert C.sizeof(capi.PackedPairs) == 9 * 8 + 2 * 8
    assert capi.PackedPairs.cap_l.offset == 72 and capi.PackedPairs.cap_r.offset == 80
    assert C.sizeof(capi.ImageBatchInfo) == 6 * 4 + 2 * 8
    assert capi.ImageBatchInfo.fits.offset == 16 and capi.ImageBatchInfo.rows_l.offset == 24


class _NoCalls:
    """stands in for the library: any entry point looked up is a test failure"""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the inputs were checked")


class _StubCtx:
    L = _NoCalls()
    h = None
    device = 0


def test_wrappers_reject_bad_inputs_before_any_call():
    import torch
    from erp_match_eightpoint_test_amd import PairBatchRunner, spherical_surf
    ss = spherical_surf(ctx=_StubCtx())
    run = PairBatchRunner.__new__(PairBatchRunner)
    run.ctx = _StubCtx()
    good = torch.zeros((2, 8, 16, 3), dtype=torch.uint8)  # a host tensor: not CUDA
    bad = [(good, good),                                             # not on the device
           (good.float(), good.float()),                             # not uint8
           (good[:, :, ::2], good[:, :, ::2]),                       # not contiguous
           (good, good[:1]),                                         # shapes differ
           (good[0], good[0]),                                       # not a batch
           (np.zeros((2, 8, 16, 3), np.uint8), good)]                # not a tensor
    for lefts, rights in bad:
        with pytest.raises(ValueError):
            ss.do_all_batch(lefts, rights)
        with pytest.raises(ValueError):
            run.run_images(lefts, rights)
    kp = torch.zeros((8, 16, 28), dtype=torch.uint8)
    desc = torch.zeros((8, 16, 64), dtype=torch.float32)
    for k, d in [(kp, desc), (kp[:7], desc[:7]), (kp, desc[:, :8]), (kp.float(), desc)]:
        with pytest.raises(ValueError):
            ss.pack_band_features(k, d, np.zeros(8, np.int32), 672, 336)
