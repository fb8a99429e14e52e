"""The rand stream on the host (no GPU): a stream that no GPU call has used yet lives in host
memory, positioned by the polynomial jump-ahead x^n mod (x^31 - x^28 - 1) over Z/2^32.  Checked
against the oracle's glibc rand() restatement (sequential recurrence, pinned to the real libc
by tests/test_oracle.py)."""
from __future__ import annotations

import ctypes as C
import os
import re
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["erp_rand_stream_create", "erp_rand_stream_destroy", "erp_rand_stream_get",
               "erp_rand_stream_set", "erp_rand_stream_advance", "erp_rand_stream_process",
               "erp_ctx_set_rand_stream", "erp_ctx_get_rand_stream",
               "erp_rand_stream_shuffle_prefix"]


@pytest.fixture(scope="module")
def capi():
    from erp_match_eightpoint_test_amd import _build, capi
    _build.build()
    capi.load()
    return capi


def test_creation_and_counter(capi, oracle):
    """successive shuffles continue the stream: each equals the oracle's random_array at the
    draws consumed so far, and consumes m - 1 (0 for m < 2)"""
    s = capi.RandStream(1, 0)
    assert s.get() == (1, 0)
    off = 0
    for m, n in [(300, 7), (2, 2), (1, 1), (4000, 64)]:
        got = s.shuffle_prefix(m, n)
        assert np.array_equal(got, oracle.GlibcRand(1, off).random_array(m)[:n]), (m, off)
        off += m - 1 if m >= 2 else 0
        assert s.get() == (1, off)
    s.close()


@pytest.mark.parametrize("a,b", [(0, 0), (1, 30), (31, 344), (12345, 10 ** 9),
                                 (2 ** 48 + 977, 2 ** 47 + 13)])
def test_advance_advance_equals_set(capi, a, b):
    s1 = capi.RandStream(1, 0)
    s1.advance(a)
    s1.advance(b)
    s2 = capi.RandStream(7, 5)
    s2.set(1, a + b)
    assert s1.get() == s2.get() == (1, a + b)
    assert np.array_equal(s1.shuffle_prefix(64, 64), s2.shuffle_prefix(64, 64))
    s4 = capi.RandStream(1, a)  # created at a, advanced by b: the same place again
    s4.advance(b)
    assert np.array_equal(capi.RandStream(1, a + b).shuffle_prefix(64, 64),
                          s4.shuffle_prefix(64, 64))


def test_counter_wraps(capi):
    """the counter wraps mod 2^64; the window is the one 2^64 + 5 draws on, not the one at 5"""
    s = capi.RandStream(1, 2 ** 64 - 10)
    s.advance(15)
    assert s.get() == (1, 5)
    a = capi.RandStream(1, 2 ** 63)
    a.advance(2 ** 63)
    a.advance(5)
    assert np.array_equal(s.shuffle_prefix(64, 64), a.shuffle_prefix(64, 64))


@pytest.mark.parametrize("offset", [0, 1, 30, 31, 343, 344, 4096, 4097, 10 ** 6])
def test_jump_ahead_equals_sequential_recurrence(capi, oracle, offset):
    """a stream set to `offset` (jump-ahead) and erp_random_shuffle_prefix at a cfg-style offset
    (sequential below 4096, jump-ahead above) draw what the oracle's stepped stream draws"""
    L = capi.load()
    want = oracle.GlibcRand(1, offset).random_array(64)
    assert np.array_equal(capi.RandStream(1, offset).shuffle_prefix(64, 64), want)
    s = capi.RandStream(1, 0)
    s.advance(offset)  # always the polynomial, whatever the size
    assert np.array_equal(s.shuffle_prefix(64, 64), want)
    out = np.zeros(64, np.int32)
    assert L.erp_random_shuffle_prefix(1, offset, 64, 64, out.ctypes.data) == 0
    assert np.array_equal(out, want)
    # another seed takes the same path
    assert np.array_equal(capi.RandStream(12345, offset).shuffle_prefix(9, 9),
                          oracle.GlibcRand(12345, offset).random_array(9))


def test_jump_ahead_large_offset_is_fast(capi, oracle):
    """3e8 draws: the oracle steps them (a second or two), the library jumps in microseconds"""
    L = capi.load()
    offset = 3 * 10 ** 8
    t0 = time.perf_counter()
    want = oracle.GlibcRand(1, offset).random_array(64)
    t_oracle = time.perf_counter() - t0
    out = np.zeros(64, np.int32)
    t0 = time.perf_counter()
    assert L.erp_random_shuffle_prefix(1, offset, 64, 64, out.ctypes.data) == 0
    t_lib = time.perf_counter() - t0
    print(f"offset {offset}: oracle discard {t_oracle:.3f} s, library {t_lib * 1e6:.0f} us")
    assert np.array_equal(out, want)
    assert np.array_equal(capi.RandStream(1, offset).shuffle_prefix(64, 64), want)
    assert t_lib < 0.05  # ~130 products of 31 x 31 words; the stepped loop took ~1 s here


def test_process_stream_is_shared_and_undestroyable(capi):
    L = capi.load()
    a = capi.process_rand_stream(3)
    b = capi.process_rand_stream(3)
    assert a.h.value == b.h.value and a.h.value != capi.process_rand_stream(4).h.value
    assert a.get() == (1, 0)
    assert L.erp_rand_stream_destroy(a.h) == capi.ERP_INVALID_ARG
    a.advance(11)
    assert b.get() == (1, 11)
    b.set(1, 0)


def test_argument_checks(capi):
    L = capi.load()
    assert L.erp_rand_stream_create(1, 0, None) == capi.ERP_INVALID_ARG
    assert L.erp_rand_stream_get(None, None, None) == capi.ERP_INVALID_ARG
    assert L.erp_rand_stream_set(None, 1, 0) == capi.ERP_INVALID_ARG
    assert L.erp_rand_stream_advance(None, 1) == capi.ERP_INVALID_ARG
    assert L.erp_rand_stream_destroy(None) == capi.ERP_INVALID_ARG
    assert L.erp_ctx_set_rand_stream(None, None) == capi.ERP_INVALID_ARG
    assert L.erp_ctx_get_rand_stream(None, None) == capi.ERP_INVALID_ARG
    s = capi.RandStream(0, 0)  # seed 0 = 1, as srand
    assert s.get() == (1, 0)
    out = np.zeros(4, np.int32)
    assert L.erp_rand_stream_shuffle_prefix(s.h, 3, 4, out.ctypes.data) == capi.ERP_INVALID_ARG
    assert L.erp_rand_stream_shuffle_prefix(s.h, 0, 0, out.ctypes.data) == capi.ERP_INVALID_ARG
    assert s.get() == (1, 0)


def test_plumbing(capi):
    """the new symbols are declared and exported; the cfg and the ABI version are untouched"""
    L = capi.load()
    src = open(os.path.join(ROOT, "include", "erp_match.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.EXPORTED and hasattr(L, name), name
    assert L.erp_abi_version() == 2 and "#define ERP_MATCH_ABI_VERSION 2" in src
    assert "ERP_STAGE_COUNT = 19" in src
    cfg = capi.RansacCfg()
    L.erp_ransac_cfg_default(C.byref(cfg))
    assert C.sizeof(cfg) == 56
    assert (cfg.iters, cfg.sampler, cfg.sample_frac, cfg.trim_lo, cfg.trim_hi, cfg.valid_abs,
            cfg.seed, cfg.inlier_thr, cfg.offset) == (80, 0, 0.25, 0.2, 0.8, 1.57, 1, 0.0, 0)
    from erp_match_eightpoint_test_amd import _build
    out = os.popen(f"nm -DC {_build.LIB_PATH}").read()
    for sym in ["erp::rand_stream::process", "erp::rand_stream::advance",
                "erp::eight_point::use_stream"]:
        assert sym in out, sym
