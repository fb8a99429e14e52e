"""Host side of the batched rectification (include/erp_match.h "batched rectification"), no
GPU needed: erp_rectify_matrices_results -- the record -> (pose widened to double) -> matrices
step erp_rectify_results_dev goes through -- bit for bit against erp_rectify_matrices and the
oracle's composition (src/automatic.cpp:66-79 with :128-129's Vec3d(Vec3f)), and the argument
checks of the new device entries that need no device."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

N = 1000


@pytest.fixture(scope="module")
def L():
    from erp_match_eightpoint_test_amd import capi
    return capi.load()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _gemm33(a, b):
    """cv::gemm on 3x3 doubles: d[i][j] = (a[i][0] b[0][j] + a[i][1] b[1][j]) + a[i][2] b[2][j]"""
    return (a[:, 0:1] * b[0] + a[:, 1:2] * b[1]) + a[:, 2:3] * b[2]


def _eular2rot_sin_cos(e):
    """oracle/erp_oracle.c erpo_eular2rot (src/erp_rotation.cpp:14-40) with every sin(x) and
    cos(x) its own libm call, as the reference's build makes them (see
    test_rectify_matrices_results)"""
    s, c = [math.sin(x) for x in e], [math.cos(x) for x in e]
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]], np.float64)
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]], np.float64)
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]], np.float64)
    return _gemm33(_gemm33(rx, ry), rz)


@pytest.fixture(scope="module")
def records():
    from erp_match_eightpoint_test_amd.capi import RESULT_DTYPE
    rng = np.random.default_rng(31)
    rec = np.zeros(N, RESULT_DTYPE)
    rec["R"] = rng.uniform(-1.57, 1.57, (N, 3)).astype(np.float32)
    t = rng.standard_normal((N, 3)).astype(np.float32)
    rec["T"] = t / np.linalg.norm(t, axis=1, keepdims=True).astype(np.float32)
    rec["R"][0], rec["T"][0] = 0, (0, -1, 0)      # the identity: both matrices are I
    rec["T"][1] = (0, 1, 0)                       # v1 = -v2: the cross product vanishes
    status = np.zeros(N, np.int32)
    status[rng.choice(np.arange(2, N), 37, replace=False)] = rng.integers(1, 8, 37)
    rec["status"] = status
    rec["M"] = rng.integers(0, 5000, N)           # the other fields play no part
    rec["min_dist"] = rng.standard_normal(N)
    return rec


def test_rectify_matrices_results(L, oracle, records):
    """ok is 0 exactly where the status is not ERP_OK; elsewhere both matrices are bit-identical
    to erp_rectify_matrices on the widened pose and to the oracle's composition
    inv3(inv3(rot_from_vec((0, -1, 0), t))), inv3(inv3(rot_from_vec(..) * inv3(eular2rot(r)))).

    The Euler matrix of that composition is erpo_eular2rot's formula evaluated here with one
    libm call per sin and per cos.  The compiled oracle cannot serve for random angles: gcc -O2
    merges its sin(x) / cos(x) pairs into glibc's sincos(), whose results differ from sin() /
    cos() in the last bit for 0.126 % of float-valued angles in (-1.57, 1.57) (252 of 200 000
    measured), while the reference's CMake build, which sets no optimisation level, and the
    library's host code keep the calls apart.  Where oracle.eular2rot agrees with the separate
    calls -- all but a few records in a thousand -- the composition below IS the compiled
    oracle's, bit for bit; the number of records where it does not is printed and bounded
    (expected 3 * 0.126 % of the records, i.e. 3 or 4 here; 2 % would mean the explanation is
    wrong)."""
    ml, mr = np.full((N, 9), np.nan), np.full((N, 9), np.nan)
    ok = np.full(N, -1, np.int32)
    assert L.erp_rectify_matrices_results(_p(records), N, _p(ml), _p(mr), _p(ok)) == 0
    assert np.array_equal(ok, (records["status"] == 0).astype(np.int32))
    assert 0 < (ok == 0).sum() < N // 10
    a, b = np.zeros(9), np.zeros(9)
    merged = 0
    for p in np.flatnonzero(ok):
        rv = records["R"][p].astype(np.float64)   # Vec3d(Vec3f)
        tv = records["T"][p].astype(np.float64)
        assert L.erp_rectify_matrices(_p(rv), _p(tv), _p(a), _p(b)) == 0
        assert ml[p].tobytes() == a.tobytes() and mr[p].tobytes() == b.tobytes(), p
        E = _eular2rot_sin_cos(rv)
        merged += E.tobytes() != oracle.eular2rot(rv).tobytes()
        Rl = oracle.rot_from_vec([0.0, -1.0, 0.0], tv)
        Rr = _gemm33(Rl, oracle.inv3(E))
        assert ml[p].tobytes() == oracle.inv3(oracle.inv3(Rl)).tobytes(), p
        assert mr[p].tobytes() == oracle.inv3(oracle.inv3(Rr)).tobytes(), p
    print(f"records whose compiled-oracle Euler matrix differs (sincos merge): {merged} of "
          f"{int(ok.sum())}")
    assert merged <= N // 50
    eye = np.eye(3).reshape(9)
    assert np.array_equal(ml[0], eye) and np.array_equal(mr[0], eye)
    assert np.array_equal(ml[1], eye)
    # n = 0 needs no arrays; a negative n and missing arrays are rejected
    assert L.erp_rectify_matrices_results(None, 0, None, None, None) == 0
    assert L.erp_rectify_matrices_results(_p(records), -1, _p(ml), _p(mr), _p(ok)) == 1
    assert L.erp_rectify_matrices_results(_p(records), 1, None, _p(mr), _p(ok)) == 1


def test_new_device_entries_reject_null_context_and_negative_counts(L):
    """before any device is touched: a NULL context, then (with a pointer that is never
    dereferenced standing in for the context) n / n_pairs < 0"""
    from erp_match_eightpoint_test_amd import capi
    o = capi.RectifyOutputs()
    z = np.zeros(3)
    fake = C.c_void_p(8)
    for ctx, n in ((None, 1), (fake, -1)):
        assert L.erp_vertical_rotate_batch_dev(ctx, None, n, 200, 100, 0, None, None) == 1
        assert L.erp_rectify_batch_dev(ctx, None, None, n, 200, 100, _p(z), _p(z), None, 0,
                                       C.byref(o), None) == 1
        assert L.erp_rectify_results_dev(ctx, None, None, n, 200, 100, None, 0, C.byref(o),
                                         None) == 1
    # a fill outside -1 .. 255 and impossible dimensions are argument errors too
    assert L.erp_vertical_rotate_batch_dev(fake, None, 0, 200, 100, 256, None, None) == 1
    assert L.erp_vertical_rotate_batch_dev(fake, None, 0, 0, 100, 0, None, None) == 1
