"""Batched rectification on the GPU (include/erp_match.h "batched rectification"): the stacks
erp_vertical_rotate_batch_dev / erp_rectify_batch_dev / erp_rectify_results_dev write against
the per-pair calls (erp_rectify_dev, erp_vertical_rotate_dev), byte for byte, and the rectified
stacks against the oracle under test_gpu_remap's certification rule.

Shapes (H, W) = (100, 200) and (272, 300): neither dimension is a multiple of the 16-row /
256-column block; the second makes the ROT90 output (300 rows x 272 columns) cross a column
block with a tail and breaks W = 2 H.  Outputs start from a sentinel on both sides, so pixels
left unwritten compare too.  The per-image references are computed once per module."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from test_gpu_remap import _certify, _dev, _image

pytestmark = pytest.mark.gpu

SHAPES = [(100, 200), (272, 300)]
SENT = 201
# five generic poses (Vec3f values widened, as automatic.cpp:128-129 hands them to rectify); the
# first is test_gpu_remap.test_rectify_and_vertical's
RV = np.array([[0.05, -0.12, 0.03], [-0.4, 0.25, 0.7], [1.1, -0.9, 0.2], [0.0, 0.6, -1.3],
               [-0.02, 0.01, 0.015]], np.float32).astype(np.float64)
TV = np.array([[0.6, 0.1, -0.79], [0.0, -0.8, 0.6], [-0.57735, 0.57735, 0.57735],
               [0.28, 0.0, 0.96], [0.1, -0.99, 0.1]], np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def er(gpu_lib):
    from erp_match_eightpoint_test_amd import Context, erp_rotation
    return erp_rotation(ctx=Context(0))


def _stack(seed, n, H, W):
    return np.stack([_image(seed + k, H, W) for k in range(n)])


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy() if hasattr(b, "cpu") else b
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def pairs(er):
    """per shape: 5 left / right images on the device and the per-pair route's four outputs for
    the generic poses (rectify + vertical_rotate per image), fill = SENT"""
    import torch
    out = {}
    for H, W in SHAPES:
        lefts, rights = _dev(_stack(10 + H, 5, H, W)), _dev(_stack(50 + H, 5, H, W))
        ref = {k: [] for k in ("left_rectified", "right_rectified", "left_vertical",
                               "right_vertical")}
        for p in range(5):
            lo, ro = er.rectify(lefts[p], rights[p], RV[p], TV[p], fill=SENT)
            ref["left_rectified"].append(lo)
            ref["right_rectified"].append(ro)
            ref["left_vertical"].append(er.vertical_rotate(lo, fill=SENT))
            ref["right_vertical"].append(er.vertical_rotate(ro, fill=SENT))
        out[(H, W)] = (lefts, rights, {k: torch.stack(v) for k, v in ref.items()})
    return out


# ---------------------------------------------------------------- 1. the vertical stack
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 7, 17])
def test_vertical_rotate_batch(er, H, W, n):
    """n = 17 crosses the 16-image chunk of the shared-map launch (two grid slices)"""
    import torch
    ims = _dev(_stack(3 * n + H, n, H, W))
    ref = torch.stack([er.vertical_rotate(ims[i], fill=SENT) for i in range(n)])
    got = er.vertical_rotate_batch(ims, fill=SENT)
    assert got.shape == (n, W, H, 3) and _same(got, ref)
    assert not _same(got, torch.full_like(got, SENT))
    # fill = -1 keeps the caller's pre-fill where nothing is written
    mine = torch.full((n, W, H, 3), 77, dtype=torch.uint8, device=ims.device)
    assert er.vertical_rotate_batch(ims, fill=-1, out=mine) is mine
    ref77 = torch.stack([er.vertical_rotate(ims[i], fill=77) for i in range(n)])
    assert _same(mine, ref77)
    # the other route of the stage (ROT90 jobs of the per-image kernel): the same bytes
    er.ctx.set_option("vertical_shared", 0)
    try:
        assert _same(er.vertical_rotate_batch(ims, fill=SENT), ref)
    finally:
        er.ctx.set_option("vertical_shared", 1)


# ---------------------------------------------------------------- 2. host poses
@pytest.mark.parametrize("H,W", SHAPES)
def test_rectify_batch_host_poses(er, oracle, pairs, H, W):
    """P = 5: the 10 FULL jobs span two launches of the 8-job remap"""
    lefts, rights, ref = pairs[(H, W)]
    got = er.rectify_batch(lefts, rights, rot_vecs=RV, t_vecs=TV, fill=SENT)
    assert set(got) == {"left_rectified", "right_rectified", "left_vertical", "right_vertical",
                        "done"}
    for k, v in ref.items():
        assert _same(got[k], v), k
    assert got["done"].cpu().tolist() == [1] * 5
    nov = er.rectify_batch(lefts, rights, rot_vecs=RV, t_vecs=TV, fill=SENT, vertical=False)
    assert set(nov) == {"left_rectified", "right_rectified", "done"}
    assert _same(nov["left_rectified"], ref["left_rectified"])
    assert _same(nov["right_rectified"], ref["right_rectified"])
    # against the oracle: byte-exact up to certified truncation-boundary pixels
    ln, rn = lefts.cpu().numpy(), rights.cpu().numpy()
    gl, gr = got["left_rectified"].cpu().numpy(), got["right_rectified"].cpu().numpy()
    ml, mr = np.zeros(9), np.zeros(9)
    for p in range(5):
        ol, orr = oracle.rectify(ln[p], rn[p], RV[p], TV[p], fill=SENT)
        assert er.L.erp_rectify_matrices(RV[p].ctypes.data, TV[p].ctypes.data, ml.ctypes.data,
                                         mr.ctypes.data) == 0
        _certify(gl[p], ol, lambda ix: (ix[:, 0], ix[:, 1]), ml, W, H)
        _certify(gr[p], orr, lambda ix: (ix[:, 0], ix[:, 1]), mr, W, H)


# ---------------------------------------------------------------- 3. every pixel on the list
def test_identity_pose_goes_through_the_boundary_list(er):
    """R = 0, T = (0, -1, 0): both matrices are the identity and every pixel's pre-truncation
    value is an integer, so every pixel of the 10 FULL jobs is deferred to the fix-up kernel"""
    import torch
    H, W = SHAPES[0]
    lefts, rights = _dev(_stack(7, 5, H, W)), _dev(_stack(70, 5, H, W))
    rv, tv = np.zeros((5, 3)), np.tile([0.0, -1.0, 0.0], (5, 1))
    got = er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv, fill=SENT)
    for p in range(5):
        lo, ro = er.rectify(lefts[p], rights[p], rv[p], tv[p], fill=SENT)
        assert _same(got["left_rectified"][p], lo) and _same(got["right_rectified"][p], ro)
        assert _same(got["left_vertical"][p], er.vertical_rotate(lo, fill=SENT))
        assert _same(got["right_vertical"][p], er.vertical_rotate(ro, fill=SENT))
    assert got["done"].cpu().tolist() == [1] * 5
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. skipped pairs
def _records(rv, tv, status):
    from erp_match_eightpoint_test_amd.capi import RESULT_DTYPE
    rec = np.zeros(len(status), RESULT_DTYPE)
    rec["R"], rec["T"], rec["status"] = rv, tv, status
    return _dev(rec.view(np.uint8).reshape(len(status), RESULT_DTYPE.itemsize))


@pytest.mark.parametrize("route", ["skip", "results"])
def test_skipped_pair_stays_at_fill(er, pairs, route):
    import torch
    H, W = SHAPES[1]
    lefts, rights, ref = pairs[(H, W)]
    if route == "skip":
        got = er.rectify_batch(lefts[:3], rights[:3], rot_vecs=RV[:3], t_vecs=TV[:3],
                               skip=[0, 1, 0], fill=SENT)
    else:  # a record whose status is ERP_TOO_FEW_POINTS; R, T are float32 in the records
        got = er.rectify_batch(lefts[:3], rights[:3], fill=SENT,
                               results=_records(RV[:3], TV[:3], [0, 2, 0]))
    assert got["done"].cpu().tolist() == [1, 0, 1]
    blank = torch.full_like(lefts[0], SENT)
    for side in ("left", "right"):
        assert _same(got[side + "_rectified"][1], blank)
        # the vertical view of a fill-valued image, as the per-image call gives it
        assert _same(got[side + "_vertical"][1], er.vertical_rotate(blank, fill=SENT))
        for p in (0, 2):
            assert _same(got[side + "_rectified"][p], ref[side + "_rectified"][p]), (side, p)
            assert _same(got[side + "_vertical"][p], ref[side + "_vertical"][p]), (side, p)


def test_two_stacks_of_more_than_one_chunk(er):
    """P = 17: the vertical stage's launch has 2 stacks x 2 chunks of grid slices"""
    H, W = SHAPES[0]
    P = 17
    lefts, rights = _dev(_stack(300, P, H, W)), _dev(_stack(400, P, H, W))
    rv, tv = np.tile(RV, (4, 1))[:P], np.tile(TV, (4, 1))[:P]
    got = er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv, fill=SENT)
    for side in ("left", "right"):
        for p in (0, 15, 16):
            assert _same(got[side + "_vertical"][p],
                         er.vertical_rotate(got[side + "_rectified"][p], fill=SENT)), (side, p)
        assert _same(got[side + "_vertical"],
                     er.vertical_rotate_batch(got[side + "_rectified"], fill=SENT))
    lo, ro = er.rectify(lefts[16], rights[16], rv[16], tv[16], fill=SENT)
    assert _same(got["left_rectified"][16], lo) and _same(got["right_rectified"][16], ro)


# ---------------------------------------------------------------- 5. nothing to do
def test_zero_pairs(er, pairs):
    H, W = SHAPES[0]
    lefts, rights, _ = pairs[(H, W)]
    got = er.rectify_batch(lefts[:0], rights[:0], rot_vecs=np.zeros((0, 3)),
                           t_vecs=np.zeros((0, 3)))
    assert got["left_rectified"].shape == (0, H, W, 3)
    assert got["right_vertical"].shape == (0, W, H, 3) and got["done"].shape == (0,)
    got = er.rectify_batch(lefts[:0], rights[:0], results=_records(RV[:0], TV[:0], []))
    assert got["right_rectified"].shape == (0, H, W, 3)
    assert er.vertical_rotate_batch(lefts[:0]).shape == (0, W, H, 3)
    from erp_match_eightpoint_test_amd import capi
    o = capi.RectifyOutputs()
    assert er.L.erp_rectify_batch_dev(er.ctx.h, None, None, 0, W, H, None, None, None, 0,
                                      C.byref(o), None) == 0


# ---------------------------------------------------------------- 6. the wrappers' checks
def test_wrappers_reject_bad_inputs(er, pairs):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, erp_rotation
    H, W = SHAPES[0]
    lefts, rights, _ = pairs[(H, W)]
    bad = [(lefts.cpu(), rights.cpu()),                  # host tensors
           (lefts.float(), rights.float()),              # not uint8
           (lefts, rights[:4]),                          # pair counts differ
           (lefts, rights[:, : H // 2].contiguous()),    # sizes differ
           (lefts[:, :, ::2], rights[:, :, ::2]),        # not contiguous
           (lefts[0], rights[0])]                        # not a batch
    run = PairBatchRunner(ctx=er.ctx)
    for a, b in bad:
        with pytest.raises(ValueError):
            er.rectify_batch(a, b, rot_vecs=RV[:a.shape[0]], t_vecs=TV[:a.shape[0]])
        with pytest.raises(ValueError):
            run.rectify_images(a, b)
    for a in (lefts.cpu(), lefts.float(), lefts[:, :, ::2], lefts[0]):
        with pytest.raises(ValueError):
            er.vertical_rotate_batch(a)
    with pytest.raises(ValueError):                      # fill = -1 is about a caller's output
        er.vertical_rotate_batch(lefts, fill=-1)
    with pytest.raises(ValueError):                      # an output of the input's shape
        er.vertical_rotate_batch(lefts, out=torch.empty_like(lefts))
    with pytest.raises(ValueError):                      # neither poses nor records
        er.rectify_batch(lefts, rights)
    with pytest.raises(ValueError):                      # both
        er.rectify_batch(lefts, rights, rot_vecs=RV, t_vecs=TV,
                         results=_records(RV, TV, [0] * 5))
    with pytest.raises(ValueError):                      # a pose per pair
        er.rectify_batch(lefts, rights, rot_vecs=RV[:4], t_vecs=TV[:4])
    with pytest.raises(ValueError):                      # records: [P, 64] uint8 on the device
        er.rectify_batch(lefts, rights, results=_records(RV, TV, [0] * 5).cpu())
    with pytest.raises(ValueError):
        er.rectify_batch(lefts, rights, results=_records(RV[:4], TV[:4], [0] * 4))
    # a context of another device: the wrappers compare the tensors' device with the
    # context's before any call (the handle below is never used)
    other = Context(0)
    other.device = 1
    with pytest.raises(ValueError):
        erp_rotation(ctx=other).rectify_batch(lefts, rights, rot_vecs=RV, t_vecs=TV)
    with pytest.raises(ValueError):
        erp_rotation(ctx=other).vertical_rotate_batch(lefts)
    other.device = 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. automatic's main, batched
def test_rectify_images(gpu_lib, oracle):
    """the three 672 x 336 pairs of test_gpu_image_batch (statuses ok, ok, too few points)"""
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, erp_rotation,
                                                results_to_numpy, synth)
    W, H, MAX_KP = 672, 336, 512
    ctx = Context(0)
    er = erp_rotation(ctx=ctx)
    Ri = oracle.inv3(oracle.eular2rot(np.radians([10.0, 5.0, 15.0])))
    a = synth.sphere_texture(3, H, W)
    b = synth.sphere_texture(5, H, W)
    b[H // 2:] = 128
    c = synth.sphere_texture(7, H, W)
    lefts = torch.from_numpy(np.stack([a, b, c])).cuda()
    rights = torch.stack([er.rotate_image(lefts[0], Ri), er.rotate_image(lefts[1], Ri),
                          torch.full_like(lefts[2], 128)]).contiguous()
    run = PairBatchRunner(ctx=ctx)
    base = run.run_images(lefts, rights, max_kp=MAX_KP)["results"].cpu().numpy().copy()
    got = run.rectify_images(lefts, rights, rect_fill=SENT, max_kp=MAX_KP)
    assert set(got) == {"results", "left_rectified", "right_rectified", "left_vertical",
                        "right_vertical", "done"}
    assert got["results"].cpu().numpy().tobytes() == base.tobytes()
    r = results_to_numpy(got["results"])
    assert [int(x) for x in r["status"]] == [0, 0, 2]
    assert got["done"].cpu().tolist() == [1, 1, 0]
    for p in range(2):
        R_p, T_p = r["R"][p].astype(np.float64), r["T"][p].astype(np.float64)
        lo, ro = er.rectify(lefts[p], rights[p], R_p, T_p, fill=SENT)
        assert _same(got["left_rectified"][p], lo) and _same(got["right_rectified"][p], ro)
        assert _same(got["left_vertical"][p], er.vertical_rotate(lo, fill=SENT))
        assert _same(got["right_vertical"][p], er.vertical_rotate(ro, fill=SENT))
    blank = torch.full_like(lefts[2], SENT)
    assert _same(got["left_rectified"][2], blank) and _same(got["right_rectified"][2], blank)
    nov = run.rectify_images(lefts, rights, vertical=False, rect_fill=SENT, max_kp=MAX_KP)
    assert "left_vertical" not in nov and _same(nov["left_rectified"], got["left_rectified"])
