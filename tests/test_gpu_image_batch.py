"""Batched do_all on the GPU (include/erp_match.h "batched do_all"): the pack kernel against
numpy + the oracle, and erp_image_pairs_features_dev / erp_image_pairs_run against today's
per-pair code on three small ERP pairs (672 x 336, bands 84 x 672):

  A  sphere_texture(3)                      right = rotate_image(left, eular2rot(10, 5, 15 deg)^-1)
  B  sphere_texture(5), rows H/2.. = 128    right rotated likewise (few keypoints, ragged bands)
  C  sphere_texture(7)                      right = constant 128 (no keypoints: TOO_FEW_POINTS)

Everything from the images is computed once per module (the `world` fixture) and shared."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 672, 336
MAX_KP = 512
PACK_KEYS = ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r", "width", "height",
             "band_counts")


def _bytes_equal(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 1. the pack kernel alone
def test_pack_against_numpy_and_oracle(gpu_lib, oracle):
    """P = 3, max_kp = 16; the counts hold 0, max_kp, an all-zero side and unequal bands; rows
    past a count are NaN (never read); the outputs are 8 rows longer than needed and keep their
    canary there (rows past the side's total are never written)."""
    import torch
    from erp_match_eightpoint_test_amd import Context, capi
    P, K = 3, 16
    counts = np.array([[[3, 0, 16, 5], [7, 16, 1, 2]],
                       [[16, 16, 16, 16], [0, 0, 0, 0]],
                       [[1, 2, 0, 9], [0, 11, 4, 16]]], np.int32)
    rng = np.random.default_rng(11)
    kp = np.full((8 * P, K, 7), np.nan, np.float32)
    desc = np.full((8 * P, K, 64), np.nan, np.float32)
    flat = counts.reshape(-1)
    for i, c in enumerate(flat):
        kp[i, :c, 0] = rng.uniform(0, W, c).astype(np.float32)
        kp[i, :c, 1] = rng.uniform(0, H / 4, c).astype(np.float32)
        kp[i, :c, 2:] = rng.standard_normal((c, 5)).astype(np.float32)
        desc[i, :c] = rng.standard_normal((c, 64)).astype(np.float32)
    kp[:, :, 0] = np.minimum(kp[:, :, 0], np.float32(W - 0.01))
    kp[:, :, 1] = np.minimum(kp[:, :, 1], np.float32(H / 4 - 0.01))
    # the expected packed batch
    exp = {}
    for s, side in enumerate("lr"):
        d, k, off = [], [], [0]
        for p in range(P):
            c4 = counts[p, s]
            pts = np.concatenate([kp[(p * 2 + s) * 4 + b, :c4[b], :2] for b in range(4)])
            k.append(oracle.unrotate_band_keypoints(pts, c4, W, H) if len(pts) else pts)
            d.append(np.concatenate([desc[(p * 2 + s) * 4 + b, :c4[b]] for b in range(4)]))
            off.append(off[-1] + int(c4.sum()))
        exp["desc_" + side], exp["kp_" + side] = np.concatenate(d), np.concatenate(k)
        exp["off_" + side] = np.array(off, np.int64)
    dev = torch.device("cuda:0")
    rows = {s: int(exp["off_" + s][-1]) for s in "lr"}
    CANARY = -12345.5
    t = {"desc_l": torch.full((rows["l"] + 8, 64), CANARY, device=dev),
         "desc_r": torch.full((rows["r"] + 8, 64), CANARY, device=dev),
         "kp_l": torch.full((rows["l"] + 8, 2), CANARY, device=dev),
         "kp_r": torch.full((rows["r"] + 8, 2), CANARY, device=dev),
         "off_l": torch.full((P + 1,), -7, dtype=torch.int64, device=dev),
         "off_r": torch.full((P + 1,), -7, dtype=torch.int64, device=dev),
         "width": torch.full((P,), -7, dtype=torch.int32, device=dev),
         "height": torch.full((P,), -7, dtype=torch.int32, device=dev),
         "band_counts": torch.full((P, 2, 4), -7, dtype=torch.int32, device=dev)}
    pk = capi.PackedPairs(*[t[k].data_ptr() for k in PACK_KEYS], rows["l"] + 8, rows["r"] + 8)
    ctx = Context(0)
    dkp = torch.from_numpy(kp.view(np.uint8).reshape(8 * P, K, 28)).to(dev)
    ddesc, dcnt = torch.from_numpy(desc).to(dev), torch.from_numpy(flat.copy()).to(dev)
    st = gpu_lib.erp_pack_band_features_dev(ctx.h, dkp.data_ptr(), ddesc.data_ptr(),
                                            dcnt.data_ptr(), P, K, W, H, C.byref(pk),
                                            torch.cuda.current_stream().cuda_stream)
    assert st == capi.ERP_OK
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    for s in "lr":
        n = rows[s]
        assert np.array_equal(got["off_" + s], exp["off_" + s])
        assert got["desc_" + s][:n].tobytes() == exp["desc_" + s].tobytes()
        assert got["kp_" + s][:n].tobytes() == exp["kp_" + s].astype(np.float32).tobytes()
        assert (got["desc_" + s][n:] == CANARY).all() and (got["kp_" + s][n:] == CANARY).all()
        assert not np.isnan(got["desc_" + s]).any() and not np.isnan(got["kp_" + s]).any()
    assert (got["width"] == W).all() and (got["height"] == H).all()
    assert np.array_equal(got["band_counts"], counts)
    # the Python wrapper returns the same batch
    from erp_match_eightpoint_test_amd import spherical_surf
    w = spherical_surf(ctx=ctx).pack_band_features(dkp, ddesc, dcnt, W, H)
    for k in PACK_KEYS[:6]:
        n = rows[k[-1]] if k[:2] in ("de", "kp") else None
        assert w[k].cpu().numpy().tobytes() == got[k][:n].tobytes(), k
    assert (w["max_nq"], w["max_nt"]) == (64, 31)


# ---------------------------------------------------------------- the three image pairs
@pytest.fixture(scope="module")
def world(gpu_lib, oracle):
    """images, the batched result, and the same tensors assembled with the per-pair code"""
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, erp_rotation,
                                                feature_matcher, spherical_surf, synth)
    ctx = Context(0)
    er, ss, fm = erp_rotation(ctx=ctx), spherical_surf(ctx=ctx), feature_matcher(ctx=ctx)
    Ri = oracle.inv3(oracle.eular2rot(np.radians([10.0, 5.0, 15.0])))
    a = synth.sphere_texture(3, H, W)
    b = synth.sphere_texture(5, H, W)
    b[H // 2:] = 128
    c = synth.sphere_texture(7, H, W)
    lefts = torch.from_numpy(np.stack([a, b, c])).cuda()
    rights = torch.stack([er.rotate_image(lefts[0], Ri), er.rotate_image(lefts[1], Ri),
                          torch.full_like(lefts[2], 128)]).contiguous()
    # today's per-pair code: bands -> surf_dev -> unrotate_band_keypoints -> torch.cat
    ref = {k: [] for k in ("desc_l", "desc_r", "kp_l", "kp_r")}
    counts = []
    for p in range(3):
        bands = ss.bands(torch.stack([lefts[p], rights[p]]).contiguous())
        kp, desc, cnt = fm.surf_dev(bands.reshape(8, H // 4, W, 3), max_kp=MAX_KP)
        kxy = kp.view(torch.float32)[..., :2]
        counts.append(np.asarray(cnt).reshape(2, 4))
        for s, side in enumerate("lr"):
            c4 = [int(x) for x in cnt[4 * s: 4 * s + 4]]
            key = torch.cat([kxy[4 * s + bd, :c4[bd]] for bd in range(4)]).contiguous()
            if key.shape[0]:
                ss.unrotate_band_keypoints(key, c4, W, H)
            ref["kp_" + side].append(key)
            ref["desc_" + side].append(torch.cat([desc[4 * s + bd, :c4[bd]] for bd in range(4)]))
    counts = np.stack(counts).astype(np.int32)                     # [3, 2, 4]
    per = counts.sum(axis=2)
    for k in list(ref):
        ref[k] = torch.cat(ref[k]).contiguous()
    for s, side in enumerate("lr"):
        ref["off_" + side] = torch.from_numpy(
            np.concatenate([[0], np.cumsum(per[:, s])]).astype(np.int64)).cuda()
    ref["width"] = torch.full((3,), W, dtype=torch.int32, device="cuda")
    ref["height"] = torch.full((3,), H, dtype=torch.int32, device="cuda")
    ref["band_counts"] = torch.from_numpy(counts).cuda()
    ref["max_nq"], ref["max_nt"] = int(per[:, 0].max()), int(per[:, 1].max())
    got = ss.do_all_batch(lefts, rights, max_kp=MAX_KP)
    torch.cuda.synchronize()
    return {"ctx": ctx, "ss": ss, "lefts": lefts, "rights": rights, "ref": ref, "got": got,
            "counts": counts, "info": dict(ss.last_info),
            "runner": PairBatchRunner(ctx=ctx)}


def test_inputs_are_what_the_tests_need(world):
    """pairs A and B: ragged, non-zero band counts on both sides; C's right side: none"""
    c = world["counts"]
    assert (c[:2] > 0).all() and (c[2, 0] > 0).all() and (c[2, 1] == 0).all()
    for p in range(2):
        for s in range(2):
            assert len(set(c[p, s].tolist())) > 1
    assert c.max() > 64  # test_overflow's max_kp = 64 really overflows


# ---------------------------------------------------------------- 2. images vs the per-pair path
def test_do_all_batch_equals_per_pair_assembly(world):
    got, ref = world["got"], world["ref"]
    assert set(got) == set(PACK_KEYS) | {"max_nq", "max_nt"}
    for k in PACK_KEYS:
        assert _bytes_equal(got[k], ref[k]), k
    assert (got["max_nq"], got["max_nt"]) == (ref["max_nq"], ref["max_nt"])
    info = world["info"]
    assert info["fits"] == 1 and info["need_kp"] == int(world["counts"].max())
    assert (info["rows_l"], info["rows_r"]) == (ref["desc_l"].shape[0], ref["desc_r"].shape[0])


def _run_args(d):
    return [d[k] for k in ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r", "width",
                           "height", "max_nq", "max_nt")]


def test_run_images_equals_run_and_per_pair_route(world):
    import torch
    from erp_match_eightpoint_test_amd import eight_point, results_to_numpy
    run = world["runner"]
    want = ("matches",)
    ref_outs = run.run(*_run_args(world["ref"]), want=want)
    torch.cuda.synchronize()
    ref_res = ref_outs["results"].cpu().numpy().copy()
    ref_m = ref_outs["matches"].cpu().numpy().copy()
    outs = run.run_images(world["lefts"], world["rights"], want=want, max_kp=MAX_KP)
    torch.cuda.synchronize()
    assert outs["results"].cpu().numpy().tobytes() == ref_res.tobytes()
    assert outs["matches"].cpu().numpy().tobytes() == ref_m.tobytes()
    # the single library call (erp_image_pairs_run) gives the same records
    one = run.run_images(world["lefts"], world["rights"], max_kp=MAX_KP)
    torch.cuda.synchronize()
    assert set(one) == {"results"}
    assert one["results"].cpu().numpy().tobytes() == ref_res.tobytes()
    assert run.last_info["groups"] == 1 and run.last_info["fits"] == 1
    r = results_to_numpy(outs["results"])
    assert [int(x) for x in r["status"]] == [0, 0, 2]
    # the independent per-pair route: do_all + eight_point.find
    ep = eight_point(ctx=world["ctx"])
    for p in range(2):
        kl, kr, M, total = world["ss"].do_all(world["lefts"][p], world["rights"][p])
        assert int(r["M"][p]) == M and M >= 8
        R, T = ep.find(W, H, kl.cpu().numpy(), kr.cpu().numpy())
        print(f"pair {p}: M={M} max|dR|={np.abs(R - r['R'][p]).max():.3g} "
              f"max|dT|={np.abs(T - r['T'][p]).max():.3g}")
        assert np.abs(R - r["R"][p]).max() <= 1e-6 and np.abs(T - r["T"][p]).max() <= 1e-6


# ---------------------------------------------------------------- 3. grouping changes nothing
@pytest.mark.parametrize("group,groups", [(1, 3), (3, 1)])
def test_grouping_changes_nothing(world, group, groups):
    ss = world["ss"]
    got = ss.do_all_batch(world["lefts"], world["rights"], max_kp=MAX_KP, max_group_pairs=group)
    assert ss.last_info["groups"] == groups
    for k in PACK_KEYS:
        assert _bytes_equal(got[k], world["got"][k]), k
    assert (got["max_nq"], got["max_nt"]) == (world["got"]["max_nq"], world["got"]["max_nt"])


# ---------------------------------------------------------------- 4. overflow
def _raw_features(world, max_kp, cap_l, cap_r, n_pairs=3):
    import torch
    from erp_match_eightpoint_test_amd import capi
    from erp_match_eightpoint_test_amd import _PackedBuffers
    L, ctx = world["ctx"].L, world["ctx"]
    buf = _PackedBuffers(n_pairs, cap_l, cap_r, world["lefts"].device)
    pk = buf.struct()
    prm = capi.SurfParams()
    L.erp_surf_params_default(C.byref(prm))
    info = capi.ImageBatchInfo()
    st = L.erp_image_pairs_features_dev(ctx.h, world["lefts"].data_ptr(),
                                        world["rights"].data_ptr(), n_pairs, W, H, C.byref(prm),
                                        max_kp, 0, 0, C.byref(pk), C.byref(info),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, info, buf


def test_overflow_reports_and_wrapper_retries(world):
    rows_l, rows_r = world["info"]["rows_l"], world["info"]["rows_r"]
    st, info, _ = _raw_features(world, 64, rows_l, rows_r)
    assert st == 0 and info.fits == 0 and info.need_kp == int(world["counts"].max())
    st, info, _ = _raw_features(world, MAX_KP, rows_l - 1, rows_r)
    assert st == 0 and info.fits == 0 and (info.rows_l, info.rows_r) == (rows_l, rows_r)
    st, info, _ = _raw_features(world, MAX_KP, rows_l, rows_r - 1)
    assert st == 0 and info.fits == 0 and (info.rows_l, info.rows_r) == (rows_l, rows_r)
    st, info, buf = _raw_features(world, MAX_KP, rows_l, rows_r)
    assert st == 0 and info.fits == 1
    assert _bytes_equal(buf.result(rows_l, rows_r)["desc_r"], world["got"]["desc_r"])
    ss = world["ss"]
    got = ss.do_all_batch(world["lefts"], world["rights"], max_kp=64)
    assert ss.last_info["fits"] == 1
    for k in PACK_KEYS:
        assert _bytes_equal(got[k], world["got"][k]), k


# ---------------------------------------------------------------- 5. the edges that need a context
def test_zero_pairs(world):
    st, info, buf = _raw_features(world, MAX_KP, 8, 8, n_pairs=0)
    assert st == 0 and info.fits == 1
    assert (info.rows_l, info.rows_r, info.groups, info.max_nq, info.max_nt) == (0, 0, 0, 0, 0)
    assert int(buf.t["off_l"][0]) == 0 and int(buf.t["off_r"][0]) == 0
    got = world["ss"].do_all_batch(world["lefts"][:0], world["rights"][:0])
    assert got["desc_l"].shape == (0, 64) and got["off_l"].cpu().tolist() == [0]
    outs = world["runner"].run_images(world["lefts"][:0], world["rights"][:0])
    assert outs["results"].shape[0] == 0


def test_wrappers_reject_bad_device_inputs(world):
    import torch
    ss, run = world["ss"], world["runner"]
    lefts, rights = world["lefts"], world["rights"]
    bad = [(lefts[:, :, ::2], rights[:, :, ::2]),       # not contiguous
           (lefts.float(), rights.float()),             # not uint8
           (lefts, rights[:2]),                         # pair counts differ
           (lefts, rights[:, :H // 2].contiguous()),    # sizes differ
           (lefts[0], rights[0])]                       # not a batch
    for a, b in bad:
        with pytest.raises(ValueError):
            ss.do_all_batch(a, b)
        with pytest.raises(ValueError):
            run.run_images(a, b)
    with pytest.raises(ValueError):
        ss.do_all_batch(lefts, rights, hessian=1.0)     # not a SURF parameter
    torch.cuda.synchronize()
