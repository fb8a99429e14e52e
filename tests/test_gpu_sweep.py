"""Rotation sweeps on the GPU (include/erp_match.h "rotation sweep"): erp_image_sweep_features_dev
/ erp_image_sweep_run against today's route -- erp_rotation.rotate_image per pose, the left image
repeated, do_all_batch / run_images -- and erp_match_error_dev against a Python restatement of
one_image_test/main.cpp:27-50, :115-129.  672 x 336 images, three poses, two worlds:

  0  left = sphere_texture(3), base = sphere_texture(3)            (one_image_test's shape)
  1  left = sphere_texture(3), base = sphere_texture(5), rows H/2.. = 128   (ragged, unequal sides)

Today's route is computed once per module (the `worlds` fixture) and shared."""
from __future__ import annotations

import ctypes as C
import math
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 672, 336
MAX_KP = 512
PACK_KEYS = ("desc_l", "desc_r", "kp_l", "kp_r", "off_l", "off_r", "width", "height",
             "band_counts")
POSES_DEG = ((0.0, 0.0, 0.0), (10.0, 5.0, 15.0), (20.0, 20.0, 20.0))
WANT = ("matches", "key_left", "key_right")


def _bytes_equal(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def worlds(gpu_lib, oracle):
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, erp_rotation,
                                                spherical_surf, synth)
    ctx = Context(0)
    er, ss, run = erp_rotation(ctx=ctx), spherical_surf(ctx=ctx), PairBatchRunner(ctx=ctx)
    mats = np.stack([oracle.eular2rot(np.radians(d)) for d in POSES_DEG])
    left = torch.from_numpy(synth.sphere_texture(3, H, W)).cuda()
    b2 = synth.sphere_texture(5, H, W)
    b2[H // 2:] = 128
    out = []
    for base in (left.clone(), torch.from_numpy(b2).cuda()):
        lefts = torch.stack([left] * len(mats)).contiguous()
        rights = torch.stack([er.rotate_image(base, oracle.inv3(m)) for m in mats]).contiguous()
        ref = ss.do_all_batch(lefts, rights, max_kp=MAX_KP)
        info = dict(ss.last_info)
        recs = run.run_images(lefts, rights, want=WANT, max_kp=MAX_KP)
        torch.cuda.synchronize()
        out.append({"left": left, "base": base, "lefts": lefts, "rights": rights, "ref": ref,
                    "info": info, "recs": {k: v.clone() for k, v in recs.items()}})
    return {"ctx": ctx, "er": er, "ss": ss, "run": run, "mats": mats, "w": out}


# ---------------------------------------------------------------- 1. features
@pytest.mark.parametrize("wi", [0, 1])
def test_features_equal_todays_route(worlds, wi):
    ss, w, mats = worlds["ss"], worlds["w"][wi], worlds["mats"]
    got = ss.do_all_sweep(w["left"], w["base"], mats, max_kp=MAX_KP)
    assert set(got) == set(PACK_KEYS) | {"max_nq", "max_nt"}
    for k in PACK_KEYS:
        assert _bytes_equal(got[k], w["ref"][k]), k
    assert (got["max_nq"], got["max_nt"]) == (w["ref"]["max_nq"], w["ref"]["max_nt"])
    assert ss.last_info == w["info"]
    bc = w["ref"]["band_counts"].cpu().numpy()
    assert (bc[:, 0] == bc[0, 0]).all() and bc[:, 0].min() > 0     # the shared left side
    off = w["ref"]["off_l"].cpu().numpy()
    assert (off == np.arange(len(mats) + 1) * int(bc[0, 0].sum())).all()
    if wi == 1:  # ragged and unequal: the second world is what it is there for
        assert len(set(bc[0, 0].tolist())) > 1 and (bc[:, 1].sum(axis=1) != bc[0, 0].sum()).all()
    for group, groups in ((1, 3), (3, 1)):
        g = ss.do_all_sweep(w["left"], w["base"], mats, max_kp=MAX_KP, max_group_pairs=group)
        assert ss.last_info["groups"] == groups
        assert {**ss.last_info, "groups": 1} == w["info"]
        for k in PACK_KEYS:
            assert _bytes_equal(g[k], w["ref"][k]), (group, k)


# ---------------------------------------------------------------- 2. records
@pytest.mark.parametrize("wi", [0, 1])
def test_records_equal_todays_route(worlds, wi):
    import torch
    run, w, mats = worlds["run"], worlds["w"][wi], worlds["mats"]
    outs = run.run_sweep(w["left"], w["base"], mats, want=WANT, max_kp=MAX_KP)
    torch.cuda.synchronize()
    assert set(outs) == {"results", "match_error"} | set(WANT)
    assert _bytes_equal(outs["results"], w["recs"]["results"])
    assert _bytes_equal(outs["matches"], w["recs"]["matches"])
    assert _bytes_equal(outs["key_left"], w["recs"]["key_left"])
    assert _bytes_equal(outs["key_right"], w["recs"]["key_right"])
    one = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP)
    torch.cuda.synchronize()
    assert set(one) == {"results", "match_error"}
    assert _bytes_equal(one["results"], w["recs"]["results"])
    assert run.last_info["fits"] == 1 and run.last_info["groups"] == 1
    if wi == 0:  # the estimator really ran on every pose
        from erp_match_eightpoint_test_amd import results_to_numpy
        r = results_to_numpy(one["results"])
        assert (r["status"] == 0).all() and (r["M"] >= 8).all()


# ---------------------------------------------------------------- 3. rand stream
def test_rand_stream_poses_draw_one_after_the_other(worlds):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, RandStream
    w, mats = worlds["w"][0], worlds["mats"]
    rs = RandStream(1, 0)
    run = PairBatchRunner(ctx=Context(0), stream=rs)
    rs.set(1, 0)
    a = run.run_images(w["lefts"], w["rights"], max_kp=MAX_KP)["results"].cpu().numpy()
    draws_a = rs.draws
    rs.set(1, 0)
    b = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP)["results"].cpu().numpy()
    draws_b = rs.draws
    torch.cuda.synchronize()
    assert a.tobytes() == b.tobytes()
    assert draws_a == draws_b and draws_b > 0
    plain = w["recs"]["results"].cpu().numpy()
    assert any(plain[p].tobytes() != b[p].tobytes() for p in range(len(mats)))
    run.ctx.set_rand_stream(None)


# ---------------------------------------------------------------- 4. the match error alone
def _degree_error(v1, v2):
    """one_image_test/main.cpp:27-50 on (x, y) float32 points, Python floats"""
    a1, b1 = math.pi * float(v1[1]) / H, 2 * math.pi * float(v1[0]) / W
    a2, b2 = math.pi * float(v2[1]) / H, 2 * math.pi * float(v2[0]) / W
    c1 = (math.sin(a1) * math.cos(b1), math.sin(a1) * math.sin(b1), math.cos(a1))
    c2 = (math.sin(a2) * math.cos(b2), math.sin(a2) * math.sin(b2), math.cos(a2))
    product = c1[0] * c2[0] + c1[1] * c2[1] + c1[2] * c2[2]
    return math.acos(product) if product < 1 else 0.0


def _left_keys(rng, n):
    k = np.stack([rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)], axis=1).astype(np.float32)
    whole = rng.random(n) < 1 / 3
    k[whole] = np.floor(k[whole])
    return k


def test_match_error_kernel_against_python(worlds, oracle):
    import torch
    er = worlds["er"]
    Ms, S = [0, 1, 64, 65, 1000], 1024
    P = len(Ms)
    rng = np.random.default_rng(2024)
    mats = np.stack([oracle.eular2rot(np.radians(d)) for d in
                     ((7.0, 3.0, 11.0), (10.0, 5.0, 15.0), (20.0, 20.0, 20.0), (-13.0, 8.0, 31.0),
                      (2.5, -17.0, 6.0))])
    kl = np.zeros((P, S, 2), np.float32)
    kr = np.zeros((P, S, 2), np.float32)
    want = np.full(P, np.nan)
    generated = redrawn = 0
    sides = [0, 0]
    for p, M in enumerate(Ms):
        keys = _left_keys(rng, M)
        generated += M
        while M:  # redraw the keys whose truncated values the last ulp of libm decides
            pre = oracle.rotate_pixel_prefix(keys[:, 1].astype(np.int32),
                                             keys[:, 0].astype(np.int32), mats[p], W, H)
            bad = (np.abs(pre - np.rint(pre)) < 1e-6).any(axis=1)
            if not bad.any():
                break
            redrawn += int(bad.sum())
            keys[bad] = _left_keys(rng, int(bad.sum()))
        acc = 0.0
        for i in range(M):
            r, c = oracle.rotate_pixel(int(keys[i, 1]), int(keys[i, 0]), mats[p], W, H)
            v1 = np.array([c, r], np.float32)
            t = rng.uniform(0, 2 * math.pi)
            size = 0.0 if rng.random() < 0.1 else rng.uniform(0, 3)
            v2 = (v1 + size * np.array([math.cos(t), math.sin(t)])).astype(np.float32)
            kl[p, i], kr[p, i] = keys[i], v2
            e = _degree_error(v1, v2)
            sides[e == 0.0] += 1
            acc = acc + e
        if M:
            want[p] = acc / M
    assert redrawn <= 0.01 * generated, (redrawn, generated)   # guards the generator only
    assert min(sides) > 0, sides                                # both sides of product < 1
    dkl, dkr = torch.from_numpy(kl).cuda(), torch.from_numpy(kr).cuda()
    c1 = torch.tensor(Ms, dtype=torch.int32, device="cuda")
    c16 = torch.full((P * 16,), -3, dtype=torch.int32, device="cuda")
    c16[::16] = c1
    got1 = er.match_error(dkl, dkr, c1, mats, W, H).cpu().numpy()
    got1b = er.match_error(dkl, dkr, c1, mats, W, H).cpu().numpy()
    got16 = er.match_error(dkl, dkr, c16[::16], mats, W, H).cpu().numpy()
    for p, M in enumerate(Ms):
        print(f"M={M}: got {got1[p]!r} want {want[p]!r} diff {abs(got1[p] - want[p]):.3g}")
    assert np.isnan(got1[0]) and not np.isnan(got1[1:]).any()
    # derived: the transcendentals differ from glibc's by a few ulp, so the product by < 1e-15,
    # which acos amplifies at product -> 1 to at most sqrt(2e-15) = 4.5e-8
    assert (np.abs(got1[1:] - want[1:]) <= 1e-7).all()
    assert got1.tobytes() == got1b.tobytes() == got16.tobytes()
    # a negative count is no match
    neg = er.match_error(dkl, dkr, torch.full((P,), -5, dtype=torch.int32, device="cuda"), mats,
                         W, H).cpu().numpy()
    assert np.isnan(neg).all()


# ---------------------------------------------------------------- 5. the match error end to end
def test_match_error_end_to_end(worlds):
    import torch
    from erp_match_eightpoint_test_amd import RESULT_DTYPE
    run, er, w, mats = worlds["run"], worlds["er"], worlds["w"][0], worlds["mats"]
    one = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP)
    recs = w["recs"]
    m_col = recs["results"].view(torch.int32)[:, RESULT_DTYPE.fields["M"][1] // 4]
    ref = er.match_error(recs["key_left"], recs["key_right"], m_col, mats, W, H)
    torch.cuda.synchronize()
    print("surf match error (rad), poses", POSES_DEG, ":", ref.cpu().numpy().tolist())
    assert _bytes_equal(one["match_error"], ref)
    wanted = run.run_sweep(w["left"], w["base"], mats, want=("matches",), max_kp=MAX_KP)
    assert _bytes_equal(wanted["match_error"], ref) and set(wanted) == {"results", "matches",
                                                                         "match_error"}
    none = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP, match_error=False)
    assert set(none) == {"results"} and _bytes_equal(none["results"], recs["results"])


# ---------------------------------------------------------------- 6. edges
def _raw_features(worlds, w, mats, max_kp, cap_l, cap_r):
    import torch
    from erp_match_eightpoint_test_amd import _PackedBuffers, capi
    ctx = worlds["ctx"]
    n = len(mats)
    buf = _PackedBuffers(n, cap_l, cap_r, w["left"].device)
    buf.t["off_l"].fill_(-7)
    buf.t["off_r"].fill_(-7)
    pk = buf.struct()
    prm = capi.SurfParams()
    ctx.L.erp_surf_params_default(C.byref(prm))
    info = capi.ImageBatchInfo()
    m = np.ascontiguousarray(mats, np.float64)
    st = ctx.L.erp_image_sweep_features_dev(ctx.h, w["left"].data_ptr(), w["base"].data_ptr(), n,
                                            m.ctypes.data if n else None, W, H, C.byref(prm),
                                            max_kp, 0, 0, C.byref(pk), C.byref(info),
                                            torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, info, buf


def test_zero_poses_and_singular_pose(worlds):
    from erp_match_eightpoint_test_amd import ErpError
    w, mats = worlds["w"][0], worlds["mats"]
    st, info, buf = _raw_features(worlds, w, mats[:0], MAX_KP, 8, 8)
    assert st == 0 and info.fits == 1
    assert (info.rows_l, info.rows_r, info.groups, info.max_nq, info.max_nt) == (0, 0, 0, 0, 0)
    assert int(buf.t["off_l"][0]) == 0 and int(buf.t["off_r"][0]) == 0
    outs = worlds["run"].run_sweep(w["left"], w["base"], mats[:0])
    assert outs["results"].shape[0] == 0 and outs["match_error"].shape[0] == 0
    bad = mats.copy()
    bad[1, 2] = bad[1, 0]  # two equal rows: det == 0
    st, info, _ = _raw_features(worlds, w, bad, MAX_KP, 8, 8)
    assert st == 1 and info.groups == 0
    with pytest.raises(ErpError) as e:
        worlds["run"].run_sweep(w["left"], w["base"], bad, max_kp=MAX_KP)
    assert e.value.status == 1


def test_overflow_reports_and_wrapper_retries(worlds):
    ss, w, mats = worlds["ss"], worlds["w"][1], worlds["mats"]
    bc = w["ref"]["band_counts"].cpu().numpy()
    # the largest band is a left one here, so need_kp shows whether the left bands count
    assert bc[:, 0].max() > bc[:, 1].max() and bc.max() > 64
    rows_l, rows_r = w["info"]["rows_l"], w["info"]["rows_r"]
    st, info, _ = _raw_features(worlds, w, mats, 64, rows_l, rows_r)
    assert st == 0 and info.fits == 0 and info.need_kp == int(bc.max())
    st, info, _ = _raw_features(worlds, w, mats, MAX_KP, rows_l - 1, rows_r)
    assert st == 0 and info.fits == 0 and (info.rows_l, info.rows_r) == (rows_l, rows_r)
    st, info, buf = _raw_features(worlds, w, mats, MAX_KP, rows_l, rows_r)
    assert st == 0 and info.fits == 1
    assert _bytes_equal(buf.result(rows_l, rows_r)["desc_r"], w["ref"]["desc_r"])
    got = ss.do_all_sweep(w["left"], w["base"], mats, max_kp=64)
    assert ss.last_info["fits"] == 1
    for k in PACK_KEYS:
        assert _bytes_equal(got[k], w["ref"][k]), k


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} after a bad argument")


def test_wrappers_reject_bad_inputs_before_any_call(worlds):
    from erp_match_eightpoint_test_amd import PairBatchRunner, spherical_surf
    w, mats = worlds["w"][0], worlds["mats"]
    left, base = w["left"], w["base"]
    fake = types.SimpleNamespace(device=0, L=_NoCalls(), h=None, rand_stream=None)
    other = types.SimpleNamespace(device=1, L=_NoCalls(), h=None, rand_stream=None)
    bad = [(left.cpu(), base.cpu()),                        # host tensors
           (left, base[: H // 2].contiguous()),             # sizes differ
           (left[:, ::2], base[:, ::2]),                    # not contiguous
           (left.float(), base.float())]                    # not uint8
    for ctx, cases in ((fake, bad), (other, [(left, base)])):   # other: a wrong device
        ss, run = spherical_surf(ctx=ctx), PairBatchRunner(ctx=ctx)
        for a, b in cases:
            with pytest.raises(ValueError):
                ss.do_all_sweep(a, b, mats)
            with pytest.raises(ValueError):
                run.run_sweep(a, b, mats)
    run = PairBatchRunner(ctx=fake)
    with pytest.raises(ValueError):
        run.run_sweep(left, base, mats, want=("matches",), chunk=2)
    with pytest.raises(ValueError):
        run.run_sweep(left, base, mats[:, :2])              # not 3x3 matrices


def test_chunks_give_the_same_estimates(worlds):
    from erp_match_eightpoint_test_amd import results_to_numpy
    run, w, mats = worlds["run"], worlds["w"][0], worlds["mats"]
    a = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP, chunk=128)
    b = run.run_sweep(w["left"], w["base"], mats, max_kp=MAX_KP, chunk=2)
    ra, rb = results_to_numpy(a["results"]), results_to_numpy(b["results"])
    for f in ("R", "T", "status", "M", "K", "min_idx"):
        assert ra[f].tobytes() == rb[f].tobytes(), f
    assert _bytes_equal(a["match_error"], b["match_error"])
