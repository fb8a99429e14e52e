#!/usr/bin/env python
"""The support stage (erp_pair_batch_run_support) against the route it
replaces: per-iteration inlier counts through cfg.inlier_thr and the hypothesis records.

Five runs, interleaved repetition by repetition in one process on one stream, HIP events:
  (a)  records_thr   erp_pair_batch_run with out->hyps and cfg.inlier_thr = thr: the unchanged
                     VALU count into the 120-byte records (the yardstick);
       records       the same without inlier_thr (so (a)'s count stage = records_thr - records);
  (b)  lite          erp_pair_batch_run on the lite route, no stage;
       support_mfma  erp_pair_batch_run_support on the lite route, the count on bf16 MFMA;
       support_valu  the same with the f32 VALU count (Context option support_count = 0);
                     the stage = support_* - lite, per repetition.
Two shapes: the headline (768 pairs, 4096 keypoints, 10 000 iterations, sample_frac 0.25) and
the same batch with sample_frac chosen for about 10 rows per sample (the RANSAC shape).  Per run
and shape: median, min, max over --reps and spread.  The support counts of both forms must equal
(a)'s hyps[].inliers byte for byte: asserted.  The share of residuals inside each form's band
(the ones redone in fp64) is measured on the host from --band-pairs pairs' records.  Writes one
JSON document (--out) and prints it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BANDS = {"mfma": 2.0 ** -15, "valu": 2.0 ** -19}   # support.hip's d per form


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "spread": float((v.max() - v.min()) / np.median(v))}


def band_share(hyps, kl, kr, W, H, M, thr, pairs):
    """the share of (match, iteration) residuals within d of thr, per form, on `pairs` pairs"""
    import oracle
    oracle.build()
    inside = {k: 0 for k in BANDS}
    total = 0
    for p in pairs:
        m = int(M[p])
        bl = oracle.pixel_to_bearing(int(W[p]), int(H[p]), kl[p, :m])
        br = oracle.pixel_to_bearing(int(W[p]), int(H[p]), kr[p, :m])
        U = (bl[:, :, None] * br[:, None, :]).reshape(m, 9)
        Ec = np.stack([oracle.rank2(e) for e in hyps[p]["E"]])
        res = np.abs(U @ Ec.T)
        total += res.size
        for k, d in BANDS.items():
            inside[k] += int((np.abs(res - thr) < d).sum())
    return {k: v / max(total, 1) for k, v in inside.items()}, total


def measure(name, frac, b, args):
    import torch
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, hyps_to_numpy,
                                               results_to_numpy, support_to_numpy)
    thr = float(np.float32(args.thr))

    def runner(inlier_thr=0.0, arm=None):
        c = Context(0)
        if arm is not None:
            c.set_option("support_count", arm)
        return PairBatchRunner(ctx=c, iters=args.iters, reuse_outputs=True, sample_frac=frac,
                               inlier_thr=inlier_thr)
    sup = ("support", "support_counts")
    routes = {"records_thr": (runner(thr), ("hyps",), None),
              "records": (runner(), ("hyps",), None),
              "lite": (runner(), (), None),
              "support_mfma": (runner(arm=1), sup, thr),
              "support_valu": (runner(arm=0), sup, thr)}

    def feed(route):
        r, want, t = routes[route]
        return r.run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"],
                     b["width"], b["height"], b["max_nq"], b["max_nt"], want=want, support_thr=t)

    print(f"{name}: sample_frac {frac:.6f}", file=sys.stderr, flush=True)
    t = {r: [] for r in routes}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    last = {}
    for rep in range(-1, args.reps):  # (rep -1 warms every route)
        for route in routes:
            ev[0].record()
            last[route] = feed(route)
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 0:
                t[route].append(ev[0].elapsed_time(ev[1]))
    res = results_to_numpy(last["lite"]["results"])
    ok = res["status"] == 0
    inl = np.ascontiguousarray(hyps_to_numpy(last["records_thr"]["hyps"])["inliers"])
    for arm in ("support_mfma", "support_valu"):
        got = last[arm]["support_counts"].cpu().numpy()
        assert got[ok].tobytes() == inl[ok].tobytes(), f"{name}: {arm} counts differ"
        assert not got[~ok].any(), f"{name}: {arm} counted a pair that is not ERP_OK"
        assert torch.equal(last[arm]["results"], last["records_thr"]["results"]), name
    assert torch.equal(last["support_mfma"]["support"], last["support_valu"]["support"]), name
    s = support_to_numpy(last["support_mfma"]["support"])
    assert (s["status"] == res["status"]).all(), f"{name}: a support record failed its self-check"
    # the band shares on a few pairs' records (a second, untimed records run with the keys)
    r, _, _ = routes["records"]
    o = PairBatchRunner(ctx=r.ctx, iters=args.iters, sample_frac=frac).run(
        b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"], b["width"],
        b["height"], b["max_nq"], b["max_nt"], want=("hyps", "key_left", "key_right"))
    torch.cuda.synchronize()
    pairs = [int(p) for p in np.nonzero(ok)[0][:args.band_pairs]]
    share, cells = band_share(hyps_to_numpy(o["hyps"]), o["key_left"].cpu().numpy(),
                              o["key_right"].cpu().numpy(), b["width"].cpu().numpy(),
                              b["height"].cpu().numpy(), res["M"], thr, pairs)
    a = np.asarray
    diff = lambda x, y: stats(a(t[x]) - a(t[y]))  # noqa: E731
    residuals = float(res["M"][ok].astype(np.float64).sum() * args.iters)
    return {"shape": name, "pairs": int(len(res)), "kpts": args.kpts, "iters": args.iters,
            "sample_frac": frac, "thr": thr, "reps": args.reps, "pairs_ok": int(ok.sum()),
            "M_mean": float(res["M"][ok].mean()), "residuals_per_step": residuals,
            "sample_n_hist": np.bincount(res["sample_n"][ok]).tolist() if frac < 0.1 else None,
            "run_ms": {k: stats(v) for k, v in t.items()},
            "stage_ms": {"a_inlier_thr_count": diff("records_thr", "records"),
                         "b_support_mfma": diff("support_mfma", "lite"),
                         "b_support_valu": diff("support_valu", "lite")},
            "b_over_a_run": {k: float(np.median(t[k]) / np.median(t["records_thr"]))
                             for k in ("support_mfma", "support_valu")},
            "band_share": share, "band_cells": cells, "band_pairs": pairs,
            "inliers_median": {"support": float(np.median(s["inliers"][ok])),
                               "consensus": float(np.median(s["consensus_inliers"][ok]))},
            "hyps_bytes": int(len(res)) * args.iters * 120,
            "counts_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=768)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--thr", type=float, default=0.005)
    ap.add_argument("--rows", type=float, default=10.5, help="the RANSAC shape's rows per sample")
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--band-pairs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20a_bench_support.json"))
    args = ap.parse_args()
    import torch
    import bench
    from erp_match_eightpoint_test_amd import PairBatchRunner, results_to_numpy
    assert torch.cuda.is_available(), "bench_support needs a HIP device"
    b = bench.to_device(bench.make_batch(0, args.pairs, args.kpts, args.seed), torch.device("cuda:0"))
    probe = PairBatchRunner(iters=1).run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"],
                                         b["off_r"], b["width"], b["height"], b["max_nq"],
                                         b["max_nt"])
    M = results_to_numpy(probe["results"])["M"]
    print(f"batch ready: {args.pairs} pairs, median M {np.median(M[M > 0]):.0f}", file=sys.stderr,
          flush=True)
    frac = float(args.rows / np.median(M[M > 0]))
    # the kernels' registers, LDS and scratch as the compiler reports them for gfx950
    # (-Rpass-analysis=kernel-resource-usage on support.hip; they do not change at run time)
    doc = {"bench": "support", "device": torch.cuda.get_device_name(0),
           "lib": os.path.basename(os.environ.get("ERP_LIB_PATH", "")),  # a development variant
           "kernel_resources": {
               "support_count_mfma_kernel": {"vgprs": 138, "agprs": 0, "lds_bytes": 16384,
                                             "scratch_bytes": 0, "waves_per_simd": 3},
               "support_count_valu_kernel": {"vgprs": 70, "agprs": 0, "lds_bytes": 0,
                                             "scratch_bytes": 0, "waves_per_simd": 7}},
           "shapes": [measure("headline", 0.25, b, args), measure("ransac", frac, b, args)]}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
