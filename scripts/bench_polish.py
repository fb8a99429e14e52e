#!/usr/bin/env python
"""The polish stage (erp_polish_dev) next to the call that feeds it.

256 pairs of synth.make_pair(n_kpts=1024, mismatch_frac=0.2), 1000 iterations, thr 0.01, 3
rounds: the HIP-event time of one polish call (PairBatchRunner.polish: one launch, records, mask
and per-round records written) and of the erp_pair_batch_run with records (want = hyps, key_left,
key_right) whose outputs it reads -- same process, same stream, interleaved repetition by
repetition; their ratio; and the mean largest Euler error against euler_gt before (find's R) and
after (the polish's R) over the pairs whose status is ok.  Per repetition the polish is enqueued
--inner times between one event pair (a single call is too short for the event clock's
resolution to say much); reported: median, min, max over --reps and spread = (max - min) / median.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "spread": float((v.max() - v.min()) / np.median(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--kpts", type=int, default=1024)
    ap.add_argument("--mismatch", type=float, default=0.2)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--thr", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="polish calls per timed window")
    args = ap.parse_args()
    import torch
    import bench
    from erp_match_eightpoint_test_amd import (PairBatchRunner, polish_to_numpy, results_to_numpy,
                                               synth)
    assert torch.cuda.is_available(), "bench_polish needs a HIP device"
    dev = torch.device("cuda:0")
    pairs = bench._map_pairs(lambda k: synth.make_pair(args.seed + k, n_kpts=args.kpts,
                                                       mismatch_frac=args.mismatch), args.pairs)
    b = bench.to_device(pairs, dev)
    runner = PairBatchRunner(iters=args.iters, reuse_outputs=True)
    want = ("hyps", "key_left", "key_right")

    def feed():
        return runner.run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"],
                          b["width"], b["height"], b["max_nq"], b["max_nt"], want=want)

    def polish(outs):
        return runner.polish(outs, b["width"], b["height"], args.thr, rounds=args.rounds,
                             want_rounds=True)

    outs = feed()   # warm both shapes; the records of two runs must agree
    first = polish(outs)
    torch.cuda.synchronize()
    rec0 = {k: v.cpu().numpy().copy() for k, v in first.items()}
    t_feed, t_pol = [], []
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for _ in range(args.reps):
        ev[0].record()
        outs = feed()
        ev[1].record()
        ev[2].record()
        for _ in range(args.inner):
            pol = polish(outs)
        ev[3].record()
        torch.cuda.synchronize()
        t_feed.append(ev[0].elapsed_time(ev[1]))
        t_pol.append(ev[2].elapsed_time(ev[3]) / args.inner)
    identical = all(np.array_equal(rec0[k], pol[k].cpu().numpy()) for k in rec0)
    # accuracy only (untimed): the same records through the most rounds a call takes
    rec8 = polish_to_numpy(runner.polish(outs, b["width"], b["height"], args.thr, rounds=8)["polish"])
    res = results_to_numpy(outs["results"])
    rec = polish_to_numpy(pol["polish"])
    ok = res["status"] == 0
    gt = np.array([p["euler_gt"] for p in pairs])
    before = np.abs(res["R"].astype(np.float64) - gt).max(axis=1)[ok]
    after = np.abs(rec["R"].astype(np.float64) - gt).max(axis=1)[ok]
    M = res["M"][ok]
    row = {"bench": "polish", "pairs": args.pairs, "kpts": args.kpts, "mismatch_frac": args.mismatch,
           "iters": args.iters, "thr": args.thr, "rounds": args.rounds, "reps": args.reps,
           "inner": args.inner, "pairs_ok": int(ok.sum()),
           "M_mean": float(M.mean()), "M_min": int(M.min()), "M_max": int(M.max()),
           "polish_ms": stats(t_pol), "batch_run_records_ms": stats(t_feed),
           "polish_over_batch_run": float(np.median(t_pol) / np.median(t_feed)),
           "euler_err_mean_before_rad": float(before.mean()),
           "euler_err_mean_after_rad": float(after.mean()),
           "euler_err_median_before_rad": float(np.median(before)),
           "euler_err_median_after_rad": float(np.median(after)),
           "euler_err_mean_after_8_rounds_rad": float(
               np.abs(rec8["R"].astype(np.float64) - gt).max(axis=1)[ok].mean()),
           "rounds_done_hist_8_rounds": np.bincount(rec8["rounds_done"][ok], minlength=9).tolist(),
           "pairs_under_1deg_before": int((before < np.radians(1.0)).sum()),
           "pairs_under_1deg_after": int((after < np.radians(1.0)).sum()),
           "rounds_done_hist": np.bincount(rec["rounds_done"][ok], minlength=args.rounds + 1).tolist(),
           "inliers_mean_winner": float(rec["n_inliers_winner"][ok].mean()),
           "inliers_mean_final": float(rec["n_inliers"][ok].mean()),
           "hyps_bytes_read_max": int(args.pairs) * args.iters * 120,
           "records_identical": bool(identical),
           "lib": os.path.basename(os.environ.get("ERP_LIB_PATH", ""))}  # a development variant
    print(json.dumps(row))


if __name__ == "__main__":
    main()
