#!/usr/bin/env python
"""Guided matching (erp_match_guided_dev) next to the calls that feed it
and to the exact sweep over the same batch.

Per shape, in one process on one stream, HIP events, interleaved repetition by repetition:
  run      erp_pair_batch_run_winners on the lite route (want = winners, key_left, key_right);
  polish   erp_polish_winners_dev, thr 0.01, 3 rounds (--inner calls per timed window);
  guided   erp_match_guided_dev from the polish's E, ratio 0.8, max_dist 0.8, unique, every
           optional output, once per gate threshold of --thrs (0.003 and 0.01);
  sweep    the exact sweep of the same batch (ERP_MATCHER_VALU_EXACT: every distance, stage
           ERP_STAGE_KNN2_EXACT of the stage timer) on a second context that enqueues the
           matcher group only -- it computes nq x nt distances, the guided stage the gated few
           per cent of them plus nq x nt gate tests.
Two shapes: 256 pairs of synth.make_pair(n_kpts=1024, mismatch_frac=0.2), 1000 iterations, and
the headline's (768 pairs, 4096 keypoints, 10 000 iterations, bench.py's batch).  Median, min,
max over --reps and spread = (max - min) / median; the guided outputs of the first and the last
repetition must be byte-identical: asserted.  Also reported: the plain and the guided match
counts, how many guided matches sit at the true partner, the gated share of the nq x nt tests.
Writes one JSON document (--out) and prints it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"polish": dict(pairs=256, kpts=1024, iters=1000, mismatch=0.2),
          "headline": dict(pairs=768, kpts=4096, iters=10000, mismatch=0.0)}


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "spread": float((v.max() - v.min()) / np.median(v))}


def measure(name, shape, args):
    import torch
    import bench
    from erp_match_eightpoint_test_amd import (Context, PairBatchRunner, capi, polish_to_numpy,
                                               results_to_numpy, synth)
    dev = torch.device("cuda:0")
    if shape["mismatch"] > 0:
        pairs = bench._map_pairs(lambda k: synth.make_pair(args.seed + k, n_kpts=shape["kpts"],
                                                           mismatch_frac=shape["mismatch"]),
                                 shape["pairs"])
    else:
        pairs = bench.make_batch(0, shape["pairs"], shape["kpts"], args.seed)
    b = bench.to_device(pairs, dev)
    batch = (b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"], b["width"],
             b["height"], b["max_nq"], b["max_nt"])
    runner = PairBatchRunner(iters=shape["iters"], reuse_outputs=True)
    # the exact sweep: a context of its own with the stage timer on and the matcher group only
    sweep_ctx = Context(0)
    sweep_ctx.set_matcher(capi.MATCHER_VALU_EXACT)
    sweep_ctx.set_option("debug_stages", 1)
    sweep_ctx.set_profiling(True)
    sweeper = PairBatchRunner(ctx=sweep_ctx, iters=shape["iters"], reuse_outputs=True)
    thrs = [float(t) for t in args.thrs.split(",")]

    def guided(outs, pol, thr):
        return runner.guided_match(outs, *batch, source="polish", polish=pol, thr=thr,
                                   ratio=args.ratio, max_dist=args.max_dist, unique=True)

    t = {"run": [], "polish": [], "sweep": [], **{f"guided_{thr}": [] for thr in thrs}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4 + 2 * len(thrs))]
    first, last = None, {}
    for rep in range(-1, args.reps):  # (rep -1 warms every call)
        ev[0].record()
        outs = runner.run(*batch, want=("winners", "key_left", "key_right"))
        ev[1].record()
        ev[2].record()
        for _ in range(args.inner):
            pol = runner.polish(outs, b["width"], b["height"], args.polish_thr, rounds=args.rounds)
        ev[3].record()
        for k, thr in enumerate(thrs):
            ev[4 + 2 * k].record()
            for _ in range(args.inner):
                last[thr] = guided(outs, pol, thr)
            ev[5 + 2 * k].record()
        torch.cuda.synchronize()
        sweeper.run(*batch)
        torch.cuda.synchronize()
        sweep_ms = sweep_ctx.stage_times()["knn2_exact"][0]
        if first is None:
            first = {thr: {k: v.clone() for k, v in last[thr].items()} for thr in thrs}
        if rep < 0:
            continue
        t["run"].append(ev[0].elapsed_time(ev[1]))
        t["polish"].append(ev[2].elapsed_time(ev[3]) / args.inner)
        t["sweep"].append(sweep_ms)
        for k, thr in enumerate(thrs):
            t[f"guided_{thr}"].append(ev[4 + 2 * k].elapsed_time(ev[5 + 2 * k]) / args.inner)
    for thr in thrs:
        for k in first[thr]:
            assert torch.equal(first[thr][k], last[thr][k]), \
                f"{name}: guided output {k} at thr {thr} differs between runs"
    res = results_to_numpy(outs["results"])
    ok = (res["status"] == 0) & (polish_to_numpy(pol["polish"])["status"] == 0)
    med = lambda k: float(np.median(t[k]))  # noqa: E731
    tests = float(sum(len(p["desc_l"]) * len(p["desc_r"]) for p in pairs))
    per_thr = {}
    for thr in thrs:
        g = last[thr]
        cnt = g["count"].cpu().numpy()
        m = g["matches"].cpu().numpy().view(capi.DMATCH_DTYPE).reshape(len(pairs), -1)
        correct = [int((pairs[i]["gt_partner"][m[i, :cnt[i]]["queryIdx"]]
                        == m[i, :cnt[i]]["trainIdx"]).sum()) for i in range(len(pairs))]
        per_thr[str(thr)] = {
            "ms": stats(t[f"guided_{thr}"]),
            "over_run_plus_polish": med(f"guided_{thr}") / (med("run") + med("polish")),
            "over_exact_sweep": med(f"guided_{thr}") / med("sweep"),
            "matches_mean": float(cnt[ok].mean()) if ok.any() else 0.0,
            "at_true_partner_mean": float(np.asarray(correct)[ok].mean()) if ok.any() else 0.0,
            "gated_share": float(g["gated"].cpu().numpy().sum() / tests)}
    return {"shape": name, **shape, "polish_thr": args.polish_thr, "rounds": args.rounds,
            "ratio": args.ratio, "max_dist": args.max_dist, "reps": args.reps, "inner": args.inner,
            "pairs_ok": int(ok.sum()),
            "plain_matches_mean": float(res["M"][ok].mean()) if ok.any() else 0.0,
            "true_partners_mean": float(np.mean([(p["gt_partner"] >= 0).sum() for p in pairs])),
            "ms": {k: stats(t[k]) for k in ("run", "polish", "sweep")}, "guided": per_thr,
            "guided_outputs_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="polish,headline")
    ap.add_argument("--thrs", default="0.003,0.01", help="gate thresholds of the guided stage")
    ap.add_argument("--ratio", type=float, default=0.8)
    ap.add_argument("--max-dist", dest="max_dist", type=float, default=0.8)
    ap.add_argument("--polish-thr", dest="polish_thr", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3, help="stage calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18a_bench_guided.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_guided needs a HIP device"
    doc = {"bench": "guided", "device": torch.cuda.get_device_name(0),
           "lib": os.environ.get("ERP_LIB_PATH", ""),  # a development variant
           "shapes": [measure(n, SHAPES[n], args) for n in args.shapes.split(",")]}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
