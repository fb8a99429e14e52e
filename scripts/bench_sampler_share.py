#!/usr/bin/env python
"""Shared replays (Context option sampler_share) on one 128-pair launch:
the serial stage times of the alias table's producers and consumer (jump_prep, windows, sampler,
gram) with sharing on (-1) against off (0), in one process and one build, the two contexts
interleaved, and how many distinct match counts the launch holds -- the saving is the share of
pairs that repeat a count within the launch, so both ends are measured:

  --batch distinct  128 pairs with pairwise distinct M = --base .. --base + pairs - 1 (exact
                    counts: synth.make_pair(n_kpts=M, inlier_frac=1.0, sigma=0.005)): the alias
                    table is the identity, sharing must cost nothing measurable
  --batch bench     the first sub-batch of bench.py's default batch (4096 keypoints, M ~ 2689)
  --batch hard | worst   the first sub-batch of bench.py's hard / worst-case batch

Each repetition runs every variant once with stage timing on (HIP events around each stage, the
launches serial on one stream); reported per stage: median, min and max over --reps, and spread
= (max - min) / median.  The records of the two variants must be byte-identical.

--count-batches instead runs bench.py's default, hard and worst-case batches once (768 pairs in
six sub-batches of 128, as the bench launches them) and prints the distinct match counts per
sub-batch.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = ("jump_prep", "windows", "sampler", "gram")


def run_once(runner, b, want=()):
    import torch
    o = runner.run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"],
                   b["width"], b["height"], b["max_nq"], b["max_nt"], want=want)
    torch.cuda.synchronize()
    return o


def bench_batches(args):
    import bench
    return {"bench": lambda n: bench.make_batch(0, n, args.kpts, args.seed, 0.8, 0.03),
            "hard": lambda n: bench.make_batch(0, n, args.kpts, args.seed + 7777, 0.5, 0.035, 0.3),
            "worst": lambda n: bench.make_worst_batch(0, n, args.kpts, 0.03)}


def count_batches(args, dev):
    import bench
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    out = {}
    runner = PairBatchRunner(ctx=Context(0), iters=64)  # (the counts come from the matcher)
    for name, make in bench_batches(args).items():
        pairs = make(args.total)
        S = args.total // args.pairs
        rows = []
        for i in range(S):
            b = bench.to_device(pairs[i * args.pairs:(i + 1) * args.pairs], dev)
            M = results_to_numpy(run_once(runner, b)["results"])["M"]
            rows.append({"pairs": int(M.size), "distinct": int(np.unique(M).size),
                         "M_min": int(M.min()), "M_max": int(M.max())})
        out[name] = {"sub_batches": rows, "pairs": sum(r["pairs"] for r in rows),
                     "replays_needed": sum(r["distinct"] for r in rows)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", choices=["distinct", "bench", "hard", "worst"], default="distinct")
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--base", type=int, default=2625, help="distinct: the smallest M")
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--count-batches", action="store_true")
    ap.add_argument("--total", type=int, default=768, help="--count-batches: pairs per batch")
    args = ap.parse_args()
    import torch
    import bench
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy, synth
    dev = torch.device("cuda:0")
    if args.count_batches:
        print(json.dumps({"distinct_match_counts": count_batches(args, dev)}))
        return
    if args.batch == "distinct":
        pairs = bench._map_pairs(lambda k: synth.make_pair(args.seed + k, n_kpts=args.base + k,
                                                           inlier_frac=1.0, sigma=0.005),
                                 args.pairs)
    else:
        pairs = bench_batches(args)[args.batch](args.pairs)
    b = bench.to_device(pairs, dev)
    variants = {}
    for name, share in (("share", -1), ("own", 0)):
        ctx = Context(0)
        ctx.set_option("sampler_share", share)
        runner = PairBatchRunner(ctx=ctx, iters=args.iters)
        runner.reserve(args.pairs, b["max_nq"], b["max_nt"])
        variants[name] = (ctx, runner)
    recs = {}
    for name, (ctx, runner) in variants.items():  # warm the shape; the records must agree
        recs[name] = run_once(runner, b)["results"].cpu().numpy().copy()
    assert np.array_equal(recs["share"], recs["own"]), "records differ between the variants"
    M = results_to_numpy(torch.from_numpy(recs["share"]))["M"]
    times = {name: {s: [] for s in STAGES} for name in variants}
    for _ in range(args.reps):
        for name, (ctx, runner) in variants.items():
            ctx.set_profiling(True)
            run_once(runner, b)
            st = ctx.stage_times()
            ctx.set_profiling(False)
            for s in STAGES:
                times[name][s].append(st[s][0])
    row = {"batch": args.batch, "pairs": args.pairs, "iters": args.iters,
           "distinct_M": int(np.unique(M).size), "M_min": int(M.min()), "M_max": int(M.max()),
           "reps": args.reps, "records_identical": True, "stages_ms": {}}
    for name in variants:
        row["stages_ms"][name] = {}
        for s in STAGES:
            v = np.array(times[name][s])
            row["stages_ms"][name][s] = {"median": float(np.median(v)), "min": float(v.min()),
                                         "max": float(v.max()),
                                         "spread": float((v.max() - v.min()) / np.median(v))}
    print(json.dumps(row))


if __name__ == "__main__":
    main()
