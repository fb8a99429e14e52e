#!/usr/bin/env python
"""What a shared rand stream costs: the headline shape as bench.py runs it (768 pairs, 6
sub-batches on 6 HIP streams with a context each, 10k iterations), once with no stream and
once with all contexts on ONE shared RandStream, interleaved on the same box, three runs
each; the single-pair latency (HIP-graph replay) both ways; and the stream kernels' time per
launch from the stage timer (they are timed under jump_prep: the difference of that stage with
and without a stream).

  python scripts/bench_stream.py [--pairs 768] [--streams 6] [--iters 10000] [--kpts 4096]
                                 [--steps 5] [--warmup 2] [--runs 3] [--out FILE]

Prints one JSON line per measurement (and appends them to --out)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=768)
    ap.add_argument("--streams", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--kpts", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--latency-calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import bench
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, RandStream, results_to_numpy

    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        lines.append(line)

    pairs = bench.make_batch(0, args.pairs, args.kpts, 20200423)
    S = max(1, min(args.streams, args.pairs))
    parts = [pairs[i * args.pairs // S:(i + 1) * args.pairs // S] for i in range(S)]
    subs = []
    for part in parts:
        b = bench.to_device(part, dev)
        ctx = Context(0)
        runner = PairBatchRunner(ctx=ctx, iters=args.iters)
        runner.reserve(len(part), b["max_nq"], b["max_nt"])
        subs.append(dict(b=b, ctx=ctx, runner=runner, stream=torch.cuda.Stream(dev)))
    shared = RandStream(1, 0)

    def attach(on: bool):
        for sb in subs:
            sb["ctx"].set_rand_stream(shared if on else None)

    def run_sub(sb):
        b = sb["b"]
        with torch.cuda.stream(sb["stream"]):
            sb["out"] = sb["runner"].run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"],
                                         b["off_l"], b["off_r"], b["width"], b["height"],
                                         b["max_nq"], b["max_nt"], stream=sb["stream"].cuda_stream)

    def step():
        for sb in subs:
            run_sub(sb)

    def timed(on: bool) -> float:
        attach(on)
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return args.pairs * args.steps / (time.perf_counter() - t0)

    for run in range(args.runs):  # interleaved: plain, stream, plain, stream, ...
        for on in (False, True):
            emit(metric="pairs_per_s", rand_stream=on, run=run, value=round(timed(on), 1),
                 pairs=args.pairs, streams=S, iters=args.iters, kpts=args.kpts, steps=args.steps)
    st = results_to_numpy(torch.cat([sb["out"]["results"] for sb in subs]))
    emit(metric="draws_consumed", value=shared.draws, statuses_ok=int((st["status"] == 0).sum()))

    # the stream kernels' time: the jump_prep stage with and without a stream, sub-batches one
    # after the other (standalone launches)
    for on in (False, True):
        attach(on)
        for sb in subs:
            sb["ctx"].set_profiling(True)
        tot, n = 0.0, 0
        for sb in subs:
            run_sub(sb)
            sb["stream"].synchronize()
            ms, k = sb["ctx"].stage_times()["jump_prep"]
            tot, n = tot + ms, n + 1
        for sb in subs:
            sb["ctx"].set_profiling(False)
        emit(metric="jump_prep_ms_per_sub_batch", rand_stream=on, value=round(tot / n, 4),
             pairs_per_launch=len(parts[0]))
    attach(False)

    # single pair, HIP-graph replay (bench.py's latency shape), both ways
    one = bench.to_device(pairs[:1], dev)
    for on in (False, True, False, True):
        ctx = Context(0)
        ctx.set_graphs(True)
        if on:
            ctx.set_rand_stream(shared)
        r = PairBatchRunner(ctx=ctx, iters=args.iters, reuse_outputs=True)
        s = torch.cuda.Stream(dev)

        def call():
            r.run(one["desc_l"], one["desc_r"], one["kp_l"], one["kp_r"], one["off_l"],
                  one["off_r"], one["width"], one["height"], one["max_nq"], one["max_nt"],
                  stream=s.cuda_stream)
        with torch.cuda.stream(s):
            for _ in range(5):
                call()
            s.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.latency_calls):
                call()
                s.synchronize()
            dt = (time.perf_counter() - t0) / args.latency_calls
        emit(metric="single_pair_ms", rand_stream=on, value=round(dt * 1e3, 4), iters=args.iters,
             graphs=True)
        ctx.set_rand_stream(None)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
