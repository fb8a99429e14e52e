#!/usr/bin/env python
"""Winner records (erp_pair_batch_run_winners) against the records route
they replace, as the feed of the polish stage.

Two routes, interleaved repetition by repetition in one process on one stream, HIP events:
  (a) records  erp_pair_batch_run with out->hyps (want = hyps, key_left, key_right), then
               erp_polish_dev on the records;
  (b) winners  erp_pair_batch_run_winners on the lite route (want = winners, key_left,
               key_right), then erp_polish_winners_dev.
Two shapes: scripts/bench_polish.py's (256 pairs of synth.make_pair(n_kpts=1024,
mismatch_frac=0.2), 1000 iterations) and the headline's (768 pairs, 4096 keypoints, 10 000
iterations, bench.py's batch).  thr 0.01, 3 rounds.  Per route and shape: the batch run, the
polish (--inner calls per timed window: one call is short for the event clock) and their sum;
median, min, max over --reps and spread = (max - min) / median.  The two routes' polish outputs
(records, per-round records, masks) must be byte-identical: asserted.  Writes one JSON document
(--out) and prints it."""
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
    from erp_match_eightpoint_test_amd import (PairBatchRunner, polish_to_numpy, results_to_numpy,
                                               synth, winners_to_numpy)
    dev = torch.device("cuda:0")
    if shape["mismatch"] > 0:
        pairs = bench._map_pairs(lambda k: synth.make_pair(args.seed + k, n_kpts=shape["kpts"],
                                                           mismatch_frac=shape["mismatch"]),
                                 shape["pairs"])
    else:
        pairs = bench.make_batch(0, shape["pairs"], shape["kpts"], args.seed)
    b = bench.to_device(pairs, dev)
    # one runner (context) per route: each keeps its own outputs and scratch
    routes = {"records": (PairBatchRunner(iters=shape["iters"], reuse_outputs=True),
                          ("hyps", "key_left", "key_right")),
              "winners": (PairBatchRunner(iters=shape["iters"], reuse_outputs=True),
                          ("winners", "key_left", "key_right"))}

    def feed(route):
        runner, want = routes[route]
        return runner.run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"],
                          b["width"], b["height"], b["max_nq"], b["max_nt"], want=want)

    def polish(route, outs):
        return routes[route][0].polish(outs, b["width"], b["height"], args.thr, rounds=args.rounds,
                                       want_rounds=True)

    t = {r: {"run": [], "polish": [], "total": []} for r in routes}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    last = {}
    for rep in range(-1, args.reps):  # (rep -1 warms both routes)
        for route in routes:
            ev[0].record()
            outs = feed(route)
            ev[1].record()
            ev[2].record()
            for _ in range(args.inner):
                pol = polish(route, outs)
            ev[3].record()
            torch.cuda.synchronize()
            last[route] = (outs, pol)
            if rep < 0:
                continue
            run_ms = ev[0].elapsed_time(ev[1])
            pol_ms = ev[2].elapsed_time(ev[3]) / args.inner
            t[route]["run"].append(run_ms)
            t[route]["polish"].append(pol_ms)
            t[route]["total"].append(run_ms + pol_ms)
    (o_r, p_r), (o_w, p_w) = last["records"], last["winners"]
    for f in ("polish", "rounds", "mask"):
        assert torch.equal(p_r[f], p_w[f]), f"{name}: polish output {f} differs between the routes"
    assert torch.equal(o_r["results"], o_w["results"]), f"{name}: result records differ"
    res = results_to_numpy(o_w["results"])
    win = winners_to_numpy(o_w["winners"])
    ok = res["status"] == 0
    assert (win["status"] == res["status"]).all(), f"{name}: a winner record failed its self-check"
    rec = polish_to_numpy(p_w["polish"])
    med = lambda r, k: float(np.median(t[r][k]))  # noqa: E731
    return {"shape": name, **shape, "thr": args.thr, "rounds": args.rounds, "reps": args.reps,
            "inner": args.inner, "pairs_ok": int(ok.sum()), "M_mean": float(res["M"][ok].mean()),
            "records_ms": {k: stats(v) for k, v in t["records"].items()},
            "winners_ms": {k: stats(v) for k, v in t["winners"].items()},
            "winners_over_records": {k: med("winners", k) / med("records", k)
                                     for k in ("run", "polish", "total")},
            "hyps_bytes": int(shape["pairs"]) * shape["iters"] * 120,
            "winner_bytes": int(shape["pairs"]) * 88,
            "rounds_done_hist": np.bincount(rec["rounds_done"][ok],
                                            minlength=args.rounds + 1).tolist(),
            "polish_outputs_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="polish,headline")
    ap.add_argument("--thr", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10, help="polish calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_bench_winners.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_winners needs a HIP device"
    doc = {"bench": "winners", "device": torch.cuda.get_device_name(0),
           "lib": os.path.basename(os.environ.get("ERP_LIB_PATH", "")),  # a development variant
           "shapes": [measure(n, SHAPES[n], args) for n in args.shapes.split(",")]}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
