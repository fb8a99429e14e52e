#!/usr/bin/env python
"""The pose selection (erp_pose_select_dev) next to the calls that feed it.

Per shape, in one process on one stream, HIP events, interleaved repetition by repetition:
  run      erp_pair_batch_run_winners on the lite route (want = winners, key_left, key_right);
  polish   erp_polish_winners_dev, thr 0.01, 3 rounds (--inner calls per timed window);
  pose     erp_pose_select_dev from the polish's E and mask (thr 0), once with every optional
           output (depth, front, results_out) and once with none of them (pass 2 skipped);
  pose_w   the same from the winner records with thr (no mask), every optional output.
Two shapes: scripts/bench_polish.py's (256 pairs of synth.make_pair(n_kpts=1024,
mismatch_frac=0.2), 1000 iterations) and the headline's (768 pairs, 4096 keypoints, 10 000
iterations, bench.py's batch).  Median, min, max over --reps and spread = (max - min) / median;
the pose records of the first and the last repetition must be byte-identical: asserted.  Also
reported: how the votes fell (pairs whose pose differs from find's rotation / T sign).  Writes
one JSON document (--out) and prints it."""
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
    from erp_match_eightpoint_test_amd import (PairBatchRunner, pose_to_numpy, results_to_numpy,
                                               synth)
    dev = torch.device("cuda:0")
    if shape["mismatch"] > 0:
        pairs = bench._map_pairs(lambda k: synth.make_pair(args.seed + k, n_kpts=shape["kpts"],
                                                           mismatch_frac=shape["mismatch"]),
                                 shape["pairs"])
    else:
        pairs = bench.make_batch(0, shape["pairs"], shape["kpts"], args.seed)
    b = bench.to_device(pairs, dev)
    runner = PairBatchRunner(iters=shape["iters"], reuse_outputs=True)

    def feed():
        return runner.run(b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"],
                          b["width"], b["height"], b["max_nq"], b["max_nt"],
                          want=("winners", "key_left", "key_right"))

    def polish(outs):
        return runner.polish(outs, b["width"], b["height"], args.thr, rounds=args.rounds)

    def pose(outs, pol, want):
        return runner.select_pose(outs, b["width"], b["height"], source="polish", polish=pol,
                                  min_sin2=args.min_sin2, want=want)

    def pose_w(outs):
        return runner.select_pose(outs, b["width"], b["height"], source="winners", thr=args.thr,
                                  min_sin2=args.min_sin2)

    full = ("depth", "front", "results")
    t = {k: [] for k in ("run", "polish", "pose", "pose_record_only", "pose_w")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
    first = None
    for rep in range(-1, args.reps):  # (rep -1 warms every call)
        ev[0].record()
        outs = feed()
        ev[1].record()
        ev[2].record()
        for _ in range(args.inner):
            pol = polish(outs)
        ev[3].record()
        ev[4].record()
        for _ in range(args.inner):
            sel = pose(outs, pol, full)
        ev[5].record()
        ev[6].record()
        for _ in range(args.inner):
            pose(outs, pol, ())
        ev[7].record()
        ev[8].record()
        for _ in range(args.inner):
            sel_w = pose_w(outs)
        ev[9].record()
        torch.cuda.synchronize()
        if first is None:
            first = {k: v.clone() for k, v in sel.items()}
        if rep < 0:
            continue
        t["run"].append(ev[0].elapsed_time(ev[1]))
        for k, i in (("polish", 2), ("pose", 4), ("pose_record_only", 6), ("pose_w", 8)):
            t[k].append(ev[i].elapsed_time(ev[i + 1]) / args.inner)
    for k in first:
        assert torch.equal(first[k], sel[k]), f"{name}: pose output {k} differs between runs"
    res = results_to_numpy(outs["results"])
    rec, rec_w = pose_to_numpy(sel["pose"]), pose_to_numpy(sel_w["pose"])
    ok = rec["status"] == 0
    med = lambda k: float(np.median(t[k]))  # noqa: E731
    feeders = med("run") + med("polish")
    return {"shape": name, **shape, "thr": args.thr, "rounds": args.rounds,
            "min_sin2": args.min_sin2, "reps": args.reps, "inner": args.inner,
            "pairs_find_ok": int((res["status"] == 0).sum()), "pairs_pose_ok": int(ok.sum()),
            "M_mean": float(res["M"][res["status"] == 0].mean()),
            "ms": {k: stats(v) for k, v in t.items()},
            "pose_over_run_plus_polish": med("pose") / feeders,
            "pose_over_polish": med("pose") / med("polish"),
            "voters_mean": float(rec["n_voters"][ok].mean()),
            "winning_vote_share_mean": float((rec["votes"][ok].max(axis=1)
                                              / np.maximum(rec["n_voters"][ok], 1)).mean()),
            "candidate_hist": np.bincount(2 * rec["which"][ok] + (rec["t_sign"][ok] < 0),
                                          minlength=4).tolist(),
            "pairs_t_flipped": int(rec["t_flipped"][ok].sum()),
            "pairs_rot_agrees_from_winners": int(rec_w["rot_agrees"][rec_w["status"] == 0].sum()),
            "pairs_pose_ok_from_winners": int((rec_w["status"] == 0).sum()),
            "pose_outputs_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="polish,headline")
    ap.add_argument("--thr", type=float, default=0.01)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-sin2", dest="min_sin2", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=20200423)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--inner", type=int, default=10, help="stage calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17a_bench_pose.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pose needs a HIP device"
    doc = {"bench": "pose", "device": torch.cuda.get_device_name(0),
           "lib": os.path.basename(os.environ.get("ERP_LIB_PATH", "")),  # a development variant
           "shapes": [measure(n, SHAPES[n], args) for n in args.shapes.split(",")]}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
