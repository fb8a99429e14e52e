#!/usr/bin/env python
"""Poses/s of a rotation sweep, images -> (R, T) + match error: PairBatchRunner.run_sweep (the
left image's features once, the rotated right images group by group on the device) against
today's route (erp_rotation.rotate_image per pose, the left image repeated P times,
run_images), same process, same images, same poses.

Images are synthetic and seeded, generated like bench_images.py's (a blob texture on the
sphere, upsampled, plus noise); the right base image is the left one, as in one_image_test,
and the poses are the first P of its {0, 5, 10, 15, 20}^3 degree grid in the driver's loop
order.  Nothing is read from disk.  For every (size, P):

  1. both routes run once (this warms the shape) and their records must be byte-equal;
  2. --steps timed steps per route, alternating sweep / today, each ended by a device
     synchronise; a step of today's route includes its P rotate_image calls and the stacking,
     which is what a user of it pays; reported: the median step and the min..max spread;
  3. `sweep_every_step_faster`: the slowest sweep step against the fastest step of today's route.

At the largest P of every size the match error alone (erp_match_error_dev on the sweep's
matched keypoints) is timed with device events over --me-calls calls.

Prints one JSON line per (size, P).  --only WxH:P restricts the shapes (repeatable);
--no-baseline times the sweep alone (for a profiler run) and skips the checks."""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_image(W, H, seed, dev):
    import torch
    from erp_match_eightpoint_test_amd import synth
    tex = torch.from_numpy(synth.sphere_texture(seed, H // 4, W // 4)).to(dev)
    up = torch.nn.functional.interpolate(tex.permute(2, 0, 1)[None].float(), size=(H, W),
                                         mode="bilinear", align_corners=False)
    g = torch.Generator(device=dev).manual_seed(seed * 1000)
    up = up + torch.randn(up.shape, device=dev, generator=g) * 3
    return up.clamp(0, 255).round().to(torch.uint8)[0].permute(1, 2, 0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", action="append", default=[], help="WxH:P (repeatable)")
    ap.add_argument("--me-calls", type=int, default=20)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    from erp_match_eightpoint_test_amd import (RESULT_DTYPE, Context, PairBatchRunner,
                                                erp_rotation, results_to_numpy)
    shapes = [(1344, 672, p) for p in (16, 64)] + [(5376, 2688, p) for p in (16, 64)]
    if args.only:
        shapes = []
        for o in args.only:
            wh, p = o.split(":")
            w, h = wh.split("x")
            shapes.append((int(w), int(h), int(p)))
    dev = torch.device("cuda:0")
    ctx = Context(0)
    er = erp_rotation(ctx=ctx)
    run = PairBatchRunner(ctx=ctx, iters=args.iters)
    grid = [np.radians(a) for a in itertools.product((0.0, 5.0, 10.0, 15.0, 20.0), repeat=3)]

    def sweep(left, base, mats, **kw):
        outs = run.run_sweep(left, base, mats, chunk=max(len(mats), 1), **kw)
        torch.cuda.synchronize()
        return outs

    def today(left, base, mats):
        rights = torch.stack([er.rotate_image(base, er.inv(m)) for m in mats])
        lefts = left.unsqueeze(0).repeat(len(mats), 1, 1, 1)
        outs = run.run_images(lefts, rights)
        torch.cuda.synchronize()
        return outs

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    def rate(ts, P):
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        return {"poses_per_s": P / med, "ms_per_step_median": med * 1e3,
                "ms_per_step_min": ts[0] * 1e3, "ms_per_step_max": ts[-1] * 1e3}

    images = {}
    largest = {(w, h): max(p for ww, hh, p in shapes if (ww, hh) == (w, h)) for w, h, _ in shapes}
    for W, H, P in shapes:
        if (W, H) not in images:
            images[(W, H)] = make_image(W, H, args.seed, dev)
        left = base = images[(W, H)]
        mats = np.stack([er.eular2rot(grid[p % len(grid)]) for p in range(P)])
        row = {"metric": "rotation sweep, images -> (R, T) + match error: run_sweep vs "
                         "rotate_image per pose + run_images", "unit": "poses/s", "W": W, "H": H,
               "P": P, "steps": args.steps, "iters": args.iters}
        outs = sweep(left, base, mats)                          # warms the shape
        row["groups"], row["max_nq"] = run.last_info["groups"], run.last_info["max_nq"]
        r = results_to_numpy(outs["results"])
        err = outs["match_error"].cpu().numpy()
        row["M"] = [int(x) for x in r["M"][:8]]
        row["match_error_rad"] = [float(x) for x in err[:8]]
        if not args.no_baseline:
            ref = today(left, base, mats)
            assert ref["results"].cpu().numpy().tobytes() == outs["results"].cpu().numpy().tobytes()
            row["check"] = {"poses": P, "records_bytes_equal": True,
                            "today_input_bytes": 2 * P * W * H * 3}
            del ref
        ts, tt = [], []
        for _ in range(args.steps):
            ts.append(timed(lambda: sweep(left, base, mats)))
            if not args.no_baseline:
                tt.append(timed(lambda: today(left, base, mats)))
        row["sweep"] = rate(ts, P)
        if tt:
            row["today"] = rate(tt, P)
            row["speedup"] = row["today"]["ms_per_step_median"] / row["sweep"]["ms_per_step_median"]
            row["sweep_every_step_faster"] = max(ts) < min(tt)
        if P == largest[(W, H)] and args.me_calls > 0:
            w = sweep(left, base, mats, want=("key_left", "key_right"))
            m_col = w["results"].view(torch.int32)[:, RESULT_DTYPE.fields["M"][1] // 4]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            er.match_error(w["key_left"], w["key_right"], m_col, mats, W, H)
            e0.record()
            for _ in range(args.me_calls):
                me = er.match_error(w["key_left"], w["key_right"], m_col, mats, W, H)
            e1.record()
            torch.cuda.synchronize()
            assert me.cpu().numpy().tobytes() == outs["match_error"].cpu().numpy().tobytes()
            row["match_error_us_per_call"] = e0.elapsed_time(e1) * 1e3 / args.me_calls
        print(json.dumps(row), flush=True)
        print(f"{W}x{H} P={P}: sweep {row['sweep']['ms_per_step_median']:.1f} ms"
              + (f", today {row['today']['ms_per_step_median']:.1f} ms" if tt else ""),
              file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
