#!/usr/bin/env python
"""The last stage of automatic's main (src/automatic.cpp:138-160) for P pairs: the batched
calls (erp_rotation.rectify_batch / vertical_rotate_batch) against the route of the per-pair
entry points, a loop of rectify + 2 x vertical_rotate per pair.  Same process, same images,
the variants interleaved.

Images are synthetic and seeded (an integer texture plus noise, generated on the device); the
poses are P generic float32-valued (R, T).  For every (size, P):

  1. every variant runs once (this warms the shape) and the batched outputs must be
     byte-identical to the loop's, on both routes of the vertical stage
     (Context option vertical_shared = 1: the shared-map kernel; 0: ROT90 jobs of remap_kernel);
  2. --reps repetitions; each runs every variant once, in turn, as --inner back-to-back calls
     ended by a device synchronise.  Reported per variant: the median time of one call, min and
     max over the repetitions, and spread = (max - min) / median.

Variants: rectify_batch (vertical=False) | rectify_loop (P x rectify) | vertical_shared,
vertical_rot90 (vertical_rotate_batch over the 2 P rectified images, either route) |
vertical_loop (2 P x vertical_rotate) | vertical_shared_kernel (the same call into a caller's
output with fill = -1: no pre-fill, the launch alone) | all_batch (rectify_batch, vertical=True)
| all_loop.  hbm_fraction = 6 bytes x pixels x images / time / 8 TB/s for the kernel-only variant.

Prints one JSON line.  --only WxH:P restricts the shapes (repeatable)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def make_images(W, H, n, seed, dev):
    import torch
    y = torch.arange(H, device=dev)[:, None]
    x = torch.arange(W, device=dev)[None, :]
    base = torch.stack([(x * 7 + y * 3) % 256, (x * 2 + y * 11) % 256, (x ^ y) % 256], -1)
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    for i in range(n):
        noise = torch.randint(0, 16, (H, W, 3), device=dev, generator=g)
        out[i] = ((base + noise + 31 * i) % 256).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", action="append", default=[], help="WxH:P (repeatable)")
    args = ap.parse_args()
    import torch
    from erp_match_eightpoint_test_amd import Context, erp_rotation
    shapes = [(5376, 2688, 1), (5376, 2688, 8)]
    if args.only:
        shapes = []
        for o in args.only:
            wh, p = o.split(":")
            w, h = wh.split("x")
            shapes.append((int(w), int(h), int(p)))
    dev = torch.device("cuda:0")
    ctx = Context(0)
    er = erp_rotation(ctx=ctx)
    rng = np.random.default_rng(args.seed)
    rows = []
    for W, H, P in shapes:
        lefts = make_images(W, H, P, args.seed, dev)
        rights = make_images(W, H, P, args.seed + 1, dev)
        rv = rng.uniform(-0.3, 0.3, (P, 3)).astype(np.float32).astype(np.float64)
        tv = rng.standard_normal((P, 3))
        tv = (tv / np.linalg.norm(tv, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        rect = er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv, vertical=False)
        stack = torch.cat([rect["left_rectified"], rect["right_rectified"]]).contiguous()
        mine = torch.zeros((2 * P, W, H, 3), dtype=torch.uint8, device=dev)

        def rectify_loop():
            return [er.rectify(lefts[p], rights[p], rv[p], tv[p]) for p in range(P)]

        def vertical_loop():
            return [er.vertical_rotate(stack[i]) for i in range(2 * P)]

        def vertical_route(shared):
            ctx.set_option("vertical_shared", shared)
            try:
                return er.vertical_rotate_batch(stack)
            finally:
                ctx.set_option("vertical_shared", 1)

        def all_loop():
            out = []
            for p in range(P):
                lo, ro = er.rectify(lefts[p], rights[p], rv[p], tv[p])
                out.append((lo, ro, er.vertical_rotate(lo), er.vertical_rotate(ro)))
            return out

        variants = {
            "rectify_batch": lambda: er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv,
                                                      vertical=False),
            "rectify_loop": rectify_loop,
            "vertical_shared": lambda: vertical_route(1),
            "vertical_rot90": lambda: vertical_route(0),
            "vertical_loop": vertical_loop,
            "vertical_shared_kernel": lambda: er.vertical_rotate_batch(stack, fill=-1, out=mine),
            "all_batch": lambda: er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv),
            "all_loop": all_loop,
        }
        # 1. warm every variant; the bytes of the batched calls are the loop's
        warm = {k: f() for k, f in variants.items()}
        torch.cuda.synchronize()
        vl = torch.stack(warm["vertical_loop"])
        assert torch.equal(warm["vertical_shared"], vl) and torch.equal(warm["vertical_rot90"], vl)
        assert torch.equal(mine, vl)  # unwritten pixels keep the caller's 0, the loop's fill
        rl = warm["rectify_loop"]
        assert torch.equal(warm["rectify_batch"]["left_rectified"], torch.stack([a for a, _ in rl]))
        assert torch.equal(warm["rectify_batch"]["right_rectified"], torch.stack([b for _, b in rl]))
        al = warm["all_loop"]
        for i, k in enumerate(("left_rectified", "right_rectified", "left_vertical",
                               "right_vertical")):
            assert torch.equal(warm["all_batch"][k], torch.stack([t[i] for t in al])), k
        del warm, vl, rl, al
        # 2. interleaved repetitions
        ts = {k: [] for k in variants}
        for _ in range(args.reps):
            for k, f in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    f()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) / args.inner)
        row = {"W": W, "H": H, "P": P, "bytes_identical": True}
        for k, v in ts.items():
            v = sorted(v)
            med = v[len(v) // 2]
            row[k] = {"ms": med * 1e3, "ms_min": v[0] * 1e3, "ms_max": v[-1] * 1e3,
                      "spread": (v[-1] - v[0]) / med}
        px_images = 2.0 * P * W * H
        row["vertical_shared_kernel"]["hbm_fraction"] = (
            6.0 * px_images / (row["vertical_shared_kernel"]["ms"] * 1e-3) / HBM_BYTES_PER_S)
        row["vertical_loop"]["hbm_fraction"] = (
            9.0 * px_images / (row["vertical_loop"]["ms"] * 1e-3) / HBM_BYTES_PER_S)  # + the fill
        row["vertical_loop_over_shared"] = row["vertical_loop"]["ms"] / row["vertical_shared"]["ms"]
        row["vertical_loop_over_rot90"] = row["vertical_loop"]["ms"] / row["vertical_rot90"]["ms"]
        row["rectify_loop_over_batch"] = row["rectify_loop"]["ms"] / row["rectify_batch"]["ms"]
        row["all_loop_over_batch"] = row["all_loop"]["ms"] / row["all_batch"]["ms"]
        rows.append(row)
        print(f"{W}x{H} P={P}: vertical loop / shared = {row['vertical_loop_over_shared']:.2f}",
              file=sys.stderr, flush=True)
        del lefts, rights, rect, stack, mine
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "batched rectification (rectify_batch, vertical_rotate_batch) vs "
                                "the per-pair loop of rectify + 2 x vertical_rotate",
                      "unit": "ms per call (median of reps; each rep = inner calls + one sync)",
                      "reps": args.reps, "inner": args.inner, "shapes": rows}))


if __name__ == "__main__":
    main()
