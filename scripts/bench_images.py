#!/usr/bin/env python
"""Image pairs/s from ERP images to (R, T): the batched route (PairBatchRunner.run_images:
bands -> SURF -> pack -> match -> gather -> find for B pairs in one call) against the per-pair
route (spherical_surf.do_all + eight_point.find in a loop), same process, same images.

Images are synthetic and seeded, generated like bench.py's e2e workload (a blob texture on the
sphere, upsampled, plus noise; right = rotate_image(left, R^-1) for a small known rotation);
nothing is read from disk.  For every (size, B):

  1. both routes run once (this warms the shape) and must agree: M equal, R and T within 1e-6,
     for every pair; the packed tensors of pair 0 must be byte-equal to the per-pair assembly
     (bands -> surf_dev -> unrotate_band_keypoints -> cat);
  2. --steps timed steps per route, alternating batched / per-pair, each ended by a device
     synchronise; reported: pairs/s of the median step and the min..max spread;
  3. at the largest B of the largest size, the group size A/B: max_group_pairs in --groups
     (at 5376 x 2688 SURF scratch is ~1 GB per pair, so 4 / 8 / 16 pairs ~ 4 / 8 / 16 GiB).

Prints one JSON line.  --only WxH:B restricts the shapes (repeatable); --no-baseline times the
batched route alone (for a profiler run) and skips the checks."""
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


def make_pairs(W, H, B, seed, er, dev, n_tex=4):
    import torch
    from erp_match_eightpoint_test_amd import synth
    rng = np.random.default_rng(seed)
    tex = [torch.from_numpy(synth.sphere_texture(seed + k, H // 4, W // 4)).to(dev)
           .permute(2, 0, 1)[None].float() for k in range(min(B, n_tex))]
    lefts = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    rights = torch.empty_like(lefts)
    for b in range(B):
        up = torch.nn.functional.interpolate(tex[b % len(tex)], size=(H, W), mode="bilinear",
                                             align_corners=False)
        g = torch.Generator(device=dev).manual_seed(seed * 1000 + b)
        up = up + torch.randn(up.shape, device=dev, generator=g) * 3
        lefts[b] = up.clamp(0, 255).round().to(torch.uint8)[0].permute(1, 2, 0)
        R = er.eular2rot(np.radians(rng.uniform(0, 15, 3)))
        rights[b] = er.rotate_image(lefts[b], er.inv(R))
    return lefts, rights


def assemble_pair(ss, fm, left, right, W, H):
    """the per-pair assembly of do_all's matcher inputs with the single-pair entry points"""
    import torch
    bands = ss.bands(torch.stack([left, right]).contiguous())
    kp, desc, cnt = fm.surf_dev(bands.reshape(8, H // 4, W, 3))
    kxy = kp.view(torch.float32)[..., :2]
    out = {}
    for s, side in enumerate("lr"):
        c4 = [int(x) for x in cnt[4 * s: 4 * s + 4]]
        key = torch.cat([kxy[4 * s + b, :c4[b]] for b in range(4)]).contiguous()
        if key.shape[0]:
            ss.unrotate_band_keypoints(key, c4, W, H)
        out["kp_" + side] = key
        out["desc_" + side] = torch.cat([desc[4 * s + b, :c4[b]] for b in range(4)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", action="append", default=[], help="WxH:B (repeatable)")
    ap.add_argument("--groups", type=int, nargs="*", default=[4, 8, 16])
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    import torch
    from erp_match_eightpoint_test_amd import (Context, ErpError, PairBatchRunner, eight_point,
                                                erp_rotation, feature_matcher, results_to_numpy,
                                                spherical_surf)
    shapes = [(5376, 2688, b) for b in (1, 16, 64)] + [(1344, 672, b) for b in (1, 16, 64)]
    if args.only:
        shapes = []
        for o in args.only:
            wh, b = o.split(":")
            w, h = wh.split("x")
            shapes.append((int(w), int(h), int(b)))
    dev = torch.device("cuda:0")
    ctx = Context(0)
    ss, er, fm = spherical_surf(ctx=ctx), erp_rotation(ctx=ctx), feature_matcher(ctx=ctx)
    ep = eight_point(ctx=ctx, iters=args.iters)
    run = PairBatchRunner(ctx=ctx, iters=args.iters)

    def per_pair(lefts, rights, W, H):
        res = []
        for b in range(lefts.shape[0]):
            kl, kr, M, _ = ss.do_all(lefts[b], rights[b])
            try:
                R, T = ep.find(W, H, kl.cpu().numpy(), kr.cpu().numpy())
                res.append((M, R, T, 0))
            except ErpError as e:
                res.append((M, None, None, e.status))
        torch.cuda.synchronize()
        return res

    def batched(lefts, rights, **kw):
        outs = run.run_images(lefts, rights, **kw)
        torch.cuda.synchronize()
        return outs

    def timed(f):
        t0 = time.perf_counter()
        f()
        return time.perf_counter() - t0

    def rate(ts, B):
        ts = sorted(ts)
        return {"pairs_per_s": B / ts[len(ts) // 2], "pairs_per_s_min": B / ts[-1],
                "pairs_per_s_max": B / ts[0], "ms_per_step_median": ts[len(ts) // 2] * 1e3}

    rows, cache = [], {}
    for W, H, B in shapes:
        if (W, H) not in cache or cache[(W, H)][0].shape[0] < B:
            cache[(W, H)] = make_pairs(W, H, max(b for w, h, b in shapes if (w, h) == (W, H)),
                                       args.seed, er, dev)
        lefts, rights = cache[(W, H)][0][:B], cache[(W, H)][1][:B]
        row = {"W": W, "H": H, "B": B}
        outs = batched(lefts, rights)                           # warms the shape
        row["groups"] = run.last_info["groups"]
        row["max_nq"], row["max_nt"] = run.last_info["max_nq"], run.last_info["max_nt"]
        if not args.no_baseline:
            r = results_to_numpy(outs["results"])
            ref = per_pair(lefts, rights, W, H)
            dR = dT = 0.0
            for b, (M, R, T, status) in enumerate(ref):
                assert int(r["M"][b]) == M and int(r["status"][b]) == status, (b, r[b], M, status)
                if status == 0:
                    dR = max(dR, float(np.abs(R - r["R"][b]).max()))
                    dT = max(dT, float(np.abs(T - r["T"][b]).max()))
            assert dR <= 1e-6 and dT <= 1e-6, (dR, dT)
            p, a = run.last_packed, assemble_pair(ss, fm, lefts[0], rights[0], W, H)
            nl, nr = int(p["off_l"][1]), int(p["off_r"][1])
            for k, n in (("desc_l", nl), ("kp_l", nl), ("desc_r", nr), ("kp_r", nr)):
                assert a[k].shape[0] == n and torch.equal(
                    p[k][:n].view(torch.int32), a[k].contiguous().view(torch.int32)), k
            row["check"] = {"pairs": B, "M": [int(x) for x in r["M"][:8]], "max_dR": dR,
                            "max_dT": dT, "packed_pair0_bytes_equal": True}
        tb, tp = [], []
        for _ in range(args.steps):
            tb.append(timed(lambda: batched(lefts, rights)))
            if not args.no_baseline:
                tp.append(timed(lambda: per_pair(lefts, rights, W, H)))
        row["batched"] = rate(tb, B)
        if tp:
            row["per_pair"] = rate(tp, B)
            row["speedup"] = row["batched"]["pairs_per_s"] / row["per_pair"]["pairs_per_s"]
        rows.append(row)
        print(f"{W}x{H} B={B}: {row['batched']['pairs_per_s']:.1f} pairs/s batched", file=sys.stderr,
              flush=True)
    ab = None
    if args.groups and shapes:
        W, H, B = max(shapes, key=lambda s: (s[0] * s[1], s[2]))
        lefts, rights = cache[(W, H)][0][:B], cache[(W, H)][1][:B]
        ab = {"W": W, "H": H, "B": B, "max_group_pairs": {}}
        for g in args.groups:
            batched(lefts, rights, max_group_pairs=g)           # warm (scratch growth)
            ts = [timed(lambda: batched(lefts, rights, max_group_pairs=g))
                  for _ in range(args.steps)]
            ab["max_group_pairs"][str(g)] = dict(rate(ts, B), groups=run.last_info["groups"])
    print(json.dumps({"metric": "ERP image pairs/s, images -> (R, T): batched run_images vs the "
                                "per-pair do_all + find loop", "unit": "pairs/s",
                      "steps": args.steps, "iters": args.iters, "shapes": rows,
                      "group_ab": ab}))


if __name__ == "__main__":
    main()
