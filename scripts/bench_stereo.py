#!/usr/bin/env python
"""The dense-stereo stage (erp_stereo_rows_dev and erp_stereo_rows_ex_dev, DESIGN.md sections
3.20 and 3.21) next to the call that feeds it.

Per shape, in one process on one stream, HIP events, interleaved repetition by repetition:
  rectify   erp_rectify_batch_dev: the rectified and the vertical views of the P pairs;
  stereo    stereo.vertical on the vertical views where they lie, disp16 only;
  stereo_z  the same with the depth;
  stereo8   disp16 with n_paths = 8 (the diagonal paths, erp_stereo_rows_ex_dev);
  stereo8_u the same with uniqueness = 15.
Two shapes: one pair of 5376 x 2688 images (views of 5376 rows x 2688 columns) with D = 128, and
8 pairs of 1344 x 672 with D = 64.  Images are bench_rectify's seeded device textures, the poses
generic.  Median, min, max over --reps and spread = (max - min) / median; disp16 of the first and
the last repetition must be byte-identical: asserted.

The S volume is rows * cols * D * 2 bytes per pair.  The kernels move, in volumes: paths along
rows 3 (the forward walk stores, the backward walk loads and stores), paths along columns 4,
winner 1 + (D - 1) / 1024 (each row once, plus the D - 1 columns to the left of every
1024-column segment a second time): about 8.1 in all.  With eight paths each of the two diagonal
launches moves 4 more (both of its walks load and store): about 16.1.
hbm_fraction = those volumes / time / 8 TB/s for the whole call; --kernel-stats CSV (the kernel
statistics of a profiler run of this script, columns Name and TotalDurationNs or
AverageNs + Calls) adds the time, volumes and bandwidth per kernel.  Writes one JSON document
(--out) and prints it."""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
SHAPES = {"full": dict(W=5376, H=2688, P=1, D=128), "batch8": dict(W=1344, H=672, P=8, D=64)}
WIN_SEGMENT = 1024  # csrc/stereo.hip kWinT


def volumes(D):
    """S volumes each kernel moves, by a pattern of its name"""
    return {"stereo_path_kernel<*, false>": 3.0, "stereo_path_kernel<*, true>": 4.0,
            "stereo_diag_kernel": 4.0,  # per launch; an eight-path call has two
            "stereo_winner_kernel": 1.0 + (D - 1) / WIN_SEGMENT}


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()),
            "spread": float((v.max() - v.min()) / np.median(v))}


def measure(name, shape, args):
    import torch
    from bench_rectify import make_images
    from erp_match_eightpoint_test_amd import Context, capi, erp_rotation, stereo
    W, H, P, D = shape["W"], shape["H"], shape["P"], shape["D"]
    dev = torch.device("cuda:0")
    ctx = Context(0)
    er = erp_rotation(ctx=ctx)
    rng = np.random.default_rng(args.seed)
    lefts, rights = make_images(W, H, P, args.seed, dev), make_images(W, H, P, args.seed + 1, dev)
    rv = rng.uniform(-0.3, 0.3, (P, 3)).astype(np.float32).astype(np.float64)
    tv = rng.standard_normal((P, 3))
    tv = (tv / np.linalg.norm(tv, axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    kw = dict(d_min=-D // 2, n_disp=D, ctx=ctx)
    t = {k: [] for k in ("rectify", "stereo", "stereo_z", "stereo8", "stereo8_u")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(10)]
    first = None
    for rep in range(-1, args.reps):  # (rep -1 warms every call and grows the scratch)
        ev[0].record()
        out = er.rectify_batch(lefts, rights, rot_vecs=rv, t_vecs=tv)
        ev[1].record()
        lv, rvv = out["left_vertical"], out["right_vertical"]
        ev[2].record()
        disp = stereo.vertical(lv, rvv, **kw)
        ev[3].record()
        ev[4].record()
        disp_z, z = stereo.vertical(lv, rvv, depth=True, **kw)
        ev[5].record()
        ev[6].record()
        disp8 = stereo.vertical(lv, rvv, n_paths=8, **kw)
        ev[7].record()
        ev[8].record()
        disp8_u = stereo.vertical(lv, rvv, n_paths=8, uniqueness=15, **kw)
        ev[9].record()
        torch.cuda.synchronize()
        if first is None:
            first, first8 = disp.clone(), disp8.clone()
        if rep < 0:
            continue
        for k, i in (("rectify", 0), ("stereo", 2), ("stereo_z", 4), ("stereo8", 6),
                     ("stereo8_u", 8)):
            t[k].append(ev[i].elapsed_time(ev[i + 1]))
    assert torch.equal(first, disp) and torch.equal(first, disp_z), f"{name}: disp16 differs"
    assert torch.equal(first8, disp8), f"{name}: eight-path disp16 differs"
    kept = disp8 != capi.STEREO_INVALID
    assert bool((disp8_u[kept] == disp8[kept]).logical_or(disp8_u[kept] == capi.STEREO_INVALID).all())
    vol = float(W) * H * D * 2
    med = float(np.median(t["stereo"]))
    valid = disp != capi.STEREO_INVALID
    vols = volumes(D)
    nvol = sum(v for k, v in vols.items() if "diag" not in k)
    nvol8 = nvol + 2 * vols["stereo_diag_kernel"]
    med8 = float(np.median(t["stereo8"]))
    doc = {"shape": name, **shape, "rows": W, "cols": H, "d_min": kw["d_min"], "reps": args.reps,
           "s_volume_bytes_per_pair": vol,
           "chunk_pairs": max(1, min(P, int((ctx.get_option("stereo_chunk_mb") << 20) // vol))),
           "ms": {k: stats(v) for k, v in t.items()},
           "stereo_ms_per_pair": med / P,
           "stereo_over_rectify": med / float(np.median(t["rectify"])),
           "volumes_moved": nvol, "bytes_moved": nvol * vol * P,
           "hbm_bytes_per_s": nvol * vol * P / (med * 1e-3),
           "hbm_fraction": nvol * vol * P / (med * 1e-3) / HBM_BYTES_PER_S,
           "stereo8_over_stereo": med8 / med,
           "volumes_moved_8": nvol8,
           "hbm_bytes_per_s_8": nvol8 * vol * P / (med8 * 1e-3),
           "hbm_fraction_8": nvol8 * vol * P / (med8 * 1e-3) / HBM_BYTES_PER_S,
           "valid_fraction": float(valid.float().mean()),
           "valid_fraction_8": float(kept.float().mean()),
           "valid_fraction_8_u15": float((disp8_u != capi.STEREO_INVALID).float().mean()),
           "disp16_changed_by_8_paths": float((disp8 != disp).float().mean()),
           "finite_depth_fraction": float(torch.isfinite(z).float().mean()),
           "disp16_identical": True}
    del lefts, rights, out, disp, disp_z, z, disp8, disp8_u
    torch.cuda.empty_cache()
    return doc


def kernel_table(path, shape):
    """per stereo kernel of a profiler's kernel statistics over a run of one shape: time per
    call, the volumes it moves and the bandwidth that implies"""
    vol = float(shape["W"]) * shape["H"] * shape["D"] * 2 * shape["P"]
    rows = []
    for r in csv.DictReader(open(path)):
        n = r.get("Name") or r.get("KernelName") or ""
        if "stereo_" not in n:
            continue
        calls = int(r["Calls"])
        total = float(r.get("TotalDurationNs") or float(r["AverageNs"]) * calls)
        ms = total / calls * 1e-6
        row = {"kernel": n, "calls": calls, "ms_per_call": ms}
        for pat, v in volumes(shape["D"]).items():
            head, _, tail = pat.partition("*")
            if head in n and tail in n:
                # the chunks of a call share the kernel: calls per stereo call = chunks (the
                # diagonal kernel: two launches per chunk, 4 volumes each)
                row["volumes"] = v
                row["hbm_bytes_per_s"] = v * vol / shape["chunks"] / (ms * 1e-3)
                row["hbm_fraction"] = row["hbm_bytes_per_s"] / HBM_BYTES_PER_S
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="full,batch8")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-stats", dest="kernel_stats", default=None,
                    help="kernel statistics CSV of a profiler run of ONE shape (--shapes)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22a_bench_stereo.json"))
    args = ap.parse_args()
    names = args.shapes.split(",")
    if args.kernel_stats:
        assert len(names) == 1, "--kernel-stats describes a run of one shape"
        s = dict(SHAPES[names[0]])
        vol = float(s["W"]) * s["H"] * s["D"] * 2
        s["chunks"] = -(-s["P"] // max(1, min(s["P"], int((1024 << 20) // vol))))
        doc = {"bench": "stereo_kernels", "shape": names[0], **s,
               "kernels": kernel_table(args.kernel_stats, s)}
    else:
        import torch
        assert torch.cuda.is_available(), "bench_stereo needs a HIP device"
        doc = {"bench": "stereo", "device": torch.cuda.get_device_name(0),
               "shapes": [measure(n, SHAPES[n], args) for n in names]}
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
