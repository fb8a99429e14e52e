#!/usr/bin/env python3
"""Speed-of-light probe of the glibc-replay sampler (scripts/dev/sampler_sol.hip), on the GPU.

One 128-pair sub-batch of the bench workload (bench.make_batch, configs[1] shape) goes through
the library once with stage timing on: that gives the batch's match counts M and the real
sampler_kernel's time for the launch.  The probe variants then run on the same counts, the same
grid and 10k iterations:
  V0 generator only, V1 generator + modulo (the floor), V2 + the i >= s bookkeeping on every step,
  V3 V2 with constant magic shifts, V4 V3 with the carry-accumulated selection bit,
  V5 V2 on the position-major bitmap ([half][position] words, one bit per lane), V6 V5 plus the
  prefix and straddling blocks in that form (the whole replay), V7 the whole replay on the
  lane-major bitmap (the shipped blocks restated: V6's stand-in for sampler_kernel<0>),
  V8 / V9 V5 / V6 with the draws clamped to per-lane words s + (lane & 31) instead of word s,
  V10 V9 launched with the library's bound-sized LDS allocation (positions 0 .. max_nq / 4 + 31
  per half) while it still initialises and uses only the batch's own size: V10 - V9 is what the
  allocation alone costs (fewer workgroups per CU), the rest of the gap to the library's kernel
  belongs to that kernel's window loads and word stores.
Prints one JSON line: ms per launch and cycles per wave-draw per SIMD at the measured clock.
--merge-pmc DIR adds the per-launch means of the SQ counters of a counter-only rocprofv3 run of
this script (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU -d DIR ... --
python scripts/dev/sampler_sol.py --variants 2,5,6,7,8,9,10 --reps 1 --no-real).

  hipcc -O3 -std=c++17 --offload-arch=gfx950 -shared -fPIC scripts/dev/sampler_sol.hip \
      -o scripts/dev/libs/sol/libsampler_sol.so
  python scripts/dev/sampler_sol.py [--pairs 128] [--reps 10]
"""
import argparse
import collections
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def magic_table(n=65539):
    """m_d | (l_d - 1) << 32 with l_d = ceil(log2 d), m_d = ceil(2^(31 + l_d) / d): the
    library's build_magic_table (kernels.hip), restated"""
    t = np.zeros(n, np.uint64)
    for d in range(2, n):
        l = (d - 1).bit_length()
        m = -(-(1 << (31 + l)) // d)
        assert m < (1 << 32) and m * d - (1 << (31 + l)) <= (1 << l)
        t[d] = m | ((l - 1) << 32)
    return t


KERNEL_OF = {"V0": "sol_kernel<0>", "V1": "sol_kernel<1>", "V2": "sol_kernel<2>",
             "V3": "sol_kernel<3>", "V4": "sol_kernel<4>", "V5": "sol_pm_kernel<true,false,false>",
             "V6": "sol_pm_kernel<true,true,false>", "V7": "sol_pm_kernel<false,true,false>",
             "V8": "sol_pm_kernel<true,false,true>", "V9": "sol_pm_kernel<true,true,true,0>",
             "V10": "sol_pm_kernel<true,true,true,1>"}


def pmc_means(d):
    """{variant: {counter: mean per launch}} of a rocprofv3 --pmc output folder"""
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    disp = collections.defaultdict(set)
    for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row["Kernel_Name"].replace(" ", "")
            for v, k in KERNEL_OF.items():
                if k in name or k.replace(">", ",0>") in name:
                    acc[v][row["Counter_Name"]] += float(row["Counter_Value"])
                    disp[v].add(row["Dispatch_Id"])
    return {v: {c: x / len(disp[v]) for c, x in sorted(cs.items())} for v, cs in sorted(acc.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="0,1,2,3,4,5,6,7,8,9,10")
    ap.add_argument("--no-real", action="store_true", help="skip the library's own kernel")
    ap.add_argument("--merge-pmc", default=None, help="rocprofv3 --pmc output folder to add")
    ap.add_argument("--bound-lds", type=int, default=0,
                    help="V10's dynamic LDS in bytes (default: the library's bound-sized one)")
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lib", default=os.path.join(ROOT, "scripts", "dev", "libs", "sol",
                                                  "libsampler_sol.so"))
    a = ap.parse_args()
    import torch
    import bench
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    dev = torch.device("cuda:0")
    pairs = bench.make_batch(0, a.pairs, 4096, 20200423)
    b = bench.to_device(pairs, dev)
    ctx = Context(0)
    run = PairBatchRunner(ctx=ctx, iters=a.iters)
    run.reserve(a.pairs, b["max_nq"], b["max_nt"])
    args = (b["desc_l"], b["desc_r"], b["kp_l"], b["kp_r"], b["off_l"], b["off_r"], b["width"],
            b["height"], b["max_nq"], b["max_nt"])
    run.run(*args)
    torch.cuda.synchronize()
    ctx.set_profiling(True)
    ctx.stage_times()
    real = []
    for _ in range(1 if a.no_real else 3):
        o = run.run(*args)
        torch.cuda.synchronize()
        st = ctx.stage_times()
        real.append(st["sampler"][0] / st["sampler"][1])
    M = results_to_numpy(o["results"])["M"].astype(np.int64)
    s = (M * 0.25).astype(np.int64)
    counts = torch.from_numpy(M.astype(np.int32)).to(dev)
    mt = torch.from_numpy(magic_table().view(np.int64)).to(dev)
    nwaves = (a.iters + 63) // 64
    nbw = int((M.max() - 1) // 31 + 2)
    nalloc = int(s.max() >> 5) + 1
    # position-major (V5 / V6 / V8 / V9): positions 0 .. max s + 31 (the per-lane clamp words of
    # V8 / V9) per half-wave, the 2 halves together rounded up to the 1280-B LDS allocation
    # granule (320 words)
    nalloc_pm = (2 * (int(s.max()) + 32) + 319) // 320 * 160
    # V10: the library's allocation for the host-known bound max_s = (int)(max_nq * sample_frac)
    bound_lds = a.bound_lds or (2 * (int(b["max_nq"] * 0.25) + 32) + 319) // 320 * 160 * 2 * 4
    out = torch.empty(a.pairs * nwaves * nbw * 64, dtype=torch.int32, device=dev)
    L = C.CDLL(a.lib)
    L.sol_run.restype = C.c_float
    L.sol_run.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p,
                          C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    draws = float(np.sum(M - 1)) * nwaves * 64          # lane-draws per launch (incl. idle lanes)
    wave_draws_per_simd = draws / 64 / 1024
    res = {}
    for v in [int(x) for x in a.variants.split(",")]:
        na = nalloc_pm if v in (5, 6, 8, 9, 10) else nalloc
        lds = bound_lds if v == 10 else 0
        L.sol_run(v, counts.data_ptr(), a.pairs, a.iters, 0.25, mt.data_ptr(), out.data_ptr(),
                  nbw, na, 2, lds)
        ms = [L.sol_run(v, counts.data_ptr(), a.pairs, a.iters, 0.25, mt.data_ptr(),
                        out.data_ptr(), nbw, na, a.reps, lds) for _ in range(3)]
        if min(ms) < 0:
            raise SystemExit(f"variant {v}: launch failed")
        res[f"V{v}"] = {"ms": min(ms), "ms_all": ms}
    real_ms = min(real)
    clk = 2.4e9
    line = {"probe": "sampler speed of light (scripts/dev/sampler_sol.hip)",
            "pairs": a.pairs, "iters": a.iters, "M_mean": float(M.mean()), "s_mean": float(s.mean()),
            "wave_draws_per_simd": wave_draws_per_simd,
            "lds_bytes": {"batch_sized": nalloc_pm * 8, "bound_sized": bound_lds},
            "real_sampler_kernel_ms": real_ms, "real_all": real,
            "variants": res,
            "cycles_per_wave_draw_at_2.4GHz": {k: v["ms"] * 1e-3 * clk / wave_draws_per_simd
                                               for k, v in res.items()},
            "real_cycles_per_wave_draw_at_2.4GHz": real_ms * 1e-3 * clk / wave_draws_per_simd,
            "notes": "V0 generator; V1 generator + magic modulo (floor); V2 + i>=s bookkeeping on "
                     "every step; V3 V2 + constant shifts; V4 V3 + carry-accumulated bits; V5 V2 on "
                     "the position-major bitmap; V6 V5 + prefix / straddling blocks (whole replay); "
                     "V7 the whole replay on the lane-major bitmap (the shipped blocks); V8 / V9 "
                     "V5 / V6 with the draws clamped to s + (lane & 31), one clamp word per lane; "
                     "V10 V9 with the launch's LDS forced to the library's bound-sized allocation"}
    if "V1" in res:
        line["real_over_floor_V1"] = real_ms / res["V1"]["ms"]
    for cand in ("V6", "V9"):
        if cand in res and "V7" in res:
            # the gate: the whole replay position-major against V7 beyond the spread of the three
            # repeated runs of each
            a6, a7 = res[cand]["ms_all"], res["V7"]["ms_all"]
            line[f"gate_{cand}_vs_V7"] = {
                f"{cand}_max": max(a6), "V7_min": min(a7), f"spread_{cand}": max(a6) - min(a6),
                "spread_V7": max(a7) - min(a7), f"{cand}_over_V7": min(a6) / min(a7),
                "passes": max(a6) < min(a7)}
    if "V9" in res and "V10" in res:
        # the occupancy effect: the same kernel under the batch-sized and the bound-sized
        # allocation, against the spread of the three repeated runs of each
        a9, a10 = res["V9"]["ms_all"], res["V10"]["ms_all"]
        d_ms = min(a10) - min(a9)
        line["occupancy_V10_vs_V9"] = {
            "V9_min": min(a9), "V9_max": max(a9), "V10_min": min(a10), "V10_max": max(a10),
            "effect_ms": d_ms,
            "effect_cycles_per_wave_draw": d_ms * 1e-3 * clk / wave_draws_per_simd,
            "library_gap_ms": real_ms - min(a9),
            "beyond_spread": max(a9) < min(a10)}
    if a.merge_pmc:
        pm = pmc_means(a.merge_pmc)
        wave_draws = draws / 64
        for v, cs in pm.items():
            if "SQ_INSTS_VALU" in cs:
                cs["valu_per_wave_draw"] = cs["SQ_INSTS_VALU"] / wave_draws
            if "SQ_LDS_BANK_CONFLICT" in cs and cs.get("SQ_LDS_IDX_ACTIVE"):
                cs["bank_conflict_over_idx_active"] = cs["SQ_LDS_BANK_CONFLICT"] / cs["SQ_LDS_IDX_ACTIVE"]
        line["counters_per_launch"] = pm
    print(json.dumps(line))


if __name__ == "__main__":
    main()
