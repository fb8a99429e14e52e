"""tests/golden/gram_pipeline_parent.npz: the essential matrices of every iteration, as the Gram
kernel of the commit BEFORE the pipelined K step computed them, on the inputs of
tests/test_gpu_gram_pipeline.py.  The int8-MFMA sums are exact, so a reordered or re-pipelined
K loop must reproduce them byte for byte.

Run on a GPU with the library to record (ERP_LIB_PATH names it; the records in the repository
come from the parent commit's build):

    ERP_LIB_PATH=<parent>/liberp_match.so python tests/golden/gen_gram_pipeline.py --out X.npz

Keys: m{m}_kl / m{m}_kr (float32 [m, 2], synth.make_correspondences(SEED0 + m, m)), W, H,
m{m}_it{iters}_E (float64 [iters, 9]).  The two row-tile settings of the parent must agree
before anything is written.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

MS = (36, 63, 125, 311, 1000)
ITERS = (64, 500, 700)
SEED0 = 9000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from erp_match_eightpoint_test_amd import Context, capi, dist, synth
    print("library:", capi.lib_path())
    ctxs = {}
    for wt in (1, 2):
        ctxs[wt] = Context(0)
        ctxs[wt].set_option("gram_tiles", wt)
    out = {}
    for m in MS:
        c = synth.make_correspondences(SEED0 + m, m=m)
        out["W"], out["H"] = np.int32(c["W"]), np.int32(c["H"])
        out[f"m{m}_kl"], out[f"m{m}_kr"] = c["kp_l"], c["kp_r"]
        dkl = torch.from_numpy(c["kp_l"]).cuda()
        dkr = torch.from_numpy(c["kp_r"]).cuda()
        for iters in ITERS:
            E = {wt: dist.gpu_hypotheses(ctxs[wt], c["W"], c["H"], dkl, dkr, m, {})(iters, 0)["E"]
                 for wt in (1, 2)}
            assert np.array_equal(E[1].view(np.uint8), E[2].view(np.uint8)), (m, iters)
            out[f"m{m}_it{iters}_E"] = np.ascontiguousarray(E[2])
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
