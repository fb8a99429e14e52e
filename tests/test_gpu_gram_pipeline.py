"""The Gram kernel's pipelined K step (gram_mfma_kernel: the B fragments of a step go through
register quads, reads ahead of the MFMAs) on the shapes where the step loop can go wrong:

* m = 36: 2 selection words, one step, shorter than the DMA ring;
* m = 63: 3 words, the second step's second word is masked;
* m = 125: 5 words, 3 steps, fewer than ring - 1;
* m = 311: 11 words, 6 steps, more than the ring;
* m = 1000;
* 64, 500 and 700 iterations: blocks that end past the last iteration, at 128 and at 256
  iterations per block (one and two row tiles per wave, ERP_OPT_GRAM_TILES 1 / 2).

The int8-MFMA sums are exact, so the two kernels must agree byte for byte with each other and
with the records of the commit before the pipeline (tests/golden/gram_pipeline_parent.npz,
tests/golden/gen_gram_pipeline.py); the oracle bounds are those of tests/test_gpu_parity.py.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

from erp_match_eightpoint_test_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
import gen_gram_pipeline as G  # noqa: E402  (the cases: MS, ITERS, SEED0)

CASES = [(m, it) for m in G.MS for it in G.ITERS]
TOL_RT = 1e-6  # tests/test_gpu_parity.py: R (rad) / T against the oracle; E within 1e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "gram_pipeline_parent.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def records(gpu_lib, gold):
    """{(wt, m, iters): hypothesis records} of every case on both row-tile settings, computed
    once and left unchanged"""
    import torch
    from erp_match_eightpoint_test_amd import Context, dist
    out = {}
    for wt in (1, 2):
        c = Context(0)
        c.set_option("gram_tiles", wt)
        for m in G.MS:
            dkl = torch.from_numpy(np.ascontiguousarray(gold[f"m{m}_kl"])).cuda()
            dkr = torch.from_numpy(np.ascontiguousarray(gold[f"m{m}_kr"])).cuda()
            fn = dist.gpu_hypotheses(c, int(gold["W"]), int(gold["H"]), dkl, dkr, m, {})
            for it in G.ITERS:
                out[wt, m, it] = fn(it, 0)
    return out


def test_inputs_regenerate(gold):
    """the stored keypoints are synth.make_correspondences(SEED0 + m, m)"""
    for m in G.MS:
        c = synth.make_correspondences(G.SEED0 + m, m=m)
        assert np.array_equal(c["kp_l"], gold[f"m{m}_kl"]) and np.array_equal(c["kp_r"], gold[f"m{m}_kr"])
        assert (c["W"], c["H"]) == (int(gold["W"]), int(gold["H"]))


@pytest.mark.parametrize("m,iters", CASES)
def test_row_tiles_identical(records, m, iters):
    a, b = records[1, m, iters], records[2, m, iters]
    assert len(a) == len(b) == iters
    for f in ("E", "R1", "R2", "T", "R1_valid", "R2_valid"):
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint8),
                              np.ascontiguousarray(b[f]).view(np.uint8)), f


@pytest.mark.parametrize("wt", [1, 2])
@pytest.mark.parametrize("m,iters", CASES)
def test_E_equals_parent_records(records, gold, wt, m, iters):
    e = np.ascontiguousarray(records[wt, m, iters]["E"])
    g = gold[f"m{m}_it{iters}_E"]
    assert e.shape == g.shape == (iters, 9)
    assert np.array_equal(e.view(np.uint8), g.view(np.uint8))


@pytest.mark.parametrize("m,iters", CASES)
def test_hypotheses_vs_oracle(records, gold, oracle, m, iters):
    o = oracle.find(int(gold["W"]), int(gold["H"]), gold[f"m{m}_kl"], gold[f"m{m}_kr"],
                    oracle.make_cfg(iters=iters), detail=True)
    assert len(o["hyp"]) == iters
    for wt in (1, 2):
        for a, b in zip(records[wt, m, iters], o["hyp"]):  # test_gpu_parity._check_hyps
            assert a["R1_valid"] + a["R2_valid"] == b["R1_valid"] + b["R2_valid"]
            same = max(np.abs(a["R1"] - b["R1"]).max(), np.abs(a["R2"] - b["R2"]).max())
            swap = max(np.abs(a["R1"] - b["R2"]).max(), np.abs(a["R2"] - b["R1"]).max())
            e = min(np.abs(a["E"] - b["E"]).max(), np.abs(a["E"] + b["E"]).max())
            assert min(same, swap) <= TOL_RT
            assert np.abs(a["T"] - b["T"]).max() <= TOL_RT
            assert e <= 1e-6


def _pair_with_matches(seed: int, M: int, extra: int = 40) -> dict:
    """a descriptor pair whose ratio test keeps exactly the first M queries (their train rows are
    copies; every other row is random on both sides), keypoints from make_correspondences"""
    rng = np.random.default_rng(seed)
    c = synth.make_correspondences(seed, m=M)
    n = M + extra
    dl = synth.random_descriptors(rng, n)
    dr = synth.random_descriptors(rng, n)
    dr[:M] = dl[:M]
    px = lambda k: (rng.random((k, 2)) * [c["W"], c["H"]]).astype(np.float32)  # noqa: E731
    return {"desc_l": dl, "desc_r": dr, "kp_l": np.concatenate([c["kp_l"], px(extra)]),
            "kp_r": np.concatenate([c["kp_r"], px(extra)]), "W": c["W"], "H": c["H"]}


def test_ragged_batch_row_tiles_identical(gpu_lib):
    """three pairs of one batch: s < 9 (the thin path: the kernel stores plain Grams), m = 63 and
    m = 311 -- results, hypothesis records and sample sets byte-identical between the kernels"""
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    want_m = (20, 63, 311)
    pairs = [_pair_with_matches(7700 + i, M) for i, M in enumerate(want_m)]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    off = np.concatenate([[0], np.cumsum([len(p["desc_l"]) for p in pairs])]).astype(np.int64)
    args = (t(np.concatenate([p["desc_l"] for p in pairs])),
            t(np.concatenate([p["desc_r"] for p in pairs])),
            t(np.concatenate([p["kp_l"] for p in pairs])),
            t(np.concatenate([p["kp_r"] for p in pairs])), t(off), t(off),
            t(np.array([p["W"] for p in pairs], np.int32)),
            t(np.array([p["H"] for p in pairs], np.int32)),
            int(np.diff(off).max()), int(np.diff(off).max()))
    outs = {}
    for wt in (1, 2):
        c = Context(0)
        c.set_option("gram_tiles", wt)
        o = PairBatchRunner(ctx=c, iters=500).run(*args, want=("hyps", "samples"))
        torch.cuda.synchronize()
        outs[wt] = {k: v.cpu().numpy() for k, v in o.items()}
    res = results_to_numpy(torch.from_numpy(outs[2]["results"]))
    assert tuple(int(x) for x in res["M"]) == want_m
    assert int(res["sample_n"][0]) < 9 <= int(res["sample_n"][1])
    for k in ("results", "hyps", "samples"):
        assert np.array_equal(outs[1][k].view(np.uint8), outs[2][k].view(np.uint8)), k
