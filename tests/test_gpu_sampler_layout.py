"""The throughput sampler (sampler_kernel<0>) on its position-major bitmap (one word per
position, one bit per lane): every iteration's sample set against the
oracle's glibc replay and, byte for byte, against the latency kernel (lane-major bitmap).

Small batches are forced onto the throughput kernel with ERP_OPT_SAMPLER_LAT = 0 (and the split
replay off).  130 iterations: two full waves and one partial wave.  Match counts M (sample_frac
0.25, s = (int)(M / 4)):
  5, 9        s = 1, 2: all 64 lanes hammer the same one or two words (same-address atomics)
  128, 132    s = 32, 33: a word boundary of the lane-major form, then the first position after it
  257         a d >= 256 block, then the straddling block
  1000        all-draw, straddling, prefix (d >= 256 and below) and ending blocks
  9+257+1000  one ragged batch: the per-pair s against the batch-wide allocation (max_s)
These are the smallest shapes that exercise the clamp word, the prefix / draw straddling block,
the block running below step 1 and multi-lane collisions on one word.
"""
from __future__ import annotations

import numpy as np
import pytest

from erp_match_eightpoint_test_amd import synth

pytestmark = pytest.mark.gpu

ITERS = 130
FRAC = 0.25
OFFSETS = (0, 12345)


def _pair(seed, m):
    """a pair with exactly m matches: every left keypoint has its partner on the right (descriptor
    noise far inside the ratio test) and there is no other right keypoint"""
    return synth.make_pair(seed, n_kpts=m, inlier_frac=1.0, sigma=0.005)


def _batch(pairs):
    import torch
    cat = lambda k: np.concatenate([p[k] for p in pairs])  # noqa: E731
    off = lambda k: np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]).astype(np.int64)  # noqa: E731
    ol, orr = off("desc_l"), off("desc_r")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    return (t(cat("desc_l")), t(cat("desc_r")), t(cat("kp_l")), t(cat("kp_r")), t(ol), t(orr),
            t(np.array([p["W"] for p in pairs], np.int32)),
            t(np.array([p["H"] for p in pairs], np.int32)),
            int(np.diff(ol).max()), int(np.diff(orr).max()))


def _run(args, offset, **opts):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    c = Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    o = PairBatchRunner(ctx=c, iters=ITERS, seed=1, offset=offset, sample_frac=FRAC).run(
        *args, want=("samples",))
    torch.cuda.synchronize()
    return results_to_numpy(o["results"]).copy(), o["samples"].cpu().numpy()


def _check(oracle, ms, offset):
    pairs = [_pair(7100 + 13 * k + m, m) for k, m in enumerate(ms)]
    args = _batch(pairs)
    res, smp = _run(args, offset, sampler_lat=0, sampler_split=0)      # sampler_kernel<0>
    res_l, smp_l = _run(args, offset, sampler_lat=2, sampler_split=0)  # sampler_kernel<3>
    assert np.array_equal(smp, smp_l)
    assert np.array_equal(res.view(np.uint8), res_l.view(np.uint8))
    for p, m in enumerate(ms):
        s = int(m * FRAC)
        assert res[p]["M"] == m and res[p]["sample_n"] == s, (m, res[p])
        g = oracle.GlibcRand(1, offset)
        for it in range(ITERS):
            a = g.random_array(m)
            assert np.array_equal(np.sort(smp[p, it, :s]), np.sort(a[:s])), (m, offset, it)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("m", [5, 9, 128, 132, 257, 1000])
def test_throughput_sampler_vs_oracle_and_latency_kernel(gpu_lib, oracle, m, offset):
    _check(oracle, [m], offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_throughput_sampler_ragged_batch(gpu_lib, oracle, offset):
    _check(oracle, [9, 257, 1000], offset)
