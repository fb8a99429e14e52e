"""The throughput sampler's launch tiers (launch_sampler): sampler_kernel<0>
runs once per tier, each launch with the LDS bitmap of its own range of sample counts, and a
pair's selection words come from exactly one of them.  Every iteration's sample set against the
oracle's glibc replay and, byte for byte, against the latency kernel (sampler_lat = 2, one
bound-sized launch) and against the single bound-sized throughput launch (sampler_tiers = 0).

Small batches are forced onto the throughput kernel with sampler_lat = 0, sampler_split = 0.
130 iterations: two full waves and one partial wave.  sample_frac 0.25, s = (int)(M / 4); the
tiers end at s = 768 (6 waves per SIMD), 928 (5) and the batch's bound max_nq / 4:
  ragged    M = 9, 1000, 3072 (s = 768), 3076 (769), 3712 (928), 3716 (929): both boundaries and
            the first count after each, every tier populated, the bound (929) one past a boundary
  top       M = 3716 twice: the two lower launches find no pair of theirs
  low       M = 1000, 3072 under max_nq = 4096 (bound 1024): the two upper launches are empty
  single    M = 9, 1000 with max_nq = 1000 (bound 250): the bound fits the first tier, one launch
  boundary  M = 3072 beside a pair without matches: that pair is skipped in every launch
A pair's flags surface as its status (a set bit is ERP_INTERNAL / ERP_INVALID_ARG), so status 0
is "no flags bit set".
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from erp_match_eightpoint_test_amd import synth

pytestmark = pytest.mark.gpu

ITERS = 130
FRAC = 0.25
OFFSETS = (0, 12345)


@functools.lru_cache(maxsize=None)
def _pair(m):
    """a pair with exactly m matches (every left keypoint has its partner on the right, no other
    right keypoint); m = 0: eight unrelated keypoints a side, none passes the ratio test"""
    if m == 0:
        return synth.make_pair(7300, n_kpts=8, inlier_frac=0.0)
    return synth.make_pair(7300 + m, n_kpts=m, inlier_frac=1.0, sigma=0.005)


_ORACLE_SETS: dict = {}


def _oracle_sets(oracle, m, offset):
    """[ITERS][s] sorted sample sets of a pair with m matches (each pair replays the stream from
    `offset`): computed once per (m, offset), read-only afterwards"""
    key = (m, offset)
    if key not in _ORACLE_SETS:
        s = int(m * FRAC)
        g = oracle.GlibcRand(1, offset)
        a = np.stack([np.sort(g.random_array(m)[:s]) for _ in range(ITERS)])
        a.setflags(write=False)
        _ORACLE_SETS[key] = a
    return _ORACLE_SETS[key]


def _batch(ms):
    import torch
    pairs = [_pair(m) for m in ms]
    cat = lambda k: np.concatenate([p[k] for p in pairs])  # noqa: E731
    off = lambda k: np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]).astype(np.int64)  # noqa: E731
    ol, orr = off("desc_l"), off("desc_r")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")  # noqa: E731
    return (t(cat("desc_l")), t(cat("desc_r")), t(cat("kp_l")), t(cat("kp_r")), t(ol), t(orr),
            t(np.array([p["W"] for p in pairs], np.int32)),
            t(np.array([p["H"] for p in pairs], np.int32))), int(np.diff(ol).max())


def _run(tensors, max_n, offset, **opts):
    import torch
    from erp_match_eightpoint_test_amd import Context, PairBatchRunner, results_to_numpy
    c = Context(0)
    for k, v in opts.items():
        c.set_option(k, v)
    r = PairBatchRunner(ctx=c, iters=ITERS, seed=1, offset=offset, sample_frac=FRAC)
    r.reserve(len(tensors[6]), max_n, max_n)
    o = r.run(*tensors, max_n, max_n, want=("samples",))
    torch.cuda.synchronize()
    return results_to_numpy(o["results"]).copy(), o["samples"].cpu().numpy()


def _check(oracle, ms, offset, max_n=None):
    tensors, largest = _batch(ms)
    max_n = largest if max_n is None else max_n
    assert max_n >= largest
    res, smp = _run(tensors, max_n, offset, sampler_lat=0, sampler_split=0)
    res_1, smp_1 = _run(tensors, max_n, offset, sampler_lat=0, sampler_split=0, sampler_tiers=0)
    res_l, smp_l = _run(tensors, max_n, offset, sampler_lat=2, sampler_split=0)
    for other_res, other_smp in ((res_1, smp_1), (res_l, smp_l)):
        assert np.array_equal(smp, other_smp)
        assert np.array_equal(res.view(np.uint8), other_res.view(np.uint8))
    for p, m in enumerate(ms):
        if m < 2:
            assert res[p]["M"] < 2, res[p]
            continue
        s = int(m * FRAC)
        assert res[p]["M"] == m and res[p]["sample_n"] == s, (m, res[p])
        assert res[p]["status"] == 0, (m, res[p])
        want = _oracle_sets(oracle, m, offset)
        got = np.sort(smp[p, :, :s], axis=1)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (m, offset, bad[:8])


@pytest.mark.parametrize("offset", OFFSETS)
def test_ragged_batch_populates_every_tier(gpu_lib, oracle, offset):
    _check(oracle, [9, 1000, 3072, 3076, 3712, 3716], offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_all_pairs_in_top_tier(gpu_lib, oracle, offset):
    _check(oracle, [3716, 3716], offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_all_pairs_in_lowest_tier_under_large_bound(gpu_lib, oracle, offset):
    _check(oracle, [1000, 3072], offset, max_n=4096)


@pytest.mark.parametrize("offset", OFFSETS)
def test_bound_within_first_tier_is_one_launch(gpu_lib, oracle, offset):
    _check(oracle, [9, 1000], offset)


@pytest.mark.parametrize("offset", OFFSETS)
def test_boundary_pair_beside_pair_without_matches(gpu_lib, oracle, offset):
    _check(oracle, [3072, 0], offset)


def test_tier_option_range(gpu_lib):
    from erp_match_eightpoint_test_amd import Context, ErpError
    c = Context(0)
    assert c.get_option("sampler_tiers") == -1
    for v in (-1, 0, 1, 2, 4):
        c.set_option("sampler_tiers", v)
        assert c.get_option("sampler_tiers") == v
    for v in (-2, 5):
        with pytest.raises(ErpError):
            c.set_option("sampler_tiers", v)
