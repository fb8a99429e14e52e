"""bench.py's plain run on the device, in process and at a small shape (6 pairs of 512 x 512
keypoints on 3 streams, 80 iterations): the line it prints, the --dump-outputs arrays against
the oracle, and the --steps 0 branch.  Bars: status, M, K exact, R and T within 1e-6 of the oracle
(the parity bars of the bench's own check)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS, KPTS, ITERS, SEED = 6, 512, 80, 20200423
SHAPE = ["--gpus", "1", "--pairs", str(PAIRS), "--streams", "3", "--kpts", str(KPTS),
         "--iters", str(ITERS), "--seed", str(SEED)]
MOVED = ("roofline", "roofline_stages", "cpu_baseline", "latency", "hard_data", "worst_case",
         "stages_ms_serial_step", "overlap", "exact")


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *SHAPE, *argv])
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {p.name[:-4]: np.load(p) for p in sorted(d.iterdir())}


@pytest.fixture(scope="module")
def reference(oracle):
    """the oracle's answer for the bench's own (seeded) pairs, computed once"""
    ref = []
    for p in bench.make_batch(0, PAIRS, KPTS, SEED, 0.8, 0.03):
        mt, _, _, _ = oracle.match_two_image(p["desc_l"], p["desc_r"])
        o = oracle.find(p["W"], p["H"], p["kp_l"][mt["queryIdx"]], p["kp_r"][mt["trainIdx"]],
                        oracle.make_cfg(iters=ITERS))
        ref.append(dict(M=len(mt), K=o["K"], status=o["status"], R=o["R"], T=o["T"]))
    return ref


@pytest.fixture(scope="module")
def plain_dump(gpu_lib, tmp_path_factory):
    """one plain run with --dump-outputs (3 timed steps), shared by the tests below"""
    mp = pytest.MonkeyPatch()
    d = tmp_path_factory.mktemp("dump")
    mp.setattr(sys, "argv", ["bench.py", *SHAPE, "--steps", "3", "--warmup", "1",
                             "--dump-outputs", str(d)])
    import contextlib
    import io
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        mp.undo()
    lines = [ln for ln in buf.getvalue().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), _load(d)


def test_plain_line(plain_dump):
    line, _ = plain_dump
    assert line["full"] is False and not [k for k in MOVED if k in line]
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (3, 1, 1)
    assert line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32+f64" and line["metric"].startswith("ERP image-pairs/sec")
    assert line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: pairs per step over the step's time
    assert line["value"] == pytest.approx(PAIRS / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert line["check"]["all_status_ok"] is True
    assert line["config"]["pairs_per_step_per_gpu"] == PAIRS and line["config"]["streams"] == 3


def test_plain_dump_against_oracle(plain_dump, reference):
    _, got = plain_dump
    assert got["R"].dtype == got["T"].dtype == np.float32
    assert got["R"].shape == got["T"].shape == (PAIRS, 3)
    for f in ("status", "M", "K", "min_idx", "sample_n", "near_ties", "min_dist"):
        assert got[f].dtype == np.float64 and got[f].shape == (PAIRS,), f
    for i, o in enumerate(reference):
        assert (got["status"][i], got["M"][i], got["K"][i]) == (o["status"], o["M"], o["K"]), i
        assert np.abs(got["R"][i] - o["R"]).max() <= 1e-6, i
        assert np.abs(got["T"][i] - o["T"]).max() <= 1e-6, i


@pytest.mark.parametrize("warmup", [1, 0])
def test_plain_steps0_gives_the_same_records(plain_dump, monkeypatch, capsys, tmp_path, warmup):
    """--steps 0 times nothing (value null) and dumps the records of its serial pass: the same
    inputs, so the same arrays as the timed, overlapped run's"""
    _, want = plain_dump
    line = _run(monkeypatch, capsys, "--steps", "0", "--warmup", str(warmup),
                "--dump-outputs", str(tmp_path))
    assert line["value"] is None and line["steps"] == 0 and line["full"] is False
    got = _load(tmp_path)
    assert got.keys() == want.keys()
    for f in want:
        assert np.array_equal(got[f], want[f]), f
