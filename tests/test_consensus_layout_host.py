"""The consensus scratch layout (erp_match_eightpoint_test_amd/csrc/erp_consensus_ws.hpp) on the
host, no GPU: tests/cpp/consensus_layout_check.cpp (g++ -std=c++17, only that header) checks
containment, overlap and alignment of every part and prints the numbers; here they are compared
with the formulas the allocation and the launchers used before the layout had one owner, written
out again independently.  Sizes must be EQUAL (the footprint does not move), and the offsets the
kernels are handed are pinned."""
from __future__ import annotations

import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "consensus_layout_check.cpp")
SHAPES = [(1, 1), (1, 80), (3, 33), (9, 1100), (128, 10000), (768, 10000), (1, 100000)]
NB = 576           # bins of the bounds pass
HINT_CANDS = 4
HINT_CAND_BYTES = 24   # f64 T, i32 row, u32 va, vb, pad
RECIP = 65538


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layout") / "consensus_layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # containment / overlap / alignment, checked in C++
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    assert [(d["n_pairs"], d["iters"]) for d in rows] == SHAPES
    return {(d["n_pairs"], d["iters"]): d for d in rows}


def _align16(x):
    return (x + 15) // 16 * 16


def _sortbuf_len(iters):
    p = 1
    while p < 2 * iters:
        p <<= 1
    return p


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_equal_the_former_formulas(layouts, shape):
    P, I = shape
    S = 2 * I
    d = layouts[shape]
    cap = gcap = S // 4 + 64
    assert (d["cap"], d["gcap"]) == (cap, gcap)
    assert d["lb"] == d["ub"] == d["bsel"] == d["zsel"] == P * S * 8
    assert d["surv"] == P * S * 4
    assert d["nsurv"]["bytes"] == 20 * P + 8
    assert d["edges"]["bytes"] == 4 * NB * 4 * P + 4 * P
    assert d["lipref"]["bytes"] == (P * cap * 16 + P * 16 + P * S * 4 + 64 + P * gcap * 2 * 16
                                    + P * gcap * 4 + P * 8 + 128 + P * 4 + 16
                                    + P * HINT_CANDS * HINT_CAND_BYTES)
    assert d["hlite"]["bytes"] == P * 9 * I * 4 + P * ((I + 63) // 64) * 8 * 4
    assert d["rtab"]["bytes"] == RECIP * 16 + 8
    assert d["sortbuf_len"] == _sortbuf_len(I)
    assert d["sortbuf"]["bytes"] == 4 * P * _sortbuf_len(I)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_offsets_pinned(layouts, shape):
    P, I = shape
    S = 2 * I
    d = layouts[shape]
    cap = gcap = S // 4 + 64
    off = lambda buf, part: d[buf][part][0]  # noqa: E731
    # the counts block: nsurv [P], binned counts [P], unit prefix [P + 1], n2 [P], nfb [P]
    assert off("nsurv", "nsurv") == 0
    assert off("nsurv", "nbin") == 4 * P
    assert off("nsurv", "uoff") == 4 * 2 * P
    assert off("nsurv", "n2") == 4 * (2 * P + P + 1)
    assert off("nsurv", "nfb") == 4 * (2 * P + P + 1 + P)
    assert d["nsurv"]["uoff"][1] == P + 1
    # edges: first [P][2][NB] f32, zoom the same, then the grids
    assert off("edges", "first") == 0
    assert off("edges", "zoom") == 4 * P * 2 * NB
    assert off("edges", "zgrid") == 4 * P * 4 * NB
    # lipref: float4 ref [P][cap], U f64 [P], cnt, r2cnt i32 [P], r2list i32 [P][S]; 64 bytes on,
    # rounded up to 16: float4 gref [P][gcap][2], gsel i32 [P][gcap], gcnt [P], goff [P + 1],
    # nflat [P]; rounded up to 16: the hint candidates
    U = 16 * P * cap
    assert off("lipref", "ref") == 0
    assert off("lipref", "U") == U
    assert off("lipref", "cnt") == U + 8 * P
    assert off("lipref", "r2cnt") == U + 12 * P
    assert off("lipref", "r2list") == U + 16 * P
    gref = _align16(U + 16 * P + 4 * P * S + 64)
    assert off("lipref", "gref") == gref
    gsel = gref + 16 * P * gcap * 2
    assert off("lipref", "gsel") == gsel
    assert off("lipref", "gcnt") == gsel + 4 * P * gcap
    assert off("lipref", "goff") == gsel + 4 * P * gcap + 4 * P
    nflat = gsel + 4 * P * gcap + 4 * P + 4 * (P + 1)
    assert off("lipref", "nflat") == nflat
    assert off("lipref", "hcand") == _align16(nflat + 4 * P)
    assert d["snap"] == U + 12 * P  # the debug snapshot's share: ref, U, cnt
    # sortbuf's two roles share its start; hlite and rtab
    assert off("sortbuf", "score") == off("sortbuf", "list2") == 0
    assert off("hlite", "hl") == 0 and off("hlite", "wsum") == 4 * P * 9 * I
    assert (off("rtab", "recip"), off("rtab", "magic"), off("rtab", "bad")) == (0, RECIP * 8, RECIP * 16)
