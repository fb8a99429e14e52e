"""The register budget and the wait structure the Gram kernel's pipelined K step rests on, read
from the gfx950 assembly of csrc/kernels.hip (device-only compile with the build's flags; no
GPU): no scratch, no AGPR split, two waves per SIMD at two row tiles and three at one, and the
B-fragment reads waited for with counted lgkmcnts -- a later edit that spills or re-serialises
the loop fails here."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from erp_match_eightpoint_test_amd import _build


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{WT: (kernel text from its label to .end_amdhsa_kernel)} of gram_mfma_kernel<1>, <2>"""
    out = tmp_path_factory.mktemp("gram_asm") / "kernels.s"
    cmd = [_build.HIPCC, *_build.CXXFLAGS, "-I", os.path.join(_build.ROOT, "include"),
           "-I", _build.CSRC, "--cuda-device-only", "-S", os.path.join(_build.CSRC, "kernels.hip"),
           "-o", str(out)]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    text = out.read_text()
    found = {}
    for wt in (1, 2):
        m = re.search(r"^(_ZN\S*gram_mfma_kernelILi%dE\S*):.*?^\s*\.end_amdhsa_kernel" % wt, text,
                      re.M | re.S)
        assert m, f"gram_mfma_kernel<{wt}> not in the assembly"
        found[wt] = m.group(0)
    return found


def _directive(text: str, name: str) -> int:
    m = re.search(r"^\s*\.amdhsa_%s\s+(\d+)\s*$" % name, text, re.M)
    assert m, name
    return int(m.group(1))


@pytest.mark.parametrize("wt,max_vgpr", [(1, 168), (2, 256)])
def test_register_budget(kernels, wt, max_vgpr):
    k = kernels[wt]
    assert _directive(k, "private_segment_fixed_size") == 0
    nv = _directive(k, "next_free_vgpr")
    assert nv <= max_vgpr
    # unified register file, allocated in blocks of 4 (8 from 256 on is still 256): no AGPRs
    assert _directive(k, "accum_offset") == (nv + 3) // 4 * 4
    assert not re.search(r"\bscratch_|\bv_accvgpr_", k)


@pytest.mark.parametrize("wt", [1, 2])
def test_counted_waits_in_the_k_loop(kernels, wt):
    lines = kernels[wt].splitlines()
    mf = [i for i, l in enumerate(lines) if "v_mfma_i32_32x32x32_i8" in l]
    assert len(mf) == 14 * wt  # one unrolled K step
    body = lines[mf[0]:mf[-1] + 1]
    waits = [l for l in body if re.search(r"\bs_waitcnt\b", l)]
    drains = [l for l in waits if re.search(r"lgkmcnt\(0\)", l)]
    assert len(drains) <= 2, drains
    assert any(re.search(r"lgkmcnt\([1-9]\d*\)", l) for l in waits)
    assert sum("ds_read_b128" in l for l in body) >= 10  # the reads ride between the MFMAs
