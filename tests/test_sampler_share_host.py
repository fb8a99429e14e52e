"""The register budgets the alias table's indirection must not disturb (shared replays, DESIGN.md
section 3.3), read from the gfx950 assembly of csrc/kernels.hip as tests/test_gram_pipeline_host.py
does (device-only compile with the build's flags; no GPU): the wide Gram kernel reads the
representative's selection words through one more scalar index and stays at 256 VGPRs without
scratch (2 waves per SIMD); the throughput sampler loads one more scalar before its early return
and stays at no more than 80 VGPRs without scratch (6 waves per SIMD, the launch tiers' premise)."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

from erp_match_eightpoint_test_amd import _build

KERNELS = {"gram_mfma_kernelILi2E": 256, "sampler_kernelILi0E": 80}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = tmp_path_factory.mktemp("share_asm") / "kernels.s"
    cmd = [_build.HIPCC, *_build.CXXFLAGS, "-I", os.path.join(_build.ROOT, "include"),
           "-I", _build.CSRC, "--cuda-device-only", "-S", os.path.join(_build.CSRC, "kernels.hip"),
           "-o", str(out)]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    text = out.read_text()
    found = {}
    for name in KERNELS:
        m = re.search(r"^(_ZN\S*%s\S*):.*?^\s*\.end_amdhsa_kernel" % name, text, re.M | re.S)
        assert m, f"{name} not in the assembly"
        found[name] = m.group(0)
    return found


def _directive(text: str, name: str) -> int:
    m = re.search(r"^\s*\.amdhsa_%s\s+(\d+)\s*$" % name, text, re.M)
    assert m, name
    return int(m.group(1))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_register_budget_with_the_alias_index(kernels, name):
    k = kernels[name]
    assert _directive(k, "private_segment_fixed_size") == 0
    assert _directive(k, "next_free_vgpr") <= KERNELS[name]
    assert not re.search(r"\bscratch_", k)
