"""Register budget of the Q2 operator kernels (mf_laplace_q2.hip), read from the gfx950 code object metadata of every instance
the launch path can reach -- mf_laplace_q2_kernel<CX, CY, MODE, COMPACT> for the lane grids 16 x 8 and 8 x 8, the four
epilogues, 27 coefficients or one per cell, and the two diagonal kernels: no VGPR spill, no scratch, at most 256 VGPRs.
Resource fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

OPERATOR = re.compile(r"mf_laplace_q2_kernelILi(\d+)ELi(\d+)ELi(\d)ELb([01])EE")
DIAGONAL = re.compile(r"mf_laplace_q2_diagonal_kernelILb([01])EE")


@pytest.fixture(scope="module")
def q2_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("q2_isa") / "mf_laplace_q2.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_laplace_q2.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        m, d = OPERATOR.search(name.group(1)), DIAGONAL.search(name.group(1))
        if m:
            key = ("operator", int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "1")
        elif d:
            key = ("diagonal", d.group(1) == "1")
        else:
            continue
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        kernels[key] = {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def test_every_reachable_instance_is_there(q2_kernels):
    want = {("operator", cx, cy, mode, compact) for (cx, cy) in ((16, 8), (8, 8)) for mode in range(4) for compact in (False, True)}
    want |= {("diagonal", False), ("diagonal", True)}
    assert set(q2_kernels) == want


def test_no_spill_no_scratch_at_most_256_vgprs(q2_kernels):
    for key, v in sorted(q2_kernels.items(), key=str):
        print(key, v)
        assert v["vgpr_spill_count"] == 0, (key, v)
        assert v["private_segment_fixed_size"] == 0, (key, v)
        assert v["vgpr_count"] <= 256, (key, v)
