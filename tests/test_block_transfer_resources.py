"""The block kernels of the agglomerate-wise restrictor (structured_restrictor.hip), from the gfx950 code object metadata (no
GPU): the pair restriction <2> and <0>, the row restriction and the node prolongation with and without SUB, each at K = 2 and 4 --
every instance there exactly once, without VGPR or SGPR spill and without scratch.  The VGPR caps are conditions, not measurements:
at most 256 for the restriction kernels (two wavefronts per SIMD of the 512-register file, the floor below which a gather kernel has
nothing to switch to while its batch is in flight), at most 128 for the prolongation kernels (the one-vector node kernel uses 40;
K = 4 adds four sums and four y pairs per candidate).  Resource fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# mangled-name fragment (kernel and template arguments) -> VGPR cap
WANTED = {}
for k in (2, 4):
    WANTED[f"sr_restrict_pair_block_kernelILi2ELi{k}EE"] = 256
    WANTED[f"sr_restrict_pair_block_kernelILi0ELi{k}EE"] = 256
    WANTED[f"sr_restrict_rows_block_kernelILi{k}EE"] = 256
    WANTED[f"sr_prolong_block_kernelILb1ELi{k}EE"] = 128
    WANTED[f"sr_prolong_block_kernelILb0ELi{k}EE"] = 128
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    path = str(tmp_path_factory.mktemp("transfer_isa") / "structured_restrictor.s")
    cmd = [HIPCC, "--offload-arch=gfx950"] + _makefile_flags() + ["--cuda-device-only", "-S", "structured_restrictor.hip", "-o", path]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    found = {}
    for blk in open(path).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS}
    return found


def test_every_block_instance_without_spill_within_its_registers(kernels):
    assert len(WANTED) == 10
    for fragment, cap in WANTED.items():
        hits = {n: v for n, v in kernels.items() if fragment in n}
        assert len(hits) == 1, (fragment, sorted(kernels))
        (name, v), = hits.items()
        print(f"{fragment}: {v}")
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= cap, (name, v)
