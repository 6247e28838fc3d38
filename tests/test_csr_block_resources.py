"""The block kernels of the stored-value SpMV (sparse_matrix_block.hip), from the gfx950 code object metadata (no GPU):
bdia_sym_split_block_kernel and bdia_spmv_block_kernel for 1..4 unknowns per node with double and float planes, and
rowbase_spmv_block_kernel, each at NV = 2 and 4 columns -- every instance there exactly once, without VGPR or SGPR spill and
without scratch.  The VGPR cap of 128 is a condition, not a measurement: it is what the 1024-thread workgroup of the split
kernel allows (16 wavefronts on 4 SIMDs of 512 registers), and for the 256-thread kernels it is four wavefronts per SIMD, which
hide their gathers by switching.  The split kernel's LDS is the three quarter sums of NV columns: 3 NV 256 doubles.  Resource
fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
VGPR_CAP = 128

# mangled-name fragment (kernel and template arguments <double, C, V, NV> / <double, NV>) -> LDS bytes
WANTED = {}
for nv in (2, 4):
    for c in (1, 2, 3, 4):
        for v in "df":
            WANTED[f"bdia_sym_split_block_kernelIdLi{c}E{v}Li{nv}EE"] = 3 * nv * 256 * 8
            WANTED[f"bdia_spmv_block_kernelIdLi{c}E{v}Li{nv}EE"] = 0
    WANTED[f"rowbase_spmv_block_kernelIdLi{nv}EE"] = 0
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    path = str(tmp_path_factory.mktemp("csr_block_isa") / "sparse_matrix_block.s")
    cmd = [HIPCC, "--offload-arch=gfx950"] + _makefile_flags() + ["--cuda-device-only", "-S", "sparse_matrix_block.hip", "-o", path]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    found = {}
    for blk in open(path).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS}
    return found


def test_every_block_instance_without_spill_within_its_registers(kernels):
    assert len(WANTED) == 2 * (2 * 4 * 2 + 1)
    for fragment, lds in WANTED.items():
        hits = {n: v for n, v in kernels.items() if fragment in n}
        assert len(hits) == 1, (fragment, sorted(kernels))
        (name, v), = hits.items()
        print(f"{fragment}: {v}")
        assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
        assert v["vgpr_count"] <= VGPR_CAP, (name, v)
        assert v["group_segment_fixed_size"] == lds, (name, v)
    # (nothing else in the file is a kernel: an instance outside the table would run untested)
    assert len(kernels) == len(WANTED), sorted(kernels)
