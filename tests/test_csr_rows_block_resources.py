"""The block forms of the CSR kernels (sparse_matrix_block_csr.hip), from the gfx950 code object metadata (no GPU):
csr_block_lanes_kernel<double, LPR, NV> for LPR = 1 .. 64, csr_block_lds_kernel<double, LPR, NV> for LPR = 4 .. 64 and
csr_block_row_kernel<double, NV>, each at NV = 2 and 4 columns -- every instance there exactly once and nothing else in the file
a kernel, none with a VGPR or SGPR spill or scratch.  The VGPR cap of 128 is a condition, not a measurement: the 1024-thread
workgroup of the LDS kernel cannot launch above it (16 wavefronts on 4 SIMDs of 512 registers), and for the 256-thread kernels
it is the four wavefronts per SIMD the other block kernels are held to.  Static LDS is what the code declares: the 4 NV
wavefront sums of the row kernel, the table rp[256 + 1] of the LDS kernel (padded to the 16-byte alignment of the windows that
follow it), nothing for the lanes kernel.  Resource fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
VGPR_CAP = 128
RP_TABLE = -(-(256 + 1) * 4 // 16) * 16

# mangled-name fragment (kernel and template arguments <double, LPR, NV> / <double, NV>) -> static LDS bytes
WANTED = {}
for nv in (2, 4):
    for lpr in (1, 2, 4, 8, 16, 32, 64):
        WANTED[f"csr_block_lanes_kernelIdLi{lpr}ELi{nv}EE"] = 0
    for lpr in (4, 8, 16, 32, 64):
        WANTED[f"csr_block_lds_kernelIdLi{lpr}ELi{nv}EE"] = RP_TABLE
    WANTED[f"csr_block_row_kernelIdLi{nv}EE"] = 4 * nv * 8
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
ONE_VECTOR_NAMES = ("csr_spmv_kernel", "csr_spmv_lds_kernel", "csr_spmv_row_block_kernel", "csr_listed_rows_kernel")


def _makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    return re.search(r"^CXXFLAGS\s*\?=\s*(.+)$", text, re.M).group(1).split()


def test_the_file_is_part_of_the_library():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "sparse_matrix_block_csr.hip" in re.search(r"^SRCS\s*=\s*(.+)$", text, re.M).group(1).split()


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    path = str(tmp_path_factory.mktemp("csr_rows_block_isa") / "sparse_matrix_block_csr.s")
    cmd = [HIPCC, "--offload-arch=gfx950"] + _makefile_flags() + ["--cuda-device-only", "-S", "sparse_matrix_block_csr.hip", "-o", path]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    found = {}
    for blk in open(path).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            found[name.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS}
    return found


def test_every_instance_without_spill_within_its_registers(kernels):
    assert len(WANTED) == 14 + 10 + 2
    assert RP_TABLE == 1040 and RP_TABLE - (256 + 1) * 4 < 16
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
    # (the tests that count the one-vector kernels find theirs by name)
    assert not [n for n in kernels if any(o in n for o in ONE_VECTOR_NAMES)]
