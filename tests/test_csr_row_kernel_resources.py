"""Register budget of the CSR row kernels (sparse_matrix_device.hip), read from the gfx950 code object metadata.  The row
loops keep a batch of kRowBatch entries in flight per lane (lane_row_sum), which costs registers; it must not cost
occupancy: csr_spmv_kernel<T, LPR> and csr_spmv_row_block_kernel<T> (256 threads) keep eight wavefronts per SIMD, at most
64 VGPRs; csr_spmv_lds_kernel<T, LPR> (1024 threads) stays at or under 128, four wavefronts per SIMD; csr_listed_rows_kernel,
the launch of listed_row_wave alone, at most 64; none of them spills a VGPR or uses scratch.  (listed_row_wave is also the
tail of the class, node-split and twin kernels, whose budget is set by their node bodies: not bounded here.)"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# csr_spmv_kernel<T, LPR>, csr_spmv_lds_kernel<T, LPR>, csr_spmv_row_block_kernel<T>, csr_listed_rows_kernel<T>
KERNELS = {"lanes": re.compile(r"\d+csr_spmv_kernelI([df])Li(\d+)EE"), "lds": re.compile(r"\d+csr_spmv_lds_kernelI([df])Li(\d+)EE"),
           "row_block": re.compile(r"\d+csr_spmv_row_block_kernelI([df])E"), "listed": re.compile(r"\d+csr_listed_rows_kernelI([df])E")}
VGPR_LIMIT = {"lanes": 64, "lds": 128, "row_block": 64, "listed": 64}


@pytest.fixture(scope="module")
def row_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("csr_isa") / "sparse_matrix_device.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "sparse_matrix_device.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    txt = open(out).read()
    kernels = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        for kind, pat in KERNELS.items():
            m = pat.search(name.group(1))
            if m:
                field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                key = (kind, m.group(1), int(m.group(2)) if m.lastindex == 2 else 0)
                kernels[key] = {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def test_every_instance_found(row_kernels):
    for t in "df":
        assert sorted(k[2] for k in row_kernels if k[:2] == ("lanes", t)) == [1, 2, 4, 8, 16, 32, 64]
        assert sorted(k[2] for k in row_kernels if k[:2] == ("lds", t)) == [4, 8, 16, 32, 64]
        assert ("row_block", t, 0) in row_kernels and ("listed", t, 0) in row_kernels
    assert len(row_kernels) == 2 * (7 + 5 + 1 + 1)


def test_no_spill_no_scratch(row_kernels):
    for key, v in row_kernels.items():
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (key, v)


def test_occupancy_kept(row_kernels):
    for key, v in row_kernels.items():
        assert v["vgpr_count"] <= VGPR_LIMIT[key[0]], (key, v)
