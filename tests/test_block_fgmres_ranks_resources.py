"""The kernels of block FGMRES and of the FP32 block level on several ranks, from the gfx950 code object metadata (no GPU), after
tests/test_block_ranks_resources.py: the owned-box block kernels of block_krylov_basis.hip -- dots, update (with and without the
norm), norm partials, scale_store, each with 32- and 64-bit walks over the rows of the box, and the two finish kernels -- and
regions_copy_block_f32_kernel (vector_ops.hip: the packing and unpacking of a float block halo exchange).  Every one is there,
without VGPR or SGPR spill and without scratch, and allocates no more VGPRs than leave a SIMD the wavefronts the one-rank block
kernel of the same pass leaves it, compiled in the same run (512 VGPRs per lane of a SIMD, allocated in granules of 8, at most 8
wavefronts).  The counts are printed.  Resource fields of this project's own kernels only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# new kernel (a piece of its mangled name: I j E = uint32_t, I l E = int64_t) -> the one-rank block kernel of the same pass
PASSES = {
    "block_krylov_basis.hip": {
        "15box_dots_kernelIjE": "11dots_kernelE", "15box_dots_kernelIlE": "11dots_kernelE",
        "15box_axpy_kernelILb1EjE": "11axpy_kernelILi2ELb1EE", "15box_axpy_kernelILb1ElE": "11axpy_kernelILi2ELb1EE",
        "15box_axpy_kernelILb0EjE": "11axpy_kernelILi2ELb0EE", "15box_axpy_kernelILb0ElE": "11axpy_kernelILi2ELb0EE",
        "24box_norm_partials_kernelIjE": "20norm_partials_kernelE", "24box_norm_partials_kernelIlE": "20norm_partials_kernelE",
        "22box_scale_store_kernelIjE": "18scale_store_kernelE", "22box_scale_store_kernelIlE": "18scale_store_kernelE",
        "22box_dots_finish_kernelE": "18dots_finish_kernelE", "18norm_finish_kernelE": "18dots_finish_kernelE",
    },
    "vector_ops.hip": {"29regions_copy_block_f32_kernelE": "25regions_copy_block_kernelE"},
}
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


def waves_per_simd(vgprs):
    return min(8, 512 // max(8, -(-vgprs // 8) * 8))


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = {}
    for source in PASSES:
        path = str(tmp_path_factory.mktemp("fgmres_ranks_isa") / (source + ".s"))
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
               "--cuda-device-only", "-S", source, "-o", path]
        res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        found = {}
        for blk in open(path).read().split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name:
                found[name.group(1)] = dict({k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS},
                                            agpr_count=int(blk.split()[0]))
        out[source] = found
    return out


def _one(found, piece):
    hits = {n: v for n, v in found.items() if piece in n}
    assert len(hits) == 1, (piece, sorted(found))
    return next(iter(hits.items()))


def test_the_waves_of_a_register_count():
    assert [waves_per_simd(v) for v in (1, 64, 65, 72, 73, 128, 129, 168, 256, 512)] == [8, 8, 7, 7, 6, 4, 3, 3, 2, 1]


def test_no_spill_no_scratch_and_the_occupancy_of_the_one_rank_kernels(kernels):
    for source, passes in PASSES.items():
        for new, old in passes.items():
            name, v = _one(kernels[source], new)
            _, ref = _one(kernels[source], old)
            registers, ref_registers = v["vgpr_count"] + v["agpr_count"], ref["vgpr_count"] + ref["agpr_count"]
            print(f"{new}: {v} -> {waves_per_simd(registers)} wavefronts per SIMD; {old}: {ref_registers} VGPRs -> {waves_per_simd(ref_registers)}")
            assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
            assert waves_per_simd(registers) >= waves_per_simd(ref_registers), (name, v, ref)
