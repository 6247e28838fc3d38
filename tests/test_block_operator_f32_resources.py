"""Register budget of the FP32 block kernel of the matrix-free operator (mf_laplace_block.hip), read from the gfx950 code object
metadata of every instance the launch path can reach -- mf_laplace_block_f32_kernel<NV, TY, AFF>, NV = 2 and 4 vectors, TY = 2, 3
and 4 cell rows per wavefront, ids computed or read: no VGPR spill, no scratch, and the VGPR count of the occupancy the default
tile list plans: three wavefronts per SIMD at four vectors (at most 168), four at two vectors (at most
128).  The same file still yields the twelve FP64 instances under their names.  Resource fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

KERNEL_F32 = re.compile(r"mf_laplace_block_f32_kernelILi(\d)ELi(\d)ELb([01])EE")
KERNEL_F64 = re.compile(r"mf_laplace_block_kernelILi(\d)ELi(\d)ELb([01])EE")
INSTANCES = {(nv, ty, aff) for nv in (2, 4) for ty in (2, 3, 4) for aff in (False, True)}
WAVES_PER_SIMD = {2: 4, 4: 3}          # what choose_block_tile plans for the float lists (kBlockTilesF32)


def vgpr_budget(nv):
    """512 VGPRs per SIMD lane over the planned wavefronts, in the allocation granule of 8: 256, 168 or 128."""
    return (512 // WAVES_PER_SIMD[nv]) // 8 * 8


@pytest.fixture(scope="module")
def block_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    assert os.path.exists(os.path.join(CSRC, "mf_laplace_block.hip"))
    out = str(tmp_path_factory.mktemp("block_f32_isa") / "mf_laplace_block.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_laplace_block.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels = {"f32": {}, "f64": {}}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        for prec, pattern in (("f32", KERNEL_F32), ("f64", KERNEL_F64)):
            m = pattern.search(name.group(1))
            if not m:
                continue
            field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
            kernels[prec][(int(m.group(1)), int(m.group(2)), m.group(3) == "1")] = {
                k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def test_budgets_are_those_of_whole_occupancies():
    assert vgpr_budget(4) == 168 and vgpr_budget(2) == 128


def test_every_reachable_float_instance_is_there(block_kernels):
    assert set(block_kernels["f32"]) == INSTANCES


def test_the_fp64_instances_keep_their_names(block_kernels):
    assert set(block_kernels["f64"]) == INSTANCES


def test_no_spill_no_scratch_planned_occupancy(block_kernels):
    assert block_kernels["f32"]
    for (nv, ty, aff), v in sorted(block_kernels["f32"].items()):
        print(f"FP32 NV {nv} TY {ty} AFF {aff}: {v}")
        assert v["vgpr_spill_count"] == 0, ((nv, ty, aff), v)
        assert v["private_segment_fixed_size"] == 0, ((nv, ty, aff), v)
        assert v["vgpr_count"] <= vgpr_budget(nv), ((nv, ty, aff), v)
