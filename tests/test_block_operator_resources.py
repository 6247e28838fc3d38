"""Register budget of the block kernel of the matrix-free operator (mf_laplace_block.hip), read from the gfx950 code object
metadata of every instance the launch path can reach -- mf_laplace_block_kernel<NV, TY, AFF>, NV = 2 and 4 vectors, TY = 2, 3 and
4 cell rows per wavefront, ids computed or read: no VGPR spill, no scratch, and the VGPR count of the occupancy DESIGN.md plans
(section 3): two wavefronts per SIMD at four vectors (at most 256), three at two vectors and two rows, the default tile of that
width (at most 168), two for its other tiles.  Resource fields only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

KERNEL = re.compile(r"mf_laplace_block_kernelILi(\d)ELi(\d)ELb([01])EE")


def vgpr_budget(nv, ty):
    return 168 if (nv, ty) == (2, 2) else 256


@pytest.fixture(scope="module")
def block_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    assert os.path.exists(os.path.join(CSRC, "mf_laplace_block.hip"))
    out = str(tmp_path_factory.mktemp("block_isa") / "mf_laplace_block.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_laplace_block.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels = {}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        m = KERNEL.search(name.group(1)) if name else None
        if not m:
            continue
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        kernels[(int(m.group(1)), int(m.group(2)), m.group(3) == "1")] = {
            k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def test_every_reachable_instance_is_there(block_kernels):
    assert set(block_kernels) == {(nv, ty, aff) for nv in (2, 4) for ty in (2, 3, 4) for aff in (False, True)}


def test_no_spill_no_scratch_planned_occupancy(block_kernels):
    for (nv, ty, aff), v in block_kernels.items():
        print(f"NV {nv} TY {ty} AFF {aff}: {v}")
        assert v["vgpr_spill_count"] == 0, ((nv, ty, aff), v)
        assert v["private_segment_fixed_size"] == 0, ((nv, ty, aff), v)
        assert v["vgpr_count"] <= vgpr_budget(nv, ty), ((nv, ty, aff), v)
