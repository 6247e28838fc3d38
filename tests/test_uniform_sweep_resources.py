"""Register budget of the stencil sweep of a uniform coefficient (mf_cheb_fused.hip: mf_cheb_fused_uniform_kernel<double,
NARROW_TOO, ZERO0>), read from the gfx950 code object metadata.  Twelve wavefronts per workgroup, three per SIMD: at most 168
VGPRs; no VGPR spill, no scratch; and no more scalar spills than the mode-space twin of the same bodies and guess,
mf_cheb_fused_wg12d_kernel<double, true, NARROW_TOO, ZERO0>.  The same stencil on the other tile shapes
(mf_cheb_fused_uniform_rows_kernel<double, TY, ZERO0>, up to eight wavefronts, two per SIMD): at most 256 VGPRs, no VGPR spill, no
scratch."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

UNIFORM = re.compile(r"\d+mf_cheb_fused_uniform_kernelIdLb([01])ELb([01])EE")
ROWS = re.compile(r"\d+mf_cheb_fused_uniform_rows_kernelIdLi([234])ELb([01])EE")
TWIN = re.compile(r"\d+mf_cheb_fused_wg12d_kernelIdLb1ELb([01])ELb([01])EE")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


@pytest.fixture(scope="module")
def sweep_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("sweep_isa") / "mf_cheb_fused.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_cheb_fused.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels = {"uniform": {}, "twin": {}, "rows": {}}
    for blk in open(out).read().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        for kind, pat in (("uniform", UNIFORM), ("twin", TWIN), ("rows", ROWS)):
            m = pat.search(name.group(1))
            if m:
                kernels[kind][(int(m.group(1)), int(m.group(2)))] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS}
    return kernels


def test_every_instance_found(sweep_kernels):
    both = sorted((n, z) for n in (0, 1) for z in (0, 1))
    assert sorted(sweep_kernels["uniform"]) == both and sorted(sweep_kernels["twin"]) == both
    assert sorted(sweep_kernels["rows"]) == [(2, 0), (3, 0), (3, 1), (4, 0)]


def test_three_wavefronts_per_simd_no_spill_no_scratch(sweep_kernels):
    for key, v in sweep_kernels["uniform"].items():
        print("mf_cheb_fused_uniform_kernel<double, narrow %d, zero guess %d>:" % key, v)
        assert v["vgpr_count"] <= 168, (key, v)
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (key, v)


def test_no_more_scalar_spills_than_the_mode_space_twin(sweep_kernels):
    for key, v in sweep_kernels["uniform"].items():
        assert v["sgpr_spill_count"] <= sweep_kernels["twin"][key]["sgpr_spill_count"], (key, v, sweep_kernels["twin"][key])


def test_other_shapes_two_wavefronts_per_simd_no_spill_no_scratch(sweep_kernels):
    for key, v in sweep_kernels["rows"].items():
        print("mf_cheb_fused_uniform_rows_kernel<double, %d rows, zero guess %d>:" % key, v)
        assert v["vgpr_count"] <= 256 and v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (key, v)
