"""Register budget of the twelve-wavefront sweep kernels (mf_cheb_fused_wg12_kernel<double, MODES, NARROW_TOO, ZERO0>,
mf_cheb_fused.hip), read from the gfx950 code object metadata as test_sweep_resources.py reads that of the other sweep kernels:
three wavefronts per SIMD (at most 168 VGPRs), no VGPR spill, no scratch in the kernels of one body, and the uniform state of the
march under the scalar register file -- fewer SGPR spills than the kernels had when they re-read their coefficients and base
pointers from the kernel arguments at every use, and for the two kernels the sweep launches by default no more than
profiles/r10_a_sweep_12x2_isa.txt records."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# mf_cheb_fused_wg12_kernel<T, MODES, NARROW_TOO, ZERO0>
KERNEL = re.compile(r"mf_cheb_fused_wg12_kernelI([df])Lb([01])ELb([01])ELb([01])E")
# (MODES, NARROW_TOO, ZERO0): sgpr_spill_count before the operands were held for the tile (profiles/r09_a_sweep_12x2_isa.txt)
SGPR_SPILLS_BEFORE = {(0, 0, 0): 42, (1, 1, 1): 37, (1, 1, 0): 84, (1, 0, 1): 20, (1, 0, 0): 41}
# the two kernels of the default sweep: what holding the operands reached (profiles/r10_a_sweep_12x2_isa.txt)
SGPR_SPILLS_REACHED = {(1, 1, 0): 46, (1, 1, 1): 25}


@pytest.fixture(scope="module")
def wg12_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("sweep_12x2_isa") / "mf_cheb_fused.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_cheb_fused.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    txt = open(out).read()
    kernels = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        m = KERNEL.search(name.group(1)) if name else None
        if not m or m.group(1) != "d":
            continue
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        kernels[(int(m.group(2)), int(m.group(3)), int(m.group(4)))] = {
            k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def test_the_five_kernels_found(wg12_kernels):
    assert set(wg12_kernels) == set(SGPR_SPILLS_BEFORE)


def test_three_wavefronts_per_simd_and_no_vgpr_spill(wg12_kernels):
    for key, v in wg12_kernels.items():
        assert v["vgpr_count"] <= 168, (key, v)
        assert v["vgpr_spill_count"] == 0, (key, v)


def test_kernels_of_one_body_use_no_scratch(wg12_kernels):
    for key, v in wg12_kernels.items():
        if not key[1]:
            assert v["private_segment_fixed_size"] == 0, (key, v)


def test_fewer_sgpr_spills_than_with_operands_re_read(wg12_kernels):
    for key, v in wg12_kernels.items():
        assert v["sgpr_spill_count"] < SGPR_SPILLS_BEFORE[key], (key, v)


def test_default_kernels_keep_what_was_reached(wg12_kernels):
    for key, bound in SGPR_SPILLS_REACHED.items():
        assert wg12_kernels[key]["sgpr_spill_count"] <= bound, (key, wg12_kernels[key])
