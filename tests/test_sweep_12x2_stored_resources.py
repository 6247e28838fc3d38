"""Register budget of the twelve-wavefront sweep kernels that read D^-1 from the operator's vector
(mf_cheb_fused_wg12d_kernel<double, MODES, NARROW_TOO, ZERO0>, mf_cheb_fused.hip), read from the gfx950 code object metadata
as test_sweep_12x2_resources.py reads that of the kernels that derive it (mf_cheb_fused_wg12_kernel, their twins): three
wavefronts per SIMD (at most 168 VGPRs), no VGPR spill, no scratch in the kernels of one body, no more vector registers and no
more SGPR spills than the twin of the same build, and no FP64 division left in the march -- what remains of v_rcp_f64 and
v_div_* is the handful outside it.

Figures of the build this test came with (profiles/r11_a_sweep_isa.txt; test_figures_of_this_build prints the current ones),
(MODES, NARROW_TOO, ZERO0): VGPRs stored / derived, sgpr_spill_count stored / derived:
  (0, 0, 0) 163 / 163, 11 / 17      (1, 0, 0) 159 / 161, 5 / 7      (1, 0, 1) 132 / 134, 0 / 0
  (1, 1, 0) 167 / 167, 44 / 46      (1, 1, 1) 143 / 143, 25 / 25
With the address of the D^-1 vector as a sixth scalar pointer the two kernels that carry both bodies had 53 and 31 spills; the
kernels hold it, and one of the five base addresses, in vector register pairs (mf_cheb_fused_body, kHeldBase)."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# mf_cheb_fused_wg12_kernel / mf_cheb_fused_wg12d_kernel<T, MODES, NARROW_TOO, ZERO0>
KERNEL = re.compile(r"mf_cheb_fused_wg12(d?)_kernelI([df])Lb([01])ELb([01])ELb([01])E")
KEYS = {(0, 0, 0), (1, 1, 1), (1, 1, 0), (1, 0, 1), (1, 0, 0)}
# An IEEE FP64 division is v_div_scale (one or two: the numerator here is the constant 1), v_rcp_f64, v_div_fmas, v_div_fixup:
# at least four of these.  The march of a body is unrolled over its trip of three super-passes with three node rows each: nine
# divisions, 36 and more per body where D^-1 is derived.  A kernel with fewer than two divisions' worth has none in its march
# (what remains belongs to the prologue of a tile)
DIVISION_OPS_OUTSIDE_THE_MARCH = 7
DIVISION_OP = re.compile(r"^\s*(v_rcp_f64|v_div_\w+)\b", re.M)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("sweep_12x2_stored_isa") / "mf_cheb_fused.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_cheb_fused.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    txt = open(out).read()
    found = {"": {}, "d": {}}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        m = KERNEL.search(name.group(1)) if name else None
        if not m or m.group(2) != "d":
            continue
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        v = {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
        # the kernel's text: from its label to the end of the function
        at = re.search(r"^" + re.escape(name.group(1)) + r":", txt, re.M)
        assert at, name.group(1)
        v["division_ops"] = len(DIVISION_OP.findall(txt[at.end():txt.find(".Lfunc_end", at.end())]))
        found[m.group(1)][(int(m.group(3)), int(m.group(4)), int(m.group(5)))] = v
    return found


def test_figures_of_this_build(kernels):
    for key in sorted(KEYS):
        s, d = kernels["d"].get(key), kernels[""].get(key)
        print(key, "stored", s, "derived", d)


def test_the_five_kernels_found_beside_their_twins(kernels):
    assert set(kernels["d"]) == KEYS and set(kernels[""]) == KEYS


def test_three_wavefronts_per_simd_and_no_vgpr_spill(kernels):
    for key, v in kernels["d"].items():
        assert v["vgpr_count"] <= 168, (key, v)
        assert v["vgpr_spill_count"] == 0, (key, v)


def test_kernels_of_one_body_use_no_scratch(kernels):
    for key, v in kernels["d"].items():
        if not key[1]:
            assert v["private_segment_fixed_size"] == 0, (key, v)


def test_no_more_vector_registers_than_the_derived_twin(kernels):
    for key, v in kernels["d"].items():
        assert v["vgpr_count"] <= kernels[""][key]["vgpr_count"], (key, v, kernels[""][key])


def test_no_more_sgpr_spills_than_the_derived_twin(kernels):
    for key, v in kernels["d"].items():
        assert v["sgpr_spill_count"] <= kernels[""][key]["sgpr_spill_count"], (key, v, kernels[""][key])


def test_no_division_left_in_the_march(kernels):
    for key, v in kernels["d"].items():
        assert v["division_ops"] <= DIVISION_OPS_OUTSIDE_THE_MARCH, (key, v)
        assert kernels[""][key]["division_ops"] >= 36, (key, kernels[""][key])   # (the pattern does find the divisions of the twin)
