"""Register budget of the multi-term smoother sweep (mf_cheb_fused.hip), read from the gfx950 code object metadata: the
kernels smoother_sweep launches with its default tiles (three terms x three rows, two terms x four rows) keep two
wavefronts per SIMD (at most 256 VGPRs), spill no VGPR, and the FP64 kernels without the narrow-column body use no scratch;
the narrow-only kernels of the split launch (MFMG_MF_FUSED_NARROW=split) likewise.  Not bounded here: SGPR spills (50 - 106
per kernel, into VGPR lanes) and the 36 bytes of scratch of the kernels that carry both bodies -- the march in trips of K
super-passes does not reach the limits of <= 8 spills and no scratch; bringing the uniform state under 106 SGPRs is
separate work."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

# mf_cheb_fused_kernel<T, K, TY, DREC, MODES, DBG, NARROW_TOO, ZERO0>
KERNEL = re.compile(r"mf_cheb_fused_kernelI([df])Li(\d)ELi(\d)ELb([01])ELb([01])ELi(\d)ELb([01])ELb([01])E")
# mf_cheb_fused_narrow_kernel<T, K, TY, DREC, MODES, ZERO0>
NARROW = re.compile(r"mf_cheb_fused_narrow_kernelI([df])Li(\d)ELi(\d)ELb([01])ELb([01])ELb([01])E")


@pytest.fixture(scope="module")
def sweep_kernels(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = str(tmp_path_factory.mktemp("sweep_isa") / "mf_cheb_fused.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
           "--cuda-device-only", "-S", "mf_cheb_fused.hip", "-o", out]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    txt = open(out).read()
    kernels = {}
    for blk in txt.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        m = KERNEL.search(name.group(1)) if name else None
        mn = NARROW.search(name.group(1)) if name and not m else None
        if not m and not mn:
            continue
        field = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
        if m:
            key = (m.group(1), int(m.group(2)), int(m.group(3)), m.group(4) == "1", m.group(5) == "1", int(m.group(6)),
                   m.group(7) == "1", m.group(8) == "1")
        else:  # (narrow-only kernel: NARROW_TOO stands for "has the narrow body", DBG = -1 marks it)
            key = (mn.group(1), int(mn.group(2)), int(mn.group(3)), mn.group(4) == "1", mn.group(5) == "1", -1, True, mn.group(6) == "1")
        kernels[key] = {k: field(k) for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    return kernels


def _launched(kernels):
    return {k: v for k, v in kernels.items() if k[5] in (0, -1) and (k[1], k[2]) in ((3, 3), (2, 4))}


def test_sweep_launched_kernels_found(sweep_kernels):
    launched = _launched(sweep_kernels)
    # three terms: DREC x MODES x NARROW_TOO, plus the zero guess (mode space) with DREC x NARROW_TOO; two terms: DREC x MODES x NARROW_TOO
    assert len([k for k in launched if k[0] == "d" and k[5] == 0]) == 8 + 4 + 8
    # the narrow-only kernels: three terms DREC x MODES, the zero guess DREC, two terms DREC x MODES
    assert len([k for k in launched if k[0] == "d" and k[5] == -1]) == 4 + 2 + 4


def test_sweep_launched_kernels_registers(sweep_kernels):
    for key, v in _launched(sweep_kernels).items():
        assert v["vgpr_count"] <= 256, (key, v)
        assert v["vgpr_spill_count"] == 0, (key, v)


def test_sweep_wide_kernels_no_scratch(sweep_kernels):
    for key, v in _launched(sweep_kernels).items():
        if key[0] == "d" and not key[6]:
            assert v["private_segment_fixed_size"] == 0, (key, v)
