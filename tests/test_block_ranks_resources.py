"""The kernels of blocks of vectors on several ranks, from the gfx950 code object metadata (no GPU): regions_copy_block_kernel
(vector_ops.hip: the packing and unpacking of a block halo exchange), block_dots_box_stage1_kernel with 32- and 64-bit index
arithmetic, block_cg_direction_local_kernel and block_cg_update_local_kernel (block_krylov.hip) -- every one there, without VGPR
or SGPR spill and without scratch, and within 64 VGPRs: streaming kernels that leave a SIMD its eight wavefronts.  The direction
kernel must keep the TWO roundings of p.sadd(beta, 1., z) (a multiplication and an addition, no fma in its loop): its assembly is
read for that.  Resource fields and instruction names of this project's own kernels only."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

WANTED = {"vector_ops.hip": ["regions_copy_block_kernel"],
          "block_krylov.hip": ["block_dots_box_stage1_kernelIjE", "block_dots_box_stage1_kernelIlE", "block_cg_direction_local_kernel",
                               "block_cg_update_local_kernel"]}
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("hipcc not found")
    out = {}
    for source in WANTED:
        path = str(tmp_path_factory.mktemp("ranks_isa") / (source + ".s"))
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fopenmp", "-Wall", "-Wno-unused-function",
               "--cuda-device-only", "-S", source, "-o", path]
        res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-4000:]
        out[source] = open(path).read()
    return out


def _metadata(text):
    kernels = {}
    for blk in text.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            kernels[name.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in FIELDS}
    return kernels


def test_no_spill_no_scratch_full_occupancy(assembly):
    for source, wanted in WANTED.items():
        kernels = _metadata(assembly[source])
        for w in wanted:
            hits = {n: v for n, v in kernels.items() if w in n}
            assert len(hits) == 1, (w, sorted(kernels))
            (name, v), = hits.items()
            print(f"{w}: {v}")
            assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (name, v)
            assert v["vgpr_count"] <= 64, (name, v)


def test_the_direction_on_ranks_rounds_twice(assembly):
    text = assembly["block_krylov.hip"]
    start = re.search(r"^(_Z\w*block_cg_direction_local_kernel\w*):", text, re.M)
    assert start
    body = text[start.end(): text.index(".Lfunc_end", start.end())]
    ops = re.findall(r"\b(v_(?:fma|fmac|mul|add)_f64)\w*", body)
    # the division that forms beta brings its own fma chain; behind it: the rounded product, then the sum
    assert ops[-2:] == ["v_mul_f64", "v_add_f64"], ops
