"""The FP32 fine level on several ranks (tests/dist_fp32_worker.py under torch.distributed.run, gloo, all ranks sharing one card,
the host transport) against one process: the float halo exchange, the FP32 operator, the cycle for both "is preconditioner"
settings and FGMRES with the FP32 preconditioner.  The worker's docstring states every check and bound.
  1x1x2, one ghost agglomerate below:  slabs take the packed path; two smoother terms per sweep, x two planes deep, b one
  2x1x1, two ghost agglomerates below: the whole Chebyshev(3) polynomial is one sweep, x three planes deep, b two
  2x1x2:                               edges between boxes, a rank with two split axes
  1x1x2, mixed material:               the last rank holds a coefficient that varies inside its cells and cannot sweep: the ranks
                                       agree on a launch per term for the FP32 smoother too"""
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, grid, mesh, low_ghost, timeout=600):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "tests", "dist_fp32_worker.py"), "--mesh", mesh, "--grid", grid, "--low-ghost", str(low_ghost)]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    if res.returncode != 0:
        # the first traceback of a rank (the tail of stderr is the launcher's summary)
        at = res.stderr.find("Traceback")
        raise AssertionError(res.stdout[-1500:] + (res.stderr[at:at + 3000] if at >= 0 else res.stderr[-3000:]))
    return res.stdout


@pytest.mark.parametrize("world,grid,mesh,low_ghost", [(2, "1x1x2", "cube11", 2), (2, "2x1x1", "cube11", 4), (4, "2x1x2", "cube11", 2),
                                                       (2, "1x1x2", "mixed", 2)])
def test_fp32_fine_level_on_ranks_matches_one_process(mfmg_lib, world, grid, mesh, low_ghost):
    out = _run(world, grid, mesh, low_ghost)
    print(out)
    assert "distributed fp32 checks passed; grid " + grid in out
    assert ("sweep terms 0" if mesh == "mixed" else f"sweep terms {3 if low_ghost == 4 else 2}") in out
