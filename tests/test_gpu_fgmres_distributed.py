"""Hierarchy.solve_fgmres on several ranks (tests/dist_krylov_worker.py under torch.distributed.run, gloo, all ranks sharing one
card, the host transport) against the single-process solve: the V(0,1) cycle CG cannot take on slabs, the symmetric cycle on
boxes split along x with two ghost agglomerates below (and CG beside it), the V(0,1) cycle on a 2 x 1 x 2 grid."""
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
           os.path.join(ROOT, "tests", "dist_krylov_worker.py"), "--mesh", mesh, "--grid", grid, "--low-ghost", str(low_ghost)]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    if res.returncode != 0:
        # the first traceback of a rank (the tail of stderr is the launcher's summary)
        at = res.stderr.find("Traceback")
        raise AssertionError(res.stdout[-1500:] + (res.stderr[at:at + 3000] if at >= 0 else res.stderr[-3000:]))
    return res.stdout


@pytest.mark.parametrize("world,grid,mesh,low_ghost", [(2, "1x1x2", "deep01", 2), (2, "2x1x1", "cube11", 4), (4, "2x1x2", "cube", 2)])
def test_distributed_fgmres_matches_the_single_process_solve(mfmg_lib, world, grid, mesh, low_ghost):
    out = _run(world, grid, mesh, low_ghost)
    print(out)
    assert "distributed fgmres checks passed; grid " + grid in out
    if mesh == "cube11":
        assert "cg: iterations" in out
