"""The FP64 cycle on two ranks (tests/dist_sweep_diagonal_worker.py under torch.distributed.run, gloo, both ranks sharing one
card, the host transport) with the D^-1 vector of the twelve-wavefront sweep against the same cycle with D^-1 derived: equal
on the owned entries with torch.equal, the same exchanges.  The worker's docstring states the checks."""
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


def test_distributed_cycle_with_the_stored_diagonal_equals_derived(mfmg_lib):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "dist_sweep_diagonal_worker.py"), "--grid", "2x1x1"]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MFMG_MF_SWEEP_DINV", None)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    if res.returncode != 0:
        at = res.stderr.find("Traceback")
        raise AssertionError(res.stdout[-1500:] + (res.stderr[at:at + 3000] if at >= 0 else res.stderr[-3000:]))
    print(res.stdout)
    assert "distributed stored-diagonal checks passed; grid 2x1x1" in res.stdout
