"""The host arithmetic of flexible GMRES (FgmresColumn of fgmres_column.hpp: the Givens rotations of the Hessenberg columns, the
breakdown flag, the back-substitution with its zero-pivot rule) against its restatement in long double: host only, no GPU, no
library.  Both FGMRES drivers (krylov_drivers.cpp) share it; before it had a header of its own it could be reached through a
solve on the GPU alone.

The stand-alone program fgmres_column_check.cpp holds the cases and the bounds (its head says which): random columns for
m = 1, 2, 3, 8, a cycle cut short, two cycles on one object, an exactly zero sub-diagonal entry with and without a zero diagonal,
an exactly zero pivot; every value of rotate() to 32 m 2^-52 |g_0|, the least-squares residual from the unrotated columns to
32 m 2^-52 (||H||_F ||y|| + |g_0|).  It is built without sanitizers here (with them: make check-fgmres-column)."""
import os
import re
import shutil
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mfmg_amd", "csrc")


def test_the_rotations_and_the_back_substitution_against_long_double(tmp_path):
    make = shutil.which("make")
    assert make, "make is needed (the library itself is built with it)"
    exe = str(tmp_path / "fgmres_column_check")
    res = subprocess.run([make, "-C", CSRC, exe, f"FGMRES_COLUMN_CHECK={exe}", "FGMRES_COLUMN_CHECK_FLAGS="], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    held = re.fullmatch(r"(\d+) values held against long double; 0 failures\n", run.stdout)
    assert held and int(held.group(1)) > 10000, run.stdout       # (every case ran: none was compiled or looped away)


def test_the_header_takes_nothing_of_hip():
    """What makes the check above possible: fgmres_column.hpp includes the standard library alone."""
    with open(os.path.join(CSRC, "fgmres_column.hpp")) as f:
        includes = re.findall(r"^\s*#\s*include\s*(\S+)", f.read(), flags=re.M)
    assert includes and all(re.fullmatch(r"<[a-z_]+>", inc) for inc in includes), includes
