"""The convergence entries of the C ABI (pyvb_lds_iterate_until, pyvb_lds_get_convergence) from a host program written in C
(tests/c/abi_converge.c), against the Python front end on the same inputs.  (CPU part: it compiles under -Wall -Werror, links,
and both entries check their arguments without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import converge_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_converge")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_converge.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_stops_every_replicate_where_python_does(tmp_path):
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    c = R.CASES["A"]
    Y, st0, pri, _ = R.problem("A")
    b = LDSBatch.from_problem(Y, st0, pri)
    ran = b.iterate_until(c["max_iters"], c["tol"], 8)
    iters, conv, llb = b.convergence()
    b.close()
    assert list(iters) == [r["iters"] for r in R.alone("A")]
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([c["N"], c["T"], c["D"], c["K"]], dtype=np.float64).tofile(f)
        for a in (Y, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(c["max_iters"]), repr(c["tol"]), "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    print(r.stdout)
    assert int(re.search(r"iters_run (\d+)", r.stdout).group(1)) == ran
    got = re.findall(r"replicate \d+ iters (\d+) converged (\d) llb (\S+)", r.stdout)
    assert [int(g[0]) for g in got] == list(iters)
    assert [int(g[1]) for g in got] == list(conv.astype(int))
    assert [float(g[2]) for g in got] == list(llb)                      # same library, same inputs: bitwise
