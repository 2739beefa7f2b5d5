"""The regressor entries of the C ABI (pyvb_lds_create_regressors, pyvb_lds_set / get_regressors, pyvb_lds_set_regressor_priors,
pyvb_lds_set / get_regressor_state, pyvb_lds_update_E) from a host program written in C (tests/c/abi_regressors.c), against the
Python front end on the same inputs.  (CPU part: it compiles under -Wall -Werror, links, and the entries check their arguments and
refuse what is not served without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_regressors")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_regressors.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_iterates_a_handle_with_regressors(tmp_path):
    from pyvb_amd import synth
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    N, T, D, K, Pv, niters = 3, 40, 5, 7, 2, 3
    Y, _, V, st0, pri = synth.make_regression_problem(T, D, K, 0, Pv, N, seed=32600)
    b = LDSBatch.from_problem(Y, st0, pri, V=V)
    b.iterate(niters)
    b.update_E()
    tot = b.elbo().sum(1)
    E = b.get_regressor_state(("E_mean",))["E_mean"]
    b.close()
    assert np.isfinite(tot).all()
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([N, T, D, K, Pv], dtype=np.float64).tofile(f)
        for a in (Y, V, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"], st0["E_mean"], st0["E_colvar"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(niters)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr + r.stdout
    got = [float(v) for v in re.findall(r"replicate \d+ lower bound (\S+)", r.stdout)]
    assert got == list(tot), (got, tot)                                  # same library, same inputs: bitwise
    assert [float(v) for v in re.findall(r"^E (\S+)", r.stdout, re.M)] == list(E.ravel())
