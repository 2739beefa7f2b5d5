"""The per-model convergence entries of the C ABI (pyvb_lds_iterate_until_model, pyvb_lds_get_model_convergence) from a host
program written in C (tests/c/abi_model_converge.c), against the comparator and the Python front end on the same inputs.  (CPU
part: it compiles, links, and the entries check their arguments without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import model_converge_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_model_converge")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_model_converge.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_runs_every_model_to_its_own_stop(tmp_path):
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    name = "reference"
    c, runs = MR.CASES[name], MR.alone(name)
    Y, st0, pri, lengths, models = MR.problem(name)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=lengths, models=models)
    n_py = b.iterate_until_model(c["max_iters"], c["tol"], 1)
    it, cv, llb = b.model_convergence()
    b.close()
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([c["N"], c["T"], c["D"], c["K"]], dtype=np.float64).tofile(f)
        lengths.astype(np.float64).tofile(f)
        models.astype(np.float64).tofile(f)
        for a in (Y, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(c["max_iters"]), repr(c["tol"])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr + r.stdout
    print(r.stdout)
    got = re.findall(r"model (\d+): (\d+) iterations, (converged|still running), lower bound (\S+)", r.stdout)
    assert [int(g[0]) for g in got] == list(range(len(runs)))
    assert [int(g[1]) for g in got] == [r_["iters"] for r_ in runs] == list(it)
    assert [g[2] == "converged" for g in got] == [r_["converged"] for r_ in runs] == list(cv)
    assert [float(g[3]) for g in got] == list(llb)      # the same library on the same inputs
    assert int(re.search(r"iterations launched (\d+)", r.stdout).group(1)) == n_py == max(r_["iters"] for r_ in runs)
