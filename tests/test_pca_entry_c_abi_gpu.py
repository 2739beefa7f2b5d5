"""The sparse-loadings entries of the VB-PCA path of the C ABI (pyvb_pca_set_entry_precisions,
pyvb_pca_get_entry_precisions, pyvb_pca_update_entry_precisions) from a host program written in C (tests/c/abi_pca_entry.c),
against the Python front end on the same inputs.  (CPU part: it compiles, links, and a NULL handle is an argument error without a
device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import pca_entry_ref as PR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_pca_entry")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_pca_entry.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_iterates_a_handle_with_entry_parents(tmp_path):
    from pyvb_amd.pca import PCABatch
    exe = _build(tmp_path)
    niters = 3
    N, d, q = 20, 5, 2
    init, pri = PR.problem(N, d, q)
    hi, hp = PR.handle_problem(init, pri)
    assert np.all(hp["Mu_prior_mean"] == 0) and np.all(hp["Mu_prior_prec"] == 1e-3) and hp["beta_a0"] == hp["beta_b0"] == 1e-3
    b = PCABatch.from_problem(hi, hp)
    b.iterate(niters)
    total = b.elbo().sum()
    qb = b.entry_precisions()[1].ravel()
    b.close()
    assert np.isfinite(total)
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([N, d, q], dtype=np.float64).tofile(f)
        for a in (np.where(init["obs"], init["X"], np.nan), init["X"], init["W_mean"], init["Z"], init["Z_cov"], init["Mu_mean"],
                  [float(init["beta_b"])], pri["W_prior_mean"], pri["W_entry_a0"], pri["W_entry_b0"], init["W_entry_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(niters)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr + r.stdout
    got = float(re.search(r"lower bound (\S+)", r.stdout).group(1))
    assert got == pytest.approx(total, rel=1e-12), (got, total)
    vals = np.array([float(v) for v in re.search(r"^qb((?: \S+)+)", r.stdout, re.M).group(1).split()])
    assert vals == pytest.approx(qb, rel=1e-12)
