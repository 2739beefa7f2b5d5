"""The per-entry precision entries of the C ABI (pyvb_lds_set_entry_precisions, pyvb_lds_get_entry_precisions,
pyvb_lds_update_entry_precisions) from a host program written in C (tests/c/abi_entry.c), against the Python front end on the same
inputs.  (CPU part: it compiles, links, and a NULL handle is an argument error without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

import entry_ref as NR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_entry")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_entry.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_iterates_a_handle_with_entry_precisions(tmp_path):
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    niters = 3
    Y, st0, pri = NR.problem("d3k4_AC")
    N, T, K = Y.shape
    D = st0["A_mean"].shape[1]
    b = LDSBatch.from_problem(Y, st0, pri)
    b.iterate(niters)
    rows = b.elbo().sum(1)
    qb = {w: v[1] for w, v in b.entry_precisions().items()}
    b.close()
    assert np.isfinite(rows).all()
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([N, T, D, K], dtype=np.float64).tofile(f)
        for a in (Y, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        for w in "AC":
            for a in (pri[w + "_entry_a0"], pri[w + "_entry_b0"], st0[w + "_entry_b"]):
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(niters)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr + r.stdout
    got = [float(v) for v in re.findall(r"replicate \d+ lower bound (\S+)", r.stdout)]
    assert got == pytest.approx(list(rows), rel=1e-12), (got, rows)
    for w in "AC":
        vals = np.array([float(v) for v in re.search(r"qb %s((?: \S+)+)" % w, r.stdout).group(1).split()]).reshape(qb[w].shape)
        assert vals == pytest.approx(qb[w], rel=1e-12), w
