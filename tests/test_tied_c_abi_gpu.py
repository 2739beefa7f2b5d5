"""The shared-parameter entries of the C ABI (pyvb_lds_create_tied, pyvb_lds_get_models) from a host program written in C
(tests/c/abi_tied.c), against the Python front end on the same inputs.  (CPU part: it compiles, links, and the entries check
their arguments and refuse what is not served without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_tied")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_tied.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_iterates_a_tied_handle(tmp_path):
    from pyvb_amd import synth
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    N, T, D, K, niters = 6, 60, 4, 5, 3
    lengths = np.array([19, 60, 2, 33, 3, 17], dtype=np.int32)
    models = np.array([0, 1, 1, 1, 2, 2], dtype=np.int32)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=9300)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=lengths, models=models)
    b.iterate(niters)
    rows = b.elbo().sum(1)
    tot = [float(sum(rows[n] for n in range(N) if models[n] == m)) for m in range(3)]       # row by row, as the C program adds
    hist = b.elbo_history(1).sum(1)
    b.close()
    assert np.isfinite(tot).all()
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([N, T, D, K], dtype=np.float64).tofile(f)
        lengths.astype(np.float64).tofile(f)
        models.astype(np.float64).tofile(f)
        for a in (Y, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(niters), "1", repr(tot[1]), "2", repr(tot[2])], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert "compared models 1 and 2" in r.stdout
    assert [int(v) for v in re.search(r"models((?: \d+)+)", r.stdout).group(1).split()] == list(models)
    got = [float(v) for v in re.findall(r"model \d+ lower bound (\S+)", r.stdout)]
    assert got == pytest.approx(tot, rel=1e-12), (got, tot)
    assert float(re.search(r"history (\S+)", r.stdout).group(1)) == pytest.approx(hist[0], rel=1e-12)
