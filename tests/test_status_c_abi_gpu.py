"""The per-replicate entries of the C ABI (pyvb_lds_get_status, pyvb_lds_set_active, pyvb_lds_get_active) from a host program
written in C (tests/c/abi_status.c), compared with the Python front end on the same inputs.  (CPU part: it compiles, links,
and the three entries refuse NULL without a device.)"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_status")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_status.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_c_host_program_compiles_and_the_entries_refuse_null(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_switches_a_failed_replicate_off(tmp_path):
    from pyvb_amd import synth
    from pyvb_amd.lds import LDSBatch
    exe = _build(tmp_path)
    N, T, D, K, bad = 4, 150, 5, 7, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=654)
    st0["Q_b"][bad] = -np.abs(st0["Q_b"][bad]) * 1e-9
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        np.array([N, T, D, K], dtype=np.float64).tofile(f)
        for a in (Y, st0["X"], st0["A_mean"], st0["A_colvar"], st0["C_mean"], st0["C_colvar"], st0["Q_b"], st0["R_b"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    r = subprocess.run([exe, str(path), str(bad)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    b = LDSBatch.from_problem(Y, st0, pri)
    b.sweep("forward")
    with pytest.raises(np.linalg.LinAlgError) as ei:
        b.sync()
    assert ei.value.replicates == [bad]
    assert "sync: " + str(ei.value) in r.stdout                         # the same message, replicate index and count included
    assert [int(v) for v in re.search(r"status((?: \d+)+)", r.stdout).group(1).split()] == list(b.status())
    mask = np.ones(N, dtype=bool); mask[bad] = False
    b.set_active(mask)
    b.iterate(2)
    assert [int(v) for v in re.search(r"active((?: \d+)+)", r.stdout).group(1).split()] == [int(m) for m in mask]
    got = [float(v) for v in re.findall(r"lower bound (\S+)", r.stdout)]
    hist = b.elbo_history(2).sum(1)
    assert np.isfinite(hist).all() and got == [hist[0], hist[1]], (got, hist)      # same library, same inputs: bitwise
    b.close()
