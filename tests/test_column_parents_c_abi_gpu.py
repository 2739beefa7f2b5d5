"""The two read-only entries of the C ABI that say which kind of precision parent the columns of a matrix have
(pyvb_lds_get_column_parents, pyvb_pca_get_column_parents), from a host program written in C (tests/c/abi_column_parents.c).
(CPU part: they are declared, exported and bound, the program compiles and links, and a NULL handle is an argument error without
a device.)"""
import os
import re
import subprocess

import pytest

from pyvb_amd import _capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "abi_column_parents")
    lib = os.path.join(REPO, "pyvb_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "c", "abi_column_parents.c"),
           "-o", exe, "-L", lib, "-lpyvb_hip", "-lm", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    assert re.search(r"^int pyvb_lds_get_column_parents\(pyvb_lds\* h, int kind\[2\]\);", header, re.M)
    assert re.search(r"^int pyvb_pca_get_column_parents\(pyvb_pca\* h, int\* kind\);", header, re.M)
    for name in ("pyvb_lds_get_column_parents", "pyvb_pca_get_column_parents"):
        assert _capi.SIGNATURES[name] == (_capi.ctypes.c_int, [_capi._h, _capi._ip])
        assert getattr(_capi.lib, name).argtypes == [_capi._h, _capi._ip]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"pyvb_lds_get_column_parents", "pyvb_pca_get_column_parents"} <= exported
    assert _capi.lib.pyvb_version() >= 109


def test_c_host_program_compiles_and_checks_its_arguments(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "argument checks ok" in r.stdout, r.stderr


@pytest.mark.gpu
def test_c_host_program_reads_the_kind_after_every_setter(tmp_path):
    r = subprocess.run([_build(tmp_path), "device"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "done" in r.stdout, r.stderr + r.stdout
