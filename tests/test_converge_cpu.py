"""CPU-only: the two entries of per-replicate convergence exist (include/pyvb_hip.h: pyvb_lds_iterate_until,
pyvb_lds_get_convergence) and check their arguments without a device, and every case tests/test_converge_gpu.py compares
stop iterations on satisfies the guard of tests/converge_ref.py: no delta of the reference within 1e-6 (relative) of tol."""
import ctypes
import os
import re

import numpy as np
import pytest

import converge_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_iterate_until", "pyvb_lds_get_convergence")


def test_entries_are_declared_bound_and_exported():
    from pyvb_amd import _capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pyvb_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), "include/pyvb_hip.h does not declare " + name
        assert name in _capi.SIGNATURES, "pyvb_amd._capi does not bind " + name
        assert hasattr(lib, name), "libpyvb_hip.so does not export " + name


def test_argument_checks_need_no_device():
    from pyvb_amd import _capi
    n = ctypes.c_int(-1)
    assert _capi.lib.pyvb_lds_iterate_until(None, 10, 1e-3, 8, ctypes.byref(n)) == _capi.E_ARG
    assert b"handle is NULL" in _capi.lib.pyvb_last_error()
    assert _capi.lib.pyvb_lds_get_convergence(None, None, None, None) == _capi.E_ARG
    assert b"handle is NULL" in _capi.lib.pyvb_last_error()
    # the other argument errors come before any HIP call too: a handle that is not one is never looked into
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for args, msg in (((-1, 1e-3, 8, ctypes.byref(n)), b"max_iters"), ((10, 1e-3, 0, ctypes.byref(n)), b"check_every"),
                      ((10, float("nan"), 8, ctypes.byref(n)), b"NaN"), ((10, 1e-3, 8, None), b"iters_run")):
        assert _capi.lib.pyvb_lds_iterate_until(fake, *args) == _capi.E_ARG, msg
        assert msg in _capi.lib.pyvb_last_error(), (msg, _capi.lib.pyvb_last_error())


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_no_case_decides_by_rounding(name):
    runs = R.alone(name)                                # asserts the guard
    assert min(r["margin"] for r in runs) >= R.GUARD
    assert all(np.isfinite(r["trace"]).all() for r in runs)


def test_the_second_call_of_case_a_does_not_decide_by_rounding():
    runs = R.resumed("A", 0.5, 40)
    assert [r["moved"] for r in runs] == [False, False, False, False, True, False]
    assert runs[4]["converged"] and runs[4]["iters"] > 40


def test_case_a_covers_what_it_is_for():
    """Stops in iterations of both parities (the two ping-pongs), a stop on a decrease (quirk Q9), a replicate that runs out."""
    runs = R.alone("A")
    stops = [r["iters"] for r in runs if r["converged"]]
    assert [r["iters"] if r["converged"] else None for r in runs] == [23, 31, 25, 10, None, 24]
    assert len(set(stops)) >= 3 and {s % 2 for s in stops} == {0, 1}
    assert any(r["converged"] and r["trace"][-1].sum() < r["trace"][-2].sum() for r in runs)
    assert sum(not r["converged"] for r in runs) == 1 and runs[4]["iters"] == 40


def test_the_other_cases_stop_where_they_were_chosen_to():
    want = {"B": [18, None, 19, 26, 28, 21], "C_reference": [2, 3], "C_exact": [8, 8], "D": [22, 3, 2, 4],
            "E": [None, 28, 33, 21], "F": [4, 2, 2, 3, 2, 2], "wishart": [None, 9, 5, 21], "nan": [8, 13, 11], "split": [None, 25, 22, 5]}
    for name, stops in want.items():
        assert [r["iters"] if r["converged"] else None for r in R.alone(name)] == stops, name
