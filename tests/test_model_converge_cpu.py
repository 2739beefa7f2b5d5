"""CPU-only: the two entries of per-model convergence exist (include/pyvb_hip.h: pyvb_lds_iterate_until_model,
pyvb_lds_get_model_convergence) and check their arguments without a device; the comparator tests/model_converge_ref.py reproduces
tests/converge_ref.py where every chain is a model of its own; and every case tests/test_model_converge_gpu.py compares stop
iterations on satisfies the guard: no delta of the reference within 1e-6 (relative) of tol."""
import ctypes
import os
import re

import numpy as np
import pytest

import converge_ref as R
import model_converge_ref as MR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_iterate_until_model", "pyvb_lds_get_model_convergence")


def test_entries_are_declared_bound_and_exported():
    from pyvb_amd import _capi
    from pyvb_amd.lds import LDSBatch
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pyvb_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), "include/pyvb_hip.h does not declare " + name
        assert name in _capi.SIGNATURES, "pyvb_amd._capi does not bind " + name
        assert hasattr(lib, name), "libpyvb_hip.so does not export " + name
    assert _capi.lib.pyvb_version() >= 104
    assert callable(LDSBatch.iterate_until_model) and callable(LDSBatch.model_convergence)


def test_argument_checks_need_no_device():
    from pyvb_amd import _capi
    n = ctypes.c_int(-1)
    assert _capi.lib.pyvb_lds_iterate_until_model(None, 10, 1e-3, 8, ctypes.byref(n)) == _capi.E_ARG
    assert b"handle is NULL" in _capi.lib.pyvb_last_error()
    assert _capi.lib.pyvb_lds_get_model_convergence(None, None, None, None) == _capi.E_ARG
    assert b"handle is NULL" in _capi.lib.pyvb_last_error()
    # the other argument errors come before any HIP call too: a handle that is not one is never looked into
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    for args, msg in (((-1, 1e-3, 8, ctypes.byref(n)), b"max_iters"), ((10, 1e-3, 0, ctypes.byref(n)), b"check_every"),
                      ((10, float("nan"), 8, ctypes.byref(n)), b"NaN"), ((10, 1e-3, 8, None), b"iters_run")):
        assert _capi.lib.pyvb_lds_iterate_until_model(fake, *args) == _capi.E_ARG, msg
        assert msg in _capi.lib.pyvb_last_error(), (msg, _capi.lib.pyvb_last_error())


def test_singleton_models_reproduce_converge_ref():
    """Every chain of converge_ref's case D (ragged lengths, T_n = 2 among them) as a model of its own: the same stop iterations,
    the same parts in every iteration and the same final states as converge_ref.learn_alone on the same chains.  Both run the
    same oracle functions on the same numbers; what differs is the composition (tied_ref sums one chain's statistics, an
    addition of nothing), so the agreement asked for is 1e-13 relative, a few rounding errors."""
    mine, theirs = MR.alone("singletons"), R.alone("D")
    assert len(mine) == len(theirs) == 4
    for m, (a, b) in enumerate(zip(mine, theirs)):
        assert a["rows"] == [m] and len(a["chains"]) == 1
        assert (a["iters"], a["converged"]) == (b["iters"], b["converged"]), m
        assert a["trace"].shape == b["trace"].shape
        assert np.all(np.abs(a["trace"] - b["trace"]) <= 1e-13 * np.abs(b["trace"]).sum(1, keepdims=True)), m
        for k in ("X", "A_mean", "C_mean", "Q_b", "R_b", "Sigma"):
            assert np.allclose(a["chains"][0][k], b["st"][k], rtol=1e-12, atol=0), (m, k)


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_no_case_decides_by_rounding(name):
    runs = MR.alone(name)                               # asserts the guard
    assert min(r["margin"] for r in runs) >= MR.GUARD
    assert all(np.isfinite(r["trace"]).all() for r in runs)


def test_the_base_cases_stop_where_they_were_chosen_to():
    """The two runs of the base case: a singleton beside tied models, T_n = 2 and 3, freezes in iterations of both parities (the
    two ping-pongs), and in the first a stop on a decrease in iteration 2 (quirk Q9)."""
    want = {"reference": [9, 19, 2, 19], "exact": [10, 15, 9, 13]}
    for name, stops in want.items():
        runs = MR.alone(name)
        assert all(r["converged"] for r in runs)
        assert [r["iters"] for r in runs] == stops, name
        assert {s % 2 for s in stops} == {0, 1}
        assert [r["rows"] for r in runs] == [[0], [1, 2, 3], [4, 5], [6, 7]]
    r = MR.alone("reference")[2]
    assert abs((r["trace"][1].sum() - r["trace"][0].sum()) + 20.2) < 0.05


def test_the_large_models_stop_in_three_different_iterations():
    """Models of 5, 1 and 9 chains (tests/model_converge_ref.py: sizes_5_1_9): every model stops, each in an iteration of its own,
    odd and even ones among them."""
    runs = MR.alone("sizes_5_1_9")
    assert [len(r["rows"]) for r in runs] == [5, 1, 9] and all(r["converged"] for r in runs)
    assert [r["iters"] for r in runs] == [12, 11, 17]
    assert min(r["margin"] for r in runs) >= 10 * MR.GUARD


def test_the_other_cases_cover_what_they_are_for():
    wide = MR.alone("wide")
    assert sorted(r["converged"] for r in wide) == [False, True], "the tol of the wide case stops exactly one model"
    assert [r["iters"] for r in wide if not r["converged"]] == [MR.CASES["wide"]["max_iters"]]
    nan = MR.alone("nan")
    assert [r["rows"] for r in nan] == [[0, 1], [2]] and all(r["converged"] for r in nan)
    assert all("Yobs" in st for r in nan for st in r["chains"])


def test_the_resumed_runs_do_not_decide_by_rounding():
    """test_model_converge_gpu.py's second call: after 12 iterations models 0 and 2 have stopped and models 1 and 3 go on."""
    runs = MR.resumed("reference", 12, 8.0, 30)
    assert [r["moved"] for r in runs] == [False, True, False, True]
    assert all(r["converged"] for r in runs) and all(r["iters"] > 12 for r in runs if r["moved"])
