"""CPU: several chains, one model (pyvb_lds_create_tied) -- what needs no device.

1. tests/tied_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own run
   of a graph whose chains share A, C, Q, R (tests/golden/tied_*.npz, written by tests/golden/make_golden_tied.py) at the
   tolerance tests/test_oracle_golden.py uses for the same quantities (1e-10 relative; observed about 1e-14).
2. The two C ABI entries exist everywhere they must; the argument checks and the refusals of pyvb_lds_create_tied come before any
   HIP call; models of one replicate each are pyvb_lds_create_lengths.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import tied_ref as TR
from conftest import GOLDEN_DIR
from oracle import lds_closed_form as O
from pyvb_amd import _capi, lds, synth
from test_oracle_golden import _close, _close_qld, RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pyvb_lds_create_tied", "pyvb_lds_get_models")
TIED = sorted(glob.glob(os.path.join(GOLDEN_DIR, "tied_*.npz")))


def test_both_fixtures_are_present():
    assert [os.path.basename(p) for p in TIED] == ["tied_d4k5_t19_60_3.npz", "tied_gamma_d3k2_t7_4.npz"]


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
def _check(chains, parts, z, tag, lengths):
    for n, (st, Tn) in enumerate(zip(chains, lengths)):
        what = "%schain %d " % (tag, n)
        _close(st["X"][0], z[tag + "X"][n, :Tn], what + "X")
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        _close(st["Sigma"][0][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
        _close_qld(st["qld_x"][0][cls], z[tag + "qld_x"][n][cls], what + "qld_x")
    st = chains[0]
    _close(st["A_mean"][0], z[tag + "A_mean"], tag + "A_mean")
    _close(st["C_mean"][0], z[tag + "C_mean"], tag + "C_mean")
    for nm in ("A", "C"):
        _close(np.einsum("ikk->ik", st[nm + "_cov"][0]), z[tag + nm + "_colvar"], tag + nm + "_colvar")
        assert z[tag + nm + "_cov_offdiag_max"] == 0.0
        _close_qld(st["qld_" + nm][0], z[tag + "qld_" + nm], tag + "qld_" + nm)
    for nm in ("Q_a", "Q_b", "R_a", "R_b"):
        _close(st[nm][0], z[tag + nm], tag + nm)
    ref = z[tag + "elbo_parts"]
    _close(parts, ref, tag + "elbo_parts")
    assert abs(parts.sum() - ref.sum()) <= RTOL * abs(ref.sum())


@pytest.mark.parametrize("path", TIED, ids=lambda p: os.path.basename(p)[5:-4])
def test_tied_ref_reproduces_the_reference(path):
    meta, Ys, st0s, pri, z = TR.load_tied(path)
    chains = TR.make_model(Ys, st0s, pri)
    # qa is fixed by the graph: the children of the whole model
    nq, nr = sum(T - 1 for T in meta["lengths"]), sum(meta["lengths"])
    assert np.all(chains[0]["Q_a"] == O.noise_a(meta["noise"], pri["Q_a0"], nq, meta["D"]))
    assert np.all(chains[0]["R_a"] == O.noise_a(meta["noise"], pri["R_a0"], nr, meta["K"]))
    fwd = TR.make_model(Ys, st0s, pri)
    TR.sweep(fwd, pri, Ys, "forward")
    for n, Tn in enumerate(meta["lengths"]):
        _close(fwd[n]["X"][0], z["it1_fwd_X"][n, :Tn], "forward sweep, chain %d" % n)
    assert meta["iters"] == [1, 2, 5]
    for it in range(1, 6):
        parts = TR.iterate(chains, pri, Ys)
        if it in meta["iters"]:
            _check(chains, parts, z, "it%d_" % it, meta["lengths"])
    for st in chains[1:]:           # one set of parameters
        for k in TR.SHARED:
            assert st[k] is chains[0][k], k


def test_a_model_of_one_chain_is_the_plain_oracle():
    T, D, K = 12, 3, 4
    Y, st0, pri = synth.make_problem(T, D, K, 1, seed=31)
    chains = TR.make_model([Y], [st0], pri)
    st = O.expand_state(st0, pri, T)
    for _ in range(2):
        got, want = TR.iterate(chains, pri, [Y]), O.iterate(st, pri, Y)[0]
        assert np.array_equal(got, want)
    for k in ("X", "A_mean", "C_mean", "Q_a", "Q_b", "R_a", "R_b"):
        assert np.array_equal(chains[0][k], st[k]), k


# ---- 2. the C ABI -----------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/pyvb_hip.h"
        assert name in _capi.SIGNATURES, name + " is not bound in _capi.SIGNATURES"
        assert getattr(_capi.lib, name).argtypes == _capi.SIGNATURES[name][1]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 102


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_capi._ip)


def _create(N, T, D, K, noise, lengths, model):
    h = ctypes.c_void_p()
    ln, md = (None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (lengths, model))
    rc = _capi.lib.pyvb_lds_create_tied(ctypes.byref(h), 0, N, T, D, K, noise, _ip(ln), _ip(md))
    msg = _capi.lib.pyvb_last_error().decode()
    if rc == _capi.OK:              # a machine with a device: nothing to compare the refusal with, give the handle back
        _capi.lib.pyvb_lds_destroy(h)
    else:
        assert not h.value
    return rc, msg


@pytest.mark.parametrize("model,bad", [([1, 1, 2, 2], 0), ([0, 1, 0, 1], 2), ([0, 0, 2, 2], 2), ([0, 1, 2, 4], 3), ([0, 0, 0, -1], 3)],
                         ids=["not-from-0", "decrease", "gap", "gap-at-the-end", "negative"])
def test_bad_model_ids_are_argument_errors(model, bad):
    for lengths in (None, [10, 4, 10, 2]):
        rc, msg = _create(4, 10, 4, 5, _capi.NOISE_DIAGONAL_GAMMA, lengths, model)
        assert rc == _capi.E_ARG, (rc, msg)
        assert "replicate %d " % bad in msg and "HIP" not in msg, msg


@pytest.mark.parametrize("D,K,noise", [(4, 5, _capi.NOISE_WISHART), (65, 5, _capi.NOISE_DIAGONAL_GAMMA), (4, 65, _capi.NOISE_GAMMA)])
def test_tied_models_are_refused_where_they_are_not_served(D, K, noise):
    for lengths in (None, [10, 10, 10]):        # equal lengths: it is the model of two chains that is refused
        rc, msg = _create(3, 10, D, K, noise, lengths, [0, 1, 1])
        assert rc == _capi.E_UNSUPPORTED, (rc, msg)
        assert "share" in msg and (("Wishart" in msg) if noise == _capi.NOISE_WISHART else ("64" in msg)), msg
        assert "HIP" not in msg, msg


@pytest.mark.parametrize("D,K,noise", [(4, 5, _capi.NOISE_WISHART), (65, 5, _capi.NOISE_DIAGONAL_GAMMA), (4, 65, _capi.NOISE_GAMMA),
                                       (4, 5, _capi.NOISE_GAMMA)])
@pytest.mark.parametrize("lengths", [None, [10, 10, 10], [10, 4, 10], [10, 1, 10]])
def test_singleton_models_are_create_lengths(D, K, noise, lengths):
    """Models of one replicate each: the same status and the same message as pyvb_lds_create_lengths gives for these
    arguments -- its refusals of unequal lengths, its argument errors, and past them whatever the first HIP call says."""
    h = ctypes.c_void_p()
    want = _capi.lib.pyvb_lds_create_lengths(ctypes.byref(h), 0, 3, 10, D, K, noise, _ip(lengths))
    want_msg = _capi.lib.pyvb_last_error().decode()
    if want == _capi.OK:
        _capi.lib.pyvb_lds_destroy(h)
    for model in ([0, 1, 2], None):
        rc, msg = _create(3, 10, D, K, noise, lengths, model)
        assert rc == want, (rc, msg, want, want_msg)
        if rc != _capi.OK:
            assert msg == want_msg


def test_get_models_refuses_null():
    assert _capi.lib.pyvb_lds_get_models(None, None) == _capi.E_ARG


def test_from_trials_needs_a_series_per_model():
    with pytest.raises(ValueError):
        lds.LDSBatch.from_trials([], synth.default_priors(2, 3))
    with pytest.raises(ValueError):
        lds.LDSBatch.from_trials([[]], synth.default_priors(2, 3))
