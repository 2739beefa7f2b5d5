"""CPU: LDS handles with a known input, X_t = Gaussian(q, A X_{t-1} + B u_t, Q) (pyvb_lds_create_inputs) -- what needs no device.

1. tests/inputs_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own run
   of such graphs (tests/golden/inputs_*.npz, written by tests/golden/make_golden_inputs.py) at the RTOL of
   tests/test_oracle_golden.py: after the first forward sweep alone and at every recorded iteration.
2. With P inputs and U = 0 the comparator's X, A, C, Q, R are oracle.iterate's.
3. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity after every stage and on every part of both bounds (two iterations;
   one at D = 64, where a long-double iteration takes seconds).  A seed that fails is replaced: this test decides.
4. The refusals and argument errors that come before any HIP call, and the seven C ABI entries.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import extended_ref as ER
import inputs_ref as IR
from conftest import GOLDEN_DIR
from oracle import lds_closed_form as O
from pyvb_amd import _capi, synth
from test_oracle_golden import _close, _close_qld, RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "inputs_*.npz")))
ENTRIES = ("pyvb_lds_create_inputs", "pyvb_lds_set_inputs", "pyvb_lds_get_inputs", "pyvb_lds_set_input_priors",
           "pyvb_lds_set_input_state", "pyvb_lds_get_input_state", "pyvb_lds_update_B")


def test_the_three_fixtures_are_present():
    assert [os.path.basename(p) for p in FIXTURES] == ["inputs_d2k5p1_t50.npz", "inputs_gamma_d3k4p2_t20.npz", "inputs_lengths_d4k5p3.npz"]
    assert RTOL == 1e-10
    for p in FIXTURES:
        assert os.path.getsize(p) < 1 << 20


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
def _check(ms, z, tag, lengths, T):
    s = IR.snapshot(ms, T)
    parts = np.concatenate([m.elbo_parts() for _, m in ms])
    assert z[tag + "cov_offdiag_max"] == 0.0            # the columns of all three matrices stay diagonal: lane = row survives
    for n, Tn in enumerate(lengths):
        what = "%schain %d " % (tag, n)
        m = [m for rows, m in ms if n in rows][0]
        r = [rows.index(n) for rows, _ in ms if n in rows][0]
        _close(s["X"][n, :Tn], z[tag + "X"][n, :Tn], what + "X")
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        _close(s["Sigma"][n][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
        _close_qld(m.st["qld_x"][r][cls], z[tag + "qld_x"][n][cls], what + "qld_x")
        for w in "ABC":
            _close(s[w + "_mean"][n], z[tag + w + "_mean"][n], what + w + "_mean")
            _close(s[w + "_colvar"][n], z[tag + w + "_colvar"][n], what + w + "_colvar")
            _close_qld(m.st["qld_" + w][r], z[tag + "qld_" + w][n], what + "qld_" + w)
        for nm in ("Q_a", "Q_b", "R_a", "R_b"):
            _close(m.st[nm][r], z[tag + nm][n], what + nm)
        ref = z[tag + "elbo_parts"][n]
        print(what, "parts", parts[n], "reference", ref)
        _close(parts[n], ref, what + "elbo_parts")
        assert abs(parts[n].sum() - ref.sum()) <= RTOL * abs(ref.sum())


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[7:-4])
def test_inputs_ref_reproduces_the_reference(path):
    meta, Y, U, st0, pri, lengths, z = IR.load_fixture(path)
    T = Y.shape[1]
    ms = IR.models(Y, U, st0, pri, lengths)
    assert meta["iters"] == [1, 2, 5] and U.shape[2] == meta["P"]
    for it in range(1, 6):
        if it == 1:         # the forward sweep alone, then the rest of the iteration stage by stage
            for _, m in ms:
                m.sweep("forward")
            fwd = IR.snapshot(ms, T)["X"]
            for n, Tn in enumerate(lengths):
                _close(fwd[n, :Tn], z["it1_fwd_X"][n, :Tn], "forward sweep alone, chain %d" % n)
            for _, m in ms:
                for stage in ("backward", "A", "B", "C", "Q", "R"):
                    IR.do_stage(m, stage)
        else:
            for _, m in ms:
                m.iterate()
        if it in meta["iters"]:
            _check(ms, z, "it%d_" % it, lengths, T)


def test_the_fixtures_cover_both_noise_kinds_and_the_shortest_chain():
    metas = [IR.load_fixture(p)[0] for p in FIXTURES]
    assert [m["noise"] for m in metas] == ["diagonal_gamma", "gamma", "diagonal_gamma"]
    assert [(m["D"], m["K"], m["P"]) for m in metas] == [(2, 5, 1), (3, 4, 2), (4, 5, 3)]
    assert [m["lengths"] for m in metas] == [[50], [20], [2, 7, 20]]


# ---- 2. no input: the plain graph -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["diagonal_gamma", "gamma"])
def test_with_zero_inputs_the_comparator_is_the_oracle(noise):
    T, D, K, P, N = 9, 3, 4, 2, 2
    Y, U, st0, pri = synth.make_input_problem(T, D, K, P, N, seed=5)
    if noise == "gamma":
        pri["noise"] = "gamma"
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    m = IR.Model(Y, np.zeros_like(U), st0, pri)
    st = O.expand_state(IR.split_inputs(st0)[0], pri, T)
    for it in range(3):
        m.iterate()
        O.iterate(st, pri, Y, with_elbo=False)
        for k in ("X", "A_mean", "A_cov", "C_mean", "C_cov", "Q_b", "R_b"):
            _close(m.st[k], st[k], "iteration %d %s" % (it + 1, k), rtol=1e-13)
    # B has gone to its prior: no input, no evidence
    assert not np.any(pri["B_prior_mean"]) and np.abs(m.st["B_mean"]).max() == 0.0
    _close(np.einsum("nikk->nik", m.st["B_cov"]), np.broadcast_to(1.0 / pri["B_prior_prec"], (N, P, D)), "B_colvar", rtol=1e-13)


# ---- 3. the float64 comparator against its extended-precision run -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IR.CASES))
def test_float64_comparator_is_inside_the_guard(name):
    f64, ext = IR.trace(name), IR.trace(name, extended=True)
    assert ext[0][1].dtype == ER.LD
    per_iter = len(f64) // IR.ITERS
    assert len(ext) == per_iter * IR.CASES[name][6] and IR.CASES[name][6] == (1 if name == "t40_d64k40p12" else IR.ITERS)
    for (k64, v64), (kx, vx) in zip(f64, ext):
        assert k64 == kx
        e = ER.bound_errors(v64, vx)[0].max() if k64[1] == "bound" else ER.rel(v64, vx)
        print("iteration %d %-9s %-10s e64 %.2e" % (k64[0] + 1, k64[1], k64[2], e))
        assert e <= ER.CAP, (name, k64, e)


def test_the_cases_are_the_ones_the_device_is_measured_on():
    assert {k: v[:4] for k, v in IR.CASES.items()} == {
        "t19_d6k4p2": (19, 6, 4, 2), "t33_d5k15p1": (33, 5, 15, 1), "t77_d16k16p8": (77, 16, 16, 8), "t40_d64k40p12": (40, 64, 40, 12),
        "t700_d8k8p3_w4": (700, 8, 8, 3), "lengths_d16k10p3": (77, 16, 10, 3)}
    assert IR.CASES["lengths_d16k10p3"][4] == (2, 3, 19, 60, 77) and IR.CASES["t700_d8k8p3_w4"][5] == 4


# ---- 4. refusals, argument errors, the C ABI --------------------------------------------------------------------------------
def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_capi._ip)


def _create(N, T, D, K, P, noise, lengths=None):
    h = ctypes.c_void_p()
    rc = _capi.lib.pyvb_lds_create_inputs(ctypes.byref(h), 0, N, T, D, K, P, noise, _ip(lengths))
    msg = _capi.lib.pyvb_last_error().decode()
    if rc == _capi.OK:              # a machine with a device: nothing to compare the refusal with, give the handle back
        _capi.lib.pyvb_lds_destroy(h)
    else:
        assert not h.value
    return rc, msg


@pytest.mark.parametrize("D,K,P,noise,word", [(4, 5, 2, _capi.NOISE_WISHART, "Wishart"), (65, 5, 1, _capi.NOISE_DIAGONAL_GAMMA, "max(D, K + 2 P) <= 64"),
                                              (4, 61, 2, _capi.NOISE_GAMMA, "max(D, K + 2 P) <= 64"), (4, 3, 31, _capi.NOISE_GAMMA, "max(D, K + 2 P) <= 64")])
def test_handles_with_inputs_are_refused_where_they_are_not_served(D, K, P, noise, word):
    for lengths in (None, [10, 4, 10]):
        rc, msg = _create(3, 10, D, K, P, noise, lengths)
        assert rc == _capi.E_UNSUPPORTED, (rc, msg)
        assert "inputs" in msg and word in msg and "HIP" not in msg, msg


@pytest.mark.parametrize("P", [0, -1])
def test_fewer_than_one_input_is_an_argument_error(P):
    rc, msg = _create(3, 10, 4, 5, P, _capi.NOISE_DIAGONAL_GAMMA)
    assert rc == _capi.E_ARG and "P must be >= 1" in msg, (rc, msg)


def test_bad_lengths_are_named_as_on_a_plain_handle():
    rc, msg = _create(3, 10, 4, 5, 2, _capi.NOISE_DIAGONAL_GAMMA, [10, 1, 10])
    assert rc == _capi.E_ARG and "1" in msg, (rc, msg)


def test_shared_models_take_no_inputs():
    from pyvb_amd.lds import LDSBatch
    with pytest.raises(NotImplementedError):
        LDSBatch(2, 6, 3, 4, inputs=2, models=[0, 0])


def test_a_null_handle_is_an_argument_error():
    v = np.ones(4)
    p = _capi.dptr(v)
    lib = _capi.lib
    for rc in (lib.pyvb_lds_set_inputs(None, p), lib.pyvb_lds_get_inputs(None, p), lib.pyvb_lds_set_input_priors(None, p, p),
               lib.pyvb_lds_set_input_state(None, p, p), lib.pyvb_lds_get_input_state(None, p, p, p, p), lib.pyvb_lds_update_B(None)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in lib.pyvb_last_error()
    assert lib.pyvb_lds_create_inputs(None, 0, 1, 4, 2, 2, 1, 0, None) == _capi.E_ARG


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        ENTRIES[0]: r"int pyvb_lds_create_inputs\(pyvb_lds\*\* out, int device, int N, int T, int D, int K, int P, int noise_kind, const int\* lengths\);",
        ENTRIES[1]: r"int pyvb_lds_set_inputs\(pyvb_lds\* h, const double\* U\);",
        ENTRIES[2]: r"int pyvb_lds_get_inputs\(pyvb_lds\* h, double\* U\);",
        ENTRIES[3]: r"int pyvb_lds_set_input_priors\(pyvb_lds\* h, const double\* B_prior_mean, const double\* B_prior_prec\);",
        ENTRIES[4]: r"int pyvb_lds_set_input_state\(pyvb_lds\* h, const double\* B_mean, const double\* B_colvar\);",
        ENTRIES[5]: r"int pyvb_lds_get_input_state\(pyvb_lds\* h, double\* B_mean, double\* B_colvar, double\* qld_B, double\* lnd_B\);",
        ENTRIES[6]: r"int pyvb_lds_update_B\(pyvb_lds\* h\);",
    }
    c, dp, ip, h = ctypes.c_int, _capi._dp, _capi._ip, _capi._h
    args = {ENTRIES[0]: [ctypes.POINTER(h)] + [c] * 7 + [ip], ENTRIES[1]: [h, dp], ENTRIES[2]: [h, dp], ENTRIES[3]: [h, dp, dp],
            ENTRIES[4]: [h, dp, dp], ENTRIES[5]: [h, dp, dp, dp, dp], ENTRIES[6]: [h]}
    for name in ENTRIES:
        assert re.search("^" + decl[name], header, re.M), name + " is not declared as specified in include/pyvb_hip.h"
        assert _capi.SIGNATURES[name] == (c, args[name]), name
        assert getattr(_capi.lib, name).argtypes == args[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 110
    assert "max(D, K + 2 P) <= 64" in header


def test_the_generator_of_driven_problems_leaves_make_problem_alone():
    Y, U, st0, pri = synth.make_input_problem(12, 3, 4, 2, 2, seed=77)
    assert Y.shape == (2, 12, 4) and U.shape == (2, 12, 2) and np.all(U[:, 0] == 0.0)
    assert st0["B_mean"].shape == (2, 3, 2) and st0["B_colvar"].shape == (2, 2, 3)
    assert pri["B_prior_mean"].shape == (3, 2) and pri["B_prior_prec"].shape == (2, 3)
    _, st1, pri1 = synth.make_problem(12, 3, 4, 2, seed=77)
    for k in st1:           # the same initial state beside B: a driven and a plain problem of one seed differ in the data only
        assert np.array_equal(st0[k], st1[k]), k
    assert sorted(set(pri) - set(pri1)) == ["B_prior_mean", "B_prior_prec"]


def test_pad_series_carries_the_input_gain():
    from pyvb_amd.lds import pad_series
    Y, U, st0, pri = synth.make_input_problem(9, 3, 4, 2, 3, seed=78)
    ln = [9, 2, 5]
    series = [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(ln)]
    Yp, sp, lp = pad_series(series)
    assert list(lp) == ln and np.array_equal(sp["B_mean"], st0["B_mean"]) and np.array_equal(sp["B_colvar"], st0["B_colvar"])
