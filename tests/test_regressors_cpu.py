"""CPU: LDS handles with known regressors in the output equation, Y_t = Gaussian(K, C X_t + E v_t, R) (pyvb_lds_create_regressors) --
what needs no device.

1. tests/regressors_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own
   run of such graphs (tests/golden/regressors_*.npz, written by tests/golden/make_golden_regressors.py) at the RTOL of
   tests/test_oracle_golden.py: after the first forward sweep alone and at every recorded iteration.
2. With V = 0 the comparator's X, A, C, Q, R are those of the graph without regressors.
3. On the cases the device is measured on, the float64 comparator lies within the guard of DESIGN.md section 17 of its own
   extended-precision run: e64 <= 1e-11 on every quantity after every stage and on every part of both bounds.
4. Planted defects -- Svx not subtracted in H_C, the cross term of R counted once, the v_t channel live in a padding row, v_0
   dropped -- leave the envelope e <= 16 max(e64, n 2^-52) that the device is held to: the comparison can see them.
5. The refusals and argument errors that come before any HIP call, and the seven C ABI entries.
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
import regressors_ref as RR
from conftest import GOLDEN_DIR
from oracle import lds_closed_form as O
from pyvb_amd import _capi, synth
from test_oracle_golden import _close, _close_qld, RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "regressors_*.npz")))
ENTRIES = ("pyvb_lds_create_regressors", "pyvb_lds_set_regressors", "pyvb_lds_get_regressors", "pyvb_lds_set_regressor_priors",
           "pyvb_lds_set_regressor_state", "pyvb_lds_get_regressor_state", "pyvb_lds_update_E")


def test_the_three_fixtures_are_present():
    assert [os.path.basename(p) for p in FIXTURES] == ["regressors_gamma_d3k4p2v1_t20.npz", "regressors_lengths_d4k5p1v2.npz",
                                                       "regressors_p0_d2k5v2_t30.npz"]
    assert RTOL == 1e-10
    for p in FIXTURES:
        assert os.path.getsize(p) < 1 << 20


# ---- 1. the comparator against the reference --------------------------------------------------------------------------------
def _check(ms, z, tag, lengths, T, P):
    s = RR.snapshot(ms, T)
    parts = np.concatenate([m.elbo_parts() for _, m in ms])
    assert z[tag + "cov_offdiag_max"] == 0.0            # the columns of all the matrices stay diagonal: lane = row survives
    for n, Tn in enumerate(lengths):
        what = "%schain %d " % (tag, n)
        m = [m for rows, m in ms if n in rows][0]
        r = [rows.index(n) for rows, _ in ms if n in rows][0]
        _close(s["X"][n, :Tn], z[tag + "X"][n, :Tn], what + "X")
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        _close(s["Sigma"][n][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
        _close_qld(m.st["qld_x"][r][cls], z[tag + "qld_x"][n][cls], what + "qld_x")
        for w in ("ABCE" if P else "ACE"):
            _close(s[w + "_mean"][n], z[tag + w + "_mean"][n], what + w + "_mean")
            _close(s[w + "_colvar"][n], z[tag + w + "_colvar"][n], what + w + "_colvar")
            _close_qld(m.st["qld_" + w][r], z[tag + "qld_" + w][n], what + "qld_" + w)
        for nm in ("Q_a", "Q_b", "R_a", "R_b"):
            _close(m.st[nm][r], z[tag + nm][n], what + nm)
        ref = z[tag + "elbo_parts"][n]
        print(what, "parts", parts[n], "reference", ref)
        _close(parts[n], ref, what + "elbo_parts")
        assert abs(parts[n].sum() - ref.sum()) <= RTOL * abs(ref.sum())


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[11:-4])
def test_regressors_ref_reproduces_the_reference(path):
    meta, Y, U, V, st0, pri, lengths, z = RR.load_fixture(path)
    T, P = Y.shape[1], meta["P"]
    ms = RR.models(Y, U, V, st0, pri, lengths)
    assert meta["iters"] == [1, 2, 5] and V.shape[2] == meta["Pv"] and (U is None) == (P == 0)
    for it in range(1, 6):
        if it == 1:         # the forward sweep alone, then the rest of the iteration stage by stage
            for _, m in ms:
                m.sweep("forward")
            fwd = RR.snapshot(ms, T)["X"]
            for n, Tn in enumerate(lengths):
                _close(fwd[n, :Tn], z["it1_fwd_X"][n, :Tn], "forward sweep alone, chain %d" % n)
            for _, m in ms:
                for stage, _ in RR.stages(P)[1:]:
                    RR.do_stage(m, stage)
        else:
            for _, m in ms:
                m.iterate()
        if it in meta["iters"]:
            _check(ms, z, "it%d_" % it, lengths, T, P)


def test_the_fixtures_cover_no_input_both_inputs_with_gamma_noise_and_the_shortest_chain():
    metas = [RR.load_fixture(p)[0] for p in FIXTURES]
    assert [m["noise"] for m in metas] == ["gamma", "diagonal_gamma", "diagonal_gamma"]
    assert [(m["D"], m["K"], m["P"], m["Pv"]) for m in metas] == [(3, 4, 2, 1), (4, 5, 1, 2), (2, 5, 0, 2)]
    assert [m["lengths"] for m in metas] == [[20], [2, 7, 20], [30]]


# ---- 2. no regressor: the graph without -------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,noise", [(0, "diagonal_gamma"), (0, "gamma"), (2, "diagonal_gamma")])
def test_with_zero_regressors_the_comparator_is_the_graph_without(P, noise):
    T, D, K, Pv, N = 9, 3, 4, 2, 2
    Y, U, V, st0, pri = synth.make_regression_problem(T, D, K, P, Pv, N, seed=5)
    if noise == "gamma":
        pri["noise"] = "gamma"
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    m = RR.Model(Y, U, np.zeros_like(V), st0, pri)
    plain = RR.split_regressors(st0)[0]
    if P:
        ref = IR.Model(Y, U, plain, pri)
        step, st = ref.iterate, ref.st
    else:
        st = O.expand_state(plain, pri, T)
        step = lambda: O.iterate(st, pri, Y, with_elbo=False)
    for it in range(3):
        m.iterate()
        step()
        for k in ("X", "A_mean", "A_cov", "C_mean", "C_cov", "Q_b", "R_b"):
            _close(m.st[k], st[k], "iteration %d %s" % (it + 1, k), rtol=1e-13)
    # E has gone to its prior: no regressor, no evidence
    assert not np.any(pri["E_prior_mean"]) and np.abs(m.st["E_mean"]).max() == 0.0
    _close(np.einsum("nikk->nik", m.st["E_cov"]), np.broadcast_to(1.0 / pri["E_prior_prec"], (N, Pv, K)), "E_colvar", rtol=1e-13)


# ---- 3. the float64 comparator against its extended-precision run -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_float64_comparator_is_inside_the_guard(name):
    f64, ext = RR.trace(name), RR.trace(name, extended=True)
    assert ext[0][1].dtype == ER.LD
    per_iter = len(f64) // RR.ITERS
    assert len(ext) == per_iter * RR.CASES[name][7] and RR.CASES[name][7] == (1 if name == "t40_d64k40p6v12" else RR.ITERS)
    for (k64, v64), (kx, vx) in zip(f64, ext):
        assert k64 == kx
        e = ER.bound_errors(v64, vx)[0].max() if k64[1] == "bound" else ER.rel(v64, vx)
        print("iteration %d %-9s %-10s e64 %.2e" % (k64[0] + 1, k64[1], k64[2], e))
        assert e <= ER.CAP, (name, k64, e)


def test_the_cases_are_the_ones_the_device_is_measured_on():
    assert {k: v[:5] for k, v in RR.CASES.items()} == {
        "t19_d6k4v2": (19, 6, 4, 0, 2), "t19_d6k4p2v1": (19, 6, 4, 2, 1), "t33_d5k14v3": (33, 5, 14, 0, 3), "t77_d16k16p4v8": (77, 16, 16, 4, 8),
        "t40_d64k40p6v12": (40, 64, 40, 6, 12), "t12_d3k1v63": (12, 3, 1, 0, 63), "t700_d8k8p2v3_w4": (700, 8, 8, 2, 3),
        "lengths_d16k10p2v3": (77, 16, 10, 2, 3)}
    assert RR.CASES["lengths_d16k10p2v3"][5] == (2, 3, 19, 60, 77) and RR.CASES["t700_d8k8p2v3_w4"][6] == 4
    for T, D, K, P, Pv in (v[:5] for v in RR.CASES.values()):
        assert max(D, K + 2 * P + Pv) <= 64


# ---- 4. planted defects leave the envelope ----------------------------------------------------------------------------------
class _NoSvxInHC(RR.Model):
    """H_C = Syx: the columns of C explain the regressors' share of the outputs too"""
    def _HC(self, S):
        return S["Syx"]


class _CrossOnce(RR.Model):
    """the cross term <C> Svx^T <E>^T without its transpose"""
    def _cross(self, S):
        return 0.5 * RR.Model._cross(self, S)


class _NoV0(RR.Model):
    """v_0 dropped, as row 0 of an input that drives the states is"""
    def __init__(self, Y, U, V, st0, pri):
        V = V.copy()
        V[:, 0] = 0
        RR.Model.__init__(self, Y, U, V, st0, pri)


def _run(ms, name, iters):
    return RR.run_stages(lambda stage: [RR.do_stage(m, stage) for _, m in ms], lambda: RR.snapshot(ms, RR.CASES[name][0]),
                         lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), iters, RR.CASES[name][3])


def _padding_live_models(Y, U, V, st0, pri, lengths):
    """the v_t channel live in the first padding row of every chain shorter than T: one more row of V (with y = 0 and the state
    that the chain's end leaves there) enters Svv"""
    ms = RR.models(Y, U, V, st0, pri, lengths)
    for (n,), m in ms:
        if m.T < Y.shape[1]:
            m.Svv = m.Svv + np.einsum("np,nq->npq", V[n:n + 1, m.T], V[n:n + 1, m.T])
    return ms


def _leaves_envelope(name, defective):
    """Whether some quantity of the defective float64 run lies outside 16 max(e64, n 2^-52) of the sound extended run"""
    T, D, K = RR.CASES[name][:3]
    n = max(T, D, K)
    f64, ext = RR.trace(name), RR.trace(name, extended=True)
    worst = 0.0
    for (key, v64), (_, vx), (_, vd) in zip(f64, ext, defective):
        if key[1] == "bound":
            e64 = ER.bound_errors(v64, vx)[0]
            ratios = [r[4] / ER.FACTOR for r in ER.compare_bound(vd, vx, e64, n)]
        else:
            ratios = [ER.rel(vd, vx) / (ER.FACTOR * ER.yardstick(ER.rel(v64, vx), n))]
        worst = max([worst] + ratios) if np.all(np.isfinite(ratios)) else np.nan
    print(name, "worst ratio to the envelope", worst)
    return not worst <= 1.0         # (a run that has left the reals has left the envelope)


@pytest.mark.parametrize("cls", [_NoSvxInHC, _CrossOnce, _NoV0], ids=lambda c: c.__name__)
def test_a_planted_defect_leaves_the_envelope(cls):
    name = "t19_d6k4v2"
    assert not _leaves_envelope(name, RR.trace(name))           # the sound run itself passes
    Y, U, V, st0, pri, ln = RR.problem(name)
    # (one iteration: a defect may take the next one's precisions out of the positive definite matrices)
    with np.errstate(invalid="ignore"):         # (a defective R may leave the positive numbers: its logarithms are NaN)
        assert _leaves_envelope(name, _run(RR.models(Y, U, V, st0, pri, ln, cls), name, 1))


def test_a_v_channel_live_in_a_padding_row_leaves_the_envelope():
    name = "lengths_d16k10p2v3"
    Y, U, V, st0, pri, ln = RR.problem(name)
    ms = _padding_live_models(Y, U, V, st0, pri, ln)
    assert np.abs(V[0, 2:]).max() > 0.1          # the case's padding rows of V are not zero: a handle that reads them shows
    assert _leaves_envelope(name, _run(ms, name, 1))


# ---- 5. refusals, argument errors, the C ABI --------------------------------------------------------------------------------
def _ip(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_capi._ip)


def _create(N, T, D, K, P, Pv, noise, lengths=None):
    h = ctypes.c_void_p()
    rc = _capi.lib.pyvb_lds_create_regressors(ctypes.byref(h), 0, N, T, D, K, P, Pv, noise, _ip(lengths))
    msg = _capi.lib.pyvb_last_error().decode()
    if rc == _capi.OK:              # a machine with a device: nothing to compare the refusal with, give the handle back
        _capi.lib.pyvb_lds_destroy(h)
    else:
        assert not h.value
    return rc, msg


LIMIT = "max(D, K + 2 P + Pv) <= 64"


@pytest.mark.parametrize("D,K,P,Pv,noise,word", [(4, 5, 0, 2, _capi.NOISE_WISHART, "Wishart"), (4, 5, 2, 2, _capi.NOISE_WISHART, "Wishart"),
                                                 (65, 5, 0, 1, _capi.NOISE_DIAGONAL_GAMMA, LIMIT), (4, 62, 0, 3, _capi.NOISE_GAMMA, LIMIT),
                                                 (4, 1, 0, 64, _capi.NOISE_GAMMA, LIMIT), (4, 3, 30, 2, _capi.NOISE_GAMMA, LIMIT),
                                                 (4, 70, 0, 1, _capi.NOISE_DIAGONAL_GAMMA, "128-wide")])
def test_handles_with_regressors_are_refused_where_they_are_not_served(D, K, P, Pv, noise, word):
    for lengths in (None, [10, 4, 10]):
        rc, msg = _create(3, 10, D, K, P, Pv, noise, lengths)
        assert rc == _capi.E_UNSUPPORTED, (rc, msg)
        assert "regressors" in msg and word in msg and "HIP" not in msg, msg


@pytest.mark.parametrize("P,Pv,word", [(0, 0, "Pv must be >= 1"), (2, -1, "Pv must be >= 1"), (-1, 2, "P must be >= 0")])
def test_the_channel_counts_are_checked(P, Pv, word):
    rc, msg = _create(3, 10, 4, 5, P, Pv, _capi.NOISE_DIAGONAL_GAMMA)
    assert rc == _capi.E_ARG and word in msg, (rc, msg)


def test_bad_lengths_are_named_as_on_a_plain_handle():
    rc, msg = _create(3, 10, 4, 5, 0, 2, _capi.NOISE_DIAGONAL_GAMMA, [10, 1, 10])
    assert rc == _capi.E_ARG and "1" in msg, (rc, msg)


def test_shared_models_take_no_regressors():
    from pyvb_amd.lds import LDSBatch
    with pytest.raises(NotImplementedError) as e:
        LDSBatch(2, 6, 3, 4, regressors=2, models=[0, 0])
    assert "regressors" in str(e.value)


def test_a_null_handle_is_an_argument_error():
    v = np.ones(4)
    p = _capi.dptr(v)
    lib = _capi.lib
    for rc in (lib.pyvb_lds_set_regressors(None, p), lib.pyvb_lds_get_regressors(None, p), lib.pyvb_lds_set_regressor_priors(None, p, p),
               lib.pyvb_lds_set_regressor_state(None, p, p), lib.pyvb_lds_get_regressor_state(None, p, p, p, p), lib.pyvb_lds_update_E(None)):
        assert rc == _capi.E_ARG
        assert b"handle is NULL" in lib.pyvb_last_error()
    assert lib.pyvb_lds_create_regressors(None, 0, 1, 4, 2, 2, 0, 1, 0, None) == _capi.E_ARG


def test_entries_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "pyvb_hip.h")).read()
    decl = {
        ENTRIES[0]: r"int pyvb_lds_create_regressors\(pyvb_lds\*\* out, int device, int N, int T, int D, int K, int P, int Pv, int noise_kind, const int\* lengths\);",
        ENTRIES[1]: r"int pyvb_lds_set_regressors\(pyvb_lds\* h, const double\* V\);",
        ENTRIES[2]: r"int pyvb_lds_get_regressors\(pyvb_lds\* h, double\* V\);",
        ENTRIES[3]: r"int pyvb_lds_set_regressor_priors\(pyvb_lds\* h, const double\* E_prior_mean, const double\* E_prior_prec\);",
        ENTRIES[4]: r"int pyvb_lds_set_regressor_state\(pyvb_lds\* h, const double\* E_mean, const double\* E_colvar\);",
        ENTRIES[5]: r"int pyvb_lds_get_regressor_state\(pyvb_lds\* h, double\* E_mean, double\* E_colvar, double\* qld_E, double\* lnd_E\);",
        ENTRIES[6]: r"int pyvb_lds_update_E\(pyvb_lds\* h\);",
    }
    c, dp, ip, h = ctypes.c_int, _capi._dp, _capi._ip, _capi._h
    args = {ENTRIES[0]: [ctypes.POINTER(h)] + [c] * 8 + [ip], ENTRIES[1]: [h, dp], ENTRIES[2]: [h, dp], ENTRIES[3]: [h, dp, dp],
            ENTRIES[4]: [h, dp, dp], ENTRIES[5]: [h, dp, dp, dp, dp], ENTRIES[6]: [h]}
    for name in ENTRIES:
        assert re.search("^" + decl[name], header, re.M), name + " is not declared as specified in include/pyvb_hip.h"
        assert _capi.SIGNATURES[name] == (c, args[name]), name
        assert getattr(_capi.lib, name).argtypes == args[name]
    out = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= exported
    assert _capi.lib.pyvb_version() >= 111
    assert LIMIT in header
    assert re.search(r"PYVB_K_REGRESSORS = 9\b", header) and _capi.K_REGRESSORS == 9


def test_the_generator_of_regression_problems_leaves_the_others_alone():
    Y, U, V, st0, pri = synth.make_regression_problem(12, 3, 4, 2, 3, 2, seed=77)
    assert Y.shape == (2, 12, 4) and U.shape == (2, 12, 2) and V.shape == (2, 12, 3) and np.all(V[:, :, 0] == 1.0)
    assert st0["E_mean"].shape == (2, 4, 3) and st0["E_colvar"].shape == (2, 3, 4)
    assert pri["E_prior_mean"].shape == (4, 3) and pri["E_prior_prec"].shape == (3, 4)
    _, U1, st1, pri1 = synth.make_input_problem(12, 3, 4, 2, 2, seed=77)
    assert np.array_equal(U, U1)
    for k in st1:           # the same initial state beside E
        assert np.array_equal(st0[k], st1[k]), k
    assert sorted(set(pri) - set(pri1)) == ["E_prior_mean", "E_prior_prec"]
    Y0, U0, V0, st2, _ = synth.make_regression_problem(12, 3, 4, 0, 3, 2, seed=77)
    assert U0 is None and "B_mean" not in st2 and np.array_equal(V0, V)


def test_pad_series_carries_the_regressors_gain():
    from pyvb_amd.lds import pad_series
    Y, U, V, st0, pri = synth.make_regression_problem(9, 3, 4, 0, 2, 3, seed=78)
    ln = [9, 2, 5]
    series = [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(ln)]
    Yp, sp, lp = pad_series(series)
    assert list(lp) == ln and np.array_equal(sp["E_mean"], st0["E_mean"]) and np.array_equal(sp["E_colvar"], st0["E_colvar"])
