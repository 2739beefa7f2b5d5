"""CPU: several chains, one model (pyvb_lds_create_tied) -- what needs no device.

1. tests/tied_ref.py, the composition of oracle functions that the GPU tests compare against, reproduces the reference's own run
   of a graph whose chains share A, C, Q, R (tests/golden/tied_*.npz, written by tests/golden/make_golden_tied.py) at the
   tolerance tests/test_oracle_golden.py uses for the same quantities (1e-10 relative; observed about 1e-14).
2. The two C ABI entries exist everywhere they must; the argument checks and the refusals of pyvb_lds_create_tied come before any
   HIP call; models of one replicate each are pyvb_lds_create_lengths.
3. The cases on which k_tie.hip is held to the accuracy envelope (tied_ref.CASES): the comparator's long-double
   run is long double throughout, the float64 comparator is within the cap of it on every compared quantity and part, and the
   envelope comparison catches a chain pooled at a weight of 1 + 1e-10, which the 1e-8 comparison cannot see.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import extended_ref as ER
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


# ---- 3. the envelope cases: the float64 comparator against its long-double run ----------------------------------------------
@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_envelope_cases_reach_what_they_are_for(name):
    T, D, K, sizes, kind, seed = TR.CASES[name]
    Y, st0, pri, lengths, models = TR.problem(name)
    assert Y.shape == (sum(sizes), T, K) and [len(r) for r in TR.rows_of(models)] == list(sizes)
    assert list(lengths[:3]) == [T, 2, 3] and lengths.min() == 2 and lengths.max() == T and pri["noise"] == kind
    assert not Y[np.arange(T)[None, :] >= lengths[:, None]].any()
    odd = (3 * D * D + K * D + D) % 2 == 1
    assert odd == (D % 2 == 1 and K % 2 == 1)
    want = {"d3k3": (True, True), "d4k4": (False, False), "d33k17": (True, True), "d4k5_13": (False, True)}[name]
    assert (odd, K % 2 == 1) == want                     # k_tie<double> on (the moment block, Syy)


def test_envelope_cases_cover_every_state_of_the_loop():
    """A model of c chains: (c - 1) // 4 turns of the unrolled body and a tail of (c - 1) % 4."""
    sizes = sorted({c for case in TR.CASES.values() for c in case[3]})
    assert sizes == [1, 2, 4, 5, 6, 7, 8, 9, 13]
    assert {((c - 1) // 4, (c - 1) % 4) for c in sizes if c > 1} == {(0, 1), (0, 3), (1, 0), (1, 1), (1, 2), (1, 3), (2, 0), (3, 0)}
    assert TR.CASES["d4k4"][3][:3] == (5, 1, 9) and TR.CASES["d4k5_13"][3] == (13,) and TR.CASES["d33k17"][3] == (6,)
    assert (3 * 33 * 33 + 17 * 33 + 33 + 255) // 256 > 1        # more than one block along the elements


def _all_long(st, what):
    for k, v in st.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f":
            assert v.dtype == ER.LD, "%s: %s has dtype %s" % (what, k, v.dtype)


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_long_double_run_is_long_double_throughout(name):
    ms, tr = TR.trace(name, extended=True)
    assert len(tr) == TR.ITERS == 2
    for m, (rows, chains, Ys) in enumerate(ms):
        for c, st in enumerate(chains):
            _all_long(st, "%s model %d chain %d" % (name, m, c))
        _all_long(TR.statistics(chains, Ys)[1], "%s model %d pooled statistics" % (name, m))
    for snaps in tr:
        for s in snaps:
            for k, v in s.items():
                for a in (v if isinstance(v, list) else v.values() if isinstance(v, dict) else [v]):
                    assert a.dtype == ER.LD and np.all(np.isfinite(a)), (name, k, a.dtype)


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_float64_comparator_is_within_the_cap(name):
    (ms, f64), (_, ext) = TR.trace(name), TR.trace(name, extended=True)
    worst = (0.0, None)
    for it in range(TR.ITERS):
        for m, (rows, chains, Ys) in enumerate(ms):
            for what, e64, e, ratio in TR.envelope(f64[it][m], f64[it][m], ext[it][m], TR.accumulation_length(chains)):
                assert e == e64 and ratio <= 1.0
                assert e64 <= ER.CAP, "%s iteration %d model %d %s: e64 %.3e, cap %.0e" % (name, it + 1, m, what, e64, ER.CAP)
                worst = max(worst, (e64, "iteration %d model %d %s" % (it + 1, m, what)))
    print("%s: largest e64 %.2e at %s" % ((name,) + worst))


# ---- 4. what the envelope sees and 1e-8 does not -----------------------------------------------------------------------------
def _plant(monkeypatch, size, change):
    """tied_ref.statistics with the POOLED statistics of every model of `size` chains changed by change(per, pooled, Ys); what each
    chain keeps for its own terms of the bound is untouched, as on the device, where k_tie writes only the sum."""
    clean = TR.statistics

    def statistics(chains, Ys):
        per, pooled = clean(chains, Ys)
        if len(chains) == size:
            pooled = dict(pooled)
            change(per, pooled, Ys)
        return per, pooled
    monkeypatch.setattr(TR, "statistics", statistics)


def _syy_of_one_chain_scaled(w):
    def change(per, pooled, Ys):
        pooled["Syy"] = pooled["Syy"] + w * per[4]["Syy"]
    return change


def _moments_of_the_last_chain_weighted(w):
    def change(per, pooled, Ys):
        for k in pooled:
            if k != "Syy":
                pooled[k] = pooled[k] + w * per[-1][k]
    return change


def _without_the_chain_of_length_2(per, pooled, Ys):
    (c,) = [i for i, Y in enumerate(Ys) if Y.shape[1] == 2]
    for k in pooled:
        pooled[k] = pooled[k] - per[c][k]


# (case, chains of the model, the change, passes the 1e-8 comparison of tests/test_tied_gpu.py?)
# The weight 1 + 1e-10 separates the two comparisons as it stands, no other weight was needed: one of nine contributions changed by
# 1e-10 of itself moves R_b by 5.5e-11 (a) and the states by 3.6e-11 (b) after two iterations -- the residuals are small differences
# of the large sums, which amplifies the change a little -- 200 times under 1e-8 and 3000 to 5000 times the yardstick
# max(e64, n 2^-52) = 1.1e-14 (n = 51 nodes), i.e. 200 to 300 times the envelope's bound.
MUTANTS = {
    "a_one_chains_Syy_scaled_by_1+1e-10": ("d3k3", 9, _syy_of_one_chain_scaled(1e-10), True),
    "b_last_chains_moments_at_weight_1+1e-10": ("d3k3", 9, _moments_of_the_last_chain_weighted(1e-10), True),
    "c_pooled_without_the_chain_of_length_2": ("d4k5_13", 13, _without_the_chain_of_length_2, False),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_envelope_catches_what_the_parity_tolerance_cannot(mutant, monkeypatch):
    """The comparisons of test_tied_gpu.py::test_parity_and_envelope applied to the float64 comparator with one error planted in the
    pooled statistics of one model: (a) and (b) pass the RTOL = 1e-8 comparison and fail the envelope -- the envelope is what catches
    them; (c) fails both.  The comparator without a mutant passes both (its e is e64, at most the yardstick)."""
    import test_tied_gpu as G
    name, size, change, passes_parity = MUTANTS[mutant]
    Y, st0, pri, lengths, models = TR.problem(name)
    (m,) = [i for i, c in enumerate(TR.CASES[name][3]) if c == size]
    (ms, f64), (_, ext) = TR.trace(name), TR.trace(name, extended=True)      # before the mutant is planted
    n = TR.accumulation_length(ms[m][1])
    _plant(monkeypatch, size, change)
    mut = TR.run(TR.build_models(Y, st0, pri, lengths, models, only=[m]), pri)

    def parity(got, it):
        try:
            G._parity(got, f64[it][m], "%s iteration %d: " % (mutant, it + 1))
        except AssertionError as e:
            return str(e).splitlines()[0]
        return None

    failed_parity, worst = [], (0.0, None)
    for it in range(TR.ITERS):
        assert parity(f64[it][m], it) is None
        assert max(r[3] for r in TR.envelope(f64[it][m], f64[it][m], ext[it][m], n)) <= 1.0
        why = parity(mut[it][0], it)
        if why:
            failed_parity.append(why)
        for what, e64, e, ratio in TR.envelope(mut[it][0], f64[it][m], ext[it][m], n):
            worst = max(worst, (ratio, "iteration %d %s: e64 %.2e, e %.2e" % (it + 1, what, e64, e)))
    print("%s: envelope e / y up to %.3g (%s); 1e-8 comparison: %s" % (mutant, worst[0], worst[1], failed_parity[:1] or "passes"))
    assert worst[0] > ER.FACTOR, "mutant %s stays within %g x the yardstick" % (mutant, ER.FACTOR)
    assert (not failed_parity) == passes_parity, failed_parity
