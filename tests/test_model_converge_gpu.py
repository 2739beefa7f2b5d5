"""GPU: per-model convergence on the device (include/pyvb_hip.h: pyvb_lds_iterate_until_model, pyvb_lds_get_model_convergence)
through pyvb_amd.lds.LDSBatch.

The comparator is tests/model_converge_ref.py: every model run alone in tests/tied_ref.py with network.py:53 applied on the host
to the bound of the model's graph, on inputs where that decision is not a rounding matter (its guard;
tests/test_model_converge_cpu.py asserts it for every case).  Stop iterations are compared exactly; tolerances are those of
tests/test_tied_gpu.py: RTOL = 1e-8 max-norm for states and parameters, q_ln_det through its reciprocal, the parts of a model's
bound to RTOL of the sum of their magnitudes (exact mode: of each part) and the total to RTOL of itself.

Base case: D = 4, K = 5 (no multiple of 16), T = 60, eight chains in models of [1, 3, 2, 2] chains -- a singleton beside tied
models -- with ragged lengths that include T_n = 2 and 3.  Both of its runs freeze models in odd and in even iterations.

"Bitwise" is justified as in tests/test_tied_gpu.py: rows share no arithmetic but the fixed-order sums over the chains of a model
(k_tie.hip, k_converge.hip), so two handles of the same shapes, lengths, models and time split run the same instructions in
the same order on the rows both compute.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import model_converge_ref as MR
import tied_ref as TR

pytestmark = pytest.mark.gpu

RTOL = 1e-8
HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = ("A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b", "qld_A", "qld_C", "lnd_A", "lnd_C")


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(a, b, what, rtol=RTOL):
    assert np.all(np.isfinite(a)), what + ": non-finite values"
    err = _rel(a, b)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _close_qld(a, b, what):
    sa, sb = 0.5 / np.asarray(a, dtype=float), 0.5 / np.asarray(b, dtype=float)
    ok = np.isfinite(sb)
    assert np.all(np.abs(sa - sb)[ok] <= 1e-9 * np.maximum(1.0, np.abs(sb[ok]))), what


CASE = object()         # _batch: the lengths / models of the case


def _batch(name, W=None, models=CASE, lengths=CASE):
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, ln, md = MR.problem(name)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=ln if lengths is CASE else lengths, models=md if models is CASE else models)
    if MR.CASES[name]["bound"] == "exact":
        b.set_bound_mode("exact")
    if MR.CASES[name].get("nan"):
        b.update_Y()                                    # (the bound is undefined until every unobserved output has been updated)
    if W is not None:
        b.set_time_split(W)
    return b


def _everything(b, with_elbo=True):
    """Every getter of the handle, as one dict of arrays with leading axis N."""
    out = dict(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["qld_A"], out["qld_C"] = b.get_column_qld()
    for k, v in b.get_logdets().items():
        out["lnd_" + k] = v
    out["Yq"], out["Yvar"], out["Yqld"] = b.get_outputs(with_qld=True)
    if with_elbo:
        out["elbo"] = b.elbo()
    return out


def _same_rows(a, b, rows, what):
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)


def _read(b, iters_run):
    out = dict(iters_run=iters_run)
    out["iters"], out["converged"], out["llb"] = b.model_convergence()
    out["chain_iters"], out["chain_converged"], out["chain_llb"] = b.convergence()
    out["history"], out["total"], out["active"] = b.elbo_history(), b.elbo_total(), b.active()
    out["all"] = _everything(b)
    return out


def _until(b, name, check_every=8, tol=None, max_iters=None):
    c = MR.CASES[name]
    return b.iterate_until_model(c["max_iters"] if max_iters is None else max_iters, MR._tol(name, tol), check_every)


@functools.lru_cache(maxsize=None)
def _ran(name, check_every=8, W=None, max_iters=None):
    """One handle of a case after iterate_until_model, read out once and shared: do not write to the arrays."""
    b = _batch(name, W)
    try:
        out = _read(b, _until(b, name, check_every, max_iters=max_iters))
        out["rerun"] = b.iterate_until_model(5) if out["converged"].all() else None
    finally:
        b.close()
    return out


def _compare_chains(g, rows, chains, t):
    """X, the classes and the parameters of one model's rows against the comparator's chains."""
    st = chains[0]
    for n, ch in zip(rows, chains):
        Tn = ch["X"].shape[1]
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        tn = "%sreplicate %d " % (t, n)
        _close(g["X"][n, :Tn], ch["X"][0], tn + "X")
        assert not g["X"][n, Tn:].any(), tn + "padding rows of X"
        _close(g["Sigma"][n][cls], ch["Sigma"][0][cls], tn + "Sigma")
        _close_qld(g["qld_x"][n][cls], ch["qld_x"][0][cls], tn + "qld_x")
        _close(g["A_mean"][n], st["A_mean"][0], tn + "A_mean")
        _close(g["C_mean"][n], st["C_mean"][0], tn + "C_mean")
        _close(g["A_colvar"][n], np.einsum("ikk->ik", st["A_cov"][0]), tn + "A_colvar")
        _close(g["C_colvar"][n], np.einsum("ikk->ik", st["C_cov"][0]), tn + "C_colvar")
        for nm in ("Q_a", "Q_b", "R_a", "R_b"):
            _close(g[nm][n], np.broadcast_to(st[nm][0], g[nm][n].shape), tn + nm)
        _close_qld(g["qld_A"][n], st["qld_A"][0], tn + "qld_A")
        _close_qld(g["qld_C"][n], st["qld_C"][0], tn + "qld_C")
        if "Yobs" in ch:
            _close(g["Yq"][n], ch["Yq"][0], tn + "Yq")
            _close(g["Yvar"][n], ch["Yvar"][0], tn + "Yvar")
        for k in PARAMS:                                # the rows of a model are bitwise equal in the parameters
            assert np.array_equal(g[k][n], g[k][rows[0]], equal_nan=True), "%s%s differs from row %d of its model" % (tn, k, rows[0])


def _compare_parts(got, want, what, exact):
    print("%s: parts %r want %r" % (what, got, want))
    assert np.all(np.isfinite(got)), what
    if exact:
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "%s\n%r\n%r" % (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= RTOL * np.abs(want).sum()), "%s\n%r\n%r" % (what, got, want)
        assert abs(got.sum() - want.sum()) <= RTOL * abs(want.sum()), what + ": total"


def _against_comparator(got, runs, name, tag=""):
    """Every model at its own stop (a frozen model reads back as its last iteration left it), and the bookkeeping per chain."""
    g, exact = got["all"], MR.CASES[name]["bound"] == "exact"
    assert list(got["iters"]) == [r["iters"] for r in runs], (tag, name, got["iters"])
    assert list(got["converged"]) == [r["converged"] for r in runs], (tag, name, got["converged"])
    for m, r in enumerate(runs):
        t, rows, want = "%scase %s, model %d (%d iterations): " % (tag, name, m, r["iters"]), r["rows"], r["trace"][-1]
        _compare_chains(g, rows, r["chains"], t)
        _compare_parts(g["elbo"][rows].sum(0), want, t + "parts", exact)
        assert not g["elbo"][rows[1:], 2:].any(), t + "L_A, L_C, L_Q, L_R on rows that are not the first"
        assert abs(got["llb"][m] - want.sum()) <= RTOL * abs(want.sum()), t + "llb"
        # pyvb_lds_get_convergence: the model's values on every chain
        assert np.all(got["chain_iters"][rows] == got["iters"][m]) and np.all(got["chain_converged"][rows] == got["converged"][m]), t
        assert np.all(got["chain_llb"][rows] == got["llb"][m]), t


def _totals_ok(got, runs):
    want = MR.totals(runs, got["iters_run"])
    scale = sum(np.abs(r["trace"]).sum(1).max() for r in runs)
    assert got["history"].shape == (got["iters_run"], 6)
    assert np.all(np.abs(got["history"] - want) <= RTOL * scale), np.abs(got["history"] - want).max() / scale


# ---- 1. against the comparator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reference", "exact"])
def test_every_model_stops_where_the_reference_would(name):
    got, runs = _ran(name), MR.alone(name)
    print("case %s: iters %s converged %s iters_run %d" % (name, got["iters"], got["converged"].astype(int), got["iters_run"]))
    _against_comparator(got, runs, name)
    assert {int(i) % 2 for i in got["iters"]} == {0, 1}          # freezes in odd and in even iterations (the two ping-pongs)
    assert got["active"].all()
    assert got["rerun"] == 0                            # nobody left: nothing is launched


def test_models_of_five_and_nine_chains_stop_where_the_reference_would():
    """Models of 5, 1 and 9 chains: the per-model sum of k_converge runs over more chains than any other case gives it (three), and
    the statistics behind the bound come through the unrolled body of k_tie.  Every model stops in an iteration of its own, and
    the chains of a model carry its count (_against_comparator)."""
    name = "sizes_5_1_9"
    got, runs = _ran(name, 1), MR.alone(name)
    print("case %s: iters %s converged %s iters_run %d" % (name, got["iters"], got["converged"].astype(int), got["iters_run"]))
    assert [len(r["rows"]) for r in runs] == [5, 1, 9] and len({r["iters"] for r in runs}) == 3
    _against_comparator(got, runs, name)
    for r in runs:
        assert len(set(got["chain_iters"][r["rows"]])) == 1
    assert got["iters_run"] == max(r["iters"] for r in runs) and got["converged"].all()
    _totals_ok(got, runs)
    assert got["rerun"] == 0


# ---- 2. every replicate a model of its own: the per-replicate entry, bitwise --------------------------------------------------
@pytest.mark.parametrize("plain", [False, True], ids=["singleton_models", "plain_handle"])
def test_singletons_are_the_per_replicate_entry_bitwise(plain):
    c = MR.CASES["reference"]
    N = c["N"]
    kw = dict(models=None, lengths=None) if plain else dict(models=np.arange(N, dtype=np.int32))
    a, b = _batch("reference", **kw), _batch("reference", **kw)
    try:
        ra, rb = a.iterate_until(c["max_iters"], c["tol"], 8), b.iterate_until_model(c["max_iters"], c["tol"], 8)
        assert ra == rb and ra > 0
        ca, cb = a.convergence(), b.convergence()
        assert ca[1].any()
        for x, y in zip(ca, cb):
            assert np.array_equal(x, y, equal_nan=True)
        for h in (a, b):                                # M = N: one entry per replicate
            for x, y in zip(h.model_convergence(), ca):
                assert np.array_equal(x, y, equal_nan=True)
        assert np.array_equal(a.elbo_history(), b.elbo_history())
        assert np.array_equal(a.elbo_total(), b.elbo_total())
        _same_rows(_everything(a), _everything(b), slice(None), "iterate_until against iterate_until_model")
    finally:
        a.close(); b.close()


# ---- 3. frozen stays frozen, on either side of the two ping-pongs -------------------------------------------------------------
def test_frozen_models_stay_frozen_and_the_others_go_on():
    name, first_iters = "reference", 12
    runs, pri = MR.alone(name, None, first_iters), MR.problem(name)[2]
    T = MR.CASES[name]["T"]
    assert [r["converged"] for r in runs] == [True, False, True, False]
    assert {r["iters"] % 2 for r in runs if r["converged"]} == {0, 1}        # rows frozen in an odd and in an even iteration
    b = _batch(name)
    try:
        assert _until(b, name, max_iters=first_iters) == first_iters
        first = _read(b, first_iters)
        _against_comparator(first, runs, name, "first call, ")
        frozen = first["chain_converged"]
        assert list(np.nonzero(frozen)[0]) == [0, 4, 5]
        live = [(r["rows"], MR.continued(r), r["Ys"]) for r in runs if not r["converged"]]

        def check(what):
            now = _everything(b)
            _same_rows(now, first["all"], frozen, "frozen rows after " + what)
            for rows, chains, Ys in live:
                _compare_chains(now, rows, chains, "after %s, " % what)
            return now

        b.iterate(3)
        for rows, chains, Ys in live:
            for _ in range(3):
                parts = TR.iterate(chains, pri, Ys)
        now = check("iterate(3)")
        for rows, chains, Ys in live:
            _compare_parts(now["elbo"][rows].sum(0), TR.elbo_parts(chains, pri, Ys), "after iterate(3), rows %r" % (rows,), False)
        for direction in ("forward", "backward"):       # (after the first: an odd number of flips)
            b.sweep(direction)
            for rows, chains, Ys in live:
                TR.sweep(chains, pri, Ys, direction)
            check("a %s sweep" % direction)
        for t in (0, 2, T - 1):
            b.update_x(t)
            for rows, chains, Ys in live:
                TR.update_x(chains, pri, Ys, t)
        check("update_x")
        pooled = [TR.statistics(chains, Ys)[1] for rows, chains, Ys in live]
        b.update_A(); b.update_C(); b.update_Q(); b.update_R()
        for (rows, chains, Ys), S in zip(live, pooled):
            TR.update_A(chains, pri, S); TR.update_C(chains, pri, S); TR.update_Q(chains, pri, S, Ys); TR.update_R(chains, pri, S, Ys)
        check("update_A/C/Q/R")
        it, cv, _ = b.model_convergence()
        assert list(it) == [9, 12, 2, 12] and list(cv) == [True, False, True, False]     # iterate() and the others are not counted
    finally:
        b.close()


# ---- 4. history and totals ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["reference", "exact"])
def test_history_and_totals_hold_converged_models_at_their_final_bound(name):
    got, runs = _ran(name), MR.alone(name)
    _totals_ok(got, runs)
    rows = got["all"]["elbo"]
    N = rows.shape[0]
    assert np.all(np.abs(got["total"] - rows.sum(0)) <= N * 2.0 ** -52 * np.abs(rows).sum(0)), (got["total"], rows.sum(0))
    assert np.array_equal(got["history"][-1], got["total"])


# ---- 5. a second call ---------------------------------------------------------------------------------------------------------
def test_a_second_call_resumes_from_minus_infinity():
    name, first_iters = "reference", 12
    c = MR.CASES[name]
    runs2 = MR.resumed(name, first_iters, c["tol"], c["max_iters"])
    b = _batch(name)
    try:
        assert _until(b, name, max_iters=first_iters) == first_iters
        first = _everything(b)
        conv1 = b.convergence()[1]
        assert list(b.model_convergence()[1]) == [True, False, True, False]
        b.reset_elbo_history()
        n2 = b.iterate_until_model(c["max_iters"], c["tol"], 1)
        got = _read(b, n2)
        assert n2 == max(r["iters"] - first_iters for r in runs2 if r["moved"]) and n2 > 1, n2      # (old = -inf again: its first iteration stops nobody)
        _against_comparator(got, runs2, name, "second call, ")
        assert all(r["iters"] > first_iters for r in runs2 if r["moved"])                         # iters accumulates
        _same_rows(got["all"], first, conv1, "models that had converged in the first call")
        _totals_ok(got, runs2)
        assert b.iterate_until_model(5) == 0            # everybody has converged
    finally:
        b.close()


# ---- 6. the mask ----------------------------------------------------------------------------------------------------------------
def test_a_switched_off_model_is_not_run_tested_or_counted():
    from pyvb_amd import _capi
    name, off = "reference", 1
    runs = MR.alone(name)
    mask = np.ones(8, dtype=bool); mask[runs[off]["rows"]] = False
    b = _batch(name)
    try:
        before = _everything(b, with_elbo=False)        # (no bound exists before the first complete sweep)
        for bad in ([1, 1, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 0, 1, 1]):
            with pytest.raises(_capi.PyvbHipError) as ei:
                b.set_active(np.array(bad, dtype=bool))
            assert ei.value.code == _capi.E_ARG and "model" in str(ei.value), str(ei.value)
        b.set_active(mask)
        got = _read(b, _until(b, name))
        assert np.array_equal(got["active"], mask)
        assert got["iters"][off] == 0 and not got["converged"][off] and np.isnan(got["llb"][off])
        assert not got["chain_iters"][~mask].any() and not got["chain_converged"][~mask].any()
        _same_rows({k: v for k, v in got["all"].items() if k != "elbo"}, before, ~mask, "the switched-off model")
        assert not got["all"]["elbo"][~mask].any()
        others = [r for m, r in enumerate(runs) if m != off]
        assert list(got["iters"][[0, 2, 3]]) == [r["iters"] for r in others] and got["converged"][[0, 2, 3]].all()
        _same_rows(got["all"], _ran(name)["all"], mask, "the others against the handle where nothing was switched off")
        _totals_ok(got, others)
        assert np.array_equal(got["history"][-1], got["total"])
        # after the call: a further whole model leaves the totals; a mask that splits a model is still refused
        with pytest.raises(_capi.PyvbHipError) as ei:
            b.set_active(np.array([1, 0, 0, 0, 1, 1, 1, 0], dtype=bool))
        assert ei.value.code == _capi.E_ARG and "model 3" in str(ei.value), str(ei.value)
        mask2 = mask.copy(); mask2[runs[3]["rows"]] = False
        b.set_active(mask2)
        after = _everything(b)
        _same_rows(after, got["all"], slice(None), "set_active after the call moves nothing")
        rows = after["elbo"][mask2]
        assert np.all(np.abs(b.elbo_total() - rows.sum(0)) <= 8 * 2.0 ** -52 * np.abs(rows).sum(0))
        assert list(b.model_convergence()[0]) == list(got["iters"])
    finally:
        b.close()


# ---- 7. check_every changes nothing but iters_run -----------------------------------------------------------------------------
def test_check_every_only_moves_the_return():
    runs, base, got = MR.alone("reference"), _ran("reference", 1), _ran("reference")
    last = max(r["iters"] for r in runs)
    assert base["iters_run"] == last
    assert last <= got["iters_run"] <= last + 7, got["iters_run"]
    assert got["iters_run"] % 8 == 0
    _same_rows(got["all"], base["all"], slice(None), "check_every = 8 against 1")
    for k in ("iters", "converged", "llb", "chain_iters", "chain_converged", "chain_llb", "total"):
        assert np.array_equal(got[k], base[k]), k
    assert np.array_equal(got["history"][:last], base["history"])
    assert np.array_equal(got["history"][last:], np.repeat(base["history"][-1:], got["iters_run"] - last, axis=0))    # idle iterations


# ---- 8. one wider odd shape: the copy extents T * DP and 3 D^2 of the freeze ------------------------------------------------
def test_a_wider_odd_shape():
    runs = MR.alone("wide")
    assert sorted(r["converged"] for r in runs) == [False, True]
    b = _batch("wide")
    try:
        got = _read(b, _until(b, "wide"))
        assert got["iters_run"] == MR.CASES["wide"]["max_iters"] <= 8
        _against_comparator(got, runs, "wide")
        _totals_ok(got, runs)
        first = got["all"]
        b.iterate(1); b.sweep("forward")                # the frozen model sits out both ping-pongs, whole rows of it
        _same_rows(_everything(b), first, got["chain_converged"], "the frozen model after further updates")
    finally:
        b.close()


# ---- 9. the time axis split over two wavefronts ---------------------------------------------------------------------------------
def test_a_forced_time_split_stops_in_the_same_iterations():
    runs = MR.alone("reference")
    b = _batch("reference", W=2)
    try:
        assert b.get_time_split() == 2
        got = _read(b, _until(b, "reference"))
    finally:
        b.close()
    _against_comparator(got, runs, "reference", "W = 2, ")
    assert {int(i) % 2 for i in got["iters"]} == {0, 1}


# ---- 10. outputs with NaN on equal lengths ------------------------------------------------------------------------------------
def test_outputs_with_nan_on_equal_lengths():
    runs = MR.alone("nan")
    got = _ran("nan")
    _against_comparator(got, runs, "nan")
    _totals_ok(got, runs)
    assert np.isnan(MR.problem("nan")[0]).any()


# ---- 11. two ranks on the one GPU ---------------------------------------------------------------------------------------------
def _ranks(world, tmp_path, port):
    worker = os.path.join(HERE, "model_converge_multirank_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / ("w%d" % world))
    procs = [subprocess.Popen([sys.executable, worker, str(r), str(world), prefix], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=120)[0])  # each process under its own limit: a rank that waits alone ends the test
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    return [dict(np.load(prefix + "_%d.npz" % r)) for r in range(world)]


def test_models_sharded_over_two_ranks_stop_together(tmp_path):
    """Rank 0 holds models 0 and 1, rank 1 holds models 2 and 3; a model never spans ranks, so the rows are bitwise those of the
    single handle, and the running count rides through the all-reduce: both ranks launch the same number of iterations."""
    one = _ranks(1, tmp_path, 29880)[0]
    many = _ranks(2, tmp_path, 29884)
    runs = MR.alone("reference")
    assert [tuple(m["rows"]) for m in many] == [(0, 4), (4, 8)]
    assert int(many[0]["iters_run"]) == int(many[1]["iters_run"]) == int(one["iters_run"])
    assert list(np.concatenate([m["iters"] for m in many])) == list(one["iters"]) == [r["iters"] for r in runs]
    assert list(np.concatenate([m["converged"] for m in many])) == list(one["converged"])
    for k in ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b", "Sigma", "qld_x", "elbo", "llb", "chain_iters"):
        np.testing.assert_array_equal(np.concatenate([m[k] for m in many]), one[k], err_msg=k)
    scale = np.abs(one["history"]).max()
    for m in many:
        assert m["history"].shape == one["history"].shape
        assert np.abs(m["history"] - one["history"]).max() <= 1e-12 * scale
        assert np.abs(m["elbo_total"] - one["elbo_total"]).max() <= 1e-12 * scale
    assert np.array_equal(many[0]["history"], many[1]["history"])


def test_argument_errors_and_the_refusal_that_stays():
    from pyvb_amd import _capi
    b = _batch("reference")
    try:
        for args in ((-1, 1e-3, 8), (10, 1e-3, 0), (10, float("nan"), 8)):
            with pytest.raises(_capi.PyvbHipError) as ei:
                b.iterate_until_model(*args)
            assert ei.value.code == _capi.E_ARG
        with pytest.raises(_capi.PyvbHipError) as ei:   # the per-replicate entry still refuses a tied handle, and names this one
            b.iterate_until(5)
        assert ei.value.code == _capi.E_UNSUPPORTED and "per model" in str(ei.value) and "pyvb_lds_iterate_until_model" in str(ei.value)
        assert b.iterate_until_model(0) == 0
        it, cv, llb = b.model_convergence()
        assert it.shape == (4,) and not it.any() and not cv.any() and np.isnan(llb).all()
    finally:
        b.close()
