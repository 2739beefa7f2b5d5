"""GPU: per-replicate convergence on the device (include/pyvb_hip.h: pyvb_lds_iterate_until, pyvb_lds_get_convergence) through
pyvb_amd.lds.LDSBatch.

The comparator is always the oracle run alone on one replicate with network.py:53 applied on the host (tests/converge_ref.py),
on inputs where that decision is not a rounding matter (its guard; tests/test_converge_cpu.py asserts it for every case).  Stop
iterations are compared exactly, states at RTOL = 1e-8 (tests/test_gpu_parity.py), the bound as in its _stagewise.

"Bitwise" is justified as in tests/test_status_mask_gpu.py: replicates share no arithmetic, and a twin handle of the same
N, T, D, K and time split runs the same instructions in the same order on the rows both compute.  The one tolerance there:
the totals sum the rows in another order than numpy does -- at most N additions per part, N * 2^-52 of the magnitudes.
"""
import functools

import numpy as np
import pytest

import converge_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-8


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


def _batch(name, W=None):
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, lengths = R.problem(name)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=lengths)
    if R.CASES[name]["bound"] == "exact":
        b.set_bound_mode("exact")
    if R.CASES[name].get("nan"):
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
    if b.noise == "wishart":
        out.update(b.get_wishart_state())
        out["A_cov"], out["C_cov"] = b.get_column_cov()
    if with_elbo:
        out["elbo"] = b.elbo()
    return out


def _same_rows(a, b, rows, what):
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)


def _until(b, name, check_every=8, tol=None, max_iters=None):
    c = R.CASES[name]
    return b.iterate_until(c["max_iters"] if max_iters is None else max_iters, c["tol"] if tol is None else tol, check_every)


@functools.lru_cache(maxsize=None)
def _ran(name, check_every=8):
    """One handle of a case after iterate_until, read out once and shared: do not write to the arrays."""
    b = _batch(name)
    try:
        out = dict(iters_run=_until(b, name, check_every))
        out["iters"], out["converged"], out["llb"] = b.convergence()
        out["history"], out["total"], out["active"] = b.elbo_history(), b.elbo_total(), b.active()
        out["all"] = _everything(b)
        out["rerun"] = b.iterate_until(5) if out["converged"].all() else None
    finally:
        b.close()
    return out


def _against_oracle(got, runs, name, tag=""):
    """The state of every replicate at its own stop (a frozen replicate reads back as its last iteration left it)."""
    g, pri = got["all"], R.problem(name)[2]
    for n, r in enumerate(runs):
        st, t = r["st"], "%scase %s, replicate %d (%d iterations): " % (tag, name, n, r["iters"])
        Tn = st["X"].shape[1]
        cls = [0, 1, 2] if Tn > 2 else [0, 2]
        _close(g["X"][n, :Tn], st["X"][0], t + "X")
        _close(g["A_mean"][n], st["A_mean"][0], t + "A_mean")
        _close(g["C_mean"][n], st["C_mean"][0], t + "C_mean")
        _close(g["A_colvar"][n], np.einsum("ikk->ik", st["A_cov"][0]), t + "A_colvar")
        _close(g["C_colvar"][n], np.einsum("ikk->ik", st["C_cov"][0]), t + "C_colvar")
        if pri["noise"] == "wishart":
            for nm, key in (("Q_v", "Q_a"), ("Q_w", "Q_b"), ("R_v", "R_a"), ("R_w", "R_b")):
                _close(g[nm][n], st[key][0], t + nm)
        else:
            for nm in ("Q_a", "Q_b", "R_a", "R_b"):
                _close(g[nm][n], np.broadcast_to(st[nm][0], g[nm][n].shape), t + nm)
        _close(g["Sigma"][n][cls], st["Sigma"][0][cls], t + "Sigma")
        _close_qld(g["qld_x"][n][cls], st["qld_x"][0][cls], t + "qld_x")
        _close_qld(g["qld_A"][n], st["qld_A"][0], t + "qld_A")
        _close_qld(g["qld_C"][n], st["qld_C"][0], t + "qld_C")
        want = r["trace"][-1]
        assert np.all(np.abs(g["elbo"][n] - want) <= RTOL * np.abs(want).sum()), "%sparts\n%r\n%r" % (t, g["elbo"][n], want)
        assert abs(got["llb"][n] - want.sum()) <= RTOL * abs(want.sum()), t + "llb"


def _same_decisions(got, runs, what):
    assert list(got["iters"]) == [r["iters"] for r in runs], (what, got["iters"])
    assert list(got["converged"]) == [r["converged"] for r in runs], (what, got["converged"])


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C_reference", "C_exact", "D", "E", "F", "wishart", "nan"])
def test_every_replicate_stops_where_the_reference_would(name):
    got, runs = _ran(name), R.alone(name)
    print("case %s: iters %s converged %s iters_run %d" % (name, got["iters"], got["converged"].astype(int), got["iters_run"]))
    _same_decisions(got, runs, name)
    _against_oracle(got, runs, name)
    assert got["active"].all()
    if got["rerun"] is not None:                        # nobody left: nothing is launched
        assert got["rerun"] == 0


# ---- 2. bitwise against a twin that ran iterate() --------------------------------------------------------------------------
def test_a_stopped_replicate_is_the_twin_that_ran_as_many_iterations():
    got = _ran("A")
    twin, done = _batch("A"), 0
    try:
        for k in sorted(set(got["iters"])):             # (the replicate that never stops has 40)
            twin.iterate(int(k) - done); done = int(k)
            _same_rows(got["all"], _everything(twin), got["iters"] == k, "replicates with %d iterations" % k)
    finally:
        twin.close()


# ---- 3. frozen stays frozen, on either side of the two ping-pongs ----------------------------------------------------------
def test_frozen_replicates_stay_frozen_through_later_updates():
    b, twin = _batch("A"), _batch("A")
    try:
        assert _until(b, "A") == 40
        _, conv, _ = b.convergence()
        assert {int(i) % 2 for i in b.convergence()[0][conv]} == {0, 1}     # rows frozen in odd and in even iterations
        first = _everything(b)
        twin.iterate(40)
        for more in (1, 2):
            b.iterate(more); twin.iterate(more)
            now = _everything(b)
            _same_rows(now, first, conv, "converged rows after %d more iteration(s)" % more)
            _same_rows(now, _everything(twin), ~conv, "the running replicate against the twin")
        b.sweep("forward")                              # (an odd number of flips: the getters meet the parked rows in the other buffer)
        _same_rows(_everything(b), first, conv, "converged rows after a single sweep")
        assert list(b.convergence()[0]) == [23, 31, 25, 10, 40, 24]          # iterate() and sweep() are not counted
    finally:
        b.close(); twin.close()


# ---- 4. check_every changes nothing but iters_run ---------------------------------------------------------------------------
def test_check_every_only_moves_the_return():
    runs, base = R.alone("F"), _ran("F", 1)
    last = max(r["iters"] for r in runs)
    assert last == 4 and base["iters_run"] == 4
    for ce in (3, 64):
        got = _ran("F", ce)
        assert last <= got["iters_run"] <= min(last + ce - 1, R.CASES["F"]["max_iters"]), (ce, got["iters_run"])
        _same_rows(got["all"], base["all"], slice(None), "check_every = %d" % ce)
        for k in ("iters", "converged", "llb", "total"):
            assert np.array_equal(got[k], base[k]), (ce, k)
        assert np.array_equal(got["history"][:4], base["history"])
        assert np.array_equal(got["history"][4:], np.repeat(base["history"][-1:], got["iters_run"] - 4, axis=0))    # idle iterations
    assert _ran("A")["iters_run"] == 40                 # one replicate of case A never stops


# ---- 5. the totals count the converged replicates at their final bound ------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "F"])
def test_totals_hold_converged_replicates_at_their_final_bound(name):
    got, runs = _ran(name), R.alone(name)
    N = len(runs)
    assert got["history"].shape == (got["iters_run"], 6)
    want = R.totals(runs, got["iters_run"])
    scale = sum(np.abs(r["trace"]).sum(1).max() for r in runs)
    assert np.all(np.abs(got["history"] - want) <= RTOL * scale), np.abs(got["history"] - want).max() / scale
    rows = got["all"]["elbo"]
    assert np.all(np.abs(got["total"] - rows.sum(0)) <= N * 2.0 ** -52 * np.abs(rows).sum(0)), (got["total"], rows.sum(0))
    assert np.array_equal(got["history"][-1], got["total"])
    assert got["active"].all()


# ---- 6. a replicate the caller switched off ---------------------------------------------------------------------------------
def test_a_switched_off_replicate_is_not_run_tested_or_counted():
    runs, off = R.alone("A"), 2
    mask = np.ones(6, dtype=bool); mask[off] = False
    b = _batch("A")
    try:
        before = _everything(b, with_elbo=False)        # (no bound exists before the first complete sweep)
        b.set_active(mask)
        got = dict(iters_run=_until(b, "A"), all=_everything(b), history=b.elbo_history(), total=b.elbo_total())
        got["iters"], got["converged"], got["llb"] = b.convergence()
        assert np.array_equal(b.active(), mask)
    finally:
        b.close()
    assert got["iters"][off] == 0 and not got["converged"][off] and np.isnan(got["llb"][off])
    _same_rows({k: v for k, v in got["all"].items() if k != "elbo"}, before, ~mask, "the switched-off row")
    assert not got["all"]["elbo"][off].any()
    others = [r for n, r in enumerate(runs) if mask[n]]
    assert list(got["iters"][mask]) == [r["iters"] for r in others] and list(got["converged"][mask]) == [r["converged"] for r in others]
    _same_rows(got["all"], _ran("A")["all"], mask, "the others against the handle where nothing was switched off")
    want = R.totals(others, got["iters_run"])
    scale = sum(np.abs(r["trace"]).sum(1).max() for r in others)
    assert got["history"].shape == (40, 6) and np.all(np.abs(got["history"] - want) <= RTOL * scale)
    assert np.array_equal(got["history"][-1], got["total"])


# ---- 7. a second call ----------------------------------------------------------------------------------------------------------
def test_a_second_call_moves_only_what_still_runs_and_starts_from_minus_infinity():
    runs2 = R.resumed("A", 0.5, 40)
    b = _batch("A")
    try:
        assert _until(b, "A") == 40
        first = _everything(b)
        conv1 = b.convergence()[1]
        b.reset_elbo_history()
        n2 = b.iterate_until(40, 0.5, 1)
        got = dict(iters_run=n2, all=_everything(b), history=b.elbo_history())
        got["iters"], got["converged"], got["llb"] = b.convergence()
        assert n2 == runs2[4]["iters"] - 40 and n2 > 1, n2          # (old = -inf again: its first iteration stops nobody)
        _same_decisions(got, runs2, "second call")
        _same_rows(got["all"], first, conv1, "replicates that had converged in the first call")
        _against_oracle(got, runs2, "A", "second call, ")
        want = R.totals(runs2, n2)
        scale = sum(np.abs(r["trace"]).sum(1).max() for r in runs2)
        assert got["history"].shape == (n2, 6) and np.all(np.abs(got["history"] - want) <= RTOL * scale)
        assert b.iterate_until(5) == 0                  # everybody has converged
    finally:
        b.close()


# ---- 8. the time axis split over several wavefronts ------------------------------------------------------------------------
def test_a_forced_time_split_stops_in_the_same_iterations():
    runs = R.alone("split")
    for W in (1, 2):
        b = _batch("split", W)
        try:
            assert b.get_time_split() == W
            got = dict(iters_run=_until(b, "split"), all=_everything(b))
            got["iters"], got["converged"], got["llb"] = b.convergence()
        finally:
            b.close()
        _same_decisions(got, runs, "W = %d" % W)
        _against_oracle(got, runs, "split", "W = %d, " % W)


def test_argument_errors():
    from pyvb_amd import _capi
    b = _batch("F")
    try:
        for args in ((-1, 1e-3, 8), (10, 1e-3, 0), (10, float("nan"), 8)):
            with pytest.raises(_capi.PyvbHipError) as ei:
                b.iterate_until(*args)
            assert ei.value.code == _capi.E_ARG
        assert b.iterate_until(0) == 0
        it, cv, llb = b.convergence()
        assert not it.any() and not cv.any() and np.isnan(llb).all()
    finally:
        b.close()


# ---- 9. what a refactor of the stopping loop must not move -------------------------------------------------------------------
def _small(models=None):
    """N = 5, T = 12, D = 4, K = 5, DiagonalGamma, chains of 12, 2, 7, 3, 12 nodes (padding zeroed as R.problem does)."""
    from pyvb_amd import synth
    from pyvb_amd.lds import LDSBatch
    lengths = np.array([12, 2, 7, 3, 12], dtype=np.int32)
    Y, st0, pri = synth.make_problem(12, 4, 5, 5, seed=8500)
    live = np.arange(12)[None, :] < lengths[:, None]
    Y = np.where(live[:, :, None], Y, 0.0)
    st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
    return LDSBatch.from_problem(Y, st0, pri, lengths=lengths, models=models)


def test_the_three_loops_agree_bitwise_when_nobody_stops():
    """iterate(6), iterate_until(6, -inf) and iterate_until_model(6, -inf): llb - old < -inf is never true, so nobody stops and
    the three loops carry out the same six iterations -- the bound on the side stream in one, on the main stream in the others."""
    ninf = float("-inf")
    loops = {"iterate": lambda b: b.iterate(6), "until": lambda b: b.iterate_until(6, ninf, 4), "until_model": lambda b: b.iterate_until_model(6, ninf, 4)}
    for models, names in ((None, ("iterate", "until", "until_model")), (np.array([0, 0, 1, 2, 2], dtype=np.int32), ("iterate", "until_model"))):
        got = {}
        for nm in names:
            b = _small(models)
            try:
                ran = loops[nm](b)
                assert ran in (None, 6), (nm, ran)
                g = dict(history=b.elbo_history(), total=b.elbo_total(), all=_everything(b, with_elbo=False))
                g["iters"], g["converged"], g["llb"] = b.convergence()
                got[nm] = g
            finally:
                b.close()
        base = got["iterate"]
        assert base["history"].shape == (6, 6) and np.all(np.isfinite(base["history"]))
        for nm in names[1:]:
            what = "%s against iterate, models %r" % (nm, models)
            assert np.array_equal(got[nm]["history"], base["history"]), what
            assert np.array_equal(got[nm]["total"], base["total"]), what
            _same_rows(got[nm]["all"], base["all"], slice(None), what)
            assert list(got[nm]["iters"]) == [6] * 5 and not got[nm]["converged"].any(), what
            assert np.all(np.isfinite(got[nm]["llb"])), what
        if "until" in got:      # the last bound the test saw is defined in both
            assert np.array_equal(got["until"]["llb"], got["until_model"]["llb"])


SUM_OFF = (0, 41, 97, 150, 255, 256, 299)       # switched off: row 0 and row 299 among them, a pair that shares a thread (0 and 256)


@functools.lru_cache(maxsize=None)
def _sum_problem():
    """N = 300 (the smallest N at which some of the 256 threads of the totals kernel add two rows), T = 4, D = 2, K = 2: the
    problem, the oracle's bound over four iterations, and a tol at which some replicates but not all stop within them.  The
    oracle runs the batch at once (replicates share no arithmetic); tol is the middle of the widest gap between deltas at which
    20-80 % of the replicates that are switched on stop."""
    from oracle import lds_closed_form as O
    from pyvb_amd import synth
    N, T, D, K = 300, 4, 2, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=8600)
    st = O.expand_state(st0, pri, T)
    trace = np.array([O.iterate(st, pri, Y) for _ in range(4)])            # [4, N, 6]
    mask = np.ones(N, dtype=bool); mask[list(SUM_OFF)] = False
    d = np.diff(trace.sum(2), axis=0)[:, mask]                              # [3, on] the deltas a run with tol = -inf meets
    cand = np.sort(d.ravel())
    mid, gap = 0.5 * (cand[1:] + cand[:-1]), np.diff(cand)
    share = np.array([(d.min(0) < t).mean() for t in mid])
    ok = (share >= 0.2) & (share <= 0.8)
    tol = float(mid[ok][np.argmax(gap[ok])])
    return Y, st0, pri, mask, trace, tol


def _kernel_order_total(rows, mask):
    """The totals as the kernel forms them: thread tid adds rows tid, tid + 256, .. that count, in turn; then the 256 partial
    sums are added in ascending order."""
    out = np.zeros(6)
    for p in range(6):
        t = np.float64(0.0)
        for tid in range(256):
            s = np.float64(0.0)
            for n in range(tid, len(rows), 256):
                if mask[n]:
                    s = s + rows[n, p]
            t = t + s
        out[p] = t
    return out


def test_the_totals_are_the_kernel_s_own_sum_order():
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, mask, trace, tol = _sum_problem()
    # the reference's decisions at this tol, through converge_ref's loop and its guard, asserted before anything is compared
    runs = []
    for n in np.nonzero(mask)[0]:
        rows = iter(trace[:, n])
        runs.append(R.guarded(R.learn(lambda: next(rows), tol, 4), tol, "totals, replicate %d" % n))
    stopped = sum(r[1] for r in runs)
    print("tol %.6g: %d of %d replicates stop within 4 iterations, smallest margin %.2e" % (tol, stopped, len(runs), min(r[3] for r in runs)))
    assert 0 < stopped < len(runs)
    for loop in ("until", "iterate"):
        b = LDSBatch.from_problem(Y, st0, pri)
        try:
            b.set_active(mask)
            if loop == "until":
                assert b.iterate_until(4, tol, 8) == 4
                it, cv, _ = b.convergence()
                assert list(it[mask]) == [r[0] for r in runs] and list(cv[mask]) == [r[1] for r in runs]
                assert not it[~mask].any() and not cv[~mask].any()
            else:
                b.iterate(2)
            history, total = b.elbo_history(), b.elbo_total()
            rows = b.elbo()
            assert np.array_equal(b.active(), mask)
            want = _kernel_order_total(rows, b.active())
            print("%s: total %r" % (loop, total))
            assert np.array_equal(total, want), (loop, total - want)
            assert np.array_equal(history[-1], want), (loop, history[-1] - want)
            assert np.array_equal(b.elbo_total(), want), loop
        finally:
            b.close()
