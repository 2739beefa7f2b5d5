"""GPU: LDS handles whose chains share A, C, Q, R (include/pyvb_hip.h: pyvb_lds_create_tied) -- several time series, one model.

The comparator is tests/tied_ref.py, the composition of oracle functions that tests/test_tied_cpu.py pins against the reference's
own run of such a graph, and that run itself (tests/golden/tied_*.npz).  Tolerances are those of tests/test_gpu_parity.py and
tests/test_lengths_gpu.py: RTOL = 1e-8 max-norm for states and parameters, q_ln_det through its reciprocal, the parts of the bound
to RTOL of the sum of their magnitudes and the total to RTOL of itself.

Shapes: D = 4, K = 5 (no multiple of 16), T = 60, six chains in models of [1, 3, 2] chains -- a singleton beside two tied models;
one test puts it between them, [3, 1, 2] -- with ragged lengths that include T_n = 2 and 3.

Section 8 holds models of five and more chains (tests/tied_ref.py: CASES, with the argument which case reaches which path of
k_tie.hip) to the accuracy envelope of DESIGN.md section 17 against the comparator's long-double run, and covers a handle with more
models than the grid of k_tie has rows.

"Bitwise" is justified as in tests/test_lengths_gpu.py: rows share no arithmetic but the sums of k_tie.hip, which adds the chains
of a model in ascending replicate order whatever the launch, so two handles of the same shapes, lengths, models and time split run
the same instructions in the same order.
"""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_bound_ref as XR
import extended_ref as ER
import tied_ref as TR
from conftest import GOLDEN_DIR
from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-8
HERE = os.path.dirname(os.path.abspath(__file__))
T, D, K = 60, 4, 5
LENGTHS = [19, 60, 2, 33, 3, 17]
MODELS = [0, 1, 1, 1, 2, 2]
TIED = sorted(glob.glob(os.path.join(GOLDEN_DIR, "tied_*.npz")))


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


def _gamma(pri):
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)


def _problem(seed, kind="diagonal_gamma", fill=0.0, lengths=LENGTHS, T=T, D=D, K=K):
    N = len(lengths)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=seed)
    if kind == "gamma":
        _gamma(pri)
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    Y = np.where(live[:, :, None], Y, fill)
    st0["X"] = np.where(live[:, :, None], st0["X"], fill)
    return Y, st0, pri


def _batch(Y, st0, pri, lengths=LENGTHS, models=MODELS):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=None if lengths is None else np.asarray(lengths, dtype=np.int32),
                                 models=None if models is None else np.asarray(models, dtype=np.int32))


def _rows(models):
    models = np.asarray(models)
    return [list(np.nonzero(models == m)[0]) for m in range(models.max() + 1)]


def _ref(Y, st0, pri, lengths=LENGTHS, models=MODELS):
    """Per model: (rows, chain states, outputs per chain) -- the comparator's view of what the handle was given."""
    out = []
    for rows in _rows(models):
        f = rows[0]
        Ys = [Y[n:n + 1, :lengths[n]].copy() for n in rows]
        st0s = [{k: (v[n:n + 1, :lengths[n]] if k in ("X", "Yq", "Yrowvar") else v[f:f + 1]).copy() for k, v in st0.items()} for n in rows]
        out.append((rows, TR.make_model(Ys, st0s, pri), Ys))
    return out


def _cls(Tn):
    return [0, 1, 2] if Tn > 2 else [0, 2]


def _compare_x(b, ref, tag):
    X = b.get_state(("X",))["X"]
    for rows, chains, Ys in ref:
        for n, st in zip(rows, chains):
            Tn = st["X"].shape[1]
            _close(X[n, :Tn], st["X"][0], "%sX of replicate %d (T_n = %d)" % (tag, n, Tn))
            assert np.array_equal(X[n, Tn:], np.zeros_like(X[n, Tn:])), "%spadding rows of X, replicate %d" % (tag, n)


def _compare_classes(b, ref, tag):
    Sig, qld = b.get_posterior_classes()
    for rows, chains, Ys in ref:
        for n, st in zip(rows, chains):
            c = _cls(st["X"].shape[1])
            _close(Sig[n][c], st["Sigma"][0][c], tag + "Sigma of replicate %d" % n)
            _close_qld(qld[n][c], st["qld_x"][0][c], tag + "qld_x of replicate %d" % n)


def _rows_equal(g, rows, what):
    for k, v in g.items():
        if k != "X":
            for n in rows[1:]:
                assert np.array_equal(v[n], v[rows[0]], equal_nan=True), "%s%s differs between rows %d and %d of one model" % (what, k, rows[0], n)


def _compare_params(b, ref, tag, qld=True):
    g = b.get_state()
    qa, qc = b.get_column_qld()
    ld = b.get_logdets()
    g.update(qld_A=qa, qld_C=qc, lnd_A=ld["A"], lnd_C=ld["C"])
    for rows, chains, Ys in ref:
        st = chains[0]
        _rows_equal(g, rows, tag)
        for n in rows:
            t = "%sreplicate %d " % (tag, n)
            _close(g["A_mean"][n], st["A_mean"][0], t + "A_mean")
            _close(g["C_mean"][n], st["C_mean"][0], t + "C_mean")
            _close(g["A_colvar"][n], np.einsum("ikk->ik", st["A_cov"][0]), t + "A_colvar")
            _close(g["C_colvar"][n], np.einsum("ikk->ik", st["C_cov"][0]), t + "C_colvar")
            for nm in ("Q_a", "Q_b", "R_a", "R_b"):
                _close(g[nm][n], np.broadcast_to(st[nm][0], g[nm][n].shape), t + nm)
            if qld:
                _close_qld(qa[n], st["qld_A"][0], t + "qld_A")
                _close_qld(qc[n], st["qld_C"][0], t + "qld_C")


def _compare_parts(got, want, what, exact=False):
    print("%s: parts %r want %r" % (what, got, want))
    assert np.all(np.isfinite(got)), what
    if exact:       # tests/test_lengths_gpu.py::test_exact_bound_per_replicate
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "%s\n%r\n%r" % (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= RTOL * np.abs(want).sum()), "%s\n%r\n%r" % (what, got, want)
        assert abs(got.sum() - want.sum()) <= RTOL * abs(want.sum()), what + ": total"


def _compare_elbo(parts, ref, pri, tag, exact=False):
    """The rows of a model add up to the six parts of its graph; the shared nodes' parts are booked on its first row."""
    for m, (rows, chains, Ys) in enumerate(ref):
        want = TR.elbo_parts(chains, pri, Ys, XR.elbo_parts_exact if exact else None)
        _compare_parts(parts[rows].sum(0), want, "%smodel %d" % (tag, m), exact)
        assert np.all(parts[rows[1:], 2:] == 0.0), "%smodel %d: L_A, L_C, L_Q, L_R on rows that are not the first" % (tag, m)
        assert np.all(parts[rows[0], 2:] != 0.0)


def _everything(b):
    out = dict(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["qld_A"], out["qld_C"] = b.get_column_qld()
    for k, v in b.get_logdets().items():
        out["lnd_" + k] = v
    out["Yq"], out["Yvar"], out["Yqld"] = b.get_outputs(with_qld=True)
    out["elbo"] = b.elbo()
    return out


def _same(a, b, rows=slice(None), what=""):
    for k in a:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)


# ---- 1. the reference's own run of the shared-parameter graph ---------------------------------------------------------------
@pytest.mark.parametrize("path", TIED, ids=lambda p: os.path.basename(p)[5:-4])
def test_reference_run_is_reproduced(path):
    """The fixture's model, with a singleton in front of it (its first chain on its own): at every recorded iteration the
    chains, the shared parameters and the six parts are the reference's."""
    from pyvb_amd.lds import LDSBatch
    meta, Ys, st0s, pri, z = TR.load_tied(path)
    lengths = meta["lengths"]
    trial = [(Y[0], st) for Y, st in zip(Ys, st0s)]
    b = LDSBatch.from_trials([trial[:1], trial], pri)
    C = len(lengths)
    assert list(b.models) == [0] + [1] * C and list(b.lengths) == lengths[:1] + lengths
    b.sweep("forward")
    X = b.get_state(("X",))["X"]
    for n, Tn in enumerate(lengths):
        _close(X[1 + n, :Tn], z["it1_fwd_X"][n, :Tn], "forward sweep, chain %d" % n)
    b.sweep("backward")
    for it in range(1, max(meta["iters"]) + 1):
        if it > 1:
            b.sweep("forward"); b.sweep("backward")
        b.update_A(); b.update_C(); b.update_Q(); b.update_R()
        if it not in meta["iters"]:
            continue
        tag = "it%d_" % it
        g = b.get_state()
        Sig, qld = b.get_posterior_classes()
        qa, qc = b.get_column_qld()
        parts = b.elbo()
        for n, Tn in enumerate(lengths):
            r, what = 1 + n, "%schain %d (T_n = %d) " % (tag, n, Tn)
            _close(g["X"][r, :Tn], z[tag + "X"][n, :Tn], what + "X")
            _close(Sig[r][_cls(Tn)], z[tag + "Sigma"][n][_cls(Tn)], what + "Sigma")
            _close_qld(qld[r][_cls(Tn)], z[tag + "qld_x"][n][_cls(Tn)], what + "qld_x")
            _close(g["A_mean"][r], z[tag + "A_mean"], what + "A_mean")
            _close(g["C_mean"][r], z[tag + "C_mean"], what + "C_mean")
            _close(g["A_colvar"][r], z[tag + "A_colvar"], what + "A_colvar")
            _close(g["C_colvar"][r], z[tag + "C_colvar"], what + "C_colvar")
            _close_qld(qa[r], z[tag + "qld_A"], what + "qld_A")
            _close_qld(qc[r], z[tag + "qld_C"], what + "qld_C")
            for nm in ("Q_a", "Q_b", "R_a", "R_b"):
                _close(g[nm][r], np.broadcast_to(z[tag + nm], g[nm][r].shape), what + nm)
        _compare_parts(parts[1:].sum(0), z[tag + "elbo_parts"], tag + "the model")
        assert np.all(parts[2:, 2:] == 0.0)
        assert np.allclose(b.elbo_total(), parts.sum(0), rtol=1e-12)
    b.close()


# ---- 2. stage by stage against the comparator -------------------------------------------------------------------------------
def _stagewise(Y, st0, pri, lengths, models, iters, bound="reference", W=None, missing=False):
    b = _batch(Y, st0, pri, lengths, models)
    if W is not None:
        b.set_time_split(W)
    b.set_bound_mode(bound)
    lens = list(b.lengths)
    ref = _ref(Y, st0, pri, lens, models)
    assert np.array_equal(b.models, np.asarray(models))
    for it in range(iters):
        tag = "it%d " % it
        for direction in ("forward", "backward"):
            for rows, chains, Ys in ref:
                TR.sweep(chains, pri, Ys, direction)
            b.sweep(direction)
            _compare_x(b, ref, tag + direction + " sweep: ")
        _compare_classes(b, ref, tag)
        if missing:
            b.update_Y()
            q, v = b.get_outputs()
            for rows, chains, Ys in ref:
                TR.update_Y(chains, pri)
                for n, st in zip(rows, chains):
                    _close(q[n], st["Yq"][0], tag + "Yq of replicate %d" % n)
                    _close(v[n], st["Yvar"][0], tag + "Yvar of replicate %d" % n)
        pooled = [TR.statistics(chains, Ys)[1] for rows, chains, Ys in ref]
        for (rows, chains, Ys), S in zip(ref, pooled):
            TR.update_A(chains, pri, S)
        b.update_A()
        A = b.get_state(("A_mean",))["A_mean"]
        for rows, chains, Ys in ref:
            for n in rows:
                _close(A[n], chains[0]["A_mean"][0], tag + "A_mean after update_A, replicate %d" % n)
        for (rows, chains, Ys), S in zip(ref, pooled):
            TR.update_C(chains, pri, S)
        b.update_C()
        Cm = b.get_state(("C_mean",))["C_mean"]
        for rows, chains, Ys in ref:
            for n in rows:
                _close(Cm[n], chains[0]["C_mean"][0], tag + "C_mean after update_C, replicate %d" % n)
        for (rows, chains, Ys), S in zip(ref, pooled):
            TR.update_Q(chains, pri, S, Ys)
        b.update_Q()
        Qb = b.get_state(("Q_b",))["Q_b"]
        for rows, chains, Ys in ref:
            for n in rows:
                _close(Qb[n], np.broadcast_to(chains[0]["Q_b"][0], Qb[n].shape), tag + "Q_b after update_Q, replicate %d" % n)
        for (rows, chains, Ys), S in zip(ref, pooled):
            TR.update_R(chains, pri, S, Ys)
        b.update_R()
        _compare_params(b, ref, tag, qld=pri.get("A_obs") is None)
        _compare_elbo(b.elbo(), ref, pri, tag, exact=bound == "exact")
    b.close()


@pytest.mark.parametrize("bound", ["reference", "exact"])
@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_stagewise_vs_tied_ref(kind, bound):
    Y, st0, pri = _problem(9000, kind)
    _stagewise(Y, st0, pri, LENGTHS, MODELS, iters=2, bound=bound)


def test_a_singleton_between_two_tied_models():
    Y, st0, pri = _problem(9005)
    _stagewise(Y, st0, pri, LENGTHS, [0, 0, 0, 1, 2, 2], iters=2)


def test_a_larger_odd_shape():
    """D = 33, K = 17 (three and two 16-tiles, padded): the moment block has an odd number of entries, so k_tie takes its
    8-byte path, and its grid has more than one block along the elements."""
    lengths = [5, 40, 2, 3, 40]
    Y, st0, pri = _problem(9010, lengths=lengths, T=40, D=33, K=17)
    _stagewise(Y, st0, pri, lengths, [0, 0, 0, 1, 1], iters=1)


def test_known_entries_of_A_and_C():
    Y, st0, pri = _problem(9020)
    rng = np.random.default_rng(D)
    A_obs = np.where(rng.random((D, D)) < 0.2, 0.3 * rng.standard_normal((D, D)), np.nan)
    C_obs = np.where(rng.random((K, D)) < 0.2, rng.standard_normal((K, D)), np.nan)
    A_obs[:, 1] = 0.1
    C_obs[:, 0] = np.nan
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    _stagewise(Y, st0, pri, LENGTHS, MODELS, iters=2)


@pytest.mark.parametrize("bound", ["reference", "exact"])
def test_outputs_with_nan_on_equal_lengths(bound):
    """Outputs that hold NaN are variational nodes (update_Y); <y y^T> of a model then sums the chains' variances too."""
    Tm, N = 20, len(MODELS)
    Y, st0, pri = _problem(9030, lengths=[Tm] * N, T=Tm)
    rng = np.random.default_rng(5)
    mask = rng.random((N, Tm, K)) < 0.2
    mask[:, 1] = True; mask[:, 3] = False; mask[2, 0, 0] = True
    Y = np.where(mask, np.nan, Y)
    st0["Yq"] = rng.standard_normal((N, Tm, K))
    st0["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, Tm))
    _stagewise(Y, st0, pri, None, MODELS, iters=2, bound=bound, missing=True)


@pytest.mark.parametrize("W", [1, 2, 3])
def test_every_time_split(W):
    """(T - 2) / W >= 16 allows W = 1, 2, 3 at T = 60.  Short chains leave whole parts of the time axis without nodes."""
    Y, st0, pri = _problem(9040)
    _stagewise(Y, st0, pri, LENGTHS, MODELS, iters=1, W=W)
    b = _batch(Y, st0, pri)
    b.set_time_split(W)
    ref = _ref(Y, st0, pri)
    b.iterate(2)
    for rows, chains, Ys in ref:
        TR.iterate(chains, pri, Ys); TR.iterate(chains, pri, Ys)
    _compare_x(b, ref, "iterate, W = %d: " % W)
    _compare_params(b, ref, "iterate, W = %d: " % W)
    _compare_elbo(b.elbo(), ref, pri, "iterate, W = %d: " % W)
    b.close()


# ---- 3. calling orders ------------------------------------------------------------------------------------------------------
def test_iterate_equals_the_staged_calls_and_the_totals_sum_the_rows():
    Y, st0, pri = _problem(9050)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.iterate(2)
    for _ in range(2):
        b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.allclose(a.elbo(), b.elbo(), rtol=1e-12)
    hist = a.elbo_history(2)
    assert hist.shape == (2, 6)
    assert np.allclose(hist[-1], a.elbo().sum(0), rtol=1e-12)
    assert np.allclose(a.elbo_total(), a.elbo().sum(0), rtol=1e-12)
    # the statistics of a model are summed once per production: asking for the same update twice changes nothing
    b.update_A(); A1 = b.get_state(("A_mean",))["A_mean"]
    b.update_Q(); b.update_R(); e1 = b.elbo(); e2 = b.elbo()
    assert np.array_equal(e1, e2)
    c = _batch(Y, st0, pri)
    for _ in range(2):
        c.sweep("forward"); c.sweep("backward"); c.update_A(); c.update_C(); c.update_Q(); c.update_R()
    c.update_A()
    assert np.array_equal(A1, c.get_state(("A_mean",))["A_mean"])
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_single_updates_in_both_directions_equal_the_sweeps(kind):
    """pyvb_lds_update_x(t) for t = 0..T-1 and back against the two sweeps, through two iterations.

    Tolerance (max-norm per chain, 1e-10): the sweep kernel and the single-node kernel evaluate the same recurrence in float64
    with different summation orders, so one node differs by a few D eps of the state's norm; the Gauss-Seidel recurrence is a
    contraction, so over T = 60 nodes that stays below T D eps = 5e-14.  The second iteration starts from parameters that were
    updated from states differing by that much; the column and noise updates amplify it by the conditioning of the moment
    matrices (up to 1e3 at these shapes), which leaves 1e-10 with an order of magnitude to spare and two below the parity
    tolerance.  An element that is small beside its vector's norm has no relative accuracy of its own."""
    Y, st0, pri = _problem(9060, kind)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)

    def same_states(what):
        Xa, Xb = a.get_state(("X",))["X"], b.get_state(("X",))["X"]
        for n, Tn in enumerate(LENGTHS):
            print("%s, chain %d: rel err %.3e" % (what, n, _rel(Xa[n, :Tn], Xb[n, :Tn])))
        for n, Tn in enumerate(LENGTHS):
            _close(Xa[n, :Tn], Xb[n, :Tn], "%s, chain %d" % (what, n), rtol=1e-10)

    for it in range(2):
        a.sweep("forward")
        for t in range(T):
            b.update_x(t)
        same_states("forward, iteration %d" % it)
        a.sweep("backward")
        for t in reversed(range(T)):
            b.update_x(t)
        same_states("backward, iteration %d" % it)
        for h in (a, b):
            h.update_A(); h.update_C(); h.update_Q(); h.update_R()
        ea, eb = a.elbo(), b.elbo()
        print("iteration %d: bound rel err %.3e" % (it, _rel(ea.sum(0), eb.sum(0))))
        assert np.all(np.abs(ea - eb) <= 1e-10 * np.abs(eb).sum(0))
    ref = _ref(Y, st0, pri)
    c = _batch(Y, st0, pri)
    order = list(range(T)) + [T - 1, 5, 0, 2, 1]
    for t in order:
        c.update_x(t)
        for rows, chains, Ys in ref:
            TR.update_x(chains, pri, Ys, t)
    _compare_x(c, ref, "single updates: ")
    a.close(); b.close(); c.close()


# ---- 4. what does not change ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_singleton_models_are_a_lengths_handle(kind):
    Y, st0, pri = _problem(9070, kind)
    a, b = _batch(Y, st0, pri, LENGTHS, None), _batch(Y, st0, pri, LENGTHS, list(range(len(LENGTHS))))
    assert np.array_equal(a.models, b.models) and list(a.models) == list(range(len(LENGTHS)))
    for it in range(3):
        a.iterate(1); b.iterate(1)
        _same(_everything(a), _everything(b), what="iteration %d" % it)
    assert np.array_equal(a.elbo_history(), b.elbo_history())
    a.close(); b.close()


def test_rows_of_a_model_are_bitwise_equal():
    Y, st0, pri = _problem(9080)
    b = _batch(Y, st0, pri)
    for it in range(3):
        b.iterate(1)
        e = _everything(b)
        par = {k: e[k] for k in ("A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b", "qld_A", "qld_C", "lnd_A", "lnd_C")}
        for rows in _rows(MODELS):
            _rows_equal(par, rows, "iteration %d: " % it)
        assert not np.array_equal(e["A_mean"][0], e["A_mean"][1]) and not np.array_equal(e["A_mean"][1], e["A_mean"][4])
    b.close()


def test_set_state_reads_the_first_row_of_a_model_only():
    Y, st0, pri = _problem(9090)
    junk = {k: v.copy() for k, v in st0.items()}
    for rows in _rows(MODELS):
        for k in ("A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b"):
            junk[k][rows[1:]] = np.nan
    a, b = _batch(Y, st0, pri), _batch(Y, junk, pri)
    _same(b.get_state(), a.get_state(), what="right after set_state")
    a.iterate(3); b.iterate(3)
    ea = _everything(a)
    _same(ea, _everything(b))
    assert np.all(np.isfinite(ea["X"])) and np.all(np.isfinite(ea["elbo"]))
    a.close(); b.close()


def test_padding_is_never_read():
    outs = []
    for fill in (0.0, np.nan):
        Y, st0, pri = _problem(9100, fill=fill)
        b = _batch(Y, st0, pri)
        b.iterate(3)
        outs.append(_everything(b))
        outs[-1]["history"] = b.elbo_history()
        b.close()
    _same(outs[0], outs[1])
    assert np.all(np.isfinite(outs[0]["X"])) and np.all(np.isfinite(outs[0]["elbo"])) and np.all(np.isfinite(outs[0]["history"]))


# ---- 5. mask, convergence ---------------------------------------------------------------------------------------------------
def test_mask_drops_whole_models_only():
    from pyvb_amd import _capi
    Y, st0, pri = _problem(9110)
    b, twin = _batch(Y, st0, pri), _batch(Y, st0, pri)
    try:
        b.iterate(2); twin.iterate(2)
        before = _everything(b)
        for bad, m in (([1, 1, 0, 1, 1, 1], 1), ([1, 1, 1, 1, 1, 0], 2), ([1, 0, 0, 1, 1, 1], 1)):
            with pytest.raises(_capi.PyvbHipError) as ei:
                b.set_active(np.array(bad, dtype=bool))
            assert ei.value.code == _capi.E_ARG and "model %d" % m in str(ei.value) and "HIP" not in str(ei.value), str(ei.value)
        assert b.active().all()
        mask = np.array([1, 0, 0, 0, 1, 1], dtype=bool)             # model 1 leaves
        b.set_active(mask)
        for h in (b, twin):
            h.iterate(1)
            h.sweep("forward"); h.sweep("backward")
            h.update_x(0); h.update_x(2); h.update_x(T - 1)
            h.update_A(); h.update_C(); h.update_Q(); h.update_R()
            h.iterate(2)
        after, ref = _everything(b), _everything(twin)
        _same(after, before, ~mask, "switched-off rows")
        _same(after, ref, mask, "active rows")
        tot = b.elbo_total()
        assert np.all(np.abs(tot - after["elbo"][mask].sum(0)) <= 6 * 2.0 ** -52 * np.abs(after["elbo"][mask]).sum(0))
    finally:
        b.close(); twin.close()


def test_iterate_until_is_refused():
    from pyvb_amd import _capi
    Y, st0, pri = _problem(9120)
    b = _batch(Y, st0, pri)
    with pytest.raises(_capi.PyvbHipError) as ei:
        b.iterate_until(5)
    assert ei.value.code == _capi.E_UNSUPPORTED and "per model" in str(ei.value), str(ei.value)
    b.iterate(1)
    assert np.all(np.isfinite(b.elbo()))
    b.close()
    c = _batch(Y, st0, pri, LENGTHS, list(range(len(LENGTHS))))       # singleton models: served as before
    assert c.iterate_until(3, tol=-np.inf) == 3
    c.close()


# ---- 6. ranks ---------------------------------------------------------------------------------------------------------------
def test_models_sharded_over_two_ranks(tmp_path):
    """Two processes on the one GPU, the host transport for the all-reduce (tests/test_multirank_gpu.py): rank 0 holds models
    0 and 1, rank 1 holds model 2.  A model never spans ranks, so the rows are bitwise those of the single handle."""
    worker = os.path.join(HERE, "tied_multirank_worker.py")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29860", HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / "tied")
    procs = [subprocess.Popen([sys.executable, worker, str(r), "2", prefix], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=300)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    many = [dict(np.load(prefix + "_%d.npz" % r)) for r in range(2)]
    import tied_multirank_worker as MW
    one = MW.run(0, 1, None)
    assert [list(m["rows"]) for m in many] == [[0, 4], [4, 6]]
    for k in ("X", "A_mean", "C_mean", "Q_b", "R_b", "elbo"):
        np.testing.assert_array_equal(np.concatenate([m[k] for m in many]), one[k])
    total = sum(m["elbo"].sum(0) for m in many)
    for m in many:
        assert _rel(m["elbo_total"], total) < 1e-13
        assert _rel(m["elbo_total"], one["elbo_total"]) < 1e-12
        assert _rel(m["history"][-1], one["history"][-1]) < 1e-12


# ---- 7. the node front end --------------------------------------------------------------------------------------------------
def test_the_same_graph_through_the_node_front_end():
    """The shared-parameter graph built through pyvb_amd.nodes is not recognised as a fused LDS: it runs on the generic plan
    (the tape interpreter) and agrees with the tied handle."""
    import importlib.util
    from pyvb_amd import nodes
    from pyvb_amd.generic import GenericPlan
    from pyvb_amd.lds import LDSBatch
    spec = importlib.util.spec_from_file_location("make_golden_tied", os.path.join(HERE, "golden", "make_golden_tied.py"))
    MT = importlib.util.module_from_spec(spec); spec.loader.exec_module(MT)
    lengths, d, k = [5, 3, 2], 2, 3
    Y, st0, pri = _problem(9130, lengths=lengths, T=5, D=d, K=k)
    g = MT.build_tied_graph(nodes, [Y[n, :Tn] for n, Tn in enumerate(lengths)], pri, st0)
    b = LDSBatch.from_problem(Y, st0, pri, lengths=np.array(lengths, dtype=np.int32), models=np.zeros(3, dtype=np.int32))
    for it in range(2):
        for Xs, _ in g["chains"]:
            [x.update() for x in Xs]
        for Xs, _ in g["chains"]:
            [x.update() for x in reversed(Xs)]
        [a.update() for a in g["As"]]
        [c.update() for c in g["Cs"]]
        g["Q"].update(); g["R"].update()
        b.iterate(1)
        assert isinstance(g["chains"][0][0][0]._plan, GenericPlan)
        st = b.get_state()
        for n, (Xs, _) in enumerate(g["chains"]):
            _close(st["X"][n, :lengths[n]], np.hstack([x.qmu for x in Xs]).T, "it%d X of chain %d" % (it, n))
        _close(st["A_mean"][0], np.hstack([a.qmu for a in g["As"]]), "A_mean")
        _close(st["C_mean"][0], np.hstack([c.qmu for c in g["Cs"]]), "C_mean")
        _close(st["Q_b"][0], np.asarray(g["Q"].qb, dtype=float), "Q_b")
        _close(st["R_b"][0], np.asarray(g["R"].qb, dtype=float), "R_b")
        _close(st["Q_a"][0], np.asarray(g["Q"].qa, dtype=float), "Q_a")
        allX = [x for Xs, _ in g["chains"] for x in Xs]
        allY = [y for _, Ys in g["chains"] for y in Ys]
        want = np.array([sum(float(n.log_lower_bound()) for n in grp) for grp in (allX, allY, g["As"], g["Cs"])]
                        + [float(g["Q"].log_lower_bound()), float(g["R"].log_lower_bound())])
        _compare_parts(b.elbo().sum(0), want, "it%d bound" % it)
    b.close()


# ---- 8. models of five and more chains: every path of k_tie, at the accuracy envelope ----------------------------------------
PARAM_ROWS = ("A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b", "qld_A", "qld_C", "lnd_A", "lnd_C")


def _bounds(b):
    """{mode: parts [N, 6]} of the handle's current state (tests/test_ard_gpu.py: _bounds); the handle is left in reference mode."""
    out = {}
    for mode in ("exact", "reference"):
        b.set_bound_mode(mode)
        out[mode] = b.elbo()
    return out


def _parameter_rows(b):
    g = b.get_state()
    g["qld_A"], g["qld_C"] = b.get_column_qld()
    ld = b.get_logdets()
    g["lnd_A"], g["lnd_C"] = ld["A"], ld["C"]
    return g


def _readout(b, rows_of_models):
    """The handle's counterpart of tied_ref.snapshot, model by model: X per chain over its own length, Sigma on the live classes,
    the parameters from the model's first row, the parts summed over the model's rows (in long double: the sum is the test's, not
    the device's).  Asserts what holds by construction: zero padding, bitwise equal parameter rows, the shared nodes' parts on the
    first row only."""
    g, parts = _parameter_rows(b), _bounds(b)
    Sig = b.get_posterior_classes()[0]
    lens = b.lengths
    out = []
    for m, rows in enumerate(rows_of_models):
        _rows_equal({k: g[k] for k in PARAM_ROWS}, rows, "model %d: " % m)
        s = {"X": [g["X"][n, :lens[n]] for n in rows], "Sigma": [Sig[n][TR.live_classes(lens[n])] for n in rows]}
        for n in rows:
            assert not g["X"][n, lens[n]:].any(), "padding rows of X, replicate %d" % n
        for k in TR.PARAMS:
            s[k] = g[k][rows[0]]
        s["parts"] = {}
        for mode in TR.BOUNDS:
            assert np.all(parts[mode][rows[1:], 2:] == 0.0), "model %d, %s: L_A, L_C, L_Q, L_R on rows that are not the first" % (m, mode)
            assert np.all(parts[mode][rows[0], 2:] != 0.0)
            s["parts"][mode] = parts[mode][rows].astype(ER.LD).sum(0)
        out.append(s)
    return out, parts


def _parity(got, want, tag):
    """A snapshot (tied_ref.snapshot, _readout) against the float64 comparator's at this file's tolerances."""
    for k in ("X", "Sigma"):
        for c, (a, w) in enumerate(zip(got[k], want[k])):
            _close(a, w, "%s%s of chain %d" % (tag, k, c))
    for k in TR.PARAMS:
        _close(got[k], want[k], tag + k)
    for mode in TR.BOUNDS:
        _compare_parts(np.asarray(got["parts"][mode], dtype=float), np.asarray(want["parts"][mode], dtype=float), tag + mode, mode == "exact")


def _envelope(got, s64, sx, n, tag, worst):
    """The rule of DESIGN.md section 17 on one model (tied_ref.envelope), printed and asserted; worst: {kind: (e64, e_gpu, ratio)},
    the largest of each over what has been compared, for the summary line."""
    for what, e64, e_gpu, ratio in TR.envelope(got, s64, sx, n):
        print("%s%-16s e64 %.2e  e_gpu %.2e  (%.2f y)" % (tag, what, e64, e_gpu, ratio))
        kind = what.split()[0] if what.split()[0] in TR.BOUNDS else "states"
        worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0.0, 0.0, 0.0)), (e64, e_gpu, ratio)))
        assert e64 <= ER.CAP, (tag, what, e64)
        assert ratio <= ER.FACTOR, "%s%s: e_gpu %.3e is %.1f x max(e64 = %.3e, %d 2^-52)" % (tag, what, e_gpu, ratio, e64, n)


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_parity_and_envelope(name):
    """After each of two iterations: the states, the covariance classes, the parameters and both bounds of every model against the
    float64 comparator at RTOL and against its long-double run by e_gpu <= 16 max(e64, n 2^-52), n = max(D, K, sum of the model's
    T_c) (tied_ref.accumulation_length); e64 is measured here, on the CPU."""
    Y, st0, pri, lengths, models = TR.problem(name)
    (ms, f64), (_, ext) = TR.trace(name), TR.trace(name, extended=True)
    b = _batch(Y, st0, pri, lengths, models)
    worst = {}
    try:
        for it in range(TR.ITERS):
            b.iterate(1)
            got, parts = _readout(b, [rows for rows, _, _ in ms])
            for m, (rows, chains, Ys) in enumerate(ms):
                tag = "%s iteration %d model %d (%d chains) " % (name, it + 1, m, len(rows))
                _parity(got[m], f64[it][m], tag)
                _envelope(got[m], f64[it][m], ext[it][m], TR.accumulation_length(chains), tag, worst)
            tot, rows_sum = b.elbo_total(), parts["reference"].sum(0)
            assert np.all(np.abs(tot - rows_sum) <= 1e-12 * np.abs(parts["reference"]).sum(0)), (tot, rows_sum)
    finally:
        b.close()
    for kind in sorted(worst):
        print("SUMMARY tied %s %s: largest e64 %.2e  e_gpu %.2e  e_gpu / y %.2f" % ((name, kind) + worst[kind]))


@pytest.mark.parametrize("name,size", [("d3k3", 9), ("d4k4", 5)], ids=["d3k3-last-of-eight", "d4k4-first-of-four"])
def test_a_models_sum_does_not_depend_on_its_neighbours(name, size):
    """k_tie shares nothing between threads: a model alone on a handle (another grid, other block and model indices) gives bitwise
    the rows it gives among its neighbours -- the 9-chain model that comes last of eight, the 5-chain model that comes first of four."""
    Y, st0, pri, lengths, models = TR.problem(name)
    (m,) = [i for i, c in enumerate(TR.CASES[name][3]) if c == size]
    rows = TR.rows_of(models)[m]
    among = _batch(Y, st0, pri, lengths, models)
    alone = _batch(Y[rows], {k: v[rows] for k, v in st0.items()}, pri, lengths[rows], np.zeros(size, dtype=np.int32))
    try:
        assert among.get_time_split() == alone.get_time_split() == 1        # (T = 12: no split to choose)
        among.iterate(2); alone.iterate(2)
        ea, eb = _everything(among), _everything(alone)
        for k in ea:
            assert ea[k][rows].shape == eb[k].shape and np.array_equal(ea[k][rows], eb[k], equal_nan=True), k
        assert np.all(np.isfinite(eb["X"])) and np.all(np.isfinite(eb["elbo"]))
    finally:
        among.close(); alone.close()


def test_more_models_than_the_grid_has_rows():
    """M = 65 537 models: 65 535 of one chain, then one of five chains (model 65 535) and one of two (65 536).  The grid of k_tie
    has min(M, 65 535) rows, so these two are summed in the second turn of `for (m = blockIdx.y; m < M; m += gridDim.y)`, the five
    chains through the unrolled body.  D = K = 1 and T = 2, the smallest pyvb_lds_create accepts; all lengths equal: tied, not
    ragged.

    Device memory, from the allocations of pyvb_lds_create at this shape (DP = KP = 16, W = 1, one statistics chunk), in doubles
    per replicate: gains 1424, stats 768, trash 512, sxx 256, X (two buffers) and the c_t cache 3 x 32, Sigma and Sigma_new 6,
    Y 2, and 40 in the parameter, log-determinant, moment, residual and bound rows: 3104 doubles = 24 832 bytes, and 32 bytes of
    flags and counters.  N = 65 542 replicates: 1.63e9 bytes (1.52 GiB), against 288 GB on the device.  Measured as the free device
    memory before and after the handle exists: 1.82e9 bytes, the granularity of some fifty separate allocations and the runtime's
    own buffers included.  Host side: the problem is drawn in 0.11 s, the handle created and filled in 0.17 s, an iteration 9 ms.

    The four models that are compared (0, 65 534 and the two tied ones) are the only ones the comparator runs."""
    from pyvb_amd.lds import LDSBatch
    T, Dm, Km = 2, 1, 1
    sizes = np.array([1] * 65535 + [5, 2])
    M, N = sizes.size, int(sizes.sum())
    models = np.repeat(np.arange(M, dtype=np.int32), sizes)
    Y, st0, pri = synth.make_problem(T, Dm, Km, N, seed=9210)
    pick = [0, 65534, 65535, 65536]
    ms = TR.build_models(Y, st0, pri, None, models, only=pick)
    mx = TR.build_models(ER.to_long(Y), ER.to_long(st0), ER.to_long(pri), None, models, only=pick)
    assert [len(r) for r, _, _ in ms] == [1, 1, 5, 2] and ms[2][0] == list(range(65535, 65540)) and ms[3][0] == [65540, 65541]
    f64, ext = TR.run(ms, pri, 1)[0], TR.run(mx, ER.to_long(pri), 1)[0]
    b = LDSBatch.from_problem(Y, st0, pri, models=models)
    try:
        assert (b.N, int(b.models[-1]) + 1) == (N, M) and np.all(b.lengths == T)
        b.iterate(1)
        got, parts = _readout(b, [rows for rows, _, _ in ms])
        worst = {}
        for i, (rows, chains, Ys) in enumerate(ms):
            tag = "M = 65537, model %d (%d chains) " % (pick[i], len(rows))
            _parity(got[i], f64[i], tag)
            _envelope(got[i], f64[i], ext[i], TR.accumulation_length(chains), tag, worst)
        g = _parameter_rows(b)
        for k in PARAM_ROWS:
            assert g[k].shape[0] == N and np.all(np.isfinite(g[k])), k
            for rows in (ms[2][0], ms[3][0]):
                assert np.all(g[k][rows] == g[k][rows[:1]]), k
        assert np.all(np.isfinite(g["X"])) and np.all(np.isfinite(parts["reference"])) and np.all(np.isfinite(parts["exact"]))
        first = np.concatenate([[True], np.diff(models) != 0])
        for mode in TR.BOUNDS:
            assert np.all(parts[mode][~first, 2:] == 0.0) and np.all(parts[mode][first, 2:] != 0.0)
        iters, conv, llb = b.model_convergence()
        assert iters.shape == conv.shape == llb.shape == (M,)
    finally:
        b.close()
    for kind in sorted(worst):
        print("SUMMARY tied M65537 %s: largest e64 %.2e  e_gpu %.2e  e_gpu / y %.2f" % ((kind,) + worst[kind]))


def test_mask_drops_a_model_of_nine_chains():
    """test_mask_drops_whole_models_only at these sizes: the 9-chain model of the D = K = 3 case switched off -- its rows stay
    bitwise what they were, every other model is bitwise what it is on a handle that was never masked."""
    Y, st0, pri, lengths, models = TR.problem("d3k3")
    rows = TR.rows_of(models)[-1]
    assert len(rows) == 9
    mask = np.ones(len(models), dtype=bool); mask[rows] = False
    b, twin = _batch(Y, st0, pri, lengths, models), _batch(Y, st0, pri, lengths, models)
    try:
        b.iterate(1); twin.iterate(1)
        before = _everything(b)
        b.set_active(mask)
        b.iterate(2); twin.iterate(2)
        after, ref = _everything(b), _everything(twin)
        _same(after, before, ~mask, "switched-off rows")
        _same(after, ref, mask, "active rows")
        assert not np.array_equal(ref["A_mean"][rows], before["A_mean"][rows])      # (the model would have moved)
        tot = b.elbo_total()
        assert np.all(np.abs(tot - after["elbo"][mask].sum(0)) <= mask.sum() * 2.0 ** -52 * np.abs(after["elbo"][mask]).sum(0))
    finally:
        b.close(); twin.close()
