"""GPU: Gamma precision parents for the columns of A and C (include/pyvb_hip.h: pyvb_lds_set_column_precisions, k_ard.hip) --
automatic relevance determination on the fused LDS path.

The comparator is tests/ard_ref.py, the composition of oracle functions that tests/test_ard_cpu.py pins against the reference's own
run of such graphs, and that run itself (tests/golden/ard_*.npz).  Parity is the suite's RTOL = 1e-8 (tests/test_gpu_parity.py,
tests/test_tied_gpu.py: max-norm for states and parameters, the parts of the bound to RTOL of the sum of their magnitudes, the total
to RTOL of itself; the exact parts to RTOL of max(|part|, 1)).  The envelope is the rule of DESIGN.md section 17, quantity by
quantity against the comparator's long-double run: e_gpu <= 16 max(e64, n 2^-52), n = max(D, K, T) -- after every iteration, except
that at D = K = 64 the long-double run stops after the first (an iteration takes it seconds); the second is held to parity only.

Shapes (tests/ard_ref.py: CASES): N = 3 replicates with different data, different initial qb and per-column priors, so that a
replicate or column stride of 0 shows; D = 3 / K = 4, ragged D = 33 / K = 17 and D = 17 / K = 33 (more than one block of 16
columns, no multiple of 4, K on either side of D), the full width D = K = 64; T between 4 and 7; hyperpriors on A only, on C only,
on both.  The tied handle has models of 1, 3, 2 chains with lengths that include 2 and 3; the time split needs T = 34.

"Bitwise" is justified as in tests/test_tied_gpu.py: two handles of the same shapes, lengths, models and time split run the same
instructions in the same order, and k_ard sums the rows of a column in ascending order into one accumulator.
"""
import glob
import os

import numpy as np
import pytest

import ard_ref as AR
import converge_ref as CR
import extended_ref as ER
from conftest import GOLDEN_DIR
from pyvb_amd import _capi, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-8
ARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ard_*.npz")))


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(a, b, what, rtol=RTOL):
    assert np.all(np.isfinite(a)), what + ": non-finite values"
    err = _rel(a, b)
    print("%-44s rel err %.3e" % (what, err))
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _compare_parts(got, want, what, exact=False):
    print("%s: parts %r want %r" % (what, got, want))
    assert np.all(np.isfinite(got)), what
    if exact:
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "%s\n%r\n%r" % (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= RTOL * np.abs(want).sum()), "%s\n%r\n%r" % (what, got, want)
        assert abs(got.sum() - want.sum()) <= RTOL * abs(want.sum()), what + ": total"


def _batch(Y, st0, pri, lengths=None, models=None):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=lengths, models=models)


def _snapshot(b):
    """The handle's counterpart of ard_ref.snapshot."""
    out = {k: v for k, v in b.get_state().items() if k in AR.QUANTITIES}
    out["Sigma"] = b.get_posterior_classes()[0]
    for w, (qa, qb) in b.column_precisions().items():
        out[w + "_alpha_b"], out[w + "_alpha_E"] = qb, qa / qb
    return out


def _bounds(b):
    """{mode: parts [N, 6]} of the handle's current state; the handle is left in reference mode."""
    out = {}
    for mode in ("exact", "reference"):
        b.set_bound_mode(mode)
        out[mode] = b.elbo()
    return out


def _compare_models(b, ms, tag):
    """Every row of the handle against its model of the comparator: states per chain, parameters and alpha per model."""
    g = _snapshot(b)
    for rows, m in ms:
        st = m.chains[0]
        for n, ch in zip(rows, m.chains):
            Tn = ch["X"].shape[1]
            t = "%sreplicate %d " % (tag, n)
            _close(g["X"][n, :Tn], ch["X"][0], t + "X")
            cls = [0, 1, 2] if Tn > 2 else [0, 2]
            _close(g["Sigma"][n][cls], ch["Sigma"][0][cls], t + "Sigma")
            _close(g["A_mean"][n], st["A_mean"][0], t + "A_mean")
            _close(g["C_mean"][n], st["C_mean"][0], t + "C_mean")
            _close(g["A_colvar"][n], np.einsum("ikk->ik", st["A_cov"][0]), t + "A_colvar")
            _close(g["C_colvar"][n], np.einsum("ikk->ik", st["C_cov"][0]), t + "C_colvar")
            for nm in ("Q_b", "R_b"):
                _close(g[nm][n], np.broadcast_to(st[nm][0], g[nm][n].shape), t + nm)
            for w, al in m.alpha.items():
                _close(g[w + "_alpha_b"][n], al["qb"], t + w + "_alpha_b")
                _close(g[w + "_alpha_E"][n], m.expectation(w), t + w + "_alpha_E")
    return g


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ARD, ids=lambda p: os.path.basename(p)[4:-4])
def test_reference_run_is_reproduced(path):
    """pyvb_lds_iterate on the fixture's graph (both matrices / C only, Gamma noise, a fully and a partly known column of A, one
    model of two chains): at every recorded iteration the states, the columns, qb of Q, R and the alpha nodes and the six parts are
    the reference's."""
    meta, Y, st0, pri, lengths, z = AR.load_ard(path)
    N = len(lengths)
    b = _batch(Y, st0, pri, np.asarray(lengths, dtype=np.int32) if N > 1 else None, np.zeros(N, dtype=np.int32) if N > 1 else None)
    assert sorted(b.column_precisions()) == sorted(meta["which"])
    for it in range(1, max(meta["iters"]) + 1):
        b.iterate(1)
        if it not in meta["iters"]:
            continue
        tag = "it%d_" % it
        g = _snapshot(b)
        parts = b.elbo()
        for n, Tn in enumerate(lengths):
            what = "%schain %d " % (tag, n)
            _close(g["X"][n, :Tn], z[tag + "X"][n, :Tn], what + "X")
            cls = [0, 1, 2] if Tn > 2 else [0, 2]
            _close(g["Sigma"][n][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
            for nm in ("A_mean", "C_mean", "A_colvar", "C_colvar"):
                _close(g[nm][n], z[tag + nm], what + nm)
            for nm in ("Q_b", "R_b"):
                _close(g[nm][n], np.broadcast_to(z[tag + nm], g[nm][n].shape), what + nm)
            for w in meta["which"]:
                _close(g[w + "_alpha_b"][n], z[tag + w + "_alpha_b"], what + w + "_alpha_b")
                _close(g[w + "_alpha_E"][n], z[tag + w + "_alpha_a"] / z[tag + w + "_alpha_b"], what + w + "_alpha_E")
        _compare_parts(parts.sum(0), z[tag + "elbo_parts"], tag + "the model")
        assert np.all(parts[1:, 2:] == 0.0)
    b.close()


# ---- 2. parity with the comparator and the accuracy envelope, after every iteration ----------------------------------------
@pytest.mark.parametrize("name", sorted(AR.CASES))
def test_parity_and_envelope(name):
    T, D, K = AR.CASES[name][:3]
    n = max(T, D, K)
    Y, st0, pri = AR.problem(name)
    f64, ext = AR.trace(name), AR.trace(name, extended=True)
    b = _batch(Y, st0, pri)
    assert sorted(b.column_precisions()) == sorted(AR.CASES[name][3])
    for it in range(AR.ITERS):
        b.iterate(1)
        g, parts = _snapshot(b), _bounds(b)
        s64, p64 = f64[it]
        assert sorted(g) == sorted(s64)
        for k in sorted(g):
            _close(g[k], s64[k], "iteration %d %s" % (it + 1, k))
        for mode in AR.BOUNDS:
            for r in range(AR.N_CASE):
                _compare_parts(parts[mode][r], p64[mode][r], "iteration %d %s bound, replicate %d" % (it + 1, mode, r), mode == "exact")
        if it >= len(ext):          # D = K = 64: the long-double run has one iteration (ard_ref.CASES); the second is held to parity above
            assert name == "d64k64_AC" and it == 1
            continue
        sx, px = ext[it]
        for k in sorted(g):
            e64, e_gpu = ER.rel(s64[k], sx[k]), ER.rel(g[k], sx[k])
            y = ER.yardstick(e64, n)
            print("iteration %d %-10s e64 %.2e  e_gpu %.2e  (%.2f of the bound)" % (it + 1, k, e64, e_gpu, e_gpu / (ER.FACTOR * y)))
            assert e64 <= ER.CAP
            assert e_gpu <= ER.FACTOR * y, (name, it, k, e64, e_gpu)
        for mode in AR.BOUNDS:
            e64 = ER.bound_errors(p64[mode], px[mode])[0]
            assert e64.max() <= ER.CAP
            for r, p, e6, eg, ratio, own in ER.compare_bound(parts[mode], px[mode], e64, n):
                print("iteration %d %-9s replicate %d %s e64 %.2e  e_gpu %.2e  (%.2f y)" % (it + 1, mode, r, ER.LDS_PARTS[p], e6, eg, ratio))
                assert ratio <= ER.FACTOR, (name, it, mode, r, p, e6, eg)
    b.close()


# ---- 3. stage-wise calls and partial column updates --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d3k4_AC", "d33k17_A", "d17k33_C"])
def test_stagewise_calls_are_iterate(name):
    Y, st0, pri = AR.problem(name)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    for it in range(2):
        a.sweep("forward"); a.sweep("backward")
        a.update_A(); a.update_C(); a.update_Q(); a.update_R()
        for w in (0, 1):
            if "AC"[w] in AR.CASES[name][3]:
                a.update_column_precisions(w)
        pa = a.elbo()
        b.iterate(1)
        pb = b.elbo()
        ga, gb = _snapshot(a), _snapshot(b)
        for k in ga:
            _close(ga[k], gb[k], "iteration %d %s" % (it + 1, k))
        for r in range(AR.N_CASE):
            _compare_parts(pa[r], pb[r], "iteration %d replicate %d" % (it + 1, r))
        assert np.allclose(b.elbo_history(1)[0], pb.sum(0), rtol=1e-12)
    a.close(); b.close()


def test_update_column_precisions_none_updates_every_matrix_that_has_them():
    Y, st0, pri = AR.problem("d3k4_AC")
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    for h in (a, b):
        h.sweep("forward"); h.sweep("backward"); h.update_A(); h.update_C()
    a.update_column_precisions()
    b.update_column_precisions("A"); b.update_column_precisions("C")
    ca, cb = a.column_precisions(), b.column_precisions()
    for w in "AC":
        assert np.array_equal(ca[w][1], cb[w][1]) and not np.array_equal(ca[w][1], st0[w + "_alpha_b"])
    a.close(); b.close()


def test_partial_column_update_then_alpha():
    """update_columns over a part of the columns that starts and ends inside a block of 16, then the alpha update: it reads every
    column as stored, the renewed ones and the others."""
    name = "d33k17_A"
    Y, st0, pri = AR.problem(name)
    ms = AR.models(Y, st0, pri)
    b = _batch(Y, st0, pri)
    b.sweep("forward"); b.sweep("backward")
    b.update_columns("A", 5, 21)
    b.update_column_precisions("A")
    b.update_columns("A", 0, 33)            # under the new precisions
    b.update_C()
    for _, m in ms:
        m.sweep("forward"); m.sweep("backward")
        m.update_A((5, 21))
        m.update_alpha("A")
        m.update_A((0, 33))
        m.update_C()
    _compare_models(b, ms, "")
    b.close()


# ---- 4. composition with the rest of the handle ------------------------------------------------------------------------------
def test_tied_models():
    """Models of 1, 3, 2 chains, lengths that include 2 and 3: the alpha rows are bitwise equal within a model (and come from its
    first row's qb), each model's rows sum to the comparator's parts in both modes, the alpha terms sit on the first row."""
    Y, st0, pri, ln, md = AR.tied_problem()
    ms = AR.models(Y, st0, pri, ln, md)
    b = _batch(Y, st0, pri, ln, md)
    c0 = b.column_precisions()
    for rows, m in ms:
        for w in "AC":
            assert np.array_equal(c0[w][1][rows], np.repeat(st0[w + "_alpha_b"][rows[:1]], len(rows), axis=0))
    for it in range(2):
        b.iterate(1)
        for _, m in ms:
            m.iterate()
        g = _compare_models(b, ms, "iteration %d " % (it + 1))
        parts = _bounds(b)
        for i, (rows, m) in enumerate(ms):
            for k in ("A_alpha_b", "C_alpha_b", "A_mean", "C_colvar"):
                for n in rows[1:]:
                    assert np.array_equal(g[k][n], g[k][rows[0]]), (k, rows[0], n)
            for mode in AR.BOUNDS:
                _compare_parts(parts[mode][rows].sum(0), m.elbo_parts(mode), "iteration %d model %d %s" % (it + 1, i, mode), mode == "exact")
                assert np.all(parts[mode][rows[1:], 2:] == 0.0)
    b.close()


def _series(Y, st0, lengths):
    return [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(lengths)]


def _everything_ard(b):
    out = _everything(b)
    for w, (qa, qb) in b.column_precisions().items():
        out[w + "_alpha_a"], out[w + "_alpha_b"] = qa, qb
    return out


def test_from_series_and_from_trials_pick_the_hyperpriors_up():
    """The constructors for real series: the priors from pri, qb from every series' own state (a model takes its first trial's).
    Bitwise the from_problem handles of the same lengths and models, before and after two iterations."""
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, ln, md = AR.tied_problem()
    series = _series(Y, st0, ln)
    trials = [[series[n] for n in np.nonzero(md == m)[0]] for m in range(int(md.max()) + 1)]
    for made, same in ((LDSBatch.from_series(series, pri), _batch(Y, st0, pri, ln)),
                       (LDSBatch.from_trials(trials, pri), _batch(Y, st0, pri, ln, md))):
        assert sorted(made.column_precisions()) == ["A", "C"]
        assert list(made.lengths) == list(ln) and list(made.models) == list(same.models)
        for it in range(2):         # as constructed (no bound yet: the X_t have no covariances before the first sweep), then iterated
            ea, eb = (_snapshot(made), _snapshot(same)) if it == 0 else (_everything_ard(made), _everything_ard(same))
            assert sorted(ea) == sorted(eb) and "C_alpha_b" in ea
            for k in ea:
                assert np.array_equal(ea[k], eb[k], equal_nan=True), (it, k)
            made.iterate(2); same.iterate(2)
        made.close(); same.close()
    # the qb a plain handle starts from is each series' own
    b = LDSBatch.from_series(series, pri)
    assert np.array_equal(b.column_precisions()["A"][1], st0["A_alpha_b"])
    b.close()


def test_a_switched_off_replicate_keeps_its_qb():
    Y, st0, pri = AR.problem("d3k4_AC")
    ms = AR.models(Y, st0, pri)
    b = _batch(Y, st0, pri)
    b.set_active([True, False, True])
    b.iterate(2)
    b.update_column_precisions()        # the explicit entry honours the mask too
    c = b.column_precisions()
    for w in "AC":
        assert np.array_equal(c[w][1][1], st0[w + "_alpha_b"][1]), w + ": qb of the switched-off row changed"
    for i in (0, 2):
        m = ms[i][1]
        m.iterate(); m.iterate(); m.update_alpha()
        for w in "AC":
            _close(c[w][1][i], m.alpha[w]["qb"], "replicate %d %s qb" % (i, w))
    b.close()


def _learn(m, bound, tol, max_iters, what):
    return CR.guarded(CR.learn(lambda: m.iterate(bound), tol, max_iters), tol, what)


def test_iterate_until_stops_where_the_comparator_does():
    """Per-replicate convergence runs the alpha updates (iterate_updates): every replicate stops in the iteration in which
    Network.learn's test stops the comparator's run of it alone -- the deltas it meets pass converge_ref's guard."""
    tol, max_iters = 1.0, 20
    Y, st0, pri = AR.problem("d3k4_AC")
    ms = AR.models(Y, st0, pri)
    runs = [_learn(m, "reference", tol, max_iters, "replicate %d" % i) for i, (_, m) in enumerate(ms)]
    assert len({r[0] for r in runs}) == 3 and all(r[1] for r in runs), [r[:2] for r in runs]        # three different stops
    b = _batch(Y, st0, pri)
    n = b.iterate_until(max_iters, tol, check_every=1)
    iters, conv, llb = b.convergence()
    print("stops", iters, [r[0] for r in runs])
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * np.abs(r[2][-1]).sum()
    _compare_models(b, ms, "at the stop: ")
    b.close()


def test_iterate_until_model_stops_where_the_comparator_does():
    tol, max_iters = 0.5, 18
    Y, st0, pri, ln, md = AR.tied_problem()
    ms = AR.models(Y, st0, pri, ln, md)
    runs = [_learn(m, "exact", tol, max_iters, "model %d" % i) for i, (_, m) in enumerate(ms)]
    assert len({r[0] for r in runs}) == 3 and all(r[1] for r in runs), [r[:2] for r in runs]
    b = _batch(Y, st0, pri, ln, md)
    b.set_bound_mode("exact")
    n = b.iterate_until_model(max_iters, tol, check_every=1)
    iters, conv, llb = b.model_convergence()
    print("stops", iters, [r[0] for r in runs])
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * max(np.abs(r[2][-1]).sum(), 1.0)
    _compare_models(b, ms, "at the stop: ")
    b.close()


def test_a_time_split():
    """W = 2 wavefronts per replicate in the sweeps (T = 34 is the shortest chain that allows it)."""
    T, D, K = 34, 3, 4
    Y, st0, pri = synth.make_problem(T, D, K, 3, seed=21600)
    AR.add_hyperpriors(st0, pri, "AC", 21601)
    ms = AR.models(Y, st0, pri)
    b = _batch(Y, st0, pri)
    b.set_time_split(2)
    assert b.get_time_split() == 2
    for it in range(2):
        b.iterate(1)
        for _, m in ms:
            m.iterate()
    _compare_models(b, ms, "W = 2: ")
    parts = b.elbo()
    for r, (_, m) in enumerate(ms):
        _compare_parts(parts[r], m.elbo_parts(), "W = 2, replicate %d" % r)
    b.close()


# ---- 5. behaviour and refusals ----------------------------------------------------------------------------------------------
def _everything(b):
    out = dict(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["qld_A"], out["qld_C"] = b.get_column_qld()
    for k, v in b.get_logdets().items():
        out["lnd_" + k] = v
    out["elbo"] = b.elbo()
    return out


def test_set_priors_returns_the_columns_to_constant_parents():
    """set_priors after set_column_precisions: bitwise the handle that never had hyperpriors, in both bound modes."""
    Y, st0, pri = AR.problem("d33k17_A")
    plain_st0, _ = AR.split_alpha(st0)
    plain_pri = {k: v for k, v in pri.items() if "_alpha_" not in k}
    a, b = _batch(Y, plain_st0, plain_pri), _batch(Y, st0, pri)
    assert a.column_precisions() == {} and sorted(b.column_precisions()) == ["A"]
    b.set_priors(plain_pri)
    assert b.column_precisions() == {}
    for mode in ("reference", "exact"):
        for h in (a, b):
            h.set_bound_mode(mode)
            h.iterate(2)
        ea, eb = _everything(a), _everything(b)
        for k in ea:
            assert np.array_equal(ea[k], eb[k], equal_nan=True), (mode, k)
        assert np.array_equal(a.elbo_history(), b.elbo_history())
    a.close(); b.close()


def _launches(b):
    return sum(v[1] for v in b.kernel_times().values())


def test_refusals_and_argument_errors_come_before_any_launch():
    from pyvb_amd.lds import LDSBatch
    one = np.ones(4)
    # Wishart noise and the 128-wide class: PYVB_E_UNSUPPORTED
    for D, K, noise, word in ((4, 5, "wishart", "Wishart"), (65, 5, "diagonal_gamma", "64"), (4, 65, "gamma", "64")):
        b = LDSBatch(2, 6, D, K, noise)
        b.timing(True)
        v = np.ones(D)
        with pytest.raises(_capi.PyvbHipError) as e:
            b.set_column_precisions(A=(v, v, np.ones((2, D))))
        assert e.value.code == _capi.E_UNSUPPORTED and word in str(e.value) and "Gamma precision parents" in str(e.value), str(e.value)
        assert _launches(b) == 0
        b.close()
    b = LDSBatch(3, 6, 4, 5)
    b.timing(True)
    h, lib, p = b._h, _capi.lib, _capi.dptr
    qb = np.ones((3, 4))
    for which in (-1, 2):
        assert lib.pyvb_lds_set_column_precisions(h, which, p(one), p(one), p(qb)) == _capi.E_ARG
        assert b"which must be 0 (A) or 1 (C)" in lib.pyvb_last_error()
        assert lib.pyvb_lds_get_column_precisions(h, which, None, None) == _capi.E_ARG
        assert lib.pyvb_lds_update_column_precisions(h, which) == _capi.E_ARG
    assert lib.pyvb_lds_set_column_precisions(h, 0, None, p(one), p(qb)) == _capi.E_ARG
    for bad in (0.0, -1.0, np.nan, np.inf):
        v = one.copy(); v[2] = bad
        for args in ((v, one), (one, v)):
            assert lib.pyvb_lds_set_column_precisions(h, 1, p(args[0]), p(args[1]), p(qb)) == _capi.E_ARG
            msg = lib.pyvb_last_error().decode()
            assert "column 2 of C" in msg and ("a0" if args[0] is v else "b0") in msg, msg
        q = qb.copy(); q[1, 3] = bad
        assert lib.pyvb_lds_set_column_precisions(h, 0, p(one), p(one), p(q)) == _capi.E_ARG
        msg = lib.pyvb_last_error().decode()
        assert "replicate 1, column 3 of A" in msg, msg
    # no matrix has hyperpriors: get and update are argument errors
    for which, nm in ((0, "A"), (1, "C")):
        assert lib.pyvb_lds_get_column_precisions(h, which, p(qb), p(qb.copy())) == _capi.E_ARG
        assert ("columns of %s have Constant precision parents" % nm).encode() in lib.pyvb_last_error()
        assert lib.pyvb_lds_update_column_precisions(h, which) == _capi.E_ARG
    assert b.column_precisions() == {}
    assert _launches(b) == 0
    # hyperpriors on C only: A still refuses, C answers
    b.set_column_precisions(C=(1e-3, 1e-3, 2.0 * qb))
    assert lib.pyvb_lds_update_column_precisions(h, 0) == _capi.E_ARG
    qa, got = b.column_precisions()["C"]
    assert np.array_equal(got, 2.0 * qb) and np.array_equal(qa, np.full((3, 4), 1e-3 + 2.5))
    b.close()
