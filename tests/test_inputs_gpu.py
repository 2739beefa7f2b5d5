"""GPU: LDS handles with a known input, X_t = Gaussian(q, A X_{t-1} + B u_t, Q) (include/pyvb_hip.h: pyvb_lds_create_inputs,
k_inputs.hip) on the fused path.

The comparator is tests/inputs_ref.py, the composition of oracle functions that tests/test_inputs_cpu.py pins against the reference's
own run of such graphs, and that run itself (tests/golden/inputs_*.npz).  The yardstick is that of tests/extended_ref.py, unchanged:
against the comparator's long-double run, e_gpu <= 16 max(e64, n 2^-52), n = max(D, K, T), for every quantity after the stage that
produces it and for the bound part by part in both modes; parity with the float64 comparator is the suite's RTOL = 1e-8.

Shapes (tests/inputs_ref.py: CASES): (T, D, K, P) = (19, 6, 4, 2) the smallest, one tile everywhere; (33, 5, 15, 1) where K + 2 P = 17
crosses a tile and B has a single column; (77, 16, 16, 8) with K + 2 P = 32; (40, 64, 40, 12) with K + 2 P = 64 and D = 64, no idle
lane or tile (one iteration in long double); (700, 8, 8, 3) with four wavefronts per chain, whose segments start from their warm-up;
chain lengths (2, 3, 19, 60, 77) at (16, 10, 3): the shortest chain, and the zeroed u_{t+1} at each chain's own end.
"""
import glob
import os

import numpy as np
import pytest

import converge_ref as CR
import extended_ref as ER
import inputs_ref as IR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi, synth

pytestmark = pytest.mark.gpu

RTOL = 1e-8
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "inputs_*.npz")))


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(a, b, what, rtol=RTOL):
    assert np.all(np.isfinite(a)), what + ": non-finite values"
    err = _rel(a, b)
    print("%-52s rel err %.3e" % (what, err))
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _compare_parts(got, want, what, exact=False):
    print("%s: parts %r want %r" % (what, got, want))
    assert np.all(np.isfinite(got)), what
    if exact:
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "%s\n%r\n%r" % (what, got, want)
    else:
        assert np.all(np.abs(got - want) <= RTOL * np.abs(want).sum()), "%s\n%r\n%r" % (what, got, want)
        assert abs(got.sum() - want.sum()) <= RTOL * abs(want.sum()), what + ": total"


def _batch(Y, U, st0, pri, lengths=None):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=lengths, U=U)


def _snapshot(b):
    """The handle's counterpart of inputs_ref.snapshot."""
    out = {k: v for k, v in b.get_state().items() if k in IR.QUANTITIES}
    out["Sigma"] = b.get_posterior_classes()[0]
    return out


def _bound(b, mode):
    b.set_bound_mode(mode)
    out = b.elbo()
    b.set_bound_mode("reference")
    return out


def _do(b, stage):
    if stage in ("forward", "backward"):
        b.sweep(stage)
    else:
        getattr(b, "update_" + stage)()


def _case_handle(name):
    Y, U, st0, pri, ln = IR.problem(name)
    b = _batch(Y, U, st0, pri, ln)
    if IR.CASES[name][5]:
        b.set_time_split(IR.CASES[name][5])
        assert b.get_time_split() == IR.CASES[name][5]
    return b


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[7:-4])
def test_reference_run_is_reproduced(path):
    """pyvb_lds_iterate on the fixture's graphs: after the forward sweep alone, and at every recorded iteration, the states, the
    three matrices, qb of Q and R and the six parts are the reference's."""
    meta, Y, U, st0, pri, lengths, z = IR.load_fixture(path)
    N = len(lengths)
    b = _batch(Y, U, st0, pri, np.asarray(lengths, dtype=np.int32) if N > 1 else None)
    assert np.array_equal(b.get_inputs(), U)
    for it in range(1, max(meta["iters"]) + 1):
        if it == 1:
            b.sweep("forward")
            X = b.get_state(("X",))["X"]
            for n, Tn in enumerate(lengths):
                _close(X[n, :Tn], z["it1_fwd_X"][n, :Tn], "forward sweep alone, chain %d" % n)
            for stage in ("backward", "A", "B", "C", "Q", "R"):
                _do(b, stage)
        else:
            b.iterate(1)
        if it not in meta["iters"]:
            continue
        tag = "it%d_" % it
        g, parts = _snapshot(b), b.elbo()
        for n, Tn in enumerate(lengths):
            what = "%schain %d " % (tag, n)
            _close(g["X"][n, :Tn], z[tag + "X"][n, :Tn], what + "X")
            cls = [0, 1, 2] if Tn > 2 else [0, 2]
            _close(g["Sigma"][n][cls], z[tag + "Sigma"][n][cls], what + "Sigma")
            for nm in ("A_mean", "B_mean", "C_mean", "A_colvar", "B_colvar", "C_colvar"):
                _close(g[nm][n], z[tag + nm][n], what + nm)
            for nm in ("Q_b", "R_b"):
                _close(g[nm][n], np.broadcast_to(z[tag + nm][n], g[nm][n].shape), what + nm)
            _compare_parts(parts[n], z[tag + "elbo_parts"][n], what + "bound")
    b.close()


# ---- 2. parity with the comparator and the accuracy envelope, after every stage ---------------------------------------------
@pytest.mark.parametrize("name", sorted(IR.CASES))
def test_parity_and_envelope(name):
    T, D, K, P = IR.CASES[name][:4]
    n = max(T, D, K)
    f64, ext = IR.trace(name), IR.trace(name, extended=True)
    b = _case_handle(name)
    got = IR.run_stages(lambda stage: _do(b, stage), lambda: _snapshot(b), lambda mode: _bound(b, mode), IR.ITERS)
    b.close()
    assert [k for k, _ in got] == [k for k, _ in f64]
    failures = []
    for i, ((key, g), (_, v64)) in enumerate(zip(got, f64)):
        it, stage, q = key
        what = "iteration %d %s %s" % (it + 1, stage, q)
        if stage == "bound":
            for r in range(g.shape[0]):
                _compare_parts(g[r], v64[r], "%s replicate %d" % (what, r), q == "exact")
        else:
            _close(g, v64, what)
        if i >= len(ext):       # D = 64: the long-double run has one iteration (inputs_ref.CASES); the second is held to parity above
            assert name == "t40_d64k40p12" and it == 1
            continue
        vx = ext[i][1]
        if stage == "bound":
            e64 = ER.bound_errors(v64, vx)[0]
            assert e64.max() <= ER.CAP
            for r, p, e6, eg, ratio, own in ER.compare_bound(g, vx, e64, n):
                print("%s replicate %d %s e64 %.2e  e_gpu %.2e  (%.2f y)" % (what, r, ER.LDS_PARTS[p], e6, eg, ratio))
                if ratio > ER.FACTOR:
                    failures.append((what, r, ER.LDS_PARTS[p], e6, eg, ratio))
        else:
            e64, e_gpu = ER.rel(v64, vx), ER.rel(g, vx)
            y = ER.yardstick(e64, n)
            print("%-40s e64 %.2e  e_gpu %.2e  (%.2f of the bound)" % (what, e64, e_gpu, e_gpu / (ER.FACTOR * y)))
            assert e64 <= ER.CAP
            if e_gpu > ER.FACTOR * y:
                failures.append((what, e64, e_gpu, e_gpu / y))
    assert not failures, failures


# ---- 3. the entry points agree with one another -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t19_d6k4p2", "lengths_d16k10p3"])
def test_stagewise_calls_are_iterate(name):
    a, b = _case_handle(name), _case_handle(name)
    N = IR.n_case(name)
    for it in range(2):
        for stage, _ in IR.STAGES:
            _do(a, stage)
        pa = a.elbo()
        b.iterate(1)
        pb = b.elbo()
        ga, gb = _snapshot(a), _snapshot(b)
        for k in ga:
            _close(ga[k], gb[k], "iteration %d %s" % (it + 1, k), rtol=1e-12)
        for r in range(N):
            _compare_parts(pa[r], pb[r], "iteration %d replicate %d" % (it + 1, r))
        assert np.allclose(b.elbo_history(1)[0], pb.sum(0), rtol=1e-12)
    a.close(); b.close()


@pytest.mark.parametrize("name", ["t19_d6k4p2", "t33_d5k15p1"])
def test_single_node_updates(name):
    """update_x at t = 0, 1, T-2, T-1 after a parameter update: both boundary nodes and the interior nodes next to them, each
    against the comparator's update of the same node."""
    Y, U, st0, pri, ln = IR.problem(name)
    T = Y.shape[1]
    (_, m), = IR.models(Y, U, st0, pri, ln)
    b = _case_handle(name)
    for h in (b, m):
        for stage, _ in IR.STAGES:
            (_do if h is b else IR.do_stage)(h, stage)
    for t in (0, 1, T - 2, T - 1, 1, 0):
        b.update_x(t)
        m.update_x(t)
        _close(b.get_state(("X",))["X"][:, t], m.st["X"][:, t], "X_%d" % t, rtol=1e-11)
    _close(b.get_state(("X",))["X"], m.st["X"], "all states")
    b.close()


def test_without_an_input_the_handle_is_a_plain_one():
    """U = 0: X, A, C, Q, R agree with a plain handle on the same data within 16 n 2^-52 after an iteration (the two run different
    instantiations of the sweeps and of k_stats: K + 2 P = 17 outputs against 15), and B has gone to its prior."""
    from pyvb_amd.lds import LDSBatch
    T, D, K, P = IR.CASES["t33_d5k15p1"][:4]
    Y, U, st0, pri, _ = IR.problem("t33_d5k15p1")
    a = _batch(Y, np.zeros_like(U), st0, pri)
    p = LDSBatch.from_problem(Y, IR.split_inputs(st0)[0], pri)
    a.iterate(1); p.iterate(1)
    ga, gp = a.get_state(), p.get_state()
    tol = ER.FACTOR * max(T, D, K) * ER.U64
    for k in ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b"):
        _close(ga[k], gp[k], k, rtol=tol)
    assert np.abs(ga["B_mean"]).max() == 0.0
    _close(ga["B_colvar"], np.broadcast_to(1.0 / pri["B_prior_prec"], ga["B_colvar"].shape), "B_colvar", rtol=1e-15)
    a.close(); p.close()


def test_a_switched_off_replicate_keeps_its_B():
    name = "t19_d6k4p2"
    Y, U, st0, pri, ln = IR.problem(name)
    b = _case_handle(name)
    b.set_active([True, False])
    b.iterate(2)
    b.update_B()            # the explicit entry honours the mask too
    g = b.get_input_state()
    assert np.array_equal(g["B_mean"][1], st0["B_mean"][1]) and np.array_equal(g["B_colvar"][1], st0["B_colvar"][1])
    assert np.all(np.isnan(g["qld_B"][1])) and np.all(np.isfinite(g["qld_B"][0]))
    m = IR.Model(Y[:1], U[:1], {k: v[:1] for k, v in st0.items()}, pri)
    m.iterate(); m.iterate(); m.update_B()
    _close(g["B_mean"][0], m.st["B_mean"][0], "B_mean of the running replicate")
    _close(g["qld_B"][0], m.st["qld_B"][0], "qld_B of the running replicate")
    b.close()


def test_iterate_until_stops_where_the_comparator_does():
    """Per-replicate convergence on a handle with inputs: every replicate stops in the iteration in which Network.learn's test
    stops the comparator's run of it alone -- the deltas it meets pass converge_ref's guard."""
    tol, max_iters = 20.0, 30       # the four stop after 2, 13, 4 and 10 iterations
    Y, U, st0, pri = synth.make_input_problem(30, 4, 5, 2, 4, seed=31500)
    ms = [IR.Model(Y[n:n + 1], U[n:n + 1], {k: v[n:n + 1] for k, v in st0.items()}, pri) for n in range(4)]
    runs = [CR.guarded(CR.learn(lambda m=m: m.iterate()[0], tol, max_iters), tol, "replicate %d" % i) for i, m in enumerate(ms)]
    assert len({r[0] for r in runs}) == 4 and all(r[1] for r in runs), [r[:2] for r in runs]
    b = _batch(Y, U, st0, pri)
    n = b.iterate_until(max_iters, tol, check_every=1)
    iters, conv, llb = b.convergence()
    print("stops", iters, [r[0] for r in runs])
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * np.abs(r[2][-1]).sum()
    g = _snapshot(b)
    for i, m in enumerate(ms):
        for k in ("X", "A_mean", "B_mean", "C_mean"):
            _close(g[k][i], m.st[k][0], "at the stop: replicate %d %s" % (i, k))
    b.close()


# ---- 4. handles without inputs are what they were ---------------------------------------------------------------------------
def test_a_plain_handle_launches_what_it_did():
    """The launches per kernel of an iteration on a handle without inputs, as the commit before inputs counted them
    (pyvb_lds_timing_get): one k_prep, one sweep each way, one k_stats, k_moments and k_cols, one k_elbo -- and none of k_inputs.hip."""
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri = synth.make_problem(19, 6, 4, 2, seed=31400)
    b = LDSBatch.from_problem(Y, st0, pri)
    b.iterate(1)
    b.sync()
    b.timing(True)
    b.iterate(3)
    b.sync()
    kt = {k: v[1] for k, v in b.kernel_times().items()}
    assert kt == {"prep": 3, "sweep_fwd": 3, "sweep_bwd": 3, "stats": 3, "params": 6, "elbo": 3, "step": 0, "gy": 0, "inputs": 0}, kt
    b.close()


# ---- 5. refusals and argument errors ----------------------------------------------------------------------------------------
def _launches(b):
    return sum(v[1] for v in b.kernel_times().values())


def test_refusals_and_argument_errors_come_before_any_launch():
    from pyvb_amd.lds import LDSBatch
    N, T, D, K, P = 2, 6, 3, 4, 2
    b = LDSBatch(N, T, D, K, inputs=P)
    b.timing(True)
    h, lib, p = b._h, _capi.lib, _capi.dptr
    # outputs that hold NaN, known entries, precision parents: PYVB_E_UNSUPPORTED, each naming the cause
    Y = np.zeros((N, T, K)); Y[1, 2, 3] = np.nan
    for call, word in ((lambda: b.set_observations(Y), "NaN"),
                       (lambda: b.set_column_observations(np.where(np.eye(D) > 0, 0.5, np.nan), None), "known entries"),
                       (lambda: b.set_column_precisions(A=(1e-3, 1e-3, np.ones((N, D)))), "Gamma precision parents"),
                       (lambda: b.set_entry_precisions(C=(1e-3, 1e-3, np.ones((N, D, K)))), "DiagonalGamma precision parents")):
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_UNSUPPORTED and word in str(e.value) and "inputs" in str(e.value), str(e.value)
    # U: NULL, non-finite
    assert lib.pyvb_lds_set_inputs(h, None) == _capi.E_ARG
    for bad in (np.nan, np.inf):
        U = np.zeros((N, T, P)); U[1, 4, 1] = bad
        assert lib.pyvb_lds_set_inputs(h, p(U)) == _capi.E_ARG
        assert "replicate 1, row 4, channel 1" in lib.pyvb_last_error().decode()
    pp = np.ones((P, D)); pp[1, 2] = 0.0
    assert lib.pyvb_lds_set_input_priors(h, p(np.zeros((D, P))), p(pp)) == _capi.E_ARG
    # an update before the inputs are there
    b.set_priors(dict(synth.default_priors(D, K), B_prior_mean=np.zeros((D, P)), B_prior_prec=np.ones((P, D))))
    b.set_observations(np.zeros((N, T, K)))
    assert lib.pyvb_lds_sweep(h, 0) == _capi.E_ARG and b"pyvb_lds_set_inputs" in lib.pyvb_last_error()
    assert _launches(b) == 0
    b.close()
    # the entries of a handle with inputs on one without
    b = LDSBatch(N, T, D, K)
    v = np.zeros(N * T * P + N * D * P)
    for rc in (lib.pyvb_lds_set_inputs(b._h, p(v)), lib.pyvb_lds_get_inputs(b._h, p(v)), lib.pyvb_lds_set_input_priors(b._h, p(v), p(v)),
               lib.pyvb_lds_set_input_state(b._h, p(v), p(v)), lib.pyvb_lds_get_input_state(b._h, p(v), None, None, None),
               lib.pyvb_lds_update_B(b._h)):
        assert rc == _capi.E_ARG and b"created without inputs" in lib.pyvb_last_error()
    b.close()
