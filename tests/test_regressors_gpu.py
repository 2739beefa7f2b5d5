"""GPU: LDS handles with known regressors in the output equation, Y_t = Gaussian(K, C X_t + E v_t, R) (include/pyvb_hip.h:
pyvb_lds_create_regressors, k_regressors.hip) on the fused path.

The comparator is tests/regressors_ref.py, the composition of oracle functions that tests/test_regressors_cpu.py pins against the
reference's own run of such graphs, and that run itself (tests/golden/regressors_*.npz).  The yardstick is that of
tests/extended_ref.py, unchanged: against the comparator's long-double run, e_gpu <= 16 max(e64, n 2^-52), n = max(D, K, T), for every
quantity after the stage that produces it and for the bound part by part in both modes; parity with the float64 comparator is the
suite's RTOL = 1e-8.

Shapes (tests/regressors_ref.py: CASES): (T, D, K, P, Pv) = (19, 6, 4, 0, 2) without inputs, one tile; (19, 6, 4, 2, 1) with both
kinds of input; (33, 5, 14, 0, 3) where Kt = K + 2 P + Pv = 17 crosses a tile; (77, 16, 16, 4, 8) with Kt = 32; (40, 64, 40, 6, 12)
with Kt = 64 and D = 64 (one iteration in long double); (12, 3, 1, 0, 63) the widest E; (700, 8, 8, 2, 3) with four wavefronts per
chain; chain lengths (2, 3, 19, 60, 77) at (16, 10, 2, 3): the v channel in a chain's own last row and, with regressors that are not
zero there, in no padding row.
"""
import glob
import os

import numpy as np
import pytest

import converge_ref as CR
import extended_ref as ER
import regressors_ref as RR
from conftest import GOLDEN_DIR
from pyvb_amd import _capi, synth
from test_inputs_gpu import RTOL, _bound, _close, _compare_parts, _do, _launches

pytestmark = pytest.mark.gpu

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "regressors_*.npz")))


def _batch(Y, U, V, st0, pri, lengths=None):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=lengths, U=U, V=V)


def _snapshot(b):
    """The handle's counterpart of regressors_ref.snapshot."""
    out = {k: v for k, v in b.get_state().items() if k in RR.quantities(b.P)}
    out["Sigma"] = b.get_posterior_classes()[0]
    return out


def _case_handle(name):
    Y, U, V, st0, pri, ln = RR.problem(name)
    b = _batch(Y, U, V, st0, pri, ln)
    if RR.CASES[name][6]:
        b.set_time_split(RR.CASES[name][6])
        assert b.get_time_split() == RR.CASES[name][6]
    return b


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[11:-4])
def test_reference_run_is_reproduced(path):
    """pyvb_lds_iterate on the fixture's graphs: after the forward sweep alone, and at every recorded iteration, the states, the
    matrices, qb of Q and R and the six parts are the reference's."""
    meta, Y, U, V, st0, pri, lengths, z = RR.load_fixture(path)
    N, P = len(lengths), meta["P"]
    b = _batch(Y, U, V, st0, pri, np.asarray(lengths, dtype=np.int32) if N > 1 else None)
    assert np.array_equal(b.get_regressors(), V)
    for it in range(1, max(meta["iters"]) + 1):
        if it == 1:
            b.sweep("forward")
            X = b.get_state(("X",))["X"]
            for n, Tn in enumerate(lengths):
                _close(X[n, :Tn], z["it1_fwd_X"][n, :Tn], "forward sweep alone, chain %d" % n)
            for stage, _ in RR.stages(P)[1:]:
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
            for nm in [w + s for w in ("ABCE" if P else "ACE") for s in ("_mean", "_colvar")]:
                _close(g[nm][n], z[tag + nm][n], what + nm)
            for nm in ("Q_b", "R_b"):
                _close(g[nm][n], np.broadcast_to(z[tag + nm][n], g[nm][n].shape), what + nm)
            _compare_parts(parts[n], z[tag + "elbo_parts"][n], what + "bound")
    b.close()


# ---- 2. parity with the comparator and the accuracy envelope, after every stage ---------------------------------------------
@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_parity_and_envelope(name):
    T, D, K, P = RR.CASES[name][:4]
    n = max(T, D, K)
    f64, ext = RR.trace(name), RR.trace(name, extended=True)
    b = _case_handle(name)
    got = RR.run_stages(lambda stage: _do(b, stage), lambda: _snapshot(b), lambda mode: _bound(b, mode), RR.ITERS, P)
    b.close()
    assert [k for k, _ in got] == [k for k, _ in f64]
    failures, worst = [], 0.0
    for i, ((key, g), (_, v64)) in enumerate(zip(got, f64)):
        it, stage, q = key
        what = "iteration %d %s %s" % (it + 1, stage, q)
        if stage == "bound":
            for r in range(g.shape[0]):
                _compare_parts(g[r], v64[r], "%s replicate %d" % (what, r), q == "exact")
        else:
            _close(g, v64, what)
        if i >= len(ext):       # D = 64: the long-double run has one iteration (regressors_ref.CASES); the second is held to parity above
            assert name == "t40_d64k40p6v12" and it == 1
            continue
        vx = ext[i][1]
        if stage == "bound":
            e64 = ER.bound_errors(v64, vx)[0]
            assert e64.max() <= ER.CAP
            for r, p, e6, eg, ratio, own in ER.compare_bound(g, vx, e64, n):
                print("%s replicate %d %s e64 %.2e  e_gpu %.2e  (%.2f y)" % (what, r, ER.LDS_PARTS[p], e6, eg, ratio))
                worst = max(worst, ratio / ER.FACTOR)
                if ratio > ER.FACTOR:
                    failures.append((what, r, ER.LDS_PARTS[p], e6, eg, ratio))
        else:
            e64, e_gpu = ER.rel(v64, vx), ER.rel(g, vx)
            y = ER.yardstick(e64, n)
            print("%-40s e64 %.2e  e_gpu %.2e  (%.2f of the bound)" % (what, e64, e_gpu, e_gpu / (ER.FACTOR * y)))
            worst = max(worst, e_gpu / (ER.FACTOR * y))
            assert e64 <= ER.CAP
            if e_gpu > ER.FACTOR * y:
                failures.append((what, e64, e_gpu, e_gpu / y))
    print("ENVELOPE %s largest share of the bound %.3f" % (name, worst))
    assert not failures, failures


# ---- 3. the entry points agree with one another -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t19_d6k4v2", "lengths_d16k10p2v3"])
def test_stagewise_calls_are_iterate(name):
    a, b = _case_handle(name), _case_handle(name)
    N, P = RR.n_case(name), RR.CASES[name][3]
    for it in range(2):
        for stage, _ in RR.stages(P):
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


@pytest.mark.parametrize("name", ["t19_d6k4v2", "t33_d5k14v3", "t19_d6k4p2v1"])
def test_single_node_updates(name):
    """update_x at t = 0, an interior t next to either end and T - 1 after a parameter update: both boundary nodes, which take the
    regressors through the rows of Ct, and interior nodes, which take them through the gains -- each against the comparator's
    update of the same node."""
    Y, U, V, st0, pri, ln = RR.problem(name)
    T, P = Y.shape[1], RR.CASES[name][3]
    (_, m), = RR.models(Y, U, V, st0, pri, ln)
    b = _case_handle(name)
    for h in (b, m):
        for stage, _ in RR.stages(P):
            (_do if h is b else RR.do_stage)(h, stage)
    for t in (0, 1, T // 2, T - 2, T - 1, 1, 0):
        b.update_x(t)
        m.update_x(t)
        _close(b.get_state(("X",))["X"][:, t], m.st["X"][:, t], "X_%d" % t, rtol=1e-11)
    _close(b.get_state(("X",))["X"], m.st["X"], "all states")
    b.close()


def test_single_node_updates_at_the_end_of_every_chain():
    """the last node of each chain of its own length, and t = 0: the v channel in a chain's own last row"""
    name = "lengths_d16k10p2v3"
    Y, U, V, st0, pri, ln = RR.problem(name)
    ms = RR.models(Y, U, V, st0, pri, ln)
    b = _case_handle(name)
    for stage, _ in RR.stages(RR.CASES[name][3]):
        _do(b, stage)
        for _, m in ms:
            RR.do_stage(m, stage)
    for t in sorted({int(x) - 1 for x in ln} | {0}):
        b.update_x(t)
        X = b.get_state(("X",))["X"]
        for (n,), m in ms:
            if t < m.T:
                m.update_x(t)
                _close(X[n, t], m.st["X"][0, t], "chain %d X_%d" % (n, t), rtol=1e-11)
    b.close()


@pytest.mark.parametrize("name", ["t19_d6k4v2", "t33_d5k14v3", "t19_d6k4p2v1"])
def test_with_zero_regressors_the_handle_is_bitwise_the_one_without(name):
    """V = 0: X, A, C, Q, R (and B) are bitwise those of the same handle without regressors after two iterations -- a plain handle
    for P = 0, a handle with inputs otherwise: the extra channels contribute exact zeros to every sum, in the sweeps (also where
    Kt = 17 takes another tile count than K = 14), in the statistics, in H_C and in the residual of R, and C with R in two launches
    are C with R in one.  E has gone to its prior."""
    from pyvb_amd.lds import LDSBatch
    Y, U, V, st0, pri, _ = RR.problem(name)
    a = _batch(Y, U, np.zeros_like(V), st0, pri)
    p = LDSBatch.from_problem(Y, RR.split_regressors(st0)[0], {k: v for k, v in pri.items() if not k.startswith("E_")}, U=U)
    assert p.Pv == 0 and a.Pv == V.shape[2] and p.P == a.P
    a.iterate(2); p.iterate(2)
    ga, gp = a.get_state(), p.get_state()
    for k in gp:
        assert np.array_equal(ga[k], gp[k]), (k, np.abs(ga[k] - gp[k]).max())
    assert np.array_equal(a.get_posterior_classes()[0], p.get_posterior_classes()[0])
    assert np.abs(ga["E_mean"]).max() == 0.0
    _close(ga["E_colvar"], np.broadcast_to(1.0 / pri["E_prior_prec"], ga["E_colvar"].shape), "E_colvar", rtol=1e-15)
    a.close(); p.close()


def test_a_switched_off_replicate_keeps_its_E():
    name = "t19_d6k4v2"
    Y, U, V, st0, pri, ln = RR.problem(name)
    b = _case_handle(name)
    b.set_active([True, False])
    b.iterate(2)
    b.update_E()            # the explicit entry honours the mask too
    g = b.get_regressor_state()
    assert np.array_equal(g["E_mean"][1], st0["E_mean"][1]) and np.array_equal(g["E_colvar"][1], st0["E_colvar"][1])
    assert np.all(np.isnan(g["qld_E"][1])) and np.all(np.isfinite(g["qld_E"][0]))
    m = RR.Model(Y[:1], None, V[:1], {k: v[:1] for k, v in st0.items()}, pri)
    m.iterate(); m.iterate(); m.update_E()
    _close(g["E_mean"][0], m.st["E_mean"][0], "E_mean of the running replicate")
    _close(g["qld_E"][0], m.st["qld_E"][0], "qld_E of the running replicate")
    b.close()


def test_iterate_until_stops_where_the_comparator_does():
    """Per-replicate convergence on a handle with regressors: every replicate stops in the iteration in which Network.learn's test
    stops the comparator's run of it alone -- the deltas it meets pass converge_ref's guard."""
    tol, max_iters = 20.0, 30       # the four stop after 2, 9, 16 and 7 iterations
    Y, U, V, st0, pri = synth.make_regression_problem(30, 4, 5, 1, 2, 4, seed=32500)
    ms = [RR.Model(Y[n:n + 1], U[n:n + 1], V[n:n + 1], {k: v[n:n + 1] for k, v in st0.items()}, pri) for n in range(4)]
    runs = [CR.guarded(CR.learn(lambda m=m: m.iterate()[0], tol, max_iters), tol, "replicate %d" % i) for i, m in enumerate(ms)]
    print("stops", [r[0] for r in runs])
    assert len({r[0] for r in runs}) == 4 and all(r[1] for r in runs), [r[:2] for r in runs]
    b = _batch(Y, U, V, st0, pri)
    n = b.iterate_until(max_iters, tol, check_every=1)
    iters, conv, llb = b.convergence()
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * np.abs(r[2][-1]).sum()
    g = _snapshot(b)
    for i, m in enumerate(ms):
        for k in ("X", "A_mean", "B_mean", "C_mean", "E_mean"):
            _close(g[k][i], m.st[k][0], "at the stop: replicate %d %s" % (i, k))
    b.close()


# ---- 4. handles without regressors are what they were -----------------------------------------------------------------------
def _counts(b):
    """launches per kernel class of three iterations of a handle that has iterated before, k_regressors.hip's class included"""
    b.iterate(1)
    b.sync()
    b.timing(True)
    b.iterate(3)
    b.sync()
    kt = {k: v[1] for k, v in b.kernel_times().items()}
    cnt = _capi.ctypes.c_int()
    _capi.check(_capi.lib.pyvb_lds_timing_get(b._h, _capi.K_REGRESSORS, None, _capi.ctypes.byref(cnt)))
    return kt, cnt.value


def test_handles_without_regressors_launch_what_they_did():
    """The launches per kernel class of an iteration on a plain handle and on a handle with inputs only are those of the commit
    before regressors (the step lists of tests/test_lds_flow_cpu.py: ITERATION, counted per class) -- and none of k_regressors.hip."""
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri = synth.make_problem(19, 6, 4, 2, seed=31400)
    b = LDSBatch.from_problem(Y, st0, pri)
    kt, rg = _counts(b)
    assert kt == {"prep": 3, "sweep_fwd": 3, "sweep_bwd": 3, "stats": 3, "params": 6, "elbo": 3, "step": 0, "gy": 0, "inputs": 0} and rg == 0, (kt, rg)
    b.close()
    Y, U, st0, pri = synth.make_input_problem(19, 6, 4, 2, 2, seed=31400)
    b = LDSBatch.from_problem(Y, st0, pri, U=U)
    kt, rg = _counts(b)
    # params: k_moments, k_cols of A, k_cols of C with R, the residual of Q, k_noise; inputs: in_gains, in_moments, in_HA twice, in_colsB,
    # in_resQ, in_elbo
    assert kt == {"prep": 3, "sweep_fwd": 3, "sweep_bwd": 3, "stats": 3, "params": 15, "elbo": 3, "step": 0, "gy": 0, "inputs": 21} and rg == 0, (kt, rg)
    b.close()


def test_a_handle_with_regressors_launches_its_own():
    Y, U, V, st0, pri, _ = RR.problem("t19_d6k4v2")
    b = _batch(Y, U, V, st0, pri)
    kt, rg = _counts(b)
    # params: k_moments, k_cols of A with Q, k_cols of C, the residual of R, k_noise; regressors: rg_gains, rg_moments, rg_HC twice,
    # rg_colsE, rg_resR, rg_elbo
    assert kt == {"prep": 3, "sweep_fwd": 3, "sweep_bwd": 3, "stats": 3, "params": 15, "elbo": 3, "step": 0, "gy": 0, "inputs": 0,
                  "regressors": 21} and rg == 21, (kt, rg)
    b.close()


# ---- 5. refusals and argument errors ----------------------------------------------------------------------------------------
def test_refusals_and_argument_errors_come_before_any_launch():
    from pyvb_amd.lds import LDSBatch
    N, T, D, K, P, Pv = 2, 6, 3, 4, 1, 2
    for P in (0, 1):
        b = LDSBatch(N, T, D, K, inputs=P, regressors=Pv)
        b.timing(True)
        h, lib, p = b._h, _capi.lib, _capi.dptr
        # outputs that hold NaN, known entries, precision parents: PYVB_E_UNSUPPORTED, each naming the regressors and the cause
        Y = np.zeros((N, T, K)); Y[1, 2, 3] = np.nan
        for call, word in ((lambda: b.set_observations(Y), "NaN"),
                           (lambda: b.set_column_observations(np.where(np.eye(D) > 0, 0.5, np.nan), None), "known entries"),
                           (lambda: b.set_column_precisions(A=(1e-3, 1e-3, np.ones((N, D)))), "Gamma precision parents"),
                           (lambda: b.set_entry_precisions(C=(1e-3, 1e-3, np.ones((N, D, K)))), "DiagonalGamma precision parents")):
            with pytest.raises(_capi.PyvbHipError) as e:
                call()
            assert e.value.code == _capi.E_UNSUPPORTED and word in str(e.value) and "regressors" in str(e.value), str(e.value)
        # V: NULL, non-finite
        assert lib.pyvb_lds_set_regressors(h, None) == _capi.E_ARG
        for bad in (np.nan, np.inf):
            V = np.zeros((N, T, Pv)); V[1, 4, 1] = bad
            assert lib.pyvb_lds_set_regressors(h, p(V)) == _capi.E_ARG
            assert "replicate 1, row 4, channel 1" in lib.pyvb_last_error().decode()
        pp = np.ones((Pv, K)); pp[1, 2] = 0.0
        assert lib.pyvb_lds_set_regressor_priors(h, p(np.zeros((K, Pv))), p(pp)) == _capi.E_ARG
        # an update before the regressors are there
        pri = dict(synth.default_priors(D, K), E_prior_mean=np.zeros((K, Pv)), E_prior_prec=np.ones((Pv, K)))
        if P:
            pri.update(B_prior_mean=np.zeros((D, P)), B_prior_prec=np.ones((P, D)))
            b.set_inputs(np.zeros((N, T, P)))
        b.set_priors(pri)
        b.set_observations(np.zeros((N, T, K)))
        for rc in (lib.pyvb_lds_sweep(h, 0), lib.pyvb_lds_update_x(h, 1), lib.pyvb_lds_iterate(h, 1)):
            assert rc == _capi.E_ARG and b"pyvb_lds_set_regressors" in lib.pyvb_last_error()
        b.set_posterior_classes(np.broadcast_to(np.eye(D), (N, 3, D, D)).copy())
        for rc in (lib.pyvb_lds_update_E(h), lib.pyvb_lds_update_C(h), lib.pyvb_lds_update_R(h), lib.pyvb_lds_elbo(h)):
            assert rc == _capi.E_ARG and b"pyvb_lds_set_regressors" in lib.pyvb_last_error()
        assert _launches(b) == 0
        b.close()
    # the entries of a handle with regressors on one without, plain or with inputs
    for P in (0, 2):
        b = LDSBatch(N, T, D, K, inputs=P)
        v = np.zeros(N * T * Pv + N * K * Pv)
        for rc in (lib.pyvb_lds_set_regressors(b._h, p(v)), lib.pyvb_lds_get_regressors(b._h, p(v)), lib.pyvb_lds_set_regressor_priors(b._h, p(v), p(v)),
                   lib.pyvb_lds_set_regressor_state(b._h, p(v), p(v)), lib.pyvb_lds_get_regressor_state(b._h, p(v), None, None, None),
                   lib.pyvb_lds_update_E(b._h)):
            assert rc == _capi.E_ARG and b"created without regressors" in lib.pyvb_last_error()
        b.close()
    # and the inputs' entries on a handle with regressors alone
    b = LDSBatch(N, T, D, K, regressors=Pv)
    assert lib.pyvb_lds_update_B(b._h) == _capi.E_ARG and b"created without inputs" in lib.pyvb_last_error()
    b.close()
