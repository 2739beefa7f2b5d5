"""GPU: DiagonalGamma precision parents for the columns of A and C, one precision per entry (include/pyvb_hip.h:
pyvb_lds_set_entry_precisions, k_ard.hip: k_entry) -- sparse transition and loading matrices on the fused LDS path.

The comparator is tests/entry_ref.py, the composition of oracle functions that tests/test_entry_cpu.py pins against the reference's own
run of such graphs, and that run itself (tests/golden/entry_*.npz).  Parity is the suite's RTOL = 1e-8 (tests/test_ard_gpu.py: max-norm
for states and parameters, the parts of the bound to RTOL of the sum of their magnitudes, the total to RTOL of itself; the exact
parts to RTOL of max(|part|, 1)).  The envelope is the rule of DESIGN.md section 17, quantity by quantity against the comparator's
long-double run: e_gpu <= 16 max(e64, n 2^-52), n = max(D, K, T) -- after every iteration, except that at D = K = 64 the long-double
run stops after the first; the second is held to parity only.

Shapes (tests/entry_ref.py: CASES): N = 3 replicates with different data, different initial qb and per-entry priors; D = 3 / K = 4,
ragged D = 33 / K = 17 and D = 17 / K = 33 (rows below and above D, a partial last group of four columns, a partial wavefront), the
full width D = K = 64, a single lane D = K = 1; T between 6 and 12; parents on A only, on C only, on both, and Gamma parents on A
with DiagonalGamma parents on C.

"Bitwise" is justified as in tests/test_ard_gpu.py: two handles of the same shapes run the same instructions in the same order, and
k_entry's per-column sums are butterflies over the lanes that add the same pairs in the same order whatever the data.
"""
import glob
import os

import numpy as np
import pytest

import ard_ref as AR
import converge_ref as CR
import entry_ref as NR
import extended_ref as ER
from conftest import GOLDEN_DIR
from pyvb_amd import _capi, synth
from test_ard_gpu import RTOL, _close, _compare_parts, _batch, _bounds, _everything, _launches

pytestmark = pytest.mark.gpu

ENTRY = sorted(glob.glob(os.path.join(GOLDEN_DIR, "entry_*.npz")))
ARD = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ard_*.npz")))


def _snapshot(b):
    """The handle's counterpart of entry_ref.snapshot."""
    out = {k: v for k, v in b.get_state().items() if k in AR.QUANTITIES}
    out["Sigma"] = b.get_posterior_classes()[0]
    for w, (qa, qb) in b.column_precisions().items():
        out[w + "_alpha_b"], out[w + "_alpha_E"] = qb, qa / qb
    for w, (qa, qb) in b.entry_precisions().items():
        out[w + "_entry_b"], out[w + "_entry_E"] = qb, qa / qb
    return out


def _compare_models(b, ms, tag):
    """Every row of the handle against its model of the comparator: states per chain, parameters and parents per model."""
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
            for w, e in m.entry.items():
                _close(g[w + "_entry_b"][n], e["qb"], t + w + "_entry_b")
                _close(g[w + "_entry_E"][n], m.expectation(w), t + w + "_entry_E")
    return g


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ENTRY, ids=lambda p: os.path.basename(p)[6:-4])
def test_reference_run_is_reproduced(path):
    """pyvb_lds_iterate on the fixture's graph (both matrices; Gamma parents on A with DiagonalGamma parents on C under Gamma noise;
    a fully and a partly known column of A; one model of two chains): at every recorded iteration the states, the columns, qb of Q,
    R and of the precision parents and the six parts are the reference's."""
    meta, Y, st0, pri, lengths, z = NR.load_entry(path)
    N = len(lengths)
    b = _batch(Y, st0, pri, np.asarray(lengths, dtype=np.int32) if N > 1 else None, np.zeros(N, dtype=np.int32) if N > 1 else None)
    assert sorted(b.entry_precisions()) == sorted(meta["which"]) and sorted(b.column_precisions()) == sorted(meta["gamma"])
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
            for w in meta["gamma"]:
                _close(g[w + "_alpha_b"][n], z[tag + w + "_alpha_b"], what + w + "_alpha_b")
            for w in meta["which"]:
                _close(g[w + "_entry_b"][n], z[tag + w + "_entry_b"], what + w + "_entry_b")
                _close(g[w + "_entry_E"][n], z[tag + w + "_entry_a"] / z[tag + w + "_entry_b"], what + w + "_entry_E")
        _compare_parts(parts.sum(0), z[tag + "elbo_parts"], tag + "the model")
        assert np.all(parts[1:, 2:] == 0.0)
    b.close()


# ---- 2. parity with the comparator and the accuracy envelope, after every iteration ----------------------------------------
@pytest.mark.parametrize("name", sorted(NR.CASES))
def test_parity_and_envelope(name):
    T, D, K = NR.CASES[name][:3]
    n = max(T, D, K)
    Y, st0, pri = NR.problem(name)
    f64, ext = NR.trace(name)[0], NR.trace(name, extended=True)[0]
    b = _batch(Y, st0, pri)
    assert sorted(b.entry_precisions()) == sorted(NR.CASES[name][3]) and sorted(b.column_precisions()) == sorted(NR.CASES[name][4])
    for it in range(NR.ITERS):
        b.iterate(1)
        g, parts = _snapshot(b), _bounds(b)
        s64, p64 = f64[it]
        assert sorted(g) == sorted(s64)
        for k in sorted(g):
            _close(g[k], s64[k], "iteration %d %s" % (it + 1, k))
        for mode in NR.BOUNDS:
            for r in range(NR.N_CASE):
                _compare_parts(parts[mode][r], p64[mode][r], "iteration %d %s bound, replicate %d" % (it + 1, mode, r), mode == "exact")
        if it >= len(ext):          # D = K = 64: the long-double run has one iteration (entry_ref.CASES); the second is held to parity above
            assert name == "d64k64_AC" and it == 1
            continue
        sx, px = ext[it]
        for k in sorted(g):
            e64, e_gpu = ER.rel(s64[k], sx[k]), ER.rel(g[k], sx[k])
            y = ER.yardstick(e64, n)
            print("iteration %d %-10s e64 %.2e  e_gpu %.2e  (%.2f of the bound)" % (it + 1, k, e64, e_gpu, e_gpu / (ER.FACTOR * y)))
            assert e64 <= ER.CAP
            assert e_gpu <= ER.FACTOR * y, (name, it, k, e64, e_gpu)
        for mode in NR.BOUNDS:
            e64 = ER.bound_errors(p64[mode], px[mode])[0]
            assert e64.max() <= ER.CAP
            for r, p, e6, eg, ratio, own in ER.compare_bound(parts[mode], px[mode], e64, n):
                print("iteration %d %-9s replicate %d %s e64 %.2e  e_gpu %.2e  (%.2f y)" % (it + 1, mode, r, ER.LDS_PARTS[p], e6, eg, ratio))
                assert ratio <= ER.FACTOR, (name, it, mode, r, p, e6, eg)
    b.close()


# ---- 3. stage-wise calls and partial column updates --------------------------------------------------------------------------
def _equal(ea, eb, what):
    assert sorted(ea) == sorted(eb)
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), (what, k)


def _everything_entry(b):
    out = _everything(b)
    for w, (qa, qb) in b.column_precisions().items():
        out[w + "_alpha_a"], out[w + "_alpha_b"] = qa, qb
    for w, (qa, qb) in b.entry_precisions().items():
        out[w + "_entry_a"], out[w + "_entry_b"] = qa, qb
    return out


@pytest.mark.parametrize("name", ["d3k4_AC", "d33k17_A", "d17k33_C", "d3k4_mixed"])
def test_stagewise_calls_are_iterate_bitwise(name):
    Y, st0, pri = NR.problem(name)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    for it in range(2):
        a.sweep("forward"); a.sweep("backward")
        a.update_A(); a.update_C(); a.update_Q(); a.update_R()
        a.update_column_precisions(); a.update_entry_precisions()
        b.iterate(1)
        _equal(_everything_entry(a), _everything_entry(b), "iteration %d" % (it + 1))
    a.close(); b.close()


def test_partial_column_update_then_the_precision_update():
    """update_columns over a part of the columns that starts and ends inside a group of four, then the precision update: it reads
    every column as stored, the renewed ones and the others."""
    Y, st0, pri = NR.problem("d33k17_A")
    ms = NR.models(Y, st0, pri)
    b = _batch(Y, st0, pri)
    b.sweep("forward"); b.sweep("backward")
    b.update_columns("A", 5, 22)
    b.update_entry_precisions("A")
    b.update_columns("A", 0, 33)            # under the new precisions
    b.update_C()
    for _, m in ms:
        m.sweep("forward"); m.sweep("backward")
        m.update_A((5, 22))
        m.update_entry("A")
        m.update_A((0, 33))
        m.update_C()
    _compare_models(b, ms, "")
    b.close()


# ---- 4. composition with the rest of the handle ------------------------------------------------------------------------------
def test_tied_models():
    """Models of 1, 3, 2 chains of unequal lengths (2 and 3 among them): the rows of a model are bitwise equal (and come from its
    first row's qb), each model's rows sum to the comparator's parts in both modes, the nodes' terms sit on the first row."""
    Y, st0, pri, ln, md = NR.tied_problem()
    ms = NR.models(Y, st0, pri, ln, md)
    b = _batch(Y, st0, pri, ln, md)
    c0 = b.entry_precisions()
    for rows, m in ms:
        for w in "AC":
            assert np.array_equal(c0[w][1][rows], np.repeat(st0[w + "_entry_b"][rows[:1]], len(rows), axis=0))
    for it in range(2):
        b.iterate(1)
        for _, m in ms:
            m.iterate()
        g = _compare_models(b, ms, "iteration %d " % (it + 1))
        parts = _bounds(b)
        for i, (rows, m) in enumerate(ms):
            for k in ("A_entry_b", "C_entry_b", "A_entry_E", "C_entry_E", "A_mean", "C_colvar"):
                for n in rows[1:]:
                    assert np.array_equal(g[k][n], g[k][rows[0]]), (k, rows[0], n)
            for mode in NR.BOUNDS:
                _compare_parts(parts[mode][rows].sum(0), m.elbo_parts(mode), "iteration %d model %d %s" % (it + 1, i, mode), mode == "exact")
                assert np.all(parts[mode][rows[1:], 2:] == 0.0)
    b.close()


def test_from_series_and_from_trials_pick_the_parents_up():
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri, ln, md = NR.tied_problem()
    series = [(Y[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}) for n, Tn in enumerate(ln)]
    trials = [[series[n] for n in np.nonzero(md == m)[0]] for m in range(int(md.max()) + 1)]
    for made, same in ((LDSBatch.from_series(series, pri), _batch(Y, st0, pri, ln)),
                       (LDSBatch.from_trials(trials, pri), _batch(Y, st0, pri, ln, md))):
        assert sorted(made.entry_precisions()) == ["A", "C"]
        made.iterate(2); same.iterate(2)
        _equal(_everything_entry(made), _everything_entry(same), "after two iterations")
        made.close(); same.close()
    b = LDSBatch.from_series(series, pri)
    assert np.array_equal(b.entry_precisions()["A"][1], st0["A_entry_b"])
    b.close()


def test_a_switched_off_replicate_keeps_its_qb_and_two_runs_are_bitwise_equal():
    Y, st0, pri = NR.problem("d3k4_AC")
    ms = NR.models(Y, st0, pri)
    runs = []
    for _ in range(2):
        b = _batch(Y, st0, pri)
        b.set_active([True, False, True])
        b.iterate(2)
        b.update_entry_precisions()         # the explicit entry honours the mask too
        runs.append(_everything_entry(b))
        b.close()
    _equal(runs[0], runs[1], "two runs")
    for w in "AC":
        assert np.array_equal(runs[0][w + "_entry_b"][1], st0[w + "_entry_b"][1]), w + ": qb of the switched-off row changed"
    for i in (0, 2):
        m = ms[i][1]
        m.iterate(); m.iterate(); m.update_entry()
        for w in "AC":
            _close(runs[0][w + "_entry_b"][i], m.entry[w]["qb"], "replicate %d %s qb" % (i, w))


def test_two_runs_at_full_width_are_bitwise_equal():
    Y, st0, pri = NR.problem("d64k64_AC")
    runs = []
    for _ in range(2):
        b = _batch(Y, st0, pri)
        b.iterate(2)
        runs.append(_everything_entry(b))
        b.close()
    _equal(runs[0], runs[1], "two runs")


def _learn(m, bound, tol, max_iters, what):
    return CR.guarded(CR.learn(lambda: m.iterate(bound), tol, max_iters), tol, what)


def test_iterate_until_stops_where_the_comparator_does():
    """Per-replicate convergence runs the precision updates (iterate_updates): every replicate stops in the iteration in which
    Network.learn's test stops the comparator's run of it alone -- the deltas it meets pass converge_ref's guard."""
    c = NR.CONVERGE
    Y, st0, pri = NR.converge_problem()
    ms = NR.models(Y, st0, pri)
    runs = [_learn(m, "reference", c["tol"], c["max_iters"], "replicate %d" % i) for i, (_, m) in enumerate(ms)]
    assert len({r[0] for r in runs}) >= 2 and all(r[1] for r in runs), [r[:2] for r in runs]        # different stops
    b = _batch(Y, st0, pri)
    n = b.iterate_until(c["max_iters"], c["tol"], check_every=1)
    iters, conv, llb = b.convergence()
    print("stops", iters, [r[0] for r in runs])
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * np.abs(r[2][-1]).sum()
    _compare_models(b, ms, "at the stop: ")
    b.close()


def test_iterate_until_model_stops_where_the_comparator_does():
    c = NR.CONVERGE_TIED
    Y, st0, pri, ln, md = NR.tied_problem()
    ms = NR.models(Y, st0, pri, ln, md)
    runs = [_learn(m, "exact", c["tol"], c["max_iters"], "model %d" % i) for i, (_, m) in enumerate(ms)]
    assert len({r[0] for r in runs}) >= 2 and all(r[1] for r in runs), [r[:2] for r in runs]
    b = _batch(Y, st0, pri, ln, md)
    b.set_bound_mode("exact")
    n = b.iterate_until_model(c["max_iters"], c["tol"], check_every=1)
    iters, conv, llb = b.model_convergence()
    print("stops", iters, [r[0] for r in runs])
    assert list(iters) == [r[0] for r in runs] and conv.all() and n == max(r[0] for r in runs)
    for i, r in enumerate(runs):
        assert abs(llb[i] - r[2][-1].sum()) <= RTOL * max(np.abs(r[2][-1]).sum(), 1.0)
    _compare_models(b, ms, "at the stop: ")
    b.close()


# ---- 5. one kind of parent per matrix ----------------------------------------------------------------------------------------
def _plain(st0, pri):
    return ({k: v for k, v in st0.items() if not (k.endswith("_entry_b") or k.endswith("_alpha_b"))},
            {k: v for k, v in pri.items() if "_entry_" not in k and "_alpha_" not in k})


def test_set_priors_returns_the_columns_to_constant_parents():
    """set_priors after set_entry_precisions: bitwise the handle that never had such parents, in both bound modes."""
    Y, st0, pri = NR.problem("d33k17_A")
    plain_st0, plain_pri = _plain(st0, pri)
    a, b = _batch(Y, plain_st0, plain_pri), _batch(Y, st0, pri)
    assert a.entry_precisions() == {} and sorted(b.entry_precisions()) == ["A"]
    b.set_priors(plain_pri)
    assert b.entry_precisions() == {} and b.column_precisions() == {}
    for mode in ("reference", "exact"):
        for h in (a, b):
            h.set_bound_mode(mode)
            h.iterate(2)
        _equal(_everything(a), _everything(b), mode)
        assert np.array_equal(a.elbo_history(), b.elbo_history())
    a.close(); b.close()


def test_the_most_recent_setter_of_a_matrix_wins():
    """set_entry_precisions then set_column_precisions on the same matrix is bitwise the handle that only made the second call, and
    the other way round; the other matrix keeps the kind it has."""
    Y, st0, pri = NR.problem("d3k4_AC")
    plain_st0, plain_pri = _plain(st0, pri)
    N, D, K = st0["A_mean"].shape[0], 3, 4
    rng = np.random.default_rng(5)
    gam = {"A": (1e-3 * (1 + np.arange(D)), 2e-3 * (1 + np.arange(D)), 0.5 + rng.random((N, D))),
           "C": (3e-3 * (1 + np.arange(D)), 1e-3 * (1 + np.arange(D)), 0.5 + rng.random((N, D)))}
    ent = {w: (pri[w + "_entry_a0"], pri[w + "_entry_b0"], st0[w + "_entry_b"]) for w in "AC"}
    for first, second in ((ent, gam), (gam, ent)):
        set1 = (lambda h, **kw: h.set_entry_precisions(**kw)) if first is ent else (lambda h, **kw: h.set_column_precisions(**kw))
        set2 = (lambda h, **kw: h.set_entry_precisions(**kw)) if second is ent else (lambda h, **kw: h.set_column_precisions(**kw))
        a, b = _batch(Y, plain_st0, plain_pri), _batch(Y, plain_st0, plain_pri)
        set1(a, A=first["A"], C=first["C"])
        set2(a, A=second["A"])              # A changes its kind, C keeps the first
        set1(b, C=first["C"])
        set2(b, A=second["A"])
        kinds = (sorted(a.entry_precisions()), sorted(a.column_precisions()))
        assert kinds == ((["C"], ["A"]) if first is ent else (["A"], ["C"])), kinds
        lib, p, q = _capi.lib, _capi.dptr, np.empty((N, D, K))
        assert lib.pyvb_lds_get_column_precisions(a._h, 0 if first is gam else 1, p(q), p(q.copy())) == _capi.E_ARG
        assert b"DiagonalGamma precision parents" in lib.pyvb_last_error()
        assert lib.pyvb_lds_update_column_precisions(a._h, 0 if first is gam else 1) == _capi.E_ARG
        assert lib.pyvb_lds_update_entry_precisions(a._h, 1 if first is gam else 0) == _capi.E_ARG
        for mode in ("reference", "exact"):
            for h in (a, b):
                h.set_bound_mode(mode)
                h.iterate(2)
            _equal(_everything_entry(a), _everything_entry(b), mode)
        a.close(); b.close()


def test_a_handle_without_the_new_setter_reproduces_the_older_fixtures():
    """An ard_* fixture (Gamma parents) and a plain lds_* fixture, on handles that never call set_entry_precisions."""
    meta, Y, st0, pri, lengths, z = AR.load_ard([p for p in ARD if p.endswith("ard_d3k4_t12.npz")][0])
    b = _batch(Y, st0, pri)
    assert b.entry_precisions() == {} and sorted(b.column_precisions()) == ["A", "C"]
    for it in range(1, 3):
        b.iterate(1)
        tag = "it%d_" % it
        g = b.get_state()
        for nm in ("A_mean", "C_mean", "A_colvar", "C_colvar"):
            _close(g[nm][0], z[tag + nm], tag + nm)
        for w in "AC":
            _close(b.column_precisions()[w][1][0], z[tag + w + "_alpha_b"], tag + w + "_alpha_b")
        _compare_parts(b.elbo().sum(0), z[tag + "elbo_parts"], tag + "parts")
    b.close()
    from conftest import golden_files, load_golden
    path = [p for p in golden_files() if not np.isnan(np.load(p)["Y"]).any() and str(np.load(p)["noise"]) == "diagonal_gamma"][0]
    meta, Y, st0, pri, z = load_golden(path)
    b = _batch(Y, st0, pri)
    b.iterate(1)
    g = b.get_state()
    _close(g["X"][0], z["it1_X"], "plain X")
    _close(g["A_mean"][0], z["it1_A_mean"], "plain A_mean")
    _compare_parts(b.elbo()[0], z["it1_elbo_parts"], "plain parts")
    b.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_and_argument_errors_come_before_any_launch():
    from pyvb_amd.lds import LDSBatch
    # Wishart noise and the 128-wide class: PYVB_E_UNSUPPORTED
    for D, K, noise, word in ((4, 5, "wishart", "Wishart"), (65, 5, "diagonal_gamma", "64"), (4, 65, "gamma", "64")):
        b = LDSBatch(2, 6, D, K, noise)
        b.timing(True)
        with pytest.raises(_capi.PyvbHipError) as e:
            b.set_entry_precisions(A=(1.0, 1.0, 1.0))
        assert e.value.code == _capi.E_UNSUPPORTED and word in str(e.value) and "DiagonalGamma precision parents" in str(e.value), str(e.value)
        assert _launches(b) == 0
        b.close()
    N, D, K = 3, 4, 5
    b = LDSBatch(N, 6, D, K)
    b.timing(True)
    h, lib, p = b._h, _capi.lib, _capi.dptr
    for which, rows, nm in ((0, D, "A"), (1, K, "C")):
        one, qb = np.ones((D, rows)), np.ones((N, D, rows))
        assert lib.pyvb_lds_set_entry_precisions(h, which, None, p(one), p(qb)) == _capi.E_ARG
        assert lib.pyvb_lds_set_entry_precisions(h, which, p(one), p(one), None) == _capi.E_ARG
        for bad in (0.0, -1.0, np.nan, np.inf):
            v = one.copy(); v[2, 1] = bad
            for args in ((v, one), (one, v)):
                assert lib.pyvb_lds_set_entry_precisions(h, which, p(args[0]), p(args[1]), p(qb)) == _capi.E_ARG
                msg = lib.pyvb_last_error().decode()
                assert "column 2, row 1 of " + nm in msg and ("a0" if args[0] is v else "b0") in msg, msg
            q = qb.copy(); q[1, 3, 2] = bad
            assert lib.pyvb_lds_set_entry_precisions(h, which, p(one), p(one), p(q)) == _capi.E_ARG
            msg = lib.pyvb_last_error().decode()
            assert "replicate 1, column 3, row 2 of " + nm in msg, msg
        # the matrix has no DiagonalGamma parents: get and update are argument errors
        assert lib.pyvb_lds_get_entry_precisions(h, which, p(qb), p(qb.copy())) == _capi.E_ARG
        assert ("columns of %s have no DiagonalGamma precision parents" % nm).encode() in lib.pyvb_last_error()
        assert lib.pyvb_lds_update_entry_precisions(h, which) == _capi.E_ARG
    for which in (-1, 2):
        one, qb = np.ones((D, K)), np.ones((N, D, K))
        assert lib.pyvb_lds_set_entry_precisions(h, which, p(one), p(one), p(qb)) == _capi.E_ARG
        assert b"which must be 0 (A) or 1 (C)" in lib.pyvb_last_error()
        assert lib.pyvb_lds_get_entry_precisions(h, which, None, None) == _capi.E_ARG
        assert lib.pyvb_lds_update_entry_precisions(h, which) == _capi.E_ARG
    assert b.entry_precisions() == {}
    assert _launches(b) == 0
    # parents on C only: A still refuses, C answers
    qb = 2.0 * np.ones((N, D, K))
    b.set_entry_precisions(C=(1e-3, 1e-3, qb))
    assert lib.pyvb_lds_update_entry_precisions(h, 0) == _capi.E_ARG
    qa, got = b.entry_precisions()["C"]
    assert np.array_equal(got, qb) and np.array_equal(qa, np.full((N, D, K), 1e-3 + 0.5))
    b.close()
