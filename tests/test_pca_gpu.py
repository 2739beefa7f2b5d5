"""GPU parity of the VB-PCA-with-missing-data path: against the fixtures produced by the reference
(tests/golden/pca_*.npz) and against the oracle, stage by stage.  Tolerance 1e-8 relative."""
import glob
import os

import numpy as np
import pytest

from oracle import pca_closed_form as P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FILES = sorted(glob.glob(os.path.join(HERE, "golden", "pca_*.npz")))
RTOL = 1e-8


def _load(path):
    from test_pca_oracle_golden import load_pca
    return load_pca(path)


def _close(a, b, what, rtol=RTOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert np.all(np.isfinite(a)), what + ": non-finite"
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _compare(b, st, tag):
    g = b.get_state()
    for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var"):
        _close(g[k], st[k], tag + k)
    _close(g["beta_a"], st["beta_a"], tag + "beta_a")
    _close(g["beta_b"], st["beta_b"], tag + "beta_b")
    nm = (~st["obs"]).sum(1)
    ref_var = np.where(nm > 0, st["X_var"].max(1), 0.0)
    _close(g["X_rowvar"][nm > 0], ref_var[nm > 0], tag + "X_rowvar")


@pytest.mark.parametrize("path", FILES, ids=lambda p: os.path.basename(p)[4:-4])
def test_golden_fixtures(path):
    from pyvb_amd.pca import PCABatch
    N, d, q, init, pri, z = _load(path)
    b = PCABatch.from_problem(init, pri)
    for it in range(1, int(max(z["iters"])) + 1):
        b.iterate(1)
        if it in z["iters"]:
            tag = "it%d_" % it
            g = b.get_state()
            for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
                _close(g[k], z[tag + k], tag + k)
            parts = b.elbo()
            ref = z[tag + "elbo_parts"]
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)
    b.close()


@pytest.mark.parametrize("sweep", ["pairs"])
@pytest.mark.parametrize("path", [f for f in FILES if "default_init" not in f], ids=lambda p: os.path.basename(p)[4:-4])
def test_golden_fixtures_through_the_pair_owning_sweep(path, sweep):
    """k_pca_pairs (a pair of wavefronts owns whole rows, half the columns each), put on the new handle with set_sweep
    (pyvb_pca_set_sweep) for problems the size rule would give to the column-owning sweep: it has to give the reference's
    numbers all the same."""
    from pyvb_amd.pca import PCABatch
    N, d, q, init, pri, z = _load(path)
    b = PCABatch.from_problem(init, pri)
    b.set_sweep(sweep)
    for it in range(1, int(max(z["iters"])) + 1):
        b.iterate(1)
        if it in z["iters"]:
            tag = "it%d_" % it
            g = b.get_state()
            for k in ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
                _close(g[k], z[tag + k], tag + k)
            parts = b.elbo()
            ref = z[tag + "elbo_parts"]
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)
    b.close()


@pytest.mark.parametrize("sweep", ["columns", "pairs"])
def test_imputed_entries_are_recomputed_not_stored(sweep):
    """Round 4: the sweep of an iteration leaves the imputed entries of X unstored (they are <W> z_n + <Mu> of what IS stored; the
    next sweep recomputes them, pyvb_pca_get_state and every other reader has them put into X first: pca_materialize_x).  A run
    that is interrupted by a read of the state and by an evaluation of the bound ends bitwise where an uninterrupted one
    ends, and both agree with a handle that stores the entries (set_sweep("store")) to rounding.  (Partial row updates and
    Z updates in between, without a read: test_lazy_state_transitions_without_a_read.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 3000, 250, 16
    init, pri = G.pca_problem(N, d, q, seed=77)
    a = PCABatch.from_problem(init, pri); a.set_sweep(sweep); a.iterate(5); sa = a.get_state(); ea = a.elbo(); a.close()
    b = PCABatch.from_problem(init, pri)
    b.set_sweep(sweep)
    b.iterate(2)
    mid = b.get_state()                                 # materialises X
    assert np.isfinite(mid["X"]).all()
    b.iterate(1)
    b.elbo()
    b.iterate(2)
    sb = b.get_state(); eb = b.elbo(); b.close()
    for k in ("X", "Z", "W_mean", "Mu_mean", "beta_b"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(ea, eb)
    c = PCABatch.from_problem(init, pri); c.set_sweep("store"); c.iterate(5); sc = c.get_state(); ec = c.elbo(); c.close()
    for k in ("X", "Z", "W_mean", "Mu_mean"):
        _close(sa[k], sc[k], "lazy vs stored: " + k)
    assert np.all(np.abs(ea - ec) <= 1e-10 * np.abs(ec).sum())
    # the oracle, too
    st = P.make_state(init, pri, N, d, q)
    for _ in range(5):
        ref = P.iterate(st, pri)
    _close(sa["X"], st["X"], "X after five iterations")
    assert np.all(np.abs(ea - ref) <= RTOL * np.abs(ref).sum())


def test_the_sweep_a_long_problem_gets_by_default_with_fewer_than_sixteen_latents():
    """From 512 rows per CU on (and d > 192) a handle takes the pair-owning sweep without being asked (api_pca.hip); here with q = 7
    and d = 250 -- padded latent indices and a padded column tile in the kernel that otherwise only meets q = 16 at that size --
    against the oracle and against the column-owning sweep on the same problem."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 140000, 250, 7
    init, pri = G.pca_problem(N, d, q, seed=5)
    a = PCABatch.from_problem(init, pri)
    assert a.sweep == "pairs"
    a.iterate(3); sa = a.get_state(); ea = a.elbo(); a.close()
    c = PCABatch.from_problem(init, pri); c.set_sweep("columns"); c.iterate(3); sc = c.get_state(); ec = c.elbo(); c.close()
    st = P.make_state(init, pri, N, d, q)
    for _ in range(3):
        ref = P.iterate(st, pri)
    for k in ("W_mean", "W_var", "Z", "X", "Mu_mean", "beta_b"):
        _close(sa[k], st[k], "default sweep vs oracle: " + k)
        _close(sa[k], sc[k], "default sweep vs column-owning sweep: " + k)
    assert np.all(np.abs(ea - ref) <= RTOL * np.abs(ref).sum()) and np.all(np.abs(ea - ec) <= 1e-10 * np.abs(ec).sum())


@pytest.mark.parametrize("case", ["a", "b", "c"])
@pytest.mark.parametrize("sweep", ["columns", "pairs"])
def test_lazy_state_transitions_without_a_read(sweep, case):
    """Stage-wise calls that meet a handle whose imputed entries are not in X, with NO read in between: whatever reads rows of X
    outside a sweep (the X_0 step reads row 0) must have them stored first.  One get_state() + elbo() at the end, against the same
    calls on the oracle.  q <= 16, no pinned rows, entries of row 0 missing (pca_problem masks at random; asserted)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 600, 250, 16
    init, pri = G.pca_problem(N, d, q, seed=4242)
    obs0 = np.asarray(init["obs"], dtype=bool)[0]
    assert (~obs0).any() and obs0.any(), "row 0 must be partially observed"
    st = P.make_state(init, pri, N, d, q)
    b = PCABatch.from_problem(init, pri)
    b.set_sweep(sweep)

    def iterate(k):
        for _ in range(k):
            P.iterate(st, pri)
        b.iterate(k)

    if case == "a":
        P.update_Z(st, pri); b.update_Z()
        P.update_X(st, pri, 0, N); b.update_X(0, N)         # a lazy sweep over ALL rows: row 0 among the unstored ones
        iterate(3)
    elif case == "b":
        iterate(1)
        P.update_X(st, pri, 150, 431); b.update_X(150, 431)
        iterate(1)
    else:
        P.update_Z(st, pri); b.update_Z()
        P.update_X(st, pri, 0, N); b.update_X(0, N)
        P.update_X(st, pri, 0, 1); b.update_X0()
        P.update_Mu(st, pri); b.update_Mu()
        iterate(1)
    _compare(b, st, "case %s (%s): " % (case, sweep))
    ref, got = P.elbo_parts(st, pri), b.elbo()
    assert np.all(np.abs(got - ref) <= RTOL * np.abs(ref).sum()), (got, ref)
    b.close()


def test_sweep_choice_ignores_the_environment(monkeypatch):
    """The library reads no environment: with the two variables that used to choose the sweep set, a new handle has the kind its
    size gives it and computes bitwise what a handle made without them computes.  The kind is changed by set_sweep alone, which
    refuses kinds it does not know."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd import _capi
    from pyvb_amd.pca import PCABatch
    N, d, q = 600, 250, 16
    init, pri = G.pca_problem(N, d, q, seed=4242)
    monkeypatch.delenv("PYVB_PCA_SWEEP", raising=False)
    monkeypatch.delenv("PYVB_PCA_WRITEBACK", raising=False)
    a = PCABatch.from_problem(init, pri)
    assert a.sweep == "columns"
    a.iterate(3); sa = a.get_state(); ea = a.elbo(); a.close()
    monkeypatch.setenv("PYVB_PCA_SWEEP", "pairs")
    monkeypatch.setenv("PYVB_PCA_WRITEBACK", "1")
    b = PCABatch.from_problem(init, pri)
    assert b.sweep == "columns"
    b.iterate(3); sb = b.get_state(); eb = b.elbo()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(ea, eb)
    for kind in (-1, 3, 7):
        with pytest.raises(_capi.PyvbHipError) as err:
            b.set_sweep(kind)
        assert err.value.code == _capi.E_ARG
        assert b.sweep == "columns"
    with pytest.raises(ValueError):
        b.set_sweep("rows")
    b.close()


@pytest.mark.parametrize("N,d,q", [(600, 250, 16), (330, 200, 5)])
def test_sweep_can_change_between_iterations(N, d, q):
    """pyvb_pca_set_sweep between iterations, with no read in between: columns -> pairs -> store -> pairs -> columns, an iteration
    under each, so that every kernel meets the unstored entries (or the stored ones) and the partials' partition another one left.
    d = 250 is k_pca_pairs<FULL>; d = 200, q = 5 the other instantiation (13 column tiles, padded latent indices).  One read at
    the end, against five iterations of the oracle and against a handle that stays with the column-owning sweep; tolerances of
    test_imputed_entries_are_recomputed_not_stored, which compares the same paths."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    init, pri = G.pca_problem(N, d, q, seed=31 + d)
    b = PCABatch.from_problem(init, pri)
    for kind in ("columns", "pairs", "store", "pairs", "columns"):
        b.set_sweep(kind)
        assert b.sweep == kind
        b.iterate(1)
    sb = b.get_state(); eb = b.elbo(); b.close()
    c = PCABatch.from_problem(init, pri)
    assert c.sweep == "columns"
    c.iterate(5); sc = c.get_state(); ec = c.elbo(); c.close()
    st = P.make_state(init, pri, N, d, q)
    for _ in range(5):
        ref = P.iterate(st, pri)
    keys = ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b")
    rel = lambda a, b: np.abs(np.asarray(a, dtype=float) - b).max() / np.abs(b).max()
    print("switched sweeps (%d, %d, %d): worst rel err vs oracle %.2e, vs the column-owning sweep %.2e; bound vs oracle %.2e, vs columns %.2e of sum |parts|"
          % (N, d, q, max(rel(sb[k], st[k]) for k in keys), max(rel(sb[k], sc[k]) for k in keys),
             np.abs(eb - ref).max() / np.abs(ref).sum(), np.abs(eb - ec).max() / np.abs(ec).sum()))
    for k in keys:
        _close(sb[k], st[k], "switched sweeps vs oracle: " + k)
        _close(sb[k], sc[k], "switched sweeps vs the column-owning sweep: " + k)
    assert np.all(np.abs(eb - ref) <= RTOL * np.abs(ref).sum()), (eb, ref)
    assert np.all(np.abs(eb - ec) <= 1e-10 * np.abs(ec).sum()), (eb, ec)


@pytest.mark.parametrize("N,d,q", [(300, 20, 4), (1000, 64, 16), (77, 33, 17), (5000, 256, 16), (16, 3, 1), (17, 250, 31)])
def test_stagewise_vs_oracle(N, d, q):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    init, pri = G.pca_problem(N, d, q, seed=1000 + N + d)
    st = P.make_state(init, pri, N, d, q)
    b = PCABatch.from_problem(init, pri)
    for it in range(2):
        tag = "it%d " % it
        P.update_W(st, pri); b.update_W()
        _close(b.get_state()["W_mean"], st["W_mean"], tag + "W after update_W")
        P.update_Z(st, pri); b.update_Z()
        _close(b.get_state()["Z"], st["Z"], tag + "Z after update_Z")
        P.update_X(st, pri, 0, 1); b.update_X(0, 1)
        P.update_Mu(st, pri); b.update_Mu()
        _close(b.get_state()["Mu_mean"], st["Mu_mean"], tag + "Mu after update_Mu")
        P.update_X(st, pri, 1, N); b.update_X(1, N)
        _close(b.get_state()["X"], st["X"], tag + "X after imputation")
        P.update_Beta(st, pri); b.update_Beta()
        _compare(b, st, tag)
        ref = P.elbo_parts(st, pri)
        got = b.elbo()
        assert np.all(np.abs(got - ref) <= RTOL * np.abs(ref).sum()), (got, ref)
    b.close()


@pytest.mark.parametrize("order", ["Z r", "Z X0 r", "Z Z r", "Z X0 Mu Xpart r X r", "Z W r X r", "Z X0 Z X r", "Z Beta r", "Z X0 Mu X Beta W Z elbo X0 r X r"])
def test_a_deferred_z_update_is_carried_out_by_whatever_comes_next(order):
    """pyvb_pca_update_Z only prepares the update (posterior covariance, gains, the sum of z from the sum of x); the rows of Z are
    written by the next sweep over X, or by the first call that reads or replaces them.  Every continuation must give what the
    reference's order of node updates gives: checked against the oracle after each read ("r")."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 150, 40, 5
    init, pri = G.pca_problem(N, d, q, seed=99)
    st = P.make_state(init, pri, N, d, q)
    b = PCABatch.from_problem(init, pri)
    P.update_W(st, pri); b.update_W()
    for op in order.split():
        if op == "Z": P.update_Z(st, pri); b.update_Z()
        elif op == "X0": P.update_X(st, pri, 0, 1); b.update_X(0, 1)
        elif op == "Mu": P.update_Mu(st, pri); b.update_Mu()
        elif op == "Xpart": P.update_X(st, pri, 20, 97); b.update_X(20, 97)
        elif op == "X": P.update_X(st, pri, 1, N); b.update_X(1, N)
        elif op == "W": P.update_W(st, pri); b.update_W()
        elif op == "Beta": P.update_Beta(st, pri); b.update_Beta()
        elif op == "elbo":
            ref, got = P.elbo_parts(st, pri), b.elbo()
            assert np.all(np.abs(got - ref) <= RTOL * np.abs(ref).sum()), (got, ref)
        else:
            _compare(b, st, order + ": ")
    _compare(b, st, order + " (end): ")
    b.close()


def test_iterate_equals_individual_calls():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 400, 24, 5
    init, pri = G.pca_problem(N, d, q, seed=5)
    a, b = PCABatch.from_problem(init, pri), PCABatch.from_problem(init, pri)
    a.iterate(3)
    for _ in range(3):
        b.update_W(); b.update_Z(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, N); b.update_Beta()
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(a.elbo(), b.elbo())
    a.close(); b.close()


def test_single_rank_communicator_is_transparent():
    """With a one-rank RCCL communicator attached every statistics exchange goes through ncclAllReduce
    (sum over one rank = identity): the results must not change."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    from pyvb_amd.lds import LDSBatch
    N, d, q = 500, 40, 6
    init, pri = G.pca_problem(N, d, q, seed=77)
    a = PCABatch.from_problem(init, pri)
    b = PCABatch(N, d, q)
    b.comm_init(LDSBatch.comm_unique_id(), 0, 1)
    b.set_priors(pri)
    b.set_data(np.where(init["obs"], init["X"], np.nan))
    b.set_state(X_missing=init["X"], W_mean=init["W_mean"], Z=init["Z"], Z_cov=init["Z_cov"], Mu_mean=init["Mu_mean"], beta_b=float(init["beta_b"]))
    a.iterate(3); b.iterate(3)
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.array_equal(a.elbo(), b.elbo())
    a.close(); b.close()


def test_baseline_config5_full_size_on_one_gpu():
    """BASELINE configs[4] at its full size on one GPU: N = 10^6 rows x d = 256, q = 16, Bernoulli(0.1) mask -- one
    Network.learn iteration against the oracle (about a minute of numpy), then a size-independent property: the rows
    after the first can be permuted without changing the posteriors of W, Mu and Beta (sums over n in another order)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    from pyvb_amd.pca import PCABatch
    N, d, q = 1000000, 256, 16
    init, pri = G.pca_problem(N, d, q, seed=2024, p_missing=0.1)
    st = P.make_state(init, pri, N, d, q)
    ref = P.iterate(st, pri)
    b = PCABatch.from_problem(init, pri)
    b.iterate(1)
    got = b.elbo()
    g = b.get_state()
    for k in ("W_mean", "W_var", "Z_cov", "Mu_mean", "Mu_var", "beta_a", "beta_b"):
        _close(g[k], st[k], "N = 10^6: " + k)
    _close(g["Z"][:2000], st["Z"][:2000], "N = 10^6: Z (first rows)")
    _close(g["X"][-2000:], st["X"][-2000:], "N = 10^6: X (last rows)")
    assert np.all(np.abs(got - ref) <= RTOL * np.abs(ref).sum()), (got, ref)
    b.close()
    del st
    perm = np.concatenate([[0], 1 + np.random.default_rng(0).permutation(N - 1)])
    init2 = {k: (v[perm] if isinstance(v, np.ndarray) and v.shape[:1] == (N,) else v) for k, v in init.items()}
    b2 = PCABatch.from_problem(init2, pri)
    b2.iterate(1)
    g2 = b2.get_state()
    for k in ("W_mean", "W_var", "Z_cov", "Mu_mean", "Mu_var", "beta_b"):
        _close(g2[k], g[k], "row permutation: " + k, 1e-10)
    _close(g2["Z"][:100], g["Z"][perm[:100]], "row permutation: Z", 1e-10)
    b2.close()
