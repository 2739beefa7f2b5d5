"""GPU: the exact lower bound of the fused LDS path (pyvb_lds_set_bound_mode(PYVB_BOUND_EXACT)) against the numpy restatement
(tests/exact_bound_ref.py), the stored log-determinants against slogdet, reference mode untouched by the new mode, and the
exact bound's monotonicity over pyvb_lds_iterate.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import exact_bound_ref as XR
from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-8


def _batch(Y, st0, pri):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri)


def _gamma(pri):
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)


def _wishart(pri, D, K):
    rng = np.random.default_rng(D + K)
    pri["noise"] = "wishart"
    W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
    W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)


def _case(name):
    """(Y, st0, pri, update_outputs) of one class the fused paths serve."""
    if name == "d64":
        Y, st0, pri = synth.make_problem(6, 64, 64, 2, seed=801)
    elif name == "d96":
        Y, st0, pri = synth.make_problem(5, 96, 96, 2, seed=802)
    elif name == "d128_gamma":
        Y, st0, pri = synth.make_problem(4, 128, 128, 1, seed=803)
        _gamma(pri)
        pri["A_prior_prec"] = np.full_like(pri["A_prior_prec"], 1e-2); pri["C_prior_prec"] = np.full_like(pri["C_prior_prec"], 1e-2)
    elif name == "gamma":
        Y, st0, pri = synth.make_problem(40, 5, 6, 2, seed=804)
        _gamma(pri)
    elif name in ("wishart8", "wishart72"):
        D = 8 if name == "wishart8" else 72
        Y, st0, pri = synth.make_problem(30 if D == 8 else 5, D, D, 2, seed=805 + D)
        _wishart(pri, D, D)
    elif name in ("knowns", "knowns_d70"):
        D, K = (6, 7) if name == "knowns" else (70, 66)
        Y, st0, pri = synth.make_problem(30 if D < 64 else 4, D, K, 2, seed=806 + D)
        rng = np.random.default_rng(D)
        A_obs = np.where(rng.random((D, D)) < 0.2, 0.3 * rng.standard_normal((D, D)), np.nan)
        C_obs = np.where(rng.random((K, D)) < 0.2, rng.standard_normal((K, D)), np.nan)
        A_obs[:, 1] = 0.1
        C_obs[:, 0] = np.nan
        pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    elif name in ("missing", "missing_d70"):
        T, D, K, N = (40, 5, 6, 2) if name == "missing" else (4, 70, 66, 1)
        Y, st0, pri = synth.make_problem(T, D, K, N, seed=807 + D)
        rng = np.random.default_rng(T + K)
        mask = rng.random((N, T, K)) < 0.15
        mask[:, 1] = True; mask[:, 3] = False
        Y = np.where(mask, np.nan, Y)
        st0["Yq"] = rng.standard_normal((N, T, K)); st0["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, T))
        return Y, st0, pri, True
    elif name == "wishart_missing":
        Y, st0, pri = synth.make_problem(30, 6, 9, 2, seed=808)
        _wishart(pri, 6, 9)
        rng = np.random.default_rng(9)
        Y = np.where(rng.random(Y.shape) < 0.2, np.nan, Y)
        Y[:, 2] = np.nan
        st0["Yq"] = np.where(np.isnan(Y), rng.standard_normal(Y.shape), Y); st0["Yrowvar"] = np.ones(Y.shape[:2])
        return Y, st0, pri, True
    else:
        raise KeyError(name)
    return Y, st0, pri, False


def _parts_close(got, want, what):
    """every part to 1e-8 of its own magnitude (floor 1)"""
    assert np.all(np.isfinite(got)), what + ": non-finite"
    assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "%s\n%r\n%r" % (what, got, want)


CASES = ["d64", "d96", "d128_gamma", "gamma", "wishart8", "wishart72", "knowns", "knowns_d70", "missing", "missing_d70",
         "wishart_missing"]


@pytest.mark.parametrize("name", CASES)
def test_exact_parts_match_the_restatement(name):
    Y, st0, pri, upd = _case(name)
    T = Y.shape[1]
    b = _batch(Y, st0, pri)
    b.set_bound_mode("exact")
    st = O.expand_state(st0, pri, T, Y)
    done = 0
    for k in (1, 2, 5):
        while done < k:
            O.iterate(st, pri, Y, with_elbo=False)
            b.iterate(1)
            if upd:
                O.update_Y(st, pri); b.update_Y()
            done += 1
        want = XR.elbo_parts_exact(st, pri, O.statistics(st, Y), T)
        _parts_close(b.elbo(), want, "%s after %d iterations" % (name, k))
        # the log-determinants the exact parts were formed from: against slogdet of the handle's own covariances (1e-10), and
        # against the restatement's (whose inversions at 1e-3 prior precisions lose more than that)
        ld, ref = b.get_logdets(), XR.logdets(st, pri)
        cls = [0, 1, 2] if T > 2 else [0, 2]
        Sig, _ = b.get_posterior_classes()
        np.testing.assert_allclose(ld["X"][:, cls], np.linalg.slogdet(Sig[:, cls])[1], rtol=1e-10, err_msg="lnd_x")
        np.testing.assert_allclose(ld["X"][:, cls], ref["X"][:, cls], rtol=1e-8, err_msg="lnd_x")
        if b.noise == "wishart":
            Ac, Cc = b.get_column_cov()
            own = {"A": np.linalg.slogdet(Ac)[1], "C": np.linalg.slogdet(Cc)[1]}
        else:
            g = b.get_state(("A_colvar", "C_colvar"))
            with np.errstate(divide="ignore"):         # known entries have variance 0 (those columns are not compared)
                own = {"A": np.log(g["A_colvar"]).sum(axis=2), "C": np.log(g["C_colvar"]).sum(axis=2)}
        for w in ("A", "C"):
            ok = np.isfinite(ref[w])
            np.testing.assert_allclose(ld[w][ok], own[w][ok], rtol=1e-10, err_msg="lnd_" + w)
            np.testing.assert_allclose(ld[w][ok], ref[w][ok], rtol=1e-8, err_msg="lnd_" + w)
        if upd:
            ok = np.isfinite(ref["Y"])
            np.testing.assert_allclose(ld["Y"][ok], ref["Y"][ok], rtol=1e-10, err_msg="Ylnd")
            assert np.array_equal(np.isnan(ld["Y"]), np.isnan(b.get_outputs(with_qld=True)[2]))
    b.close()


def test_logdets_are_nan_before_the_first_update_and_mode_is_checked():
    Y, st0, pri = synth.make_problem(8, 4, 5, 2, seed=810)
    b = _batch(Y, st0, pri)
    ld = b.get_logdets()
    assert np.isnan(ld["X"]).all() and np.isnan(ld["A"]).all() and np.isnan(ld["C"]).all() and np.isnan(ld["Y"]).all()
    from pyvb_amd import _capi as C
    assert C.lib.pyvb_lds_set_bound_mode(b._h, 2) == C.E_ARG
    with pytest.raises(ValueError):
        b.set_bound_mode("approximate")
    b.close()


@pytest.mark.parametrize("name", ["d64", "d96", "knowns", "missing", "wishart8"])
def test_reference_mode_is_unchanged(name):
    """A handle switched exact -> reference gives the reference parts of one never switched, bit for bit; the state after k
    iterations does not depend on the mode."""
    Y, st0, pri, upd = _case(name)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    b.set_bound_mode("exact")
    for _ in range(3):
        a.iterate(1); b.iterate(1)
        if upd:
            a.update_Y(); b.update_Y()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    ea = a.elbo()
    b.set_bound_mode("reference")
    assert np.array_equal(b.elbo(), ea, equal_nan=True)
    a.iterate(1); b.iterate(1)
    assert np.array_equal(a.elbo_history()[-1], b.elbo_history()[-1], equal_nan=True)
    assert len(b.elbo_history()) == 1           # the mode change emptied the history
    a.close(); b.close()


@pytest.mark.parametrize("T,D,K,N", [(200, 64, 64, 2), (60, 100, 128, 1)])
def test_exact_bound_is_monotone_over_iterate(T, D, K, N):
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=900 + D)
    if max(D, K) > 102:
        pri["A_prior_prec"] = np.full_like(pri["A_prior_prec"], 1e-2); pri["C_prior_prec"] = np.full_like(pri["C_prior_prec"], 1e-2)
    b = _batch(Y, st0, pri)
    b.set_bound_mode("exact")
    b.iterate(50)
    L = b.elbo_history().sum(axis=1)
    assert len(L) == 50 and np.all(np.isfinite(L))
    steps = np.diff(L)
    assert np.all(steps >= -1e-9 * np.abs(L[1:])), steps.min()
    b.close()


def test_logdets_of_covariances_set_by_the_caller():
    """pyvb_lds_set_posterior_classes: ln det of the given covariances, read before any sweep, and the exact L_X formed with it."""
    T, D, K, N = 10, 5, 6, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=811)
    rng = np.random.default_rng(5)
    G = rng.standard_normal((N, 3, D, D))
    Sig = np.einsum("ncij,nckj->ncik", G, G) / D + 0.5 * np.eye(D)
    qld = 0.5 / (0.5 * np.linalg.slogdet(np.linalg.inv(Sig))[1])
    b = _batch(Y, st0, pri)
    b.set_posterior_classes(Sig, qld)
    np.testing.assert_allclose(b.get_logdets()["X"], np.linalg.slogdet(Sig)[1], rtol=1e-10)
    b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    st = O.expand_state(st0, pri, T)
    st["Sigma"], st["qld_x"] = Sig.copy(), qld.copy()
    S = O.statistics(st, Y)
    O.update_A(st, pri, S); O.update_C(st, pri, S); O.update_Q(st, pri, S, T); O.update_R(st, pri, S, T)
    ref = b.elbo()
    b.set_bound_mode("exact")
    _parts_close(b.elbo(), XR.elbo_parts_exact(st, pri, S, T), "exact parts before any sweep")
    _parts_close(ref, O.elbo_parts(st, pri, S, T), "reference parts before any sweep")
    b.close()


# ---- VB-PCA -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,q,lazy", [(3000, 40, 8, True), (2000, 70, 32, False), (1500, 24, 8, False)])
def test_pca_exact_parts_and_logdets(N, d, q, lazy):
    from oracle import pca_closed_form as P
    from pyvb_amd.pca import PCABatch
    init, pri = synth.pca_problem(N, d, q, 17 + q)
    init["obs"] = init["obs"].copy(); init["obs"][5, :] = False; init["obs"][N - 2, :] = False
    init["X"] = np.where(init["obs"], init["X"], 0.0)
    b = PCABatch.from_problem(init, pri)
    b.set_bound_mode("exact")
    st = P.make_state(init, pri, N, d, q)
    done = 0
    for k in (1, 2, 5):
        while done < k:
            P.iterate(st, pri)
            if lazy:
                b.iterate(1)            # the crawl order with the Z update deferred into the pass over the rows
            else:
                b.update_W(); b.update_Z(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, N); b.update_Beta(); b.elbo()
            done += 1
        got, want = b.elbo(), XR.pca_elbo_parts_exact(st, pri)
        _parts_close(got[None], want[None], "PCA N=%d d=%d q=%d after %d iterations" % (N, d, q, k))
        ld, ref = b.get_logdets(), XR.pca_logdets(st)
        g = b.get_state()
        np.testing.assert_allclose(ld["W"], np.log(g["W_var"]).sum(axis=1), rtol=1e-10)
        np.testing.assert_allclose(ld["Z"], np.linalg.slogdet(g["Z_cov"])[1], rtol=1e-10)
        np.testing.assert_allclose(ld["Mu"], np.log(g["Mu_var"]).sum(), rtol=1e-10)
        np.testing.assert_allclose(ld["W"], ref["W"], rtol=1e-8)
        assert np.array_equal(np.isnan(ld["X"]), np.isnan(ref["X"]))
        ok = np.isfinite(ref["X"])
        np.testing.assert_allclose(ld["X"][ok], ref["X"][ok], rtol=1e-10)
    b.set_bound_mode("reference")
    want_ref = P.elbo_parts(st, pri)
    _parts_close(b.elbo()[None], want_ref[None], "PCA reference parts after a switch back")
    b.close()


def test_pca_exact_bound_is_monotone_and_reference_state_unchanged():
    from pyvb_amd.pca import PCABatch
    init, pri = synth.pca_problem(4000, 30, 8, 23)
    a, b = PCABatch.from_problem(init, pri), PCABatch.from_problem(init, pri)
    b.set_bound_mode("exact")
    L = []
    for _ in range(50):
        a.iterate(1); b.iterate(1)
        L.append(b.elbo().sum())
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    ea = a.elbo()
    b.set_bound_mode("reference")
    assert np.array_equal(b.elbo(), ea)
    L = np.array(L)
    assert np.all(np.diff(L) >= -1e-9 * np.abs(L[1:])), np.diff(L).min()
    a.close(); b.close()


# ---- node API ---------------------------------------------------------------------------------------------------------------
def _example_graph(seed=11, T=40, D=3, K=4):
    import importlib.util
    import os
    from pyvb_amd import nodes
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    Y, st0, pri = synth.make_problem(T, D, K, 1, seed)
    g = G.build_graph(nodes, Y[0], pri, st0)
    return Y, st0, pri, g


def test_network_learn_exact_bound():
    """Network.learn(..., bound="exact") on the example's graph: non-decreasing, the LDSBatch exact total, and the same graph
    forced node by node; the default call is the reference bound as before."""
    from pyvb_amd.network import Network
    from pyvb_amd import nodes
    iters = 12
    Y, st0, pri, g = _example_graph()
    order = g["Xs"] + g["Ys"] + g["As"] + g["Cs"] + [g["Q"], g["R"]]
    hist = []
    net = Network(order)
    for _ in range(iters):
        net.learn(1, tol=-np.inf, verbose=False, bound="exact")
        hist.append(net.llb)
    hist = np.array(hist)
    assert np.all(np.diff(hist) >= -1e-9 * np.abs(hist[1:])), np.diff(hist)
    # the same loop (forward sweep, A, C, Q, R) on an LDSBatch in exact mode
    b = _batch(Y, st0, pri)
    b.set_bound_mode("exact")
    for _ in range(iters):
        b.sweep("forward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    tot = b.elbo().sum()
    assert abs(net.llb - tot) <= RTOL * abs(tot), (net.llb, tot)
    # node by node: the sum of the nodes' exact terms from the generic tape path on a mirror of the same state
    plan = nodes._plan_of(g["Xs"][0])
    terms = sum(plan.mirror().node_llb(n, "exact") for n in order)
    assert abs(terms - tot) <= RTOL * abs(tot), (terms, tot)
    assert abs(sum(n.log_lower_bound(bound="exact") for n in order) - tot) <= RTOL * abs(tot)
    # reference mode: the default learn() gives what it gave before
    Y2, st02, pri2, g2 = _example_graph()
    net2 = Network(g2["Xs"] + g2["Ys"] + g2["As"] + g2["Cs"] + [g2["Q"], g2["R"]])
    net2.learn(iters, tol=-np.inf, verbose=False)
    b2 = _batch(Y2, st02, pri2)
    for _ in range(iters):
        b2.sweep("forward"); b2.update_A(); b2.update_C(); b2.update_Q(); b2.update_R()
    ref = b2.elbo().sum()
    assert abs(net2.llb - ref) <= RTOL * abs(ref)
    b.close(); b2.close()
