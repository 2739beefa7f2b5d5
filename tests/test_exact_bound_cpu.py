"""CPU: the numpy restatement of the exact lower bound (tests/exact_bound_ref.py) against an independent Monte Carlo estimate of
E_q[ln p(Y, .) - ln q(.)], and its behaviour on the oracle's coordinate-ascent loop (it must not decrease)."""
import numpy as np
import pytest
from scipy.special import gammaln

import exact_bound_ref as XR
from oracle import lds_closed_form as O
from pyvb_amd import synth

LN2PI = O.LN2PI


def _normal_lp(x, mean, prec):
    """ln N(x; mean, 1/prec), elementwise."""
    return 0.5 * np.log(prec) - 0.5 * LN2PI - 0.5 * prec * (x - mean) ** 2


def _gamma_lp(x, a, b):
    return a * np.log(b) - gammaln(a) + (a - 1.0) * np.log(x) - b * x


def _mvn_lp(x, mean, cov):
    """ln N(x; mean, cov) for samples x [S, m]."""
    L = np.linalg.cholesky(cov)
    z = np.linalg.solve(L, (x - mean).T)
    return -0.5 * x.shape[1] * LN2PI - np.log(np.diag(L)).sum() - 0.5 * (z * z).sum(axis=0)


def _mc_elbo(st, pri, Y, S, rng):
    """Monte Carlo estimate of E_q[ln p - ln q] for replicate 0 of the LDS graph with Gamma-family noise (mean, standard
    error).  q: X_t ~ N(X[t], Sigma of its class), columns ~ N(mean, cov) (known entries fixed), Q, R ~ Gamma, the outputs
    with missing entries ~ N(Yq, diag Yvar) on those entries."""
    kind = pri["noise"]
    T, D = st["X"].shape[1:]
    K = st["C_mean"].shape[1]
    lp = np.zeros(S)
    lq = np.zeros(S)
    # X_t
    X = np.empty((S, T, D))
    for t in range(T):
        c = 0 if t == 0 else (2 if t == T - 1 else 1)
        X[:, t] = rng.multivariate_normal(st["X"][0, t], st["Sigma"][0, c], size=S)
        lq += _mvn_lp(X[:, t], st["X"][0, t], st["Sigma"][0, c])
    lp += _mvn_lp(X[:, 0], pri["x0_mean"], np.linalg.inv(pri["x0_prec"]))

    def columns(which, rows):
        M, Mcov, pm, pp = st[which + "_mean"][0], st[which + "_cov"][0], pri[which + "_prior_mean"], pri[which + "_prior_prec"]
        obs = pri.get(which + "_obs")
        W = np.empty((S, rows, D))
        out_p, out_q = np.zeros(S), np.zeros(S)
        for i in range(D):
            known = np.zeros(rows, dtype=bool) if obs is None else ~np.isnan(obs[:, i])
            col = np.empty((S, rows))
            col[:, known] = obs[known, i] if known.any() else 0.0
            mi = np.nonzero(~known)[0]
            if len(mi):
                cm = Mcov[i][np.ix_(mi, mi)]
                col[:, mi] = rng.multivariate_normal(M[mi, i], cm, size=S)
                out_q += _mvn_lp(col[:, mi], M[mi, i], cm)
            out_p += _normal_lp(col, pm[:, i], pp[i]).sum(axis=1)
            W[:, :, i] = col
        return W, out_p, out_q

    A, pa, qa = columns("A", D)
    Cm, pc, qc = columns("C", K)
    lp += pa + pc
    lq += qa + qc

    def noise(which, dim):
        a, b = st[which + "_a"][0], st[which + "_b"][0]
        a0, b0 = pri[which + "_a0"], pri[which + "_b0"]
        if kind == "gamma":
            g = rng.gamma(a, 1.0 / b, size=S)
            return np.repeat(g[:, None], dim, axis=1), _gamma_lp(g, a0, b0), _gamma_lp(g, a, b)
        g = rng.gamma(a, 1.0 / b, size=(S, dim))
        return g, _gamma_lp(g, a0, b0).sum(axis=1), _gamma_lp(g, a, b).sum(axis=1)

    Q, pq, qq = noise("Q", D)
    R, pr, qr = noise("R", K)
    lp += pq + pr
    lq += qq + qr
    # X_t | X_{t-1}, A, Q
    for t in range(1, T):
        lp += _normal_lp(X[:, t], np.einsum("skj,sj->sk", A, X[:, t - 1]), Q).sum(axis=1)
    # Y_t | X_t, C, R; the missing entries drawn from their posterior
    Yo = Y[0]
    for t in range(T):
        y = np.broadcast_to(np.nan_to_num(Yo[t]), (S, K)).copy()
        miss = np.isnan(Yo[t])
        if miss.any():
            mean, var = st["Yq"][0, t, miss], st["Yvar"][0, t, miss]
            y[:, miss] = mean + np.sqrt(var) * rng.standard_normal((S, miss.sum()))
            lq += _normal_lp(y[:, miss], mean, 1.0 / var).sum(axis=1)
        lp += _normal_lp(y, np.einsum("skj,sj->sk", Cm, X[:, t]), R).sum(axis=1)
    v = lp - lq
    return v.mean(), v.std() / np.sqrt(S)


def _run(Y, st0, pri, iters, update_outputs=False):
    T = Y.shape[1]
    st = O.expand_state(st0, pri, T, Y)
    tot = []
    for _ in range(iters):
        if update_outputs:
            O.iterate(st, pri, Y, with_elbo=False)
            O.update_Y(st, pri)
            tot.append(XR.elbo_parts_exact(st, pri, O.statistics(st, Y), T).sum(axis=1))
        else:
            tot.append(XR.iterate_exact(st, pri, Y).sum(axis=1))
    return st, np.array(tot)


def _small(kind, knowns=False, missing=False, seed=5):
    T, D, K = 5, 2, 2
    Y, st0, pri = synth.make_problem(T, D, K, 1, seed=seed)
    Y = Y / 10.0                    # a well-conditioned tiny problem
    pri["noise"] = kind
    pri["A_prior_prec"] = np.full((D, D), 0.5); pri["C_prior_prec"] = np.full((D, K), 0.5)
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(2.0)
    else:
        for k, dim in (("Q_a0", D), ("Q_b0", D), ("R_a0", K), ("R_b0", K)):
            pri[k] = np.full(dim, 2.0)
    if knowns:
        pri["A_obs"] = np.array([[0.5, np.nan], [np.nan, np.nan]])
        pri["C_obs"] = np.array([[np.nan, 1.0], [np.nan, -0.5]])
    if missing:
        Y = Y.copy()
        Y[0, 1, 0] = np.nan             # partially observed row
        Y[0, 3, :] = np.nan             # latent row
        rng = np.random.default_rng(seed)
        st0["Yq"] = rng.standard_normal(Y.shape); st0["Yrowvar"] = np.ones(Y.shape[:2])
    return Y, st0, pri


@pytest.mark.parametrize("kind,knowns,missing", [("diagonal_gamma", False, False), ("gamma", True, True),
                                                 ("diagonal_gamma", True, True)])
def test_restatement_matches_monte_carlo(kind, knowns, missing):
    Y, st0, pri = _small(kind, knowns, missing)
    st, _ = _run(Y, st0, pri, 4, update_outputs=missing)
    T = Y.shape[1]
    S_ = O.statistics(st, Y)
    exact = XR.elbo_parts_exact(st, pri, S_, T)[0].sum()
    ref = O.elbo_parts(st, pri, S_, T)[0].sum()
    mc, se = _mc_elbo(st, pri, Y, 200000, np.random.default_rng(11))
    assert abs(mc - exact) <= 4.0 * se, (mc, se, exact)
    # the reference bound is not this quantity
    assert abs(mc - ref) > 4.0 * se, (mc, se, ref)


@pytest.mark.parametrize("kind,T,D,K", [("diagonal_gamma", 50, 3, 4), ("diagonal_gamma", 40, 5, 3), ("gamma", 50, 3, 4),
                                        ("gamma", 40, 5, 3)])
def test_exact_bound_never_decreases_on_the_oracle_loop(kind, T, D, K):
    Y, st0, pri = synth.make_problem(T, D, K, 2, seed=41 + T + D)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    _, tot = _run(Y, st0, pri, 30)
    steps = np.diff(tot, axis=0)
    assert np.all(steps >= -1e-9 * np.abs(tot[1:])), steps.min()


def test_exact_bound_never_decreases_with_known_entries():
    T, D, K = 40, 4, 5
    Y, st0, pri = synth.make_problem(T, D, K, 2, seed=77)
    rng = np.random.default_rng(3)
    pri["A_obs"] = np.where(rng.random((D, D)) < 0.3, 0.3 * rng.standard_normal((D, D)), np.nan)
    pri["C_obs"] = np.where(rng.random((K, D)) < 0.2, rng.standard_normal((K, D)), np.nan)
    pri["A_obs"][:, 1] = 0.2                # a fully known column
    _, tot = _run(Y, st0, pri, 30)
    steps = np.diff(tot, axis=0)
    assert np.all(steps >= -1e-9 * np.abs(tot[1:])), steps.min()


@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_exact_bound_never_decreases_with_missing_outputs(kind):
    T, D, K, N = 40, 3, 4, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=91)
    rng = np.random.default_rng(4)
    Y = np.where(rng.random(Y.shape) < 0.15, np.nan, Y)
    Y[:, 5] = np.nan
    st0["Yq"] = rng.standard_normal(Y.shape); st0["Yrowvar"] = np.ones((N, T))
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    _, tot = _run(Y, st0, pri, 30, update_outputs=True)
    steps = np.diff(tot, axis=0)
    assert np.all(steps >= -1e-9 * np.abs(tot[1:])), steps.min()


def test_logdets_restatement_is_the_covariances_log_determinant():
    Y, st0, pri = _small("diagonal_gamma", missing=True)
    st, _ = _run(Y, st0, pri, 2, update_outputs=True)
    ld = XR.logdets(st, pri)
    np.testing.assert_allclose(ld["X"], -1.0 / st["qld_x"], rtol=1e-10)
    np.testing.assert_allclose(ld["A"], -1.0 / st["qld_A"], rtol=1e-10)
    lat = np.isnan(Y[0]).all(axis=1)
    np.testing.assert_allclose(ld["Y"][0, lat], np.log(st["Yvar"][0, lat]).sum(axis=1), rtol=1e-12)


# ---- VB-PCA with missing data (oracle/pca_closed_form.py) ---------------------------------------------------------------------
def _pca_small(N=8, d=4, q=2, seed=3):
    from oracle import pca_closed_form as P
    init, pri = synth.pca_problem(N, d, q, seed)
    init["obs"] = init["obs"].copy()
    init["obs"][1, 0] = False               # a partially observed row
    init["obs"][2, :] = False               # a latent row
    init["X"] = np.where(init["obs"], init["X"], 0.0)
    pri["W_prior_prec"] = np.full((q, d), 0.5); pri["Mu_prior_prec"] = np.full(d, 0.5)
    pri["beta_a0"], pri["beta_b0"] = 2.0, 2.0
    st = P.make_state(init, pri, N, d, q)
    for _ in range(4):
        P.iterate(st, pri)
    return st, pri


def _pca_mc(st, pri, S, rng):
    N, d = st["X"].shape
    q = st["Z"].shape[1]
    lp, lq = np.zeros(S), np.zeros(S)
    W = st["W_mean"][None] + np.sqrt(st["W_var"].T)[None] * rng.standard_normal((S, d, q))
    lp += _normal_lp(W, pri["W_prior_mean"][None], pri["W_prior_prec"].T[None]).sum(axis=(1, 2))
    lq += _normal_lp(W, st["W_mean"][None], 1.0 / st["W_var"].T[None]).sum(axis=(1, 2))
    Mu = st["Mu_mean"][None] + np.sqrt(st["Mu_var"])[None] * rng.standard_normal((S, d))
    lp += _normal_lp(Mu, pri["Mu_prior_mean"][None], pri["Mu_prior_prec"][None]).sum(axis=1)
    lq += _normal_lp(Mu, st["Mu_mean"][None], 1.0 / st["Mu_var"][None]).sum(axis=1)
    a, b = st["beta_a"], st["beta_b"]
    beta = rng.gamma(a, 1.0 / b, size=S)
    lp += _gamma_lp(beta, pri["beta_a0"], pri["beta_b0"])
    lq += _gamma_lp(beta, a, b)
    for n in range(N):
        z = rng.multivariate_normal(st["Z"][n], st["Z_cov"], size=S)
        lp += _normal_lp(z, 0.0, 1.0).sum(axis=1)
        lq += _mvn_lp(z, st["Z"][n], st["Z_cov"])
        x = np.broadcast_to(st["X"][n], (S, d)).copy()
        miss = ~st["obs"][n]
        if miss.any():
            var = st["X_var"][n, miss]
            x[:, miss] = st["X"][n, miss] + np.sqrt(var) * rng.standard_normal((S, miss.sum()))
            lq += _normal_lp(x[:, miss], st["X"][n, miss], 1.0 / var).sum(axis=1)
        mean = np.einsum("skj,sj->sk", W, z) + Mu
        lp += _normal_lp(x, mean, beta[:, None]).sum(axis=1)
    v = lp - lq
    return v.mean(), v.std() / np.sqrt(S)


def test_pca_restatement_matches_monte_carlo():
    from oracle import pca_closed_form as P
    st, pri = _pca_small()
    exact = XR.pca_elbo_parts_exact(st, pri).sum()
    ref = P.elbo_parts(st, pri).sum()
    mc, se = _pca_mc(st, pri, 200000, np.random.default_rng(12))
    assert abs(mc - exact) <= 4.0 * se, (mc, se, exact)
    assert abs(mc - ref) > 4.0 * se, (mc, se, ref)


@pytest.mark.parametrize("N,d,q", [(300, 12, 3), (500, 20, 5)])
def test_pca_exact_bound_never_decreases_on_the_oracle_loop(N, d, q):
    from oracle import pca_closed_form as P
    init, pri = synth.pca_problem(N, d, q, 5)
    init["obs"] = init["obs"].copy(); init["obs"][3, :] = False
    init["X"] = np.where(init["obs"], init["X"], 0.0)
    st = P.make_state(init, pri, N, d, q)
    L = []
    for _ in range(40):
        P.iterate(st, pri)
        L.append(XR.pca_elbo_parts_exact(st, pri).sum())
    steps = np.diff(L)
    assert np.all(steps >= -1e-9 * np.abs(np.array(L[1:]))), steps.min()
