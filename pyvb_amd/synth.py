"""Synthetic linear-dynamical-system data and initial variational state.

Follows the simulator of the reference's LDS example
(examples/Linear_Dynamic_System.py:20-44) with the two changes SURVEY.md §8(d)
states: seeded generators instead of the global numpy stream, and a rescaled
transition matrix instead of the rejection loop at :20-23 (which does not
terminate for latent dimension >~6).

Everything here is host-side numpy; it only produces inputs.
"""
import numpy as np

__all__ = ["simulate_lds", "initial_state", "default_priors", "make_problem", "simulate_driven_lds", "make_input_problem",
           "make_regression_problem"]


def simulate_lds(T, D, K, N=1, seed=20240):
    """Draw N independent LDS data sets.

    x_t = A x_{t-1} + Q^{1/2} eps,   y_t = C x_t + R^{1/2} eta
    (Linear_Dynamic_System.py:40-44), A rescaled to spectral radius 0.9,
    C = 10*randn (:25), Q, R = 0.1*diag(U(0,1)) (:29, :34), x_0 ~ N(0, I) (:40).

    Returns dict with Y [N,T,K] and the true parameters.
    """
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, D, D))
    rad = np.max(np.abs(np.linalg.eigvals(A)), axis=-1)
    A *= (0.9 / rad)[:, None, None]
    C = 10.0 * rng.standard_normal((N, K, D))
    Rd = 0.1 * rng.random((N, K))
    Qd = 0.1 * rng.random((N, D))
    sq, sr = np.sqrt(Qd), np.sqrt(Rd)
    X = np.empty((N, T, D))
    Y = np.empty((N, T, K))
    x = rng.standard_normal((N, D))
    for t in range(T):
        if t > 0:
            x = np.einsum("nij,nj->ni", A, x) + sq * rng.standard_normal((N, D))
        X[:, t] = x
        Y[:, t] = np.einsum("nkj,nj->nk", C, x) + sr * rng.standard_normal((N, K))
    return {"Y": Y, "X": X, "A": A, "C": C, "Q": Qd, "R": Rd}


def initial_state(T, D, K, N=1, seed=1):
    """Initial variational state drawn the way the reference's constructors do
    (gaussian.py:70-72: qmu ~ N(0,1), qprec = I*u; nodes_todo.py:177: qb = u),
    but from an explicit generator.

    Column covariances are isotropic (I/u), so only their diagonals are kept:
    A_colvar[n, i, k] is the variance of entry k of column i of A.
    """
    rng = np.random.default_rng(seed)
    st = {
        "X": rng.standard_normal((N, T, D)),
        "A_mean": rng.standard_normal((N, D, D)),       # [row, col]
        "C_mean": rng.standard_normal((N, K, D)),       # [row, col]
        "A_colvar": np.repeat(1.0 / rng.random((N, D, 1)), D, axis=2),  # [col, entry]
        "C_colvar": np.repeat(1.0 / rng.random((N, D, 1)), K, axis=2),  # [col, entry]
        "Q_b": np.repeat(rng.random((N, 1)), D, axis=1),
        "R_b": np.repeat(rng.random((N, 1)), K, axis=1),
    }
    return st


def default_priors(D, K):
    """Priors of the example (Linear_Dynamic_System.py:47-58)."""
    return {
        "x0_mean": np.zeros(D),
        "x0_prec": np.eye(D),
        "A_prior_mean": np.zeros((D, D)),        # [row, col]
        "A_prior_prec": np.full((D, D), 1e-3),   # [col, entry] diagonal of each column's prior precision
        "C_prior_mean": np.zeros((K, D)),
        "C_prior_prec": np.full((D, K), 1e-3),
        "Q_a0": np.full(D, 1e-3), "Q_b0": np.full(D, 1e-3),
        "R_a0": np.full(K, 1e-3), "R_b0": np.full(K, 1e-3),
        "noise": "diagonal_gamma",
    }


def make_problem(T, D, K, N=1, seed=20240):
    """Data + initial state + priors for N replicates (one generator per call)."""
    sim = simulate_lds(T, D, K, N, seed)
    st = initial_state(T, D, K, N, seed + 7919)
    return sim["Y"], st, default_priors(D, K)


def simulate_driven_lds(T, D, K, P, N=1, seed=20240):
    """simulate_lds with a known input: x_t = A x_{t-1} + B u_t + Q^{1/2} eps for t >= 1, B = randn [N, D, P], and u_t a
    sum of a slow sinusoid per channel and white noise (an actuator log: persistent, but exciting every direction).  Row 0 of
    U drives nothing (x_0 ~ N(0, I)) and is zero.  Returns dict with Y [N,T,K], U [N,T,P] and the true parameters."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((N, D, D))
    rad = np.max(np.abs(np.linalg.eigvals(A)), axis=-1)
    A *= (0.9 / rad)[:, None, None]
    B = rng.standard_normal((N, D, P))
    C = 10.0 * rng.standard_normal((N, K, D))
    Rd = 0.1 * rng.random((N, K))
    Qd = 0.1 * rng.random((N, D))
    sq, sr = np.sqrt(Qd), np.sqrt(Rd)
    phase, period = rng.random((N, 1, P)), 8.0 + 24.0 * rng.random((N, 1, P))
    U = np.sin(2.0 * np.pi * (np.arange(T)[None, :, None] / period + phase)) + 0.5 * rng.standard_normal((N, T, P))
    U[:, 0] = 0.0
    X = np.empty((N, T, D))
    Y = np.empty((N, T, K))
    x = rng.standard_normal((N, D))
    for t in range(T):
        if t > 0:
            x = np.einsum("nij,nj->ni", A, x) + np.einsum("nip,np->ni", B, U[:, t]) + sq * rng.standard_normal((N, D))
        X[:, t] = x
        Y[:, t] = np.einsum("nkj,nj->nk", C, x) + sr * rng.standard_normal((N, K))
    return {"Y": Y, "U": U, "X": X, "A": A, "B": B, "C": C, "Q": Qd, "R": Rd}


def make_input_problem(T, D, K, P, N=1, seed=20240):
    """make_problem for the input-driven graph X_t = Gaussian(q, A X_{t-1} + B u_t, Q): (Y, U, st0, pri), st0 with B_mean [N, D, P]
    and B_colvar [N, P, D] (column, entry) drawn as the columns of A are, pri with B_prior_mean [D, P] and B_prior_prec [P, D]."""
    sim = simulate_driven_lds(T, D, K, P, N, seed)
    st = initial_state(T, D, K, N, seed + 7919)
    rng = np.random.default_rng(seed + 104729)
    st["B_mean"] = rng.standard_normal((N, D, P))
    st["B_colvar"] = np.repeat(1.0 / rng.random((N, P, 1)), D, axis=2)
    pri = default_priors(D, K)
    pri["B_prior_mean"] = np.zeros((D, P))
    pri["B_prior_prec"] = np.full((P, D), 1e-3)
    return sim["Y"], sim["U"], st, pri


def make_regression_problem(T, D, K, P, Pv, N=1, seed=20240):
    """make_problem for the graph with known regressors in the output equation, Y_t = Gaussian(K, C X_t + E v_t, R), and P >= 0
    inputs that drive the states: (Y, U, V, st0, pri), U None for P = 0.  V [N, T, Pv]: channel 0 is the constant 1 (an output
    offset), the others a slow sinusoid plus white noise; the simulated outputs carry E v_t with a true E = 3 randn [N, K, Pv].
    st0 has E_mean [N, K, Pv] and E_colvar [N, Pv, K] (column, entry) drawn as those of B are, pri E_prior_mean [K, Pv] and
    E_prior_prec [Pv, K]."""
    if P:
        Y, U, st, pri = make_input_problem(T, D, K, P, N, seed)
    else:
        (Y, st, pri), U = make_problem(T, D, K, N, seed), None
    rng = np.random.default_rng(seed + 1299709)
    E = 3.0 * rng.standard_normal((N, K, Pv))
    phase, period = rng.random((N, 1, Pv)), 8.0 + 24.0 * rng.random((N, 1, Pv))
    V = np.sin(2.0 * np.pi * (np.arange(T)[None, :, None] / period + phase)) + 0.5 * rng.standard_normal((N, T, Pv))
    V[:, :, 0] = 1.0
    Y = Y + np.einsum("nkp,ntp->ntk", E, V)
    st["E_mean"] = rng.standard_normal((N, K, Pv))
    st["E_colvar"] = np.repeat(1.0 / rng.random((N, Pv, 1)), K, axis=2)
    pri["E_prior_mean"] = np.zeros((K, Pv))
    pri["E_prior_prec"] = np.full((Pv, K), 1e-3)
    return Y, U, V, st, pri


def pca_rows(lo, hi, d, q, seed, block=10000):
    """Rows [lo, hi) of the synthetic VB-PCA problem (BASELINE configs[4]: low-rank rows + noise, Bernoulli(0.1) missing
    entries), generated block by block from (seed, block index) so that any row range of any total size is reproducible --
    ranks generate only their own shard.  Returns X, the observation mask, initial latent means, the initial W mean."""
    g = np.random.default_rng(seed)
    W = g.standard_normal((d, q)); mean = g.standard_normal(d); W0 = g.standard_normal((d, q))
    X, obs, Z0 = [], [], []
    for b0 in range(lo // block * block, hi, block):
        r = np.random.default_rng([seed, b0 // block])
        x = r.standard_normal((block, q)) @ W.T + mean + 0.2 * r.standard_normal((block, d))
        o = r.random((block, d)) > 0.1
        z0 = r.standard_normal((block, q))
        a, e = max(lo, b0) - b0, min(hi, b0 + block) - b0
        X.append(x[a:e]); obs.append(o[a:e]); Z0.append(z0[a:e])
    return np.concatenate(X), np.concatenate(obs), np.concatenate(Z0), W0


def pca_problem(N, d, q, seed):
    """(init, pri) for pyvb_amd.pca.PCABatch.from_problem / oracle.pca_closed_form.make_state."""
    X, obs, Z0, W0 = pca_rows(0, N, d, q, seed)
    init = {"obs": obs, "X": np.where(obs, X, 0.0), "W_mean": W0, "Z": Z0, "Z_cov": np.eye(q), "Mu_mean": np.zeros(d), "beta_b": 1.0}
    pri = {"W_prior_mean": np.zeros((d, q)), "W_prior_prec": np.full((q, d), 1e-3), "Mu_prior_mean": np.zeros(d),
           "Mu_prior_prec": np.full(d, 1e-3), "beta_a0": 1e-3, "beta_b0": 1e-3}
    return init, pri
