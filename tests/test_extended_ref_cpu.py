"""CPU: the extended-precision run of the oracles (tests/extended_ref.py, oracle/_xlinalg.py) deserves to be the reference.

  * its inversions leave the residual a long-double inversion may leave;
  * at a tiny shape it agrees with an mpmath evaluation of the same formulas at 40 digits to 1e-17;
  * nothing in it is silently cast down to float64;
  * on every case of the accuracy envelope the float64 oracle stays within CAP = 1e-11 of it (tests/test_envelope_gpu.py
    bounds the kernels by 16 max(e64, n 2^-52), so the cap keeps that bound below 1.6e-10 everywhere).

The lower bound is out of scope: digamma / gammaln exist in float64 only.
"""
import numpy as np
import pytest

import extended_ref as E
from oracle import _xlinalg as XL
from oracle import lds_closed_form as O
from pyvb_amd import synth

LD = np.longdouble


def test_long_double_is_extended_here():
    E.require_extended()
    assert E.to_long({"a": np.ones(3), "m": np.ones(3, dtype=bool), "s": "x", "f": 1.5})["a"].dtype == LD


def _inf_norm(M):
    return np.abs(M).sum(axis=-1).max(axis=-1)


def _check_inverse(Pm, what):
    """|| P inv(P) - I ||_inf <= 64 n 2^-63 kappa_inf(P), for every matrix of the batch"""
    assert Pm.dtype == LD, what
    n = Pm.shape[-1]
    X = XL.inv(Pm)
    assert X.dtype == LD
    res = _inf_norm(Pm @ X - np.eye(n, dtype=LD))
    bound = 64 * n * LD(2.0) ** -63 * _inf_norm(Pm) * _inf_norm(X)
    assert np.all(res <= bound), "%s: residual %r, bound %r" % (what, res, bound)


@pytest.mark.parametrize("name", list(E.LDS_CASES))
def test_inversion_residuals_lds(name):
    for rows, T, n, ext, e64, rec, run in E.lds_reference(name):
        post = O.state_posteriors(run.st, run.pri)
        for c in range(3):
            _check_inverse(post["P"][:, c], "%s: posterior class %d" % (name, c))
        # a column precision of A and one of C (oracle: _update_columns), from the statistics of the last iteration
        for which, Lam, G in (("A", post["Qbar"], run.S["Sxx_m"]), ("C", post["Rbar"], run.S["Sxx"])):
            i = G.shape[-1] // 2
            prec = Lam * G[:, i, i][:, None, None] + np.diag(run.pri[which + "_prior_prec"][i])[None]
            _check_inverse(prec, "%s: precision of column %d of %s" % (name, i, which))


@pytest.mark.parametrize("N,d,q", E.PCA_CASES)
def test_inversion_residuals_pca(N, d, q):
    n, ext, e64, st = E.pca_reference(N, d, q)
    beta = st["beta_a"] / st["beta_b"]
    WtW = st["W_mean"].T @ st["W_mean"]
    WtW[np.diag_indices_from(WtW)] += st["W_var"].sum(1)
    _check_inverse(np.eye(q, dtype=LD) + beta * WtW, "PCA prec")


def test_cholesky_and_slogdet_long_double():
    rng = np.random.default_rng(0)
    W = rng.standard_normal((3, 9, 9))
    A = (W @ np.swapaxes(W, -1, -2) + 9 * np.eye(9)).astype(LD)
    L = XL.cholesky(A)
    assert L.dtype == LD and np.all(np.triu(L, 1) == 0)
    assert E.rel(L @ np.swapaxes(L, -1, -2), A) <= 9 * 2.0 ** -62
    assert E.rel(L, np.linalg.cholesky(A.astype(float))) <= 1e-13
    sign, ld = XL.slogdet(A)
    assert ld.dtype == LD and np.all(sign == 1) and E.rel(ld, np.linalg.slogdet(A.astype(float))[1]) <= 1e-14
    A64 = A.astype(float)           # float64 goes to numpy itself
    assert np.array_equal(XL.inv(A64), np.linalg.inv(A64)) and np.array_equal(XL.cholesky(A64), np.linalg.cholesky(A64))
    assert np.array_equal(XL.slogdet(A64)[1], np.linalg.slogdet(A64)[1])


def test_extended_run_against_mpmath():
    """T = 5, D = 3, K = 2, N = 1, DiagonalGamma noise, one iteration: the formulas of oracle/lds_closed_form.py written out
    below in mpmath at 40 digits; every compared quantity of the long-double run within 1e-17 of them."""
    import mpmath as mp
    mp.mp.dps = 40
    T, D, K = 5, 3, 2
    Y, st0, pri = synth.make_problem(T, D, K, 1, seed=1)
    got = dict(E.lds_trace(E.OracleLDS(E.to_long(Y), E.to_long(st0), E.to_long(pri)), 1, False))

    M = lambda a: mp.matrix(np.asarray(a, dtype=float).tolist())       # float64 -> mpf is exact
    diag = lambda v: mp.diag([v[i] for i in range(len(v))])
    y = [M(Y[0, t]) for t in range(T)]
    x = [M(st0["X"][0, t]) for t in range(T)]
    A, C = M(st0["A_mean"][0]), M(st0["C_mean"][0])
    Av, Cv = M(st0["A_colvar"][0]), M(st0["C_colvar"][0])              # [col, entry]
    qb = M(pri["Q_a0"]); rb = M(pri["R_a0"])
    for k in range(D): qb[k] = (qb[k] + mp.mpf(T - 1) / 2) / mp.mpf(float(st0["Q_b"][0, k]))      # qa = a0 + (T - 1) / 2
    for k in range(K): rb[k] = (rb[k] + mp.mpf(T) / 2) / mp.mpf(float(st0["R_b"][0, k]))          # ra = a0 + T / 2
    Qm, Rm = diag(qb), diag(rb)
    MA = A.T * Qm * A + diag(Av * qb)
    MC = C.T * Rm * C + diag(Cv * rb)
    L0, m0 = M(pri["x0_prec"]), M(pri["x0_mean"])
    Sig = [mp.inverse(L0 + MC + MA), mp.inverse(Qm + MC + MA), mp.inverse(Qm + MC)]

    def step(t):
        m2 = C.T * (Rm * y[t])
        if t < T - 1:
            m2 = m2 + A.T * (Qm * x[t + 1])
        w = (L0 * m0 if t == 0 else Qm * (A * x[t - 1])) + m2
        x[t] = Sig[0 if t == 0 else (1 if t < T - 1 else 2)] * w

    want = {}
    stack = lambda vs: np.array([[[v[i] for i in range(len(v))] for v in vs]], dtype=object)
    for t in range(T): step(t)
    want[(0, "forward sweep", "X")] = stack(x)
    for t in range(T - 1, -1, -1): step(t)
    want[(0, "backward sweep", "X")] = stack(x)
    want[(0, "backward sweep", "Sigma")] = np.array([[s.tolist() for s in Sig]], dtype=object)
    zero = mp.zeros(D, D)
    XX = sum((v * v.T for v in x), zero)
    cov_all = Sig[0] + (T - 2) * Sig[1] + Sig[2]
    Sxx = XX + cov_all
    Sxx_m = XX - x[-1] * x[-1].T + cov_all - Sig[2]
    Sxx_p = XX - x[0] * x[0].T + cov_all - Sig[0]
    Sx1x = sum((x[t] * x[t - 1].T for t in range(1, T)), zero)
    Syx = sum((y[t] * x[t].T for t in range(T)), mp.zeros(K, D))
    Syy = sum((y[t] * y[t].T for t in range(T)), mp.zeros(K, K))

    def columns(Mm, var, pm, pp, Lam, G, H):
        rows = Mm.rows
        for i in range(D):
            prec = Lam * G[i, i] + diag(M(pp[i]))
            Gi = G[i, :].T.copy(); Gi[i] = 0
            w = M(pp[i] * pm[:, i]) + Lam * H[:, i] - Lam * (Mm * Gi)
            cov = mp.inverse(prec)
            mu = cov * w
            for k in range(rows):
                Mm[k, i] = mu[k]; var[i, k] = cov[k, k]

    columns(A, Av, pri["A_prior_mean"], pri["A_prior_prec"], Qm, Sxx_m, Sx1x)
    want[(0, "update_A", "A_mean")] = np.array([A.tolist()], dtype=object)
    columns(C, Cv, pri["C_prior_mean"], pri["C_prior_prec"], Rm, Sxx, Syx)
    want[(0, "update_C", "C_mean")] = np.array([C.tolist()], dtype=object)

    def noise_b(b0, own, Mm, var, G, H):
        E_ = own + Mm * G * Mm.T
        return [mp.mpf(float(b0[k])) + (E_[k, k] + sum(var[i, k] * G[i, i] for i in range(D))) / 2 - (H * Mm.T)[k, k] for k in range(Mm.rows)]

    want[(0, "update_R", "A_colvar")] = np.array([Av.tolist()], dtype=object)
    want[(0, "update_R", "C_colvar")] = np.array([Cv.tolist()], dtype=object)
    want[(0, "update_R", "Q_b")] = np.array([noise_b(pri["Q_b0"], Sxx_p, A, Av, Sxx_m, Sx1x)], dtype=object)
    want[(0, "update_R", "R_b")] = np.array([noise_b(pri["R_b0"], Syy, C, Cv, Sxx, Syx)], dtype=object)

    assert set(want) == set(got)
    for key, ref in want.items():
        g = got[key]
        assert g.dtype == LD and g.shape == ref.shape, key
        # long double -> mpf exactly, through its float64 head and tail
        hi = g.astype(float); lo = (g - hi.astype(LD)).astype(float)
        err = max(abs(mp.mpf(float(h)) + mp.mpf(float(l)) - r) for h, l, r in zip(hi.ravel(), lo.ravel(), ref.ravel()))
        scale = max(abs(r) for r in ref.ravel())
        print("%-40r rel. distance from mpmath %.2e" % (key, float(err / scale)))
        assert err <= mp.mpf("1e-17") * scale, "%r: %s" % (key, mp.nstr(err / scale, 5))


def _all_long(st, what):
    for k, v in st.items():
        if isinstance(v, np.ndarray) and v.dtype.kind != "b":
            assert v.dtype == LD, "%s: %s has dtype %s" % (what, k, v.dtype)
        elif isinstance(v, (float, np.floating)) and not np.isnan(v):
            assert isinstance(v, LD), "%s: %s is a %s" % (what, k, type(v).__name__)


@pytest.mark.parametrize("name", list(E.LDS_CASES))
def test_extended_lds_run_keeps_long_double_and_float64_oracle_is_within_the_cap(name):
    for rows, T, n, ext, e64, rec, run in E.lds_reference(name):
        _all_long(run.st, name)
        _all_long(run.S, name + " statistics")
        assert all(v.dtype == LD for v in ext.values())
        worst = max(e64, key=e64.get)
        print("%s%s: largest e64 %.2e at %r" % (name, "" if rows is None else " replicate %d" % rows, e64[worst], worst))
        for key, e in e64.items():
            assert e <= E.CAP, "%s %r: float64 oracle %.3e from the extended run, cap %.0e" % (name, key, e, E.CAP)


@pytest.mark.parametrize("N,d,q", E.PCA_CASES)
def test_extended_pca_run_keeps_long_double_and_float64_oracle_is_within_the_cap(N, d, q):
    n, ext, e64, st = E.pca_reference(N, d, q)
    _all_long(st, "PCA")
    assert all(v.dtype == LD for v in ext.values())
    worst = max(e64, key=e64.get)
    print("PCA (%d, %d, %d): largest e64 %.2e at %r" % (N, d, q, e64[worst], worst))
    for key, e in e64.items():
        assert e <= E.CAP, "PCA %r: float64 oracle %.3e from the extended run, cap %.0e" % (key, e, E.CAP)


def test_warmup_rule_in_numpy():
    """warmup_rule on matrices whose answer is known: M = r I has ||M^J|| = r^J exactly."""
    for r, want in ((0.5, 60), (0.1, 20), (0.9, 396)):
        M = (r * np.eye(3)).astype(LD)
        J = E.warmup_rule(M, "inf")
        assert J == want and r ** J <= 1e-18 < r ** (J - 4), (r, J)
        assert E.power_norm(M, J, "1") <= 1e-18
    assert E.warmup_rule(np.eye(3, dtype=LD), "inf") == 1 << 30
