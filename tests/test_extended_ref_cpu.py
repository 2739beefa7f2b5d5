"""CPU: the extended-precision run of the oracles (tests/extended_ref.py, oracle/_xlinalg.py) deserves to be the reference.

  * its inversions leave the residual a long-double inversion may leave;
  * at a tiny shape it agrees with an mpmath evaluation of the same formulas at 40 digits to 1e-17;
  * nothing in it is silently cast down to float64;
  * on every case of the accuracy envelope the float64 oracle stays within CAP = 1e-11 of it (tests/test_envelope_gpu.py
    bounds the kernels by 16 max(e64, n 2^-52), so the cap keeps that bound below 1.6e-10 everywhere).

The lower bound is part of it: oracle/_xspecial.py has digamma and gammaln in long double (checked here against mpmath on the
arguments the bounds give them), elbo_parts and elbo_parts_exact keep the dtype (checked at the tiny shape against an mpmath
evaluation of the six parts, both modes, DiagonalGamma and Wishart noise), every part of every case stays within the cap, and
the comparison tests/test_envelope_gpu.py applies to the parts catches three subtle mutants of the bound.
"""
import inspect

import numpy as np
import pytest

import exact_bound_ref as XR
import extended_ref as E
from oracle import _xlinalg as XL
from oracle import _xspecial as XS
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


# ----------------------------------------------------------------------------------------------------------------------------
# the lower bound
# ----------------------------------------------------------------------------------------------------------------------------
def _mpf(v):
    """long double -> mpf exactly, through its float64 head and tail"""
    import mpmath as mp
    v = LD(v)
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


def _mpa(a):
    """array (float64 or long double) -> object array of mpf, exactly"""
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = _mpf(a[idx])
    return out


def test_special_functions_against_mpmath():
    """digamma and gammaln in long double against mpmath at 40 digits, in units of max(1, |f|), on extended_ref.special_grid():
    1e-17, the requirement this file has for the rest of the extended run."""
    import mpmath as mp
    import scipy.special as sp
    mp.mp.dps = 40
    E.require_extended()
    x = E.special_grid()
    assert all(v in x for v in (1e-8, 1e-3, 1e-3 + 0.5, 1e-3 + 36.0, 0.5, 1.0, 1.5, 2.0, E.DIGAMMA_ROOT, 9.999, 10.0, 10.001,
                                4999.5, 7.5e4, 1e5, 1e8, -0.5, -63.5, -64.5, -1000.25))
    xl = x.astype(LD)
    for name, fn, ref, f64 in (("digamma", XS.digamma, mp.digamma, sp.digamma),
                               ("gammaln", XS.gammaln, lambda v: mp.log(abs(mp.gamma(v))), sp.gammaln)):
        got = fn(xl)
        assert got.dtype == LD and got.shape == x.shape
        assert isinstance(fn(LD(2.5)), LD) and fn(LD(2.5)) == fn(np.array([2.5], dtype=LD))[0]
        worst = w64 = (0.0, None)
        for xi, gi, si in zip(x, got, f64(x)):
            want = ref(mp.mpf(float(xi)))
            unit = max(1, abs(want))
            worst = max(worst, (float(abs(_mpf(gi) - want) / unit), float(xi)))
            w64 = max(w64, (float(abs(mp.mpf(float(si)) - want) / unit), float(xi)))
        print("%-8s %d points: long double %.2e at %r, scipy float64 %.2e at %r" % ((name, x.size) + worst + w64))
        assert worst[0] <= 1e-17, "%s: %.3e from mpmath at x = %r" % ((name,) + worst)
        # float64 and below: scipy itself, bitwise
        assert np.array_equal(fn(x), f64(x)) and fn(2.5) == f64(2.5) and fn(np.float32(2.5)).dtype == np.float32
    # poles and non-finite arguments
    edge = np.array([0.0, -3.0, np.inf, -np.inf, np.nan], dtype=LD)
    assert np.all(np.isnan(XS.digamma(edge)[[0, 1, 3, 4]])) and XS.digamma(edge)[2] == np.inf
    assert np.all(XS.gammaln(edge)[:4] == np.inf) and np.isnan(XS.gammaln(edge)[4])
    assert XS.ln2pi(xl).dtype == LD and XS.ln2pi(x) == np.log(2.0 * np.pi) and abs(_mpf(XS.ln2pi(xl)) - mp.log(2 * mp.pi)) < 1e-18
    assert abs(_mpf(XS.lnpi(xl)) - mp.log(mp.pi)) < 1e-18
    src = inspect.getsource(XS)
    assert "import mpmath" not in src and "from mpmath" not in src


def _mp_bound(st, pri, Y, T, mode):
    """The six parts of oracle/lds_closed_form.py: elbo_parts (mode "reference") and tests/exact_bound_ref.py: elbo_parts_exact
    ("exact") written out in mpmath for one replicate without missing outputs or known entries, from the state as it is: means,
    covariances and the stored q_ln_det are data, everything formed from them (the statistics, the expectations, the
    log-determinants, digamma, ln Gamma) is formed here."""
    import mpmath as mp
    kind = pri["noise"]
    X, Sig, A, C = _mpa(st["X"][0]), _mpa(st["Sigma"][0]), _mpa(st["A_mean"][0]), _mpa(st["C_mean"][0])
    Acov, Ccov = _mpa(st["A_cov"][0]), _mpa(st["C_cov"][0])
    Ym = _mpa(Y[0])
    D, K = A.shape[0], C.shape[0]
    ln2pi, half = mp.log(2 * mp.pi), mp.mpf(1) / 2
    lndet = lambda M: mp.log(mp.det(mp.matrix(M.tolist())))
    inv = lambda M: np.array(mp.inverse(mp.matrix(M.tolist())).tolist(), dtype=object)
    tr = lambda M: sum(M[i, i] for i in range(M.shape[0]))
    outer = lambda u, v: np.outer(u, v)
    nint = max(T - 2, 0)
    # the statistics (O.statistics)
    XX = sum(outer(X[t], X[t]) for t in range(T))
    cov_all = Sig[0] + nint * Sig[1] + Sig[2]
    Sxx = XX + cov_all
    Sxx_m = XX - outer(X[-1], X[-1]) + cov_all - Sig[2]
    Sxx_p = XX - outer(X[0], X[0]) + cov_all - Sig[0]
    Sx1x = sum(outer(X[t], X[t - 1]) for t in range(1, T))
    Syx = sum(outer(Ym[t], X[t]) for t in range(T))
    Syy = sum(outer(Ym[t], Ym[t]) for t in range(T))
    x0x0 = outer(X[0], X[0]) + Sig[0]

    def psi_multi(a, dim):
        return sum(mp.digamma(a - half * i) for i in range(dim))

    def lgamma_multi(a, dim):
        return mp.mpf(dim * (dim - 1)) / 4 * mp.log(mp.pi) + sum(mp.loggamma(a - half * i) for i in range(dim))

    def noise(which, dim):
        """(E[Lambda], the ln det term of the Gaussians' own terms in this mode, the node's own lower bound)"""
        a, b = st[which + "_a"][0], st[which + "_b"][0]
        a0, b0 = pri[which + "_a0"], pri[which + "_b0"]
        if kind == "wishart":
            a, a0, B, B0 = _mpf(a), _mpf(a0), _mpa(b), _mpa(b0)
            Bs = (B + B.T) / 2
            lndB = lndet(Bs)
            EL = a * inv(Bs)
            Eln = psi_multi(a, dim) - lndB
            h = mp.mpf(dim + 1) / 2
            llb = (a0 - h) * Eln - lgamma_multi(a0, dim) + a0 * lndet(B0) - tr(B0.dot(EL))
            llb -= (a - h) * Eln - lgamma_multi(a, dim) + a * lndB - a * dim
            return EL, (Eln if mode == "exact" else dim * mp.log(a) - lndB), llb
        a, b, a0, b0 = _mpa(a), _mpa(b), _mpa(np.broadcast_to(a0, (dim,))), _mpa(np.broadcast_to(b0, (dim,)))
        EL = np.diag(a / b)
        llb = 0
        for k in range(dim):
            Eln = mp.digamma(a[k]) - mp.log(b[k])
            llb += (a0[k] - 1) * Eln - mp.loggamma(a0[k]) + a0[k] * mp.log(b0[k]) - b0[k] * (a[k] / b[k])
            llb -= (a[k] - 1) * Eln - mp.loggamma(a[k]) + a[k] * mp.log(b[k]) - b[k] * (a[k] / b[k])
        lnd = sum((mp.digamma(a[k]) - mp.log(b[k])) if mode == "exact" else mp.log(a[k] / b[k]) for k in range(dim))
        return EL, lnd, llb

    def outer_expect(M, Mcov, G):
        return M.dot(G).dot(M.T) + sum(Mcov[i] * G[i, i] for i in range(D))

    Qb, lndQ, LQ = noise("Q", D)
    Rb, lndR, LR = noise("R", K)
    L0, m0 = _mpa(pri["x0_prec"]), _mpa(pri["x0_mean"])
    ex0 = x0x0 + outer(m0, m0) - 2 * outer(X[0], m0)
    LX = -half * D * ln2pi + half * lndet(L0) - half * tr(L0.dot(ex0))
    EQ = Sxx_p + outer_expect(A, Acov, Sxx_m) - 2 * Sx1x.dot(A.T)
    LX += (T - 1) * (-half * D * ln2pi + half * lndQ) - half * tr(Qb.dot(EQ))
    if mode == "exact":
        ent = [lndet(Sig[c]) for c in range(3)]
    else:
        ent = [_mpf(v) for v in st["qld_x"][0]]
    LX += T * (half * D * ln2pi + half * D) + half * (ent[0] + nint * ent[1] + ent[2])
    ER = Syy + outer_expect(C, Ccov, Sxx) - 2 * Syx.dot(C.T)
    LY = T * (-half * K * ln2pi + half * lndR) - half * tr(Rb.dot(ER))

    def cols(M, Mcov, pm, pp, qldc, rows):
        pm, pp = _mpa(pm), _mpa(pp)
        tot = 0
        for i in range(D):
            ex = [M[k, i] ** 2 + Mcov[i][k, k] + pm[k, i] ** 2 - 2 * M[k, i] * pm[k, i] for k in range(rows)]
            tot += -half * rows * ln2pi + half * sum(mp.log(pp[i][k]) for k in range(rows)) - half * sum(pp[i][k] * ex[k] for k in range(rows))
            tot += half * rows * ln2pi + half * (lndet(Mcov[i]) if mode == "exact" else _mpf(qldc[i])) + half * rows
        return tot

    LA = cols(A, Acov, pri["A_prior_mean"], pri["A_prior_prec"], st["qld_A"][0], D)
    LC = cols(C, Ccov, pri["C_prior_mean"], pri["C_prior_prec"], st["qld_C"][0], K)
    return [LX, LY, LA, LC, LQ, LR]


@pytest.mark.parametrize("noise", ["diagonal_gamma", "wishart"])
def test_extended_bound_against_mpmath(noise):
    """T = 5, D = 3, K = 2, N = 1, one iteration: the six parts of both bounds of the long-double run within 1e-17 of an mpmath
    evaluation at 40 digits, in units of s = sum_p |part_p| (the envelope's unit) -- and no part further than 1e-16 from it in
    units of itself."""
    import mpmath as mp
    mp.mp.dps = 40
    T, D, K = 5, 3, 2
    c = E._wishart(T, D, K, 1, 1, iters=1) if noise == "wishart" else E._plain(T, D, K, 1, 1)
    assert c["pri"]["noise"] == noise
    Y, pri = E.to_long(c["Y"]), E.to_long(c["pri"])
    run = E.OracleLDS(Y, E.to_long(c["st0"]), pri)
    got = {k: a for k, a in E.lds_trace(run, 1, False, E.BOUND_MODES) if E.is_bound(k)}
    assert set(got) == {(0, "bound", m) for m in E.BOUND_MODES}
    for mode in E.BOUND_MODES:
        g = got[(0, "bound", mode)]
        assert g.dtype == LD and g.shape == (1, 6)
        want = _mp_bound(run.st, pri, Y, T, mode)
        s = sum(abs(w) for w in want)
        for p, w in enumerate(want):
            err = abs(_mpf(g[0, p]) - w)
            print("%-14s %-9s %-4s %s  distance from mpmath %.2e of s, %.2e of itself"
                  % (noise, mode, E.LDS_PARTS[p], mp.nstr(w, 12), float(err / s), float(err / abs(w))))
            assert err <= mp.mpf("1e-17") * s, "%s %s %s: %s" % (noise, mode, E.LDS_PARTS[p], mp.nstr(err / s, 5))
            assert err <= mp.mpf("1e-16") * abs(w)
    # the two modes differ (the exact one is not the reference one by accident)
    assert np.all(got[(0, "bound", "exact")][0, :4] != got[(0, "bound", "reference")][0, :4])


def _check_bound_records(what, bnd, names):
    for key, (ext, e64, own) in sorted(bnd.items()):
        assert ext.dtype == LD and np.all(np.isfinite(ext)), "%s %r: dtype %s" % (what, key, ext.dtype)
        assert e64.shape == ext.shape
        for r in range(ext.shape[0]):
            print("%-34s it%d %-9s " % ((what if ext.shape[0] == 1 else "%s r%d" % (what, r)), key[0], key[2])
                  + "  ".join("%s %.1e (%.1e)" % (nm, e64[r, p], own[r, p]) for p, nm in enumerate(names)))
        assert np.all(e64 <= E.CAP), "%s %r: float64 oracle %r of s_r from the extended run, cap %.0e" % (what, key, e64, E.CAP)


@pytest.mark.parametrize("name", list(E.LDS_CASES))
def test_extended_lds_bound_keeps_long_double_and_float64_oracle_is_within_the_cap(name):
    """Every part of both bounds after every iteration: long double, and the float64 oracle within CAP of it in units of s_r.
    Printed: e64 per part, in brackets the same relative to the part itself (for the record)."""
    iters = E.lds_case(name)["iters"]
    for (rows, T, n, _, _, _, _), bnd in zip(E.lds_reference(name), E.lds_bound_reference(name)):
        assert set(bnd) == {(it, "bound", m) for it in range(iters) for m in E.BOUND_MODES}
        _check_bound_records(name if rows is None else "%s replicate %d" % (name, rows), bnd, E.LDS_PARTS)


@pytest.mark.parametrize("N,d,q", E.PCA_BOUND_CASES)
def test_extended_pca_bound_keeps_long_double_and_float64_oracle_is_within_the_cap(N, d, q):
    bnd = E.pca_bound_reference(N, d, q)
    assert set(bnd) == {(it, "bound", m) for it in range(2) for m in E.BOUND_MODES}
    _check_bound_records("PCA (%d, %d, %d)" % (N, d, q), bnd, E.PCA_PARTS)
    if (N, d, q) == E.PCA_SMALL:        # what the case is there for: the recurrence branch of the host's digamma
        init, pri = E.pca_problem(N, d, q)
        assert pri["beta_a0"] + 0.5 * d * N < 10


def _digamma_short_series(x):
    """Mutant 1: the kernels' digamma (recurrence to 10, then the series) with the series cut after its 1/120 term"""
    x = np.array(x, dtype=float)
    r = np.zeros_like(x)
    while np.any(x < 10.0):
        low = x < 10.0
        r = np.where(low, r - 1.0 / np.where(low, x, 1.0), r)
        x = np.where(low, x + 1.0, x)
    f = 1.0 / (x * x)
    return r + np.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120))


def _mutant_nint(monkeypatch):
    """Mutant 2: elbo_parts with nint = T - 1 (one interior entropy term too many)"""
    src = inspect.getsource(O.elbo_parts)
    assert src.count("nint = max(T - 2, 0)") == 1
    ns = {}
    exec(compile(src.replace("nint = max(T - 2, 0)", "nint = T - 1"), "<mutant of elbo_parts>", "exec"), vars(O), ns)
    monkeypatch.setattr(O, "elbo_parts", ns["elbo_parts"])


MUTANTS = {
    "digamma series cut after 1/120": ("reference", lambda mp: mp.setattr(O, "digamma", _digamma_short_series)),
    "nint = T - 1": ("reference", _mutant_nint),
    "exact: ln(a / b) for psi(a) - ln b": ("exact", lambda mp: mp.setattr(XR, "noise_eln", O.noise_lndet)),
}
MUTANT_CASES = ("t19_d6_k4", "t77_d33_k17_gamma", "lengths_2_17_33_d16_k16")


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bound_comparison_catches_mutants(mutant, monkeypatch):
    """The comparison the GPU tests apply to a handle's parts (extended_ref.compare_bound), applied to the float64 oracle with
    one subtle error planted in its bound: beyond FACTOR x yardstick on at least one case.  The unmutated float64 oracle is
    within it everywhere (its e64 is the yardstick's floor).  Printed: whether the mutant would have passed the 1e-8 test of
    the parity suite (|mutant - float64 oracle| <= 1e-8 sum |parts|)."""
    mode, plant = MUTANTS[mutant]
    clean = {name: E.lds_float64_bound(name) for name in MUTANT_CASES}
    refs = {name: (E.lds_reference(name), E.lds_bound_reference(name)) for name in MUTANT_CASES}     # before the mutant is planted
    plant(monkeypatch)
    caught = []
    for name in MUTANT_CASES:
        mutated = E.lds_float64_bound(name)
        for (rows, T, n, _, _, _, _), bnd, mut, cl in zip(refs[name][0], refs[name][1], mutated, clean[name]):
            for key in sorted(k for k in bnd if k[2] == mode):
                ext, e64, _ = bnd[key]
                assert max(r[4] for r in E.compare_bound(cl[key], ext, e64, n)) <= 1.0 + 1e-9       # the oracle itself: e_gpu = e64 <= y
                worst = max(E.compare_bound(mut[key], ext, e64, n), key=lambda r: r[4])
                parity = float((np.abs(mut[key] - cl[key]) / np.abs(cl[key]).sum(axis=1, keepdims=True)).max())
                print("%-36s %-28s%s it%d  worst part %-4s e/y %10.3g   1e-8 test: %.2e -> %s"
                      % (mutant, name, "" if rows is None else " r%d" % rows, key[0], E.LDS_PARTS[worst[1]], worst[4], parity,
                         "would pass" if parity <= 1e-8 else "would fail"))
                if worst[4] > E.FACTOR:
                    caught.append((name, rows, key))
    assert caught, "mutant %r stays within %g x yardstick on every case" % (mutant, E.FACTOR)
