"""TEST INFRASTRUCTURE: a numpy restatement of the EXACT lower bound (E_q[ln p] - E_q[ln q]) of the LDS graph, built from the
oracle (oracle/lds_closed_form.py) plus slogdet and digamma.  The exact mode of the HIP path (PYVB_BOUND_EXACT) is checked
against it; it is itself checked against a Monte Carlo estimate (tests/test_exact_bound_cpu.py).

The exact parts differ from the oracle's reference parts (quirks Q1, Q2 of SURVEY.md) in these terms only:
  - the entropy of a latent Gaussian: 1/2 ln det qcov instead of 1/2 q_ln_det;
  - the entropy of a partially observed Gaussian (m unknown entries): + (m/2 ln 2 pi + 1/2 ln det cov_mm + m/2) instead of
    - (m/2 ln 2 pi - 1/2 ln det cov_mm - m/2);
  - ln det Lambda in a Gaussian's own term: E[ln det Lambda] instead of ln det E[Lambda] (Gamma family: psi(a) - ln b per
    entry; Wishart: psi_dim(v) - ln det sym(qw)).
The lower-bound terms of the noise nodes and of the Constant parents are the reference's already.
"""
import numpy as np
from oracle import _xlinalg as XL
from oracle import lds_closed_form as O
from oracle import pca_closed_form as P
from oracle._xspecial import digamma, ln2pi

LN2PI = O.LN2PI

# Every function below keeps the dtype of the state it is given (float64: bitwise what it always returned; np.longdouble: the
# extended-precision reference of tests/extended_ref.py): log-determinants go through oracle/_xlinalg.py, digamma through
# oracle/_xspecial.py, accumulators take the dtype of the state.


def noise_eln(kind, a, b, dim):
    """E[ln det Lambda] per replicate (the exact counterpart of O.noise_lndet)."""
    if kind == "diagonal_gamma":
        return np.sum(digamma(a) - np.log(b), axis=-1)
    if kind == "gamma":
        return dim * (digamma(a) - np.log(b))
    if kind == "wishart":
        return O._psi_multi(a, dim) - XL.slogdet(0.5 * (b + np.swapaxes(b, -1, -2)))[1]
    raise ValueError(kind)


def logdets(st, pri):
    """ln det qcov of what the HIP handle stores it for: the X_t classes [N,3], the columns of A and C [N,D], the outputs
    with missing entries [N,T] (of inv <R>; NaN before their first update).  NaN for a column that has not been updated and
    for one with known entries (the handle keeps ln det of its covariance BEFORE the conditioning, which st does not hold)."""
    out = {"X": XL.slogdet(st["Sigma"])[1]}
    for w in ("A", "C"):
        obs = pri.get(w + "_obs")
        ld = _column_logdets(st, w, obs)
        latent = np.ones(ld.shape[1], dtype=bool) if obs is None else np.isnan(obs).all(axis=0)
        out[w] = np.where(np.isnan(st["qld_" + w]) | ~latent[None], np.nan, ld)
    if "Yobs" in st:
        kind = pri["noise"]
        K = st["C_mean"].shape[1]
        lr = -XL.slogdet(O.noise_expect(kind, st["R_a"], st["R_b"], K))[1]
        out["Y"] = np.where(np.isnan(st["Yqld"]), np.nan, lr[:, None])
    return out


def _column_logdets(st, which, obs=None):
    """ln det of the whole covariance of a latent column (the one the handle stores); NaN for a column with known entries,
    whose covariance is singular and whose value no caller uses (a Cholesky-based slogdet refuses such a matrix)."""
    cov = st[which + "_cov"]
    latent = np.ones(cov.shape[1], dtype=bool) if obs is None else np.isnan(obs).all(axis=0)
    out = np.full(cov.shape[:2], np.nan, dtype=cov.dtype)
    if latent.any():
        out[:, latent] = XL.slogdet(cov[:, latent])[1]
    return out


def _y_entropy_exact(st):
    """The true entropy of the outputs that are not fully observed, summed over t."""
    miss = np.isnan(st["Yobs"])
    K = miss.shape[2]
    nm = miss.sum(axis=2)
    LN2PI = ln2pi(st["Yvar"])
    latent, partial = nm == K, (nm > 0) & (nm < K)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.where(miss, np.log(st["Yvar"]), 0.0).sum(axis=2)
    if "Yld" in st:
        lv = np.where(np.isnan(st["Yld"]), lv, st["Yld"])
    # a latent row's ln det qcov: of inv <R> once it has been updated (NaN before, as its q_ln_det)
    lq = np.where(np.isnan(st["Yqld"]), np.nan, 0.0)
    if latent.any():
        if "Yld" in st:
            # Wishart: the row carries qcov = inv <R> of the <R> its own update met, which a later update of R does not change.
            # The state keeps that as the row's q_ln_det = 1 / ln det <R> (O._chol_qld, quirk Q1): ln det qcov = -1 / q_ln_det.
            # (Taken of the current <R> this was right only for a bound formed straight after update_Y.)
            with np.errstate(divide="ignore", invalid="ignore"):
                lq = lq - 1.0 / st["Yqld"]
        else:
            # diagonal noise: Yvar is the diagonal of qcov
            with np.errstate(divide="ignore", invalid="ignore"):
                lq = lq + np.log(st["Yvar"]).sum(axis=2)
    tp = np.where(partial, 0.5 * nm * LN2PI + 0.5 * lv + 0.5 * nm, 0.0)
    tl = np.where(latent, 0.5 * K * LN2PI + 0.5 * lq + 0.5 * K, 0.0)
    return (tp + tl).sum(axis=1)


def elbo_parts_exact(st, pri, S, T):
    """[L_X, L_Y, L_A, L_C, L_Q, L_R] per replicate of the exact bound, for the state st and statistics S that
    O.elbo_parts takes."""
    kind = pri["noise"]
    N, D = st["A_mean"].shape[:2]
    K = st["C_mean"].shape[1]
    ref = O.elbo_parts(st, pri, S, T)
    LN2PI = ln2pi(ref)
    LX, LY, LA, LC, LQ, LR = [ref[:, i].copy() for i in range(6)]
    nint = max(T - 2, 0)
    # X_t: the entropy from ln det Sigma; E ln det Q in the T - 1 own terms
    qld = st["qld_x"]
    lnd = XL.slogdet(st["Sigma"])[1]
    LX += -0.5 * (qld[:, 0] + nint * qld[:, 1] + qld[:, 2]) + 0.5 * (lnd[:, 0] + nint * lnd[:, 1] + lnd[:, 2])
    LX += (T - 1) * 0.5 * (noise_eln(kind, st["Q_a"], st["Q_b"], D) - O.noise_lndet(kind, st["Q_a"], st["Q_b"], D))
    # Y_t: E ln det R in the T own terms; the true entropy of the outputs with missing entries
    LY += T * 0.5 * (noise_eln(kind, st["R_a"], st["R_b"], K) - O.noise_lndet(kind, st["R_a"], st["R_b"], K))
    if "Yobs" in st:
        LY += O._y_entropy_terms(st) + _y_entropy_exact(st)

    def cols(which, rows):
        M, Mcov, qldc, obs = st[which + "_mean"], st[which + "_cov"], st["qld_" + which], pri.get(which + "_obs")
        lndc = _column_logdets(st, which, obs)
        tot = np.zeros(N, dtype=M.dtype)
        for i in range(D):
            known = np.zeros(rows, dtype=bool) if obs is None else ~np.isnan(obs[:, i])
            if not known.any():
                tot += 0.5 * (lndc[:, i] - qldc[:, i])
            elif not known.all():
                mi = np.nonzero(~known)[0]
                m = len(mi)
                ldm = XL.slogdet(Mcov[:, i][:, mi][:, :, mi])[1]
                tot += (0.5 * m * LN2PI - 0.5 * ldm - 0.5 * m) + (0.5 * m * LN2PI + 0.5 * ldm + 0.5 * m)
        return tot

    LA += cols("A", D)
    LC += cols("C", K)
    return np.stack([LX, LY, LA, LC, LQ, LR], axis=1)


def iterate_exact(st, pri, Y, update_outputs=False):
    """O.iterate followed by the exact parts of the same state (O.iterate returns the reference parts)."""
    T = st["X"].shape[1]
    O.iterate(st, pri, Y, with_elbo=False, update_outputs=update_outputs)
    S = O.statistics(st, Y)
    return elbo_parts_exact(st, pri, S, T)


# ----------------------------------------------------------------------------------------------------------------------------
# VB-PCA with missing data (oracle/pca_closed_form.py): parts [L_W, L_Z, L_X, L_Mu, L_Beta]
# ----------------------------------------------------------------------------------------------------------------------------
def pca_logdets(st):
    """ln det qcov of the W columns [q], the Z_n, Mu, and the X_n without any observed entry [N] (NaN for the others; NaN
    before a node's first update, like q_ln_det)."""
    d = st["X"].shape[1]
    w = np.where(np.isnan(st["qld_W"]), np.nan, np.log(st["W_var"]).sum(axis=1))
    z = np.nan if np.isnan(st["qld_Z"]) else XL.slogdet(st["Z_cov"])[1]
    m = np.nan if np.isnan(st["qld_Mu"]) else np.log(st["Mu_var"]).sum()
    none = (~st["obs"]).all(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.where(none, d * np.log(st["X_var"][:, 0]), np.nan)
    return {"W": w, "Z": z, "Mu": m, "X": x}


def pca_elbo_parts_exact(st, pri):
    ref = P.elbo_parts(st, pri)
    LW, LZ, LX, LM, LB = ref
    N, d = st["X"].shape
    LN2PI = ln2pi(st["X"])
    a, b = st["beta_a"], st["beta_b"]
    ld = pca_logdets(st)
    # E ln det (beta I) in the N own terms of the X_n
    LX += N * 0.5 * d * ((digamma(a) - np.log(b)) - (np.log(a) - np.log(b)))
    nmiss = (~st["obs"]).sum(1)
    part = (nmiss > 0) & (nmiss < d)
    none = nmiss == d
    Vm = np.where(st["obs"], 1.0, st["X_var"])
    lv = np.log(Vm[part]).sum(1)
    # partially observed rows: the true entropy of the missing entries instead of the reference's
    LX += np.sum(0.5 * nmiss[part] * LN2PI - 0.5 * lv - 0.5 * nmiss[part]) + np.sum(0.5 * nmiss[part] * LN2PI + 0.5 * lv + 0.5 * nmiss[part])
    if none.any():
        with np.errstate(divide="ignore"):
            qld_rows = 0.5 / (0.5 * d * np.log(1.0 / st["X_var"][none, 0]))
        LX += 0.5 * (ld["X"][none].sum() - qld_rows.sum())
    LZ += N * 0.5 * (ld["Z"] - st["qld_Z"])
    LW += 0.5 * np.sum(ld["W"] - st["qld_W"])
    LM += 0.5 * (ld["Mu"] - st["qld_Mu"])
    return np.array([LW, LZ, LX, LM, LB])
