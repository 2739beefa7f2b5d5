"""TEST INFRASTRUCTURE: the VB-PCA graph whose W columns have Gamma precision parents (automatic relevance determination;
pyvb_pca_set_column_precisions), as a composition of oracle/pca_closed_form.py and tests/exact_bound_ref.py -- neither is edited.

    Ws = [Gaussian(d, pmu_i, Gamma(d, a0_i, b0_i)) for i in range(q)]          (gaussian.py:55-61 accepts the node)

A column then sees pprec = (qa_i / qb_i) I (gaussian.py:113, nodes_todo.py:140-142), so every oracle function runs on priors whose
W_prior_prec[i] is (qa_i / qb_i) ones(d) (priors_now).  Added here: alpha_i.update() (nodes_todo.py:130-138) at its place in the
crawl order the fixtures record, Gamma.log_lower_bound of every alpha_i (:149-157) inside part 0, and for the exact bound
1/2 d (psi(qa_i) - ln qa_i) per column, which turns the 1/2 d ln (qa_i / qb_i) the oracle forms into 1/2 d E[ln alpha_i].

State: that of oracle/pca_closed_form.py plus W_alpha_a [q] (qa_i = a0_i + d / 2, nodes_todo.py:125-128) and W_alpha_b [q] (qb).
init carries W_alpha_b (the reference draws it at random, :119), pri carries W_alpha_a0, W_alpha_b0 [q].  Every function keeps
the dtype it is given (np.longdouble: the extended run of tests/extended_ref.py).

Parity status: PINNED by tests/golden/ward_*.npz (tests/golden/make_golden_pca_ard.py runs the reference's own nodes).
"""
import functools
import re

import numpy as np

import exact_bound_ref as XR
import extended_ref as ER
from oracle import pca_closed_form as P
from oracle._xspecial import digamma, gammaln

# the reference's crawl order on this graph, by node class (network.py:58-96 from [W]); the fixtures record the node-by-node order
ORDER = ("W", "Z", "alpha", "X0", "Mu", "X", "Beta")
ITERS = 2
BOUNDS = ER.BOUND_MODES
NAMES = ER.PCA_NAMES + ("W_alpha_b",)


def stage_order(labels):
    """The recorded node order ["W0", .., "Z0", .., "A0", .., "X0", "Mu", "X1", .., "Beta"] by class, runs collapsed."""
    out = []
    for s in labels:
        s = str(s)
        c = "X0" if s == "X0" else {"W": "W", "Z": "Z", "A": "alpha", "X": "X", "M": "Mu", "B": "Beta"}[s[0]]
        assert re.fullmatch(r"[WZAX]\d+|Mu|Beta", s), s
        if not out or out[-1] != c:
            out.append(c)
    return tuple(out)


def make_state(init, pri, N, d, q):
    st = P.make_state(init, pri, N, d, q)           # copies init["W_alpha_b"] in the state's dtype
    dt = st["X"].dtype
    st["W_alpha_a"] = np.asarray(pri["W_alpha_a0"], dtype=dt) + dt.type(d) / 2      # update_a: one child of d entries
    st["W_alpha_b"] = np.array(st["W_alpha_b"], dtype=dt)
    return st


def priors_now(st, pri):
    """pri with the columns' Constant precisions replaced by what their Gamma parents pass down now."""
    d = st["X"].shape[1]
    out = dict(pri)
    out["W_prior_prec"] = (st["W_alpha_a"] / st["W_alpha_b"])[:, None] * np.ones((1, d), dtype=st["X"].dtype)
    return out


def update_alpha(st, pri, var_scale=None):
    """[al.update() for al in alphas]: qb_i = b0_i + 1/2 tr<w w^T> + 1/2 tr(pm pm^T) - tr(<w> pm^T) (nodes_todo.py:136-138).
    var_scale [q]: a factor on each column's sum of variances -- a deliberately wrong sum, for the test of the yardstick only."""
    dw = st["W_mean"] - pri["W_prior_mean"]
    sv = st["W_var"].sum(axis=1)
    if var_scale is not None:
        sv = sv * var_scale
    st["W_alpha_b"] = pri["W_alpha_b0"] + ((dw * dw).sum(axis=0) + sv) / 2


def alpha_terms(st, pri):
    """sum_i Gamma.log_lower_bound of alpha_i (nodes_todo.py:149-157), the same in both bound modes"""
    a0, b0, a, b = pri["W_alpha_a0"], pri["W_alpha_b0"], st["W_alpha_a"], st["W_alpha_b"]
    Elnx = digamma(a) - np.log(b)
    ret = (a0 - 1) * Elnx - gammaln(a0) + a0 * np.log(b0) - b0 * (a / b)
    ret = ret - ((a - 1) * Elnx - gammaln(a) + a * np.log(b) - b * (a / b))
    return ret.sum()


def elbo_parts(st, pri, mode="reference"):
    """[L_W + alpha terms, L_Z, L_X, L_Mu, L_Beta]"""
    now = priors_now(st, pri)
    parts = np.array(P.elbo_parts(st, now) if mode == "reference" else XR.pca_elbo_parts_exact(st, now))
    parts[0] += alpha_terms(st, pri)
    if mode == "exact":         # E[ln det alpha_i I] = d (psi(qa) - ln qb) in the column's own term, as XR.noise_eln has it for Beta
        d = st["X"].shape[1]
        parts[0] += (d * (digamma(st["W_alpha_a"]) - np.log(st["W_alpha_a"])) / 2).sum()
    return parts


def stage(st, pri, name, var_scale=None):
    N = st["X"].shape[0]
    if name == "alpha":
        return update_alpha(st, pri, var_scale)
    now = priors_now(st, pri)
    if name == "X0":
        return P.update_X(st, now, 0, 1)
    if name == "X":
        return P.update_X(st, now, 1, N)
    return {"W": P.update_W, "Z": P.update_Z, "Mu": P.update_Mu, "Beta": P.update_Beta}[name](st, now)


def iterate(st, pri, order=ORDER, mode="reference", var_scale=None):
    for name in order:
        stage(st, pri, name, var_scale)
    return elbo_parts(st, pri, mode)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def load_fixture(path):
    z = dict(np.load(path, allow_pickle=False))
    init = {k[5:]: z[k] for k in z if k.startswith("init_")}
    pri = {k[6:]: (float(z[k]) if z[k].ndim == 0 else z[k]) for k in z if k.startswith("prior_")}
    return int(z["N"]), int(z["d"]), int(z["q"]), init, pri, z


# ---- the problems the device is measured on ---------------------------------------------------------------------------------
# (N, d, q): what each reaches is in tests/test_pca_ard_gpu.py
SHAPES = [(20, 5, 2), (30, 70, 5), (24, 250, 16), (36, 40, 32), (20, 256, 17), (3, 1, 1)]
UNPINNED = (30, 70, 5)          # rows left as their constructors drew them (pyvb_pca_set_unpinned_rows)


def add_hyperpriors(init, pri, seed):
    """Per-column a0, b0, qb and non-zero prior means (a stride of 0 or a dropped pm shows).  The ranges keep every column's
    1/2 ln det qprec well away from 0, where q_ln_det = 1 / ln det qprec (quirk Q1) has its pole: qa / qb >= (1 + d / 2) / 1.5 > 1
    for d >= 2 at the start, and tests/test_pca_ard_cpu.py checks |1/2 ln det qprec| on every case after every update."""
    d, q = init["W_mean"].shape
    rng = np.random.default_rng(seed)
    pri["W_prior_mean"] = 0.3 * rng.standard_normal((d, q))
    pri["W_alpha_a0"] = rng.uniform(1.0, 3.0, q)
    pri["W_alpha_b0"] = rng.uniform(0.5, 1.5, q)
    init["W_alpha_b"] = rng.uniform(0.5, 1.5, q)
    del pri["W_prior_prec"]     # the columns have no Constant precision on this graph


def problem(N, d, q):
    init, pri = ER.pca_problem(N, d, q)
    if (N, d, q) == UNPINNED:
        rng = np.random.default_rng(7)
        init["X_full"] = rng.standard_normal((N, d))
        init["X_var0"] = 1.0 / rng.uniform(0.2, 1.0, N)
    add_hyperpriors(init, pri, 2200 + N + d + q)
    return init, pri


def handle_problem(init, pri):
    """(init, pri) as PCABatch.from_problem takes them: W_prior_prec is a placeholder the setter overwrites, pri["W_alpha"] the
    hyperpriors."""
    d, q = init["W_mean"].shape
    pri = dict(pri, W_prior_prec=np.ones((q, d)), W_alpha=(pri["W_alpha_a0"], pri["W_alpha_b0"], init["W_alpha_b"]))
    return {k: v for k, v in init.items() if k != "W_alpha_b"}, pri


class OraclePCAARD(object):
    """The stage calls of PCABatch on one comparator state (tests/extended_ref.py: OraclePCA with the alpha stage)."""

    def __init__(self, init, pri, N, d, q):
        self.st, self.pri, self.N = make_state(init, pri, N, d, q), pri, N

    def update_W(self): stage(self.st, self.pri, "W")
    def update_Z(self): stage(self.st, self.pri, "Z")
    def update_column_precisions(self): stage(self.st, self.pri, "alpha")
    def update_X(self, lo, hi): P.update_X(self.st, priors_now(self.st, self.pri), lo, hi)
    def update_Mu(self): stage(self.st, self.pri, "Mu")
    def update_Beta(self): stage(self.st, self.pri, "Beta")
    def get_state(self): return self.st
    def elbo_parts(self, mode): return elbo_parts(self.st, self.pri, mode)


def trace(m, N, iters=ITERS, bounds=(), parts=None, qb=None):
    """Stage-wise in the crawl order, read at the end of each iteration (so that a handle runs its fused sweep): yields
    ((iteration, "update_Beta", name), array) for NAMES and ((iteration, "bound", mode), parts [5]).  qb: how to read W_alpha_b
    of m (a handle: lambda: b.column_precisions()[1])."""
    for it in range(iters):
        m.update_W()
        m.update_Z()
        m.update_column_precisions()
        m.update_X(0, 1)
        m.update_Mu()
        m.update_X(1, N)
        m.update_Beta()
        g = m.get_state()
        for nm in ER.PCA_NAMES:
            yield (it, "update_Beta", nm), np.array(g[nm])
        yield (it, "update_Beta", "W_alpha_b"), np.array(qb() if qb else g["W_alpha_b"])
        for mode in bounds:
            yield (it, "bound", mode), np.array((parts or m.elbo_parts)(mode))


@functools.lru_cache(maxsize=None)
def reference(N, d, q):
    """(n, ext, e64, bnd, min |1/2 ln det qprec| over the columns and iterations, f64) of the case, as
    extended_ref._pca_reference: ext {key: long-double array}, e64 {key: distance of the float64 comparator from it}, bnd {key:
    (ext [1, 5], e64 [1, 5], ..)}, f64 {key: the float64 comparator's array, the bound keys included}.  Computed once per process,
    never modified."""
    ER.require_extended()
    init, pri = problem(N, d, q)
    m64 = OraclePCAARD(init, pri, N, d, q)
    mx = OraclePCAARD(ER.to_long(init), ER.to_long(pri), N, d, q)
    ext, e64, bnd, f64, hld = {}, {}, {}, {}, np.inf
    for (k64, a64), (kx, ax) in zip(trace(m64, N, bounds=BOUNDS), trace(mx, N, bounds=BOUNDS)):
        assert k64 == kx and ax.dtype == ER.LD, (k64, kx, ax.dtype)
        a64.setflags(write=False)
        f64[k64] = a64
        if ER.is_bound(kx):
            ax = ax[None]
            ax.setflags(write=False)
            bnd[kx] = (ax,) + ER.bound_errors(a64, ax)
            continue
        ext[kx] = ax
        e64[kx] = ER.rel(a64, ax)
        ax.setflags(write=False)
        if kx[2] == "W_var":
            hld = min(hld, float(np.abs(0.5 * np.log(1.0 / ax).sum(axis=1)).min()))
    return max(d, q, N), ext, e64, bnd, hld, f64
