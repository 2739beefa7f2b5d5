"""TEST INFRASTRUCTURE: the VB-PCA graph whose W columns have DiagonalGamma precision parents, a Gamma per entry of W (sparse
loadings; pyvb_pca_set_entry_precisions), as a composition of oracle/pca_closed_form.py and tests/exact_bound_ref.py in the
pattern of tests/pca_ard_ref.py -- none of them is edited.

    Ws = [Gaussian(d, pmu_i, DiagonalGamma(d, a0_i, b0_i)) for i in range(q)]          (gaussian.py:55-61 accepts the node)

A column then sees pprec = diag(qa_i / qb_i) (gaussian.py:113, nodes_todo.py:192-193), so every oracle function runs on priors whose
W_prior_prec is qa / qb (priors_now).  Added here: dg_i.update() (nodes_todo.py:187-190) at its place in the crawl order the
fixtures record, DiagonalGamma.log_lower_bound of every parent (:199-204) inside part 0, and for the exact bound
1/2 sum_k (psi(qa_ik) - ln qa_ik) per column, which turns the 1/2 sum_k ln (qa_ik / qb_ik) the oracle forms into
1/2 sum_k E[ln of the entry's precision].

State: that of oracle/pca_closed_form.py plus W_entry_a [q][d] (qa = a0 + 1/2, nodes_todo.py:183-186) and W_entry_b [q][d] (qb).
init carries W_entry_b (the reference draws it at random, :177), pri carries W_entry_a0, W_entry_b0 [q][d].  Every function keeps
the dtype it is given (np.longdouble: the extended run of tests/extended_ref.py).

Parity status: PINNED by tests/golden/wentry_*.npz (tests/golden/make_golden_pca_entry.py runs the reference's own nodes).
"""
import functools
import re

import numpy as np

import exact_bound_ref as XR
import extended_ref as ER
import pca_ard_ref as AR
from oracle import pca_closed_form as P
from oracle._xspecial import digamma, gammaln

# the reference's crawl order on this graph, by node class (network.py:58-96 from [W]); the fixtures record the node-by-node order
ORDER = ("W", "Z", "entry", "X0", "Mu", "X", "Beta")
ITERS = 2
BOUNDS = ER.BOUND_MODES
NAMES = ER.PCA_NAMES + ("W_entry_b",)


def stage_order(labels):
    """The recorded node order ["W0", .., "Z0", .., "D0", .., "X0", "Mu", "X1", .., "Beta"] by class, runs collapsed."""
    out = []
    for s in labels:
        s = str(s)
        c = "X0" if s == "X0" else {"W": "W", "Z": "Z", "D": "entry", "X": "X", "M": "Mu", "B": "Beta"}[s[0]]
        assert re.fullmatch(r"[WZDX]\d+|Mu|Beta", s), s
        if not out or out[-1] != c:
            out.append(c)
    return tuple(out)


def make_state(init, pri, N, d, q):
    st = P.make_state(init, pri, N, d, q)           # copies init["W_entry_b"] in the state's dtype
    dt = st["X"].dtype
    st["W_entry_a"] = np.asarray(pri["W_entry_a0"], dtype=dt) + dt.type(1) / 2      # update_a: one child per entry
    st["W_entry_b"] = np.array(st["W_entry_b"], dtype=dt)
    return st


def priors_now(st, pri):
    """pri with the columns' Constant precisions replaced by what their DiagonalGamma parents pass down now."""
    out = dict(pri)
    out["W_prior_prec"] = st["W_entry_a"] / st["W_entry_b"]
    return out


def update_entry(st, pri, var_scale=None):
    """[dg.update() for dg in parents]: qb_ik = b0_ik + 1/2 <w w^T>_kk + 1/2 (pm pm^T)_kk - (<w> pm^T)_kk (nodes_todo.py:188-190).
    var_scale [q][d]: a factor on each entry's variance -- a deliberately wrong term, for the test of the yardstick only."""
    dw = (st["W_mean"] - pri["W_prior_mean"]).T
    sv = st["W_var"]
    if var_scale is not None:
        sv = sv * var_scale
    st["W_entry_b"] = pri["W_entry_b0"] + (dw * dw + sv) / 2


def entry_terms(st, pri):
    """sum_i DiagonalGamma.log_lower_bound of parent i (nodes_todo.py:199-204), the same in both bound modes"""
    a0, b0, a, b = pri["W_entry_a0"], pri["W_entry_b0"], st["W_entry_a"], st["W_entry_b"]
    Elnx = digamma(a) - np.log(b)
    ret = (a0 - 1) * Elnx - gammaln(a0) + a0 * np.log(b0) - b0 * (a / b)
    ret = ret - ((a - 1) * Elnx - gammaln(a) + a * np.log(b) - b * (a / b))
    return ret.sum()


def elbo_parts(st, pri, mode="reference"):
    """[L_W + the parents' terms, L_Z, L_X, L_Mu, L_Beta]"""
    now = priors_now(st, pri)
    parts = np.array(P.elbo_parts(st, now) if mode == "reference" else XR.pca_elbo_parts_exact(st, now))
    parts[0] += entry_terms(st, pri)
    if mode == "exact":         # E[ln det diag(.)] = sum_k (psi(qa_ik) - ln qb_ik) in the column's own term
        parts[0] += ((digamma(st["W_entry_a"]) - np.log(st["W_entry_a"])) / 2).sum()
    return parts


def stage(st, pri, name, var_scale=None):
    N = st["X"].shape[0]
    if name == "entry":
        return update_entry(st, pri, var_scale)
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


load_fixture = AR.load_fixture


# ---- the problems the device is measured on ---------------------------------------------------------------------------------
# (N, d, q): what each reaches is in tests/test_pca_entry_gpu.py
SHAPES = AR.SHAPES
UNPINNED = AR.UNPINNED          # rows left as their constructors drew them (pyvb_pca_set_unpinned_rows)


def add_hyperpriors(init, pri, seed):
    """Per-entry a0, b0, qb and non-zero prior means (a stride of 0, a transposed index or a dropped pm shows).  The ranges keep
    every column's 1/2 ln det qprec well away from 0, where q_ln_det = 1 / ln det qprec (quirk Q1) has its pole: qa / qb >=
    1.5 / 1.5 at the start, the likelihood adds to it, and tests/test_pca_entry_cpu.py checks |1/2 ln det qprec| on every case
    after every update."""
    d, q = init["W_mean"].shape
    rng = np.random.default_rng(seed)
    pri["W_prior_mean"] = 0.3 * rng.standard_normal((d, q))
    pri["W_entry_a0"] = rng.uniform(1.0, 3.0, (q, d))
    pri["W_entry_b0"] = rng.uniform(0.5, 1.5, (q, d))
    init["W_entry_b"] = rng.uniform(0.5, 1.5, (q, d))
    del pri["W_prior_prec"]     # the columns have no Constant precision on this graph


def problem(N, d, q):
    init, pri = ER.pca_problem(N, d, q)
    if (N, d, q) == UNPINNED:
        rng = np.random.default_rng(7)
        init["X_full"] = rng.standard_normal((N, d))
        init["X_var0"] = 1.0 / rng.uniform(0.2, 1.0, N)
    add_hyperpriors(init, pri, 2400 + N + d + q)
    return init, pri


def handle_problem(init, pri):
    """(init, pri) as PCABatch.from_problem takes them: W_prior_prec is a placeholder the setter overwrites, pri["W_entry"] the
    hyperpriors."""
    d, q = init["W_mean"].shape
    pri = dict(pri, W_prior_prec=np.ones((q, d)), W_entry=(pri["W_entry_a0"], pri["W_entry_b0"], init["W_entry_b"]))
    return {k: v for k, v in init.items() if k != "W_entry_b"}, pri


class OraclePCAEntry(object):
    """The stage calls of PCABatch on one comparator state (tests/extended_ref.py: OraclePCA with the parents' stage)."""

    def __init__(self, init, pri, N, d, q):
        self.st, self.pri, self.N = make_state(init, pri, N, d, q), pri, N

    def update_W(self): stage(self.st, self.pri, "W")
    def update_Z(self): stage(self.st, self.pri, "Z")
    def update_entry_precisions(self): stage(self.st, self.pri, "entry")
    def update_X(self, lo, hi): P.update_X(self.st, priors_now(self.st, self.pri), lo, hi)
    def update_Mu(self): stage(self.st, self.pri, "Mu")
    def update_Beta(self): stage(self.st, self.pri, "Beta")
    def get_state(self): return self.st
    def elbo_parts(self, mode): return elbo_parts(self.st, self.pri, mode)


def trace(m, N, iters=ITERS, bounds=(), parts=None, qb=None):
    """Stage-wise in the crawl order, read at the end of each iteration (so that a handle runs its fused sweep): yields
    ((iteration, "update_Beta", name), array) for NAMES and ((iteration, "bound", mode), parts [5]).  qb: how to read W_entry_b
    of m (a handle: lambda: b.entry_precisions()[1])."""
    for it in range(iters):
        m.update_W()
        m.update_Z()
        m.update_entry_precisions()
        m.update_X(0, 1)
        m.update_Mu()
        m.update_X(1, N)
        m.update_Beta()
        g = m.get_state()
        for nm in ER.PCA_NAMES:
            yield (it, "update_Beta", nm), np.array(g[nm])
        yield (it, "update_Beta", "W_entry_b"), np.array(qb() if qb else g["W_entry_b"])
        for mode in bounds:
            yield (it, "bound", mode), np.array((parts or m.elbo_parts)(mode))


@functools.lru_cache(maxsize=None)
def reference(N, d, q):
    """(n, ext, e64, bnd, min |1/2 ln det qprec| over the columns and iterations, f64) of the case, as pca_ard_ref.reference.
    Computed once per process, never modified."""
    ER.require_extended()
    init, pri = problem(N, d, q)
    m64 = OraclePCAEntry(init, pri, N, d, q)
    mx = OraclePCAEntry(ER.to_long(init), ER.to_long(pri), N, d, q)
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
