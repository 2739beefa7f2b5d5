"""Comparator (test infrastructure) for LDS handles whose columns of A and / or C have DiagonalGamma precision parents, one
precision per entry (include/pyvb_hip.h: pyvb_lds_set_entry_precisions): sparse transition and loading matrices.

Nothing of the algorithm is restated: a Model here is tests/ard_ref.py's Model (a model of tests/tied_ref.py with a prior dictionary of
its own; the functions of oracle/lds_closed_form.py run on it unchanged, and a matrix may have Gamma parents there) with, for the
matrices that have DiagonalGamma parents,

  pri["A_prior_prec"][i] = qa[i] / qb[i]                  before every use; O._lndet_diag of that is the reference's
                                                          DiagonalGamma.pass_down_lndet (quirk Q2, nodes_todo.py:195-197)
  dg_i.update()           qb[i][k] = b0[i][k] + 1/2 ((M[k,i] - pm[k,i])^2 + V_i[k,k])      DiagonalGamma.update, nodes_todo.py:187-190,
                          with the column as the only child and a Constant mean parent; qa = a0 + 1/2 (:183-186)
  the bound               parts 2 (A) and 3 (C) gain sum_i O.noise_llb("diagonal_gamma", a0_i, b0_i, qa_i, qb_i) (:199-204); the exact
                          mode (tests/exact_bound_ref.py) also replaces ln qa by psi(qa) in the columns' own terms: 1/2 sum_k
                          (psi(qa) - ln qa) per column, as exact_bound_ref.noise_eln does for Q and R

Arrays that carry a row index are [column][row], as A_prior_prec and A_colvar are.  tests/test_entry_cpu.py pins this composition
against the reference's own run of such graphs (tests/golden/entry_*.npz).  Everything keeps the dtype of the state it is given, so
the same code is the extended-precision reference under tests/extended_ref.py.
"""
import os

import numpy as np

import ard_ref as AR
from oracle import lds_closed_form as O
from oracle._xspecial import digamma

ROWS = AR.ROWS
pack, unpack = AR.pack, AR.unpack


class Model(AR.Model):
    """ard_ref.Model with entry: {"A" / "C": dict(a0, b0, qa, qb)} for the matrices with DiagonalGamma parents, each [D, rows].
    vscale: None, or a [D, rows] factor on the variances' contribution to qb (a planted error, tests/test_entry_cpu.py)."""

    def __init__(self, Ys, st0s, pri, alpha_b, entry_b, vscale=None):
        self.entry = {}
        self._pending = entry_b
        self.vscale = vscale
        AR.Model.__init__(self, Ys, st0s, pri, alpha_b)

    def _install(self):
        AR.Model._install(self)
        if self._pending is not None:       # first call, from ard_ref.Model.__init__: D, K and the dtype are known by now
            dt = self.chains[0]["A_mean"].dtype
            for w, qb in self._pending.items():
                shape = (self.D, ROWS[w](self.D, self.K))
                a0 = np.broadcast_to(np.asarray(self.pri[w + "_entry_a0"], dtype=dt), shape).copy()
                b0 = np.broadcast_to(np.asarray(self.pri[w + "_entry_b0"], dtype=dt), shape).copy()
                self.entry[w] = dict(a0=a0, b0=b0, qa=a0 + 0.5, qb=np.asarray(qb, dtype=dt).copy())
            self._pending = None
        for w, e in self.entry.items():
            self.pri[w + "_prior_prec"] = e["qa"] / e["qb"]

    def update_entry(self, which=None):
        for w in (self.entry if which is None else [which]):
            e, st = self.entry[w], self.chains[0]
            M, pm = st[w + "_mean"][0], self.pri[w + "_prior_mean"]
            V = np.einsum("ikk->ik", st[w + "_cov"][0])             # [D, rows]
            if self.vscale is not None and w in self.vscale:
                V = V * self.vscale[w]
            e["qb"] = e["b0"] + 0.5 * (((M - pm) ** 2).T + V)
        self._install()

    def update_precisions(self, which=None):
        """The precision parents of A, then of C, whichever kind each has."""
        for w in ("A", "C") if which is None else [which]:
            if w in self.alpha:
                self.update_alpha(w)
            if w in self.entry:
                self.update_entry(w)

    def elbo_parts(self, bound="reference"):
        out = AR.Model.elbo_parts(self, bound)
        for w, p in (("A", 2), ("C", 3)):
            if w in self.entry:
                e = self.entry[w]
                out[p] += O.noise_llb("diagonal_gamma", e["a0"], e["b0"], e["qa"], e["qb"]).sum()
                if bound == "exact":
                    out[p] += 0.5 * (digamma(e["qa"]) - np.log(e["qa"])).sum()
        return out

    def iterate(self, bound="reference"):
        """forward, backward, A, C, Q, R, the precision parents of A, then of C, bound: pyvb_lds_iterate on such a handle."""
        self.sweep("forward")
        self.sweep("backward")
        self.update_A()
        self.update_C()
        self.update_Q()
        self.update_R()
        self.update_precisions()
        return self.elbo_parts(bound)

    def expectation(self, w):
        return self.entry[w]["qa"] / self.entry[w]["qb"] if w in self.entry else AR.Model.expectation(self, w)

    def half_lndet_qprec(self):
        """min over the unknown columns of A and C of |1/2 ln det qprec|: q_ln_det = 1/2 / that (quirk Q1) has a pole at 0."""
        st = self.chains[0]
        q = np.concatenate([np.ravel(st["qld_A"]), np.ravel(st["qld_C"])]).astype(float)
        q = q[np.isfinite(q)]
        return float((0.5 / np.abs(q)).min())


def split(st0):
    """(st0 without the parents' entries, {"A" / "C": qb [N, D]} of Gamma parents, {"A" / "C": qb [N, D, rows]} of DiagonalGamma ones)"""
    alpha = {k[0]: v for k, v in st0.items() if k.endswith("_alpha_b")}
    entry = {k[0]: v for k, v in st0.items() if k.endswith("_entry_b")}
    return {k: v for k, v in st0.items() if not (k.endswith("_alpha_b") or k.endswith("_entry_b"))}, alpha, entry


def models(Y, st0, pri, lengths=None, model_ids=None, vscale=None):
    """ard_ref.models for what LDSBatch.from_problem(Y, st0, pri, lengths=, models=) was given: st0 carries A_entry_b / C_entry_b
    [N, D, rows] for the matrices with DiagonalGamma parents (and A_alpha_b / C_alpha_b for those with Gamma parents), pri their
    A_entry_a0 / A_entry_b0.  A model's parameters and qb are those of its first row."""
    N, T = Y.shape[:2]
    lengths = [T] * N if lengths is None else [int(t) for t in lengths]
    ids = np.arange(N) if model_ids is None else np.asarray(model_ids)
    st0, alpha, entry = split(st0)
    out = []
    for m in range(int(ids.max()) + 1):
        rows = [int(n) for n in np.nonzero(ids == m)[0]]
        f = rows[0]
        Ys = [Y[n:n + 1, :lengths[n]].copy() for n in rows]
        st0s = [{k: (v[n:n + 1, :lengths[n]] if k == "X" else v[f:f + 1]).copy() for k, v in st0.items()} for n in rows]
        out.append((rows, Model(Ys, st0s, pri, {w: qb[f] for w, qb in alpha.items()}, {w: qb[f] for w, qb in entry.items()}, vscale)))
    return out


def add_entry_priors(st0, pri, which, seed, a0=1e-3, b0=1e-3):
    """DiagonalGamma parents for the columns of the matrices named in `which` on a problem of synth.make_problem: broad priors that
    differ from entry to entry (a row or column stride of 0 shows), and an initial qb per replicate and entry in [0.5, 1.5) as the
    reference's rand() would draw it."""
    rng = np.random.default_rng(seed)
    N, D, K = st0["A_mean"].shape[0], st0["A_mean"].shape[1], st0["C_mean"].shape[1]
    for w in which:
        rows = ROWS[w](D, K)
        g = (np.arange(D)[:, None] * rows + np.arange(rows)[None, :]) / float(D * rows)
        pri[w + "_entry_a0"] = a0 * (1.0 + g)
        pri[w + "_entry_b0"] = b0 * (2.0 - g)
        st0[w + "_entry_b"] = 0.5 + rng.random((N, D, rows))


def load_entry(path):
    """tests/golden/entry_*.npz -> (meta, Y [N, T, K], st0, pri, lengths, raw) as ard_ref.load_ard; meta["which"] names the matrices
    with DiagonalGamma parents, meta["gamma"] those with Gamma parents."""
    meta, Y, st0, pri, lengths, z = AR.load_ard(path)
    meta["name"] = os.path.basename(path)[6:-4]
    meta["gamma"] = str(z["gamma"])
    return meta, Y, st0, pri, lengths, z


# ----------------------------------------------------------------------------------------------------------------------------
# The cases the device is measured on (tests/test_entry_gpu.py; tests/test_entry_cpu.py checks the float64 comparator's own distance
# from the extended run on them).  N = 3 replicates with different data and different initial qb, per-entry priors; D = 3 / K = 4;
# ragged D = 33 / K = 17 (rows below D on C) and D = 17 / K = 33 (rows above D), each with a partial last group of four columns;
# the full width D = K = 64; a single lane D = K = 1.  Parents on A, on C, on both; Gamma parents on A with DiagonalGamma on C.
# ----------------------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (T, D, K, matrices with DiagonalGamma parents, matrices with Gamma parents, noise, seed, iterations of the extended run)
    "d3k4_AC": (7, 3, 4, "AC", "", "diagonal_gamma", 31405, 2),
    "d33k17_A": (6, 33, 17, "A", "", "diagonal_gamma", 31417, 2),
    "d17k33_C": (6, 17, 33, "C", "", "gamma", 31421, 2),
    "d64k64_AC": (6, 64, 64, "AC", "", "diagonal_gamma", 31430, 1),     # (a long-double iteration at this width takes seconds)
    "d1k1_AC": (12, 1, 1, "AC", "", "diagonal_gamma", 31440, 2),
    "d3k4_mixed": (8, 3, 4, "C", "A", "gamma", 31450, 2),
}
N_CASE = 3
ITERS = 2
BOUNDS = ("reference", "exact")
_cache = {}


def problem(name):
    """(Y, st0, pri) of a case, st0 / pri with the parents' entries; shared between the tests: do not write to the arrays."""
    if ("problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, which, gamma, kind, seed = CASES[name][:7]
        Y, st0, pri = synth.make_problem(T, D, K, N_CASE, seed=seed)
        if kind == "gamma":
            pri["noise"] = "gamma"
            for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
                pri[k] = np.float64(1e-3)
        add_entry_priors(st0, pri, which, seed + 1)
        AR.add_hyperpriors(st0, pri, gamma, seed + 2)
        for a in [Y] + list(st0.values()):
            a.setflags(write=False)
        _cache["problem", name] = (Y, st0, pri)
    return _cache["problem", name]


def snapshot(ms):
    """ard_ref.snapshot, then qb and the expectations of the DiagonalGamma parents, [N, D, rows]."""
    out = AR.snapshot(ms)
    for w in ms[0][1].entry:
        out[w + "_entry_b"] = np.stack([m.entry[w]["qb"] for _, m in ms])
        out[w + "_entry_E"] = np.stack([m.expectation(w) for _, m in ms])
    return out


def trace(name, extended=False):
    """The comparator's run of a case, in float64 or (extended) np.longdouble: (a list over the iterations of (snapshot, {bound mode:
    parts [N, 6]}), min |1/2 ln det qprec| over the columns and iterations): ITERS iterations in float64, the case's own number in
    long double.  Cached; shared between the tests."""
    key = ("trace", name, extended)
    if key not in _cache:
        Y, st0, pri = problem(name)
        if extended:
            import extended_ref as ER
            Y, st0, pri = ER.to_long(Y), ER.to_long(st0), ER.to_long(pri)
        ms = models(Y, st0, pri)
        out, hld = [], np.inf
        for _ in range(CASES[name][7] if extended else ITERS):
            for _, m in ms:
                m.iterate()
                hld = min(hld, m.half_lndet_qprec())
            out.append((snapshot(ms), {b: np.stack([m.elbo_parts(b) for _, m in ms]) for b in BOUNDS}))
        _cache[key] = (out, hld)
    return _cache[key]


TIED = dict(T=12, D=3, K=4, lengths=(5, 12, 2, 9, 3, 7), models=(0, 1, 1, 1, 2, 2), seed=31544)     # models of 1, 3, 2 chains


def tied_problem():
    """(Y, st0, pri, lengths, models) of the tied case: DiagonalGamma parents on both matrices; the rows of a model start from
    different qb (the handle takes the first row's).  Shared: do not write to the arrays."""
    if "tied" not in _cache:
        from pyvb_amd import synth
        c = TIED
        N = len(c["lengths"])
        Y, st0, pri = synth.make_problem(c["T"], c["D"], c["K"], N, seed=c["seed"])
        live = np.arange(c["T"])[None, :] < np.asarray(c["lengths"])[:, None]
        Y = np.where(live[:, :, None], Y, 0.0)
        st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
        add_entry_priors(st0, pri, "AC", c["seed"] + 1)
        for a in [Y] + list(st0.values()):
            a.setflags(write=False)
        _cache["tied"] = (Y, st0, pri, np.asarray(c["lengths"], dtype=np.int32), np.asarray(c["models"], dtype=np.int32))
    return _cache["tied"]


# The stopping tests (tests/test_entry_gpu.py): seeds, tol and max_iters are chosen so that the comparator alone stops every
# replicate / model, at two or more different iterations, with no delta within converge_ref.GUARD of tol.
CONVERGE = dict(T=7, D=3, K=4, seed=31600, tol=1.0, max_iters=20)
CONVERGE_TIED = dict(tol=0.5, max_iters=18)


def converge_problem():
    """(Y, st0, pri) of the per-replicate stopping test: DiagonalGamma parents on both matrices.  Shared: do not write to the arrays."""
    if "converge" not in _cache:
        from pyvb_amd import synth
        c = CONVERGE
        Y, st0, pri = synth.make_problem(c["T"], c["D"], c["K"], N_CASE, seed=c["seed"])
        add_entry_priors(st0, pri, "AC", c["seed"] + 1)
        for a in [Y] + list(st0.values()):
            a.setflags(write=False)
        _cache["converge"] = (Y, st0, pri)
    return _cache["converge"]
