"""Comparator (test infrastructure) for LDS handles whose columns of A and / or C have Gamma precision parents
(include/pyvb_hip.h: pyvb_lds_set_column_precisions): automatic relevance determination.

Nothing of the algorithm is restated: a MODEL here is a model of tests/tied_ref.py (a list of chains that share A, C, Q, R; a plain
replicate is a model of one chain) with a prior dictionary of its own, and the functions of oracle/lds_closed_form.py run on it
unchanged.  Column i of a matrix with hyperpriors has the prior precision E[alpha_i] I = (qa_i / qb_i) I, so

  pri["A_prior_prec"][i] = (qa_i / qb_i) * ones(rows)     before every use; O._lndet_diag of that is rows ln(qa_i / qb_i), exactly
                                                          the reference's Gamma.pass_down_lndet (quirk Q2, nodes_todo.py:144-147)
  alpha_i.update()        qb_i = b0_i + 1/2 sum_k ((M[k,i] - pm[k,i])^2 + V_i[k,k])      Gamma.update, nodes_todo.py:130-138, with
                          the column as the only child and a Constant mean parent; qa_i = a0_i + rows / 2 (:125-128)
  the bound               parts 2 (A) and 3 (C) gain sum_i O.noise_llb("gamma", a0_i, b0_i, qa_i, qb_i) (:149-157); the exact mode
                          (tests/exact_bound_ref.py) also replaces ln qa_i by psi(qa_i) in the columns' own terms, as
                          exact_bound_ref.noise_eln does for Q and R

tests/test_ard_cpu.py pins this composition against the reference's own run of such graphs (tests/golden/ard_*.npz).  Everything
keeps the dtype of the state it is given, so the same code is the extended-precision reference under tests/extended_ref.py.
"""
import numpy as np

import exact_bound_ref as XR
import tied_ref as TR
from oracle import lds_closed_form as O
from oracle._xspecial import digamma

ROWS = {"A": lambda D, K: D, "C": lambda D, K: K}


class Model(object):
    """chains, Ys as tests/tied_ref.py has them; pri: this model's own prior dictionary; alpha: {"A" / "C": dict(a0, b0, qa, qb)}
    for the matrices with hyperpriors, each entry [D]."""

    def __init__(self, Ys, st0s, pri, alpha_b):
        self.pri = dict(pri)
        self.Ys = Ys
        self.chains = TR.make_model(Ys, st0s, self.pri)
        st = self.chains[0]
        self.D, self.K = st["A_mean"].shape[1], st["C_mean"].shape[1]
        dt = st["A_mean"].dtype
        self.alpha = {}
        for w, qb in alpha_b.items():
            rows = ROWS[w](self.D, self.K)
            a0 = np.broadcast_to(np.asarray(pri[w + "_alpha_a0"], dtype=dt), (self.D,)).copy()
            b0 = np.broadcast_to(np.asarray(pri[w + "_alpha_b0"], dtype=dt), (self.D,)).copy()
            self.alpha[w] = dict(a0=a0, b0=b0, qa=a0 + 0.5 * rows, qb=np.asarray(qb, dtype=dt).copy(), rows=rows)
        self._install()

    def _install(self):
        for w, al in self.alpha.items():
            self.pri[w + "_prior_prec"] = (al["qa"] / al["qb"])[:, None] * np.ones((self.D, al["rows"]), dtype=al["qb"].dtype)

    # ---- the updates, in the handle's vocabulary
    def sweep(self, direction):
        TR.sweep(self.chains, self.pri, self.Ys, direction)

    def pooled(self):
        return TR.statistics(self.chains, self.Ys)[1]

    def update_A(self, cols=None):
        TR.update_A(self.chains, self.pri, self.pooled(), cols)

    def update_C(self, cols=None):
        TR.update_C(self.chains, self.pri, self.pooled(), cols)

    def update_Q(self):
        TR.update_Q(self.chains, self.pri, self.pooled(), self.Ys)

    def update_R(self):
        TR.update_R(self.chains, self.pri, self.pooled(), self.Ys)

    def update_alpha(self, which=None):
        for w in (self.alpha if which is None else [which]):
            al, st = self.alpha[w], self.chains[0]
            M, pm = st[w + "_mean"][0], self.pri[w + "_prior_mean"]
            V = np.einsum("ikk->ik", st[w + "_cov"][0])             # [D, rows]
            al["qb"] = al["b0"] + 0.5 * (((M - pm) ** 2).T + V).sum(axis=1)
        self._install()

    def elbo_parts(self, bound="reference"):
        """The six parts of the model's graph, the alpha nodes' terms inside parts 2 and 3."""
        exact = bound == "exact"
        out = TR.elbo_parts(self.chains, self.pri, self.Ys, XR.elbo_parts_exact if exact else None)
        for w, p in (("A", 2), ("C", 3)):
            if w in self.alpha:
                al = self.alpha[w]
                out[p] += O.noise_llb("gamma", al["a0"], al["b0"], al["qa"], al["qb"]).sum()
                if exact:       # E[ln det alpha_i I] = rows (psi(qa) - ln qb) instead of rows (ln qa - ln qb), at weight 1/2
                    out[p] += 0.5 * al["rows"] * (digamma(al["qa"]) - np.log(al["qa"])).sum()
        return out

    def iterate(self, bound="reference"):
        """forward, backward, A, C, Q, R, alpha_A, alpha_C, bound: pyvb_lds_iterate on such a handle."""
        self.sweep("forward")
        self.sweep("backward")
        S = self.pooled()
        TR.update_A(self.chains, self.pri, S)
        TR.update_C(self.chains, self.pri, S)
        TR.update_Q(self.chains, self.pri, S, self.Ys)
        TR.update_R(self.chains, self.pri, S, self.Ys)
        self.update_alpha()
        return self.elbo_parts(bound)

    def expectation(self, w):
        return self.alpha[w]["qa"] / self.alpha[w]["qb"]


def split_alpha(st0):
    """(st0 without the alpha entries, {"A" / "C": qb [N, D]})"""
    alpha = {k[0]: v for k, v in st0.items() if k.endswith("_alpha_b")}
    return {k: v for k, v in st0.items() if not k.endswith("_alpha_b")}, alpha


def models(Y, st0, pri, lengths=None, model_ids=None):
    """What LDSBatch.from_problem(Y, st0, pri, lengths=, models=) was given, as a list of (rows, Model): st0 carries A_alpha_b /
    C_alpha_b [N, D] for the matrices with hyperpriors, pri their A_alpha_a0 / A_alpha_b0 (the same for C).  A model's
    parameters and qb are those of its first row."""
    N, T = Y.shape[:2]
    lengths = [T] * N if lengths is None else [int(t) for t in lengths]
    ids = np.arange(N) if model_ids is None else np.asarray(model_ids)
    st0, alpha = split_alpha(st0)
    out = []
    for m in range(int(ids.max()) + 1):
        rows = [int(n) for n in np.nonzero(ids == m)[0]]
        f = rows[0]
        Ys = [Y[n:n + 1, :lengths[n]].copy() for n in rows]
        st0s = [{k: (v[n:n + 1, :lengths[n]] if k == "X" else v[f:f + 1]).copy() for k, v in st0.items()} for n in rows]
        out.append((rows, Model(Ys, st0s, pri, {w: qb[f] for w, qb in alpha.items()})))
    return out


def add_hyperpriors(st0, pri, which, seed, a0=1e-3, b0=1e-3):
    """Gamma parents for the columns of the matrices named in `which` ("A", "C" or "AC") on a problem of synth.make_problem:
    broad priors, per column (slightly different ones, so that a column stride of 0 shows), and an initial qb per replicate and
    column in [0.5, 1.5) as the reference's rand() would draw it (nodes_todo.py:119)."""
    rng = np.random.default_rng(seed)
    N, D = st0["A_mean"].shape[0], st0["A_mean"].shape[1]
    for w in which:
        pri[w + "_alpha_a0"] = a0 * (1.0 + np.arange(D) / D)
        pri[w + "_alpha_b0"] = b0 * (2.0 - np.arange(D) / D)
        st0[w + "_alpha_b"] = 0.5 + rng.random((N, D))


def pack(out):
    """A fixture's dict of small arrays, numbers and strings as two .npz entries -- an entry costs more than most of these arrays
    hold: "data", every numeric value flattened into one float64 vector (integers are exact there), and "layout", one line per
    key, `name shape` for what lies in data and `name =text` for a string."""
    lines, data = [], []
    for k, v in out.items():
        if isinstance(v, str):
            lines.append("%s =%s" % (k, v))
            continue
        v = np.asarray(v)
        lines.append("%s %s%s" % (k, "i" if v.dtype.kind in "iu" else "f", ",".join(str(n) for n in v.shape)))
        data.append(v.astype(np.float64).ravel())
    return {"layout": np.array("\n".join(lines)), "data": np.concatenate(data)}


def unpack(z):
    out, pos = {}, 0
    for line in str(z["layout"]).split("\n"):
        k, spec = line.split(" ", 1)
        if spec.startswith("="):
            out[k] = spec[1:]
            continue
        shape = tuple(int(n) for n in spec[1:].split(",")) if spec[1:] else ()
        n = int(np.prod(shape, dtype=np.int64))
        v = z["data"][pos:pos + n].reshape(shape)
        out[k] = v.astype(np.int64) if spec[0] == "i" else v.copy()
        pos += n
    assert pos == z["data"].size
    return out


def load_ard(path):
    """tests/golden/ard_*.npz -> (meta, Y [N, T, K], st0, pri, lengths, raw): the inputs as LDSBatch.from_problem takes them, one
    model whose chains are the fixture's (st0's parameter rows are the model's, repeated)."""
    import os
    z = unpack(dict(np.load(path, allow_pickle=False)))
    for k in [k for k in z if k.startswith("snap_")]:       # the checkpoints are stacked per quantity: back to it<i>_<quantity>
        for i, it in enumerate(z["iters"]):
            z["it%d_%s" % (int(it), k[5:])] = z[k][i]
        del z[k]
    lengths = [int(t) for t in z["lengths"]]
    N = len(lengths)
    pri = {k[6:]: z[k].copy() for k in z if k.startswith("prior_")}
    pri["noise"] = str(z["noise"])
    st0 = {k[5:]: np.repeat(z[k][None], N, axis=0) for k in z if k.startswith("init_") and k != "init_X"}
    st0["X"] = z["init_X"].copy()
    meta = {"lengths": lengths, "D": int(z["D"]), "K": int(z["K"]), "noise": pri["noise"], "iters": [int(i) for i in z["iters"]],
            "which": str(z["which"]), "name": os.path.basename(path)[4:-4]}
    return meta, z["Y"].copy(), st0, pri, lengths, z


# ----------------------------------------------------------------------------------------------------------------------------
# The cases the device is measured on (tests/test_ard_gpu.py; tests/test_ard_cpu.py checks the float64 comparator's own distance
# from the extended run on them).  The smallest shapes at which the kernels can still go wrong: N = 3 replicates with different data
# and different initial qb (a replicate stride of 0 shows), per-column priors (a column stride of 0 shows); D = 3 / K = 4; ragged
# D = 33 / K = 17 (K < D) and D = 17 / K = 33 (K > D), each more than one block of 16 columns and no multiple of 4; the full width
# D = K = 64.  Hyperpriors on A only, on C only, on both.
# ----------------------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (T, D, K, matrices with hyperpriors, noise, seed, iterations of the extended run)
    "d3k4_AC": (7, 3, 4, "AC", "diagonal_gamma", 21400, 2),
    "d33k17_A": (5, 33, 17, "A", "diagonal_gamma", 21410, 2),
    "d17k33_C": (6, 17, 33, "C", "gamma", 21420, 2),
    "d64k64_AC": (4, 64, 64, "AC", "diagonal_gamma", 21430, 1),     # (a long-double iteration at this width takes seconds)
}
N_CASE = 3
ITERS = 2
BOUNDS = ("reference", "exact")
_cache = {}


def problem(name):
    """(Y, st0, pri) of a case, st0 / pri with the alpha entries; shared between the tests: do not write to the arrays."""
    if ("problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, which, kind, seed = CASES[name][:6]
        Y, st0, pri = synth.make_problem(T, D, K, N_CASE, seed=seed)
        if kind == "gamma":
            pri["noise"] = "gamma"
            for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
                pri[k] = np.float64(1e-3)
        add_hyperpriors(st0, pri, which, seed + 1)
        for a in [Y] + list(st0.values()):
            a.setflags(write=False)
        _cache["problem", name] = (Y, st0, pri)
    return _cache["problem", name]


QUANTITIES = ("X", "Sigma", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b")


def snapshot(ms):
    """What a trace records of a list of (rows, Model) of single-chain models: arrays [N, ...] in the handle's layout."""
    sts = [m.chains[0] for _, m in ms]
    out = {k: np.concatenate([st[k] for st in sts]) for k in ("X", "Sigma", "A_mean", "C_mean")}
    for w in ("A", "C"):
        out[w + "_colvar"] = np.concatenate([np.einsum("nikk->nik", st[w + "_cov"]) for st in sts])
    for nm, dim in (("Q_b", out["A_mean"].shape[1]), ("R_b", out["C_mean"].shape[1])):
        out[nm] = np.stack([np.broadcast_to(st[nm][0], (dim,)) for st in sts])
    for w in ms[0][1].alpha:
        out[w + "_alpha_b"] = np.stack([m.alpha[w]["qb"] for _, m in ms])
        out[w + "_alpha_E"] = np.stack([m.expectation(w) for _, m in ms])
    return out


def trace(name, extended=False):
    """The comparator's run of a case, in float64 or (extended) np.longdouble: a list over the iterations of (snapshot, {bound mode:
    parts [N, 6]}): ITERS iterations in float64, the case's own number in long double.  Cached; shared between the tests."""
    key = ("trace", name, extended)
    if key not in _cache:
        Y, st0, pri = problem(name)
        if extended:
            import extended_ref as ER
            Y, st0, pri = ER.to_long(Y), ER.to_long(st0), ER.to_long(pri)
        ms = models(Y, st0, pri)
        out = []
        for _ in range(CASES[name][6] if extended else ITERS):
            for _, m in ms:
                m.iterate()
            out.append((snapshot(ms), {b: np.stack([m.elbo_parts(b) for _, m in ms]) for b in BOUNDS}))
        _cache[key] = out
    return _cache[key]


TIED = dict(T=12, D=3, K=4, lengths=(5, 12, 2, 9, 3, 7), models=(0, 1, 1, 1, 2, 2), seed=21500)     # models of 1, 3, 2 chains; lengths 2 and 3


def tied_problem():
    """(Y, st0, pri, lengths, models) of the tied case: hyperpriors on both matrices; the rows of a model start from different qb
    (the handle takes the first row's).  Shared: do not write to the arrays."""
    if "tied" not in _cache:
        from pyvb_amd import synth
        c = TIED
        N = len(c["lengths"])
        Y, st0, pri = synth.make_problem(c["T"], c["D"], c["K"], N, seed=c["seed"])
        live = np.arange(c["T"])[None, :] < np.asarray(c["lengths"])[:, None]
        Y = np.where(live[:, :, None], Y, 0.0)
        st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
        add_hyperpriors(st0, pri, "AC", c["seed"] + 1)
        for a in [Y] + list(st0.values()):
            a.setflags(write=False)
        _cache["tied"] = (Y, st0, pri, np.asarray(c["lengths"], dtype=np.int32), np.asarray(c["models"], dtype=np.int32))
    return _cache["tied"]
