"""Comparator (test infrastructure) for LDS handles with known regressors in the output equation (include/pyvb_hip.h:
pyvb_lds_create_regressors):

    Y_t = Gaussian(K, C * X_t + E * Constant(v_t), R),    E = hstack(Es),    t = 0 .. T-1

an Addition of two Multiplications in the reference (node.py:52-129, :182-276) with hstack.pass_up_m1_m2 (nodes_todo.py:43-62) for
the columns of E; with P > 0 also the known input of tests/inputs_ref.py in the state equation.  Model subclasses inputs_ref.Model
(P = 0 allowed: U, B_mean and B_colvar are then empty arrays and B is never updated), so the functions of oracle/lds_closed_form.py
run wherever they apply and only the added terms are restated:

    states     the message of Y_t to X_t: <C>^T <R> (y_t - f_t),   f_t = <E> v_t        (Addition.pass_up_m1_m2 node.py:95-110)
    sums       Svx = sum_t v_t mu_t^T,  Svv = sum_t v_t v_t^T,  Syv = sum_t y_t v_t^T,  every t = 0 .. T-1
    columns    C with H = Syx - <E> Svx;  E with G = Svv and H = Syv - <C> Svx^T, row precisions <R>;  E sees the new C
    R          the second moment of the mean parent gains E(<E>, S^E, Svv) + <C> Svx^T <E>^T + its transpose (Addition.pass_down_ExxT
               :121-129), the cross term Syv <E>^T
    bound      the same second moment in L_Y; the columns of E add to part 3 what the columns of C do

tests/test_regressors_cpu.py pins this composition against the reference's own run of such graphs (tests/golden/regressors_*.npz).
Everything keeps the dtype of the state it is given, so the same code is the extended-precision reference under
tests/extended_ref.py.  The rows past a chain's end are never read.
"""
import numpy as np

import inputs_ref as IR
from oracle import _xlinalg as XL
from oracle import lds_closed_form as O
from oracle._xspecial import ln2pi as _ln2pi

E_KEYS = ("E_mean", "E_colvar")


def split_regressors(st0):
    """(st0 without the entries of E, those entries)"""
    return {k: v for k, v in st0.items() if k not in E_KEYS}, {k: v for k, v in st0.items() if k in E_KEYS}


class Model(IR.Model):
    """N replicates with chains of one length T: Y [N, T, K], U [N, T, P] or None (P = 0), V [N, T, Pv], st0 as
    synth.make_regression_problem gives it (E_mean [N, K, Pv], E_colvar [N, Pv, K] beside the rest), pri with E_prior_mean [K, Pv]
    and E_prior_prec [Pv, K]."""

    def __init__(self, Y, U, V, st0, pri):
        rest, e = split_regressors(st0)
        N, T = Y.shape[:2]
        D = rest["A_mean"].shape[1]
        if U is None:       # no input: empty arrays of the data's dtype, so that every sum over the channels of B is an empty one
            U = np.zeros((N, T, 0), dtype=Y.dtype)
            rest = dict(rest, B_mean=np.zeros((N, D, 0), dtype=Y.dtype), B_colvar=np.zeros((N, 0, D), dtype=Y.dtype))
            pri = dict(pri, B_prior_mean=np.zeros((D, 0), dtype=Y.dtype), B_prior_prec=np.zeros((0, D), dtype=Y.dtype))
        IR.Model.__init__(self, Y, U, rest, pri)
        st = self.st
        self.V = V
        st["E_mean"] = e["E_mean"].copy()
        st["E_cov"] = np.einsum("nik,kl->nikl", e["E_colvar"], np.eye(e["E_colvar"].shape[2]))
        st["qld_E"] = np.full(st["E_mean"].shape[:1] + st["E_mean"].shape[2:], np.nan, dtype=st["E_mean"].dtype)
        self.Pv = st["E_mean"].shape[2]
        self.Svv = np.einsum("ntp,ntq->npq", V, V)
        self.Syv = np.einsum("ntk,ntp->nkp", Y, V)

    # ---- states: the outputs enter as y_t - f_t
    def _on_residual(self, fn, *args):
        Y = self.Y
        self.Y = Y - np.einsum("nkp,ntp->ntk", self.st["E_mean"], self.V)
        try:
            fn(self, *args)
        finally:
            self.Y = Y

    def sweep(self, direction):
        self._on_residual(IR.Model.sweep, direction)

    def update_x(self, t):
        self._on_residual(IR.Model.update_x, t)

    # ---- sums
    def statistics(self):
        S = IR.Model.statistics(self)
        S["Svx"] = np.einsum("ntp,ntj->npj", self.V, self.st["X"])
        S["Svv"], S["Syv"] = self.Svv, self.Syv
        return S

    def _Rbar(self):
        return O.noise_expect(self.pri["noise"], self.st["R_a"], self.st["R_b"], self.K)

    # ---- columns, in the order As, [Bs], Cs, Es
    def _HC(self, S):
        return S["Syx"] - np.einsum("nkp,npj->nkj", self.st["E_mean"], S["Svx"])

    def update_B(self, S=None):
        if self.P:
            IR.Model.update_B(self, S)

    def update_C(self, S=None):
        S = S or self.statistics()
        st, pri = self.st, self.pri
        st["qld_C"] = O._update_columns(st["C_mean"], st["C_cov"], pri["C_prior_mean"], pri["C_prior_prec"], self._Rbar(), S["Sxx"], self._HC(S))

    def update_E(self, S=None):
        S = S or self.statistics()
        st, pri = self.st, self.pri
        H = S["Syv"] - np.einsum("nkj,npj->nkp", st["C_mean"], S["Svx"])
        st["qld_E"] = O._update_columns(st["E_mean"], st["E_cov"], pri["E_prior_mean"], pri["E_prior_prec"], self._Rbar(), S["Svv"], H)

    # ---- noise
    def _cross(self, S):
        """<C> Svx^T <E>^T: the cross term of the mean parent's second moment, which enters with its transpose"""
        return np.einsum("nkj,npj,nlp->nkl", self.st["C_mean"], S["Svx"], self.st["E_mean"])

    def _output_moments(self, S):
        """(E, HM): sum_t <y_t y_t^T> + sum_t <pmu_t pmu_t^T> and sum_t y_t <pmu_t>^T for pmu_t = C x_t + E v_t"""
        st = self.st
        E, HM = O._residual_second_moment(S["Syy"], st["C_mean"], st["C_cov"], S["Sxx"], S["Syx"])
        cross = self._cross(S)
        E = E + O.outer_expect(st["E_mean"], st["E_cov"], S["Svv"]) + cross + np.swapaxes(cross, 1, 2)
        HM = HM + np.einsum("nkp,nlp->nkl", S["Syv"], st["E_mean"])
        return E, HM

    def update_R(self, S=None):
        S = S or self.statistics()
        st, pri, kind = self.st, self.pri, self.pri["noise"]
        E, HM = self._output_moments(S)
        if kind == "diagonal_gamma":
            st["R_b"] = pri["R_b0"][None] + 0.5 * np.einsum("nii->ni", E) - np.einsum("nii->ni", HM)
        else:
            st["R_b"] = pri["R_b0"] + 0.5 * np.einsum("nii->n", E) - np.einsum("nii->n", HM)
        st["R_a"] = O._bcast_a(O.noise_a(kind, pri["R_a0"], self.T, self.K), st["R_b"], kind)

    # ---- bound
    def elbo_parts(self, bound="reference"):
        st, pri = self.st, self.pri
        out = IR.Model.elbo_parts(self, bound)
        S = self.statistics()
        exact = bound == "exact"
        # L_Y: the second moment of the mean parent with the regressors' terms
        E0, HM0 = O._residual_second_moment(S["Syy"], st["C_mean"], st["C_cov"], S["Sxx"], S["Syx"])
        E, HM = self._output_moments(S)
        out[:, 1] += -0.5 * np.einsum("nij,nji->n", self._Rbar(), (E - E0) - 2 * (HM - HM0))
        # the columns of E against their Constant parents (gaussian.py:141-147), into part 3
        M, Mcov, pm, pp = st["E_mean"], st["E_cov"], pri["E_prior_mean"], pri["E_prior_prec"]
        rows, LN2PI = self.K, _ln2pi(st["X"])
        for i in range(self.Pv):
            ex = np.einsum("nk,nl->nkl", M[:, :, i], M[:, :, i]) + Mcov[:, i] \
                + np.outer(pm[:, i], pm[:, i])[None] - 2 * np.einsum("nk,l->nkl", M[:, :, i], pm[:, i])
            out[:, 3] += -0.5 * rows * LN2PI + 0.5 * O._lndet_diag(pp[i]) - 0.5 * np.einsum("k,nkk->n", pp[i], ex)
            ent = XL.slogdet(Mcov[:, i])[1] if exact else st["qld_E"][:, i]
            out[:, 3] += 0.5 * rows * LN2PI + 0.5 * ent + 0.5 * rows
        return out

    def iterate(self, bound="reference"):
        """forward, backward, As, [Bs], Cs, Es, Q, R, bound: pyvb_lds_iterate on such a handle."""
        self.sweep("forward")
        self.sweep("backward")
        S = self.statistics()
        self.update_A(S)
        self.update_B(S)
        self.update_C(S)
        self.update_E(S)
        self.update_Q(S)
        self.update_R(S)
        return self.elbo_parts(bound)


def models(Y, U, V, st0, pri, lengths=None, cls=Model):
    """What LDSBatch.from_problem(Y, st0, pri, U=U, V=V, lengths=) was given, as a list of (rows, Model): one model of all N
    replicates where the chains have one length, one per replicate otherwise (rows past a chain's end are cut off)."""
    N, T = Y.shape[:2]
    if lengths is None or all(int(t) == T for t in lengths):
        return [(list(range(N)), cls(Y, U, V, st0, pri))]
    return [([n], cls(Y[n:n + 1, :Tn], None if U is None else U[n:n + 1, :Tn], V[n:n + 1, :Tn],
                      {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}, pri))
            for n, Tn in enumerate(int(t) for t in lengths)]


def quantities(P):
    return tuple(q for q in ("X", "Sigma", "A_mean", "A_colvar", "B_mean", "B_colvar", "C_mean", "C_colvar", "E_mean", "E_colvar", "Q_b", "R_b")
                 if P or q[0] != "B")


def snapshot(ms, T):
    """What a trace records of a list of (rows, Model): arrays [N, ...] in the handle's layout (padding rows of X: 0)."""
    out = IR.snapshot(ms, T)
    out["E_mean"] = np.concatenate([m.st["E_mean"] for _, m in ms])
    out["E_colvar"] = np.concatenate([np.einsum("nikk->nik", m.st["E_cov"]) for _, m in ms])
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# The cases the device is measured on (tests/test_regressors_gpu.py; tests/test_regressors_cpu.py checks the float64 comparator's own
# distance from the extended run on them): T, D, K, P, Pv, chain lengths or None, time split or None, iterations of the extended run.
# ----------------------------------------------------------------------------------------------------------------------------
CASES = {
    "t19_d6k4v2": (19, 6, 4, 0, 2, None, None, 2),                  # P = 0, one tile
    "t19_d6k4p2v1": (19, 6, 4, 2, 1, None, None, 2),                # both kinds of input
    "t33_d5k14v3": (33, 5, 14, 0, 3, None, None, 2),                # Kt = 17 crosses a tile
    "t77_d16k16p4v8": (77, 16, 16, 4, 8, None, None, 2),            # Kt = 32
    "t40_d64k40p6v12": (40, 64, 40, 6, 12, None, None, 1),          # Kt = 64 and D = 64 (a long-double iteration at this width takes seconds)
    "t12_d3k1v63": (12, 3, 1, 0, 63, None, None, 2),                # the widest E
    "t700_d8k8p2v3_w4": (700, 8, 8, 2, 3, None, 4, 2),              # several wavefronts per chain
    "lengths_d16k10p2v3": (77, 16, 10, 2, 3, (2, 3, 19, 60, 77), None, 2),      # the v channel in a chain's own last row and in no padding row
}
SEEDS = {"t19_d6k4v2": 32400, "t19_d6k4p2v1": 32410, "t33_d5k14v3": 32420, "t77_d16k16p4v8": 32430, "t40_d64k40p6v12": 32440,
         "t12_d3k1v63": 32450, "t700_d8k8p2v3_w4": 32460, "lengths_d16k10p2v3": 32470}
ITERS = 2
BOUNDS = IR.BOUNDS
_cache = {}


def n_case(name):
    ln = CASES[name][5]
    return 2 if ln is None else len(ln)


def problem(name):
    """(Y, U, V, st0, pri, lengths) of a case; shared between the tests: do not write to the arrays.  With chain lengths the padding
    rows of Y, U and X are zero; those of V are NOT: a v channel that is live in a padding row shows."""
    if ("problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, P, Pv, ln = CASES[name][:6]
        Y, U, V, st0, pri = synth.make_regression_problem(T, D, K, P, Pv, n_case(name), seed=SEEDS[name])
        if ln is not None:
            live = (np.arange(T)[None, :] < np.asarray(ln)[:, None])[:, :, None]
            Y = np.where(live, Y, 0.0)
            U = None if U is None else np.where(live, U, 0.0)
            st0["X"] = np.where(live, st0["X"], 0.0)
        for a in [Y, V] + ([] if U is None else [U]) + list(st0.values()):
            a.setflags(write=False)
        _cache["problem", name] = (Y, U, V, st0, pri, None if ln is None else np.asarray(ln, dtype=np.int32))
    return _cache["problem", name]


def stages(P):
    """the stages of an iteration in the order pyvb_lds_iterate runs them, each with the quantities it produces"""
    return tuple(s for s in IR.STAGES[:4] if P or s[0] != "B") + (("C", ("C_mean", "C_colvar")), ("E", ("E_mean", "E_colvar")),
                                                                  ("Q", ("Q_b",)), ("R", ("R_b",)))


def run_stages(do, snap, bound, iters, P):
    """inputs_ref.run_stages over stages(P)."""
    out = []
    for it in range(iters):
        for stage, keys in stages(P):
            do(stage)
            s = snap()
            out += [((it, stage, k), np.array(s[k])) for k in keys]
        out += [((it, "bound", mode), np.array(bound(mode))) for mode in BOUNDS]
    return out


do_stage = IR.do_stage


def trace(name, extended=False):
    """The comparator's stage-by-stage run of a case (run_stages), in float64 or (extended) np.longdouble: ITERS iterations in
    float64, the case's own number in long double.  Cached; shared between the tests."""
    key = ("trace", name, extended)
    if key not in _cache:
        Y, U, V, st0, pri, ln = problem(name)
        if extended:
            import extended_ref as ER
            Y, U, V, st0, pri = ER.to_long(Y), None if U is None else ER.to_long(U), ER.to_long(V), ER.to_long(st0), ER.to_long(pri)
        ms = models(Y, U, V, st0, pri, ln)
        _cache[key] = run_stages(lambda stage: [do_stage(m, stage) for _, m in ms], lambda: snapshot(ms, CASES[name][0]),
                                 lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), CASES[name][7] if extended else ITERS,
                                 CASES[name][3])
    return _cache[key]


# ----------------------------------------------------------------------------------------------------------------------------
# Channel by channel (tests/test_input_channels_cpu.py, tests/test_input_channels_gpu.py; extended_ref.compare_channels): as
# inputs_ref.CHANNEL_CASES, with the channels of V replaced by named patterns too -- channel 0 stays the constant 1 -- and finite
# random values in the padding rows of V as well.  T, D, K, P, Pv, chain lengths or None, time split or None, iterations of the
# extended run, big (small = 1 / big).
# ----------------------------------------------------------------------------------------------------------------------------
V_PATTERNS = ("as drawn", "x big", "x small", "impulse at t = 0", "impulse at t = T_n - 1", "as drawn", "as drawn", "as drawn")
CHANNEL_CASES = {
    "t48_d17k2p17v16": (48, 17, 2, 17, 16, None, None, 2, 30.0),        # all three groups, K0 = 36 inside a tile, Pv a full tile
    "t48_d33k1p16v31": (48, 33, 1, 16, 31, None, None, 2, 30.0),        # Kt = 64 with all three groups; PT = 2 with 15 real columns; K0 = 33
    "t40_d5k3v33": (40, 5, 3, 0, 33, None, None, 2, 30.0),              # PT = 3 with one real column, P = 0 (k_rg_gains writes the rows of <C>)
    "t40_d5k31v33": (40, 5, 31, 0, 33, None, None, 2, 30.0),            # K + Pv = 64: RE at 1023 of 1024; K = 31 in the clamped loads
    "t48_d64k2p24v14": (48, 64, 2, 24, 14, None, None, 1, 30.0),        # Kt = 64 at D = 64 (one long-double iteration)
    "lengths_d16k10p5v9": (77, 16, 10, 5, 9, (2, 3, 19, 60, 77), None, 2, 30.0),       # every pattern in every chain, live padding
}
# (chosen as inputs_ref.CHANNEL_SEEDS are.  One output, 31 regressors and 33 states on 48 rows leave the columns of E close to the cap
# on the reference side: of seeds 34410 .. 34423 this is the first under it, 2.0e-12 by channel; the others are at 1.1e-11 .. 3e-10)
CHANNEL_SEEDS = {"t48_d17k2p17v16": 34400, "t48_d33k1p16v31": 34423, "t40_d5k3v33": 34420, "t40_d5k31v33": 34430, "t48_d64k2p24v14": 34440,
                 "lengths_d16k10p5v9": 34450}


def channel_lengths(name):
    """int [N]: the chain length of every replicate of a case of CHANNEL_CASES"""
    T, ln = CHANNEL_CASES[name][0], CHANNEL_CASES[name][5]
    return np.full(2, T, dtype=np.int32) if ln is None else np.asarray(ln, dtype=np.int32)


def pattern_regressors(V, lengths, big, rng):
    """(V with channel p >= 1 of every replicate replaced by pattern p mod 8 of V_PATTERNS on the rows 0 .. T_n - 1 that are used,
    the label of every [replicate][channel]).  Channel 0 stays the constant 1 (a second constant would be collinear with it); the
    padding rows t >= T_n are redrawn: finite, not zero."""
    V = V.copy()
    N, T, Pv = V.shape
    labels = []
    for n, Tn in enumerate(int(t) for t in lengths):
        labels.append(["constant 1"])
        for p in range(1, Pv):
            k = p % 8
            v = V[n, :Tn, p]
            if k == 1:
                v *= big
            elif k == 2:
                v /= big
            elif k in (3, 4):
                v[:] = 0.0
                v[0 if k == 3 else Tn - 1] = 1.0
            labels[-1].append(V_PATTERNS[k])
        V[n, Tn:] = rng.standard_normal((T - Tn, Pv))
    assert np.all(V[:, :1, 0] == 1.0)
    return V, labels


def channel_problem(name):
    """(Y, U or None, V, st0, pri, lengths or None, the labels of U, the labels of V) of a case of CHANNEL_CASES; shared: do not write."""
    if ("channel problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, P, Pv, ln, _, _, big = CHANNEL_CASES[name]
        lengths = channel_lengths(name)
        Y, U, V, st0, pri = synth.make_regression_problem(T, D, K, P, Pv, len(lengths), seed=CHANNEL_SEEDS[name])
        rng = np.random.default_rng(CHANNEL_SEEDS[name] + 1)
        ulabels = None
        if P:
            U, ulabels = IR.pattern_inputs(U, lengths, big, rng)
        V, vlabels = pattern_regressors(V, lengths, big, rng)
        live = (np.arange(T)[None, :] < lengths[:, None])[:, :, None]
        Y = np.where(live, Y, rng.standard_normal(Y.shape))
        st0["X"] = np.where(live, st0["X"], 0.0)
        for a in [Y, V] + ([] if U is None else [U]) + list(st0.values()):
            a.setflags(write=False)
        _cache["channel problem", name] = (Y, U, V, st0, pri, None if ln is None else lengths, ulabels, vlabels)
    return _cache["channel problem", name]


def channel_run(prob, extended=False, iters=ITERS, cls=Model):
    """run_stages of the comparator on a problem (Y, U, V, st0, pri, lengths, ...), in float64 or cast up to long double"""
    Y, U, V, st0, pri, ln = prob[:6]
    if extended:
        import extended_ref as ER
        Y, U, V, st0, pri = ER.to_long(Y), None if U is None else ER.to_long(U), ER.to_long(V), ER.to_long(st0), ER.to_long(pri)
    ms = models(Y, U, V, st0, pri, ln, cls)
    return run_stages(lambda stage: [do_stage(m, stage) for _, m in ms], lambda: snapshot(ms, Y.shape[1]),
                      lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), iters, 0 if U is None else U.shape[2])


def channel_trace(name, extended=False):
    """trace() for a case of CHANNEL_CASES.  Cached; shared between the tests."""
    key = ("channel trace", name, extended)
    if key not in _cache:
        _cache[key] = channel_run(channel_problem(name), extended, CHANNEL_CASES[name][7] if extended else ITERS)
    return _cache[key]


# The kappa-clause of DESIGN.md section 17 on the residual of R.  update_R forms qb = b0 + 1/2 diag(Syy) + 1/2 diag(second moment of
# the mean parent) - diag(Syx <C>^T + Syv <E>^T).  With one output, 31 regressors and 33 states on 48 rows the fit leaves almost nothing:
# on t48_d33k1p16v31 the terms are 1.2e6, 1.1e6 and -2.2e6 for qb = 931 (replicate 1, iteration 1), kappa = sum |terms| / |qb| = 5090,
# and one rounding of the largest term is 2.5e-13 of qb in ANY float64 evaluation.  The float64 comparator happens to land at 5e-15
# there, so its e64 says nothing about the sum, and what follows from that qb -- the variances of the columns of E, 1 / (p0 + <R> Svv),
# one to one; the reference-mode L_C through quirk Q1's 1 / ln(prec) -- inherits the rounding.  For the cases listed here the
# yardstick of a unit therefore also admits what ONE such rounding does to it, measured on the reference side: the long-double run
# once more with qb (1 +- kappa 2^-52) after every update_R, kappa from that run, and every unit's distance from the unperturbed run
# (kappa_allowance; extended_ref.compare_channels takes the larger of the two signs, capped at extended_ref.CAP).
KAPPA_CASES = ("t48_d33k1p16v31",)


def residual_condition(m, S):
    """kappa [N, K] of the sum update_R is about to form on a Model with diagonal noise: sum |terms| / |sum of the terms|"""
    st = m.st
    E2, HM = O._residual_second_moment(S["Syy"], st["C_mean"], st["C_cov"], S["Sxx"], S["Syx"])
    terms = [0.5 * S["Syy"], 0.5 * (E2 - S["Syy"]), 0.5 * O.outer_expect(st["E_mean"], st["E_cov"], S["Svv"]), m._cross(S), -HM,
             -np.einsum("nkp,nlp->nkl", S["Syv"], st["E_mean"])]
    d = [np.einsum("nii->ni", t) for t in terms] + [np.broadcast_to(m.pri["R_b0"], (st["X"].shape[0], m.K))]
    return sum(np.abs(t) for t in d) / np.abs(sum(d))


class RoundedResidualR(Model):
    """Model whose update_R is followed by one rounding of the sum's largest terms: R_b (1 + sign kappa 2^-52)"""
    sign = 1

    def update_R(self, S=None):
        S = S or self.statistics()
        assert self.pri["noise"] == "diagonal_gamma"
        kappa = residual_condition(self, S)
        Model.update_R(self, S)
        self.st["R_b"] = self.st["R_b"] * (1 + self.sign * kappa * 2.0 ** -52)


def kappa_allowance(name):
    """[the long-double trace of the case with R_b rounded up after every update_R, the same rounded down] for a case of KAPPA_CASES"""
    assert name in KAPPA_CASES
    key = ("kappa", name)
    if key not in _cache:
        down = type("RoundedDown", (RoundedResidualR,), {"sign": -1})
        _cache[key] = [channel_run(channel_problem(name), True, CHANNEL_CASES[name][7], cls) for cls in (RoundedResidualR, down)]
    return _cache[key]


def load_fixture(path):
    """tests/golden/regressors_*.npz -> (meta, Y [N, T, K], U [N, T, P] or None, V [N, T, Pv], st0, pri, lengths, z)"""
    z = dict(np.load(path, allow_pickle=False))
    lengths = [int(t) for t in z["lengths"]]
    pri = {k[6:]: z[k].copy() for k in z if k.startswith("prior_")}
    pri["noise"] = str(z["noise"])
    if pri["noise"] == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(pri[k])
    st0 = {k[5:]: z[k].copy() for k in z if k.startswith("init_")}
    meta = {"lengths": lengths, "D": int(z["D"]), "K": int(z["K"]), "P": int(z["P"]), "Pv": int(z["Pv"]), "noise": pri["noise"],
            "iters": [int(i) for i in z["iters"]]}
    return meta, z["Y"].copy(), z["U"].copy() if "U" in z else None, z["V"].copy(), st0, pri, lengths, z
