"""Comparator (test infrastructure) for LDS handles with a known input (include/pyvb_hip.h: pyvb_lds_create_inputs):

    X_t = Gaussian(q, A * X_{t-1} + B * Constant(u_t), Q),    B = hstack(Bs),    t = 1 .. T-1

an Addition of two Multiplications in the reference (node.py:52-129, :182-276) with hstack.pass_up_m1_m2 (nodes_todo.py:43-62) for
the columns of B.  The functions of oracle/lds_closed_form.py run wherever they apply -- state_posteriors (the posterior precisions
of the states do not depend on the input), _update_columns (A with H = Sx1x - <B> Su1x, B with G = Suu and H = Sxu - <A> Su1x^T, C as
it is), _residual_second_moment, update_R, elbo_parts, noise_llb -- and only the added terms are restated:

    states     pmu_t = <A> mu_{t-1} + e_t,  the message of X_{t+1} to X_t: <A>^T <Q> (mu_{t+1} - e_{t+1}),   e_t = <B> u_t
               (Addition.pass_down_Ex node.py:112-119; Addition.pass_up_m1_m2 :95-110)
    sums       Su1x = sum_{t=0}^{T-2} u_{t+1} mu_t^T,  Sxu = sum_{t=1}^{T-1} mu_t u_t^T,  Suu = sum_{t=1}^{T-1} u_t u_t^T
    Q          the second moment of the mean parent gains E(<B>, S^B, Suu) + <A> Su1x^T <B>^T + its transpose (Addition.pass_down_ExxT
               :121-129), the cross term Sxu <B>^T
    bound      the same second moment in L_X; the columns of B add to part 2 what the columns of A do

tests/test_inputs_cpu.py pins this composition against the reference's own run of such graphs (tests/golden/inputs_*.npz).
Everything keeps the dtype of the state it is given, so the same code is the extended-precision reference under
tests/extended_ref.py.  u_0 and the rows past a chain's end are never read.
"""
import numpy as np

import exact_bound_ref as XR
from oracle import _xlinalg as XL
from oracle import lds_closed_form as O
from oracle._xspecial import ln2pi as _ln2pi

B_KEYS = ("B_mean", "B_colvar")


def split_inputs(st0):
    """(st0 without the entries of B, those entries)"""
    return {k: v for k, v in st0.items() if k not in B_KEYS}, {k: v for k, v in st0.items() if k in B_KEYS}


class Model(object):
    """N replicates with chains of one length T: Y [N, T, K], U [N, T, P], st0 as synth.make_input_problem gives it (B_mean [N, D, P],
    B_colvar [N, P, D] beside the rest), pri with B_prior_mean [D, P] and B_prior_prec [P, D]."""

    def __init__(self, Y, U, st0, pri):
        plain, b = split_inputs(st0)
        self.Y, self.U, self.pri = Y, U, pri
        self.T = Y.shape[1]
        self.st = O.expand_state(plain, pri, self.T)
        st = self.st
        st["B_mean"] = b["B_mean"].copy()
        st["B_cov"] = np.einsum("nik,kl->nikl", b["B_colvar"], np.eye(b["B_colvar"].shape[2]))
        st["qld_B"] = np.full(st["B_mean"].shape[:1] + st["B_mean"].shape[2:], np.nan, dtype=st["B_mean"].dtype)
        self.D, self.K, self.P = st["A_mean"].shape[1], st["C_mean"].shape[1], st["B_mean"].shape[2]
        Ud = U[:, 1:]
        self.Suu = np.einsum("ntp,ntq->npq", Ud, Ud)

    # ---- states
    def _e(self, t):
        return np.einsum("nkp,np->nk", self.st["B_mean"], self.U[:, t])

    def _x_step(self, post, t):
        """O._x_step with the input in the mean parent and in the message of X_{t+1}."""
        st, pri, X, T = self.st, self.pri, self.st["X"], self.T
        A, C = st["A_mean"], st["C_mean"]
        Qb, Rb = post["Qbar"], post["Rbar"]
        m2 = np.einsum("nki,nk->ni", C, np.einsum("nkl,nl->nk", Rb, self.Y[:, t]))
        if t < T - 1:
            m2 = m2 + np.einsum("nki,nk->ni", A, np.einsum("nkl,nl->nk", Qb, X[:, t + 1] - self._e(t + 1)))
        if t == 0:
            w = np.einsum("ij,j->i", pri["x0_prec"], pri["x0_mean"])[None] + m2
            cls = 0
        else:
            pmu = np.einsum("nki,ni->nk", A, X[:, t - 1]) + self._e(t)
            w = np.einsum("nkl,nl->nk", Qb, pmu) + m2
            cls = 1 if t < T - 1 else 2
        X[:, t] = np.einsum("nij,nj->ni", post["Sigma"][:, cls], w)

    def sweep(self, direction):
        post = O.state_posteriors(self.st, self.pri)
        for t in (range(self.T) if direction == "forward" else range(self.T - 1, -1, -1)):
            self._x_step(post, t)
        self.st["Sigma"], self.st["qld_x"] = post["Sigma"], post["qld"]

    def update_x(self, t):
        post = O.state_posteriors(self.st, self.pri)
        self._x_step(post, t)
        self.st["Sigma"], self.st["qld_x"] = post["Sigma"], post["qld"]

    # ---- sums
    def statistics(self):
        S = O.statistics(self.st, self.Y)
        X, U = self.st["X"], self.U
        S["Su1x"] = np.einsum("ntp,ntj->npj", U[:, 1:], X[:, :-1])
        S["Sxu"] = np.einsum("ntj,ntp->njp", X[:, 1:], U[:, 1:])
        S["Suu"] = self.Suu
        return S

    def _Qbar(self):
        return O.noise_expect(self.pri["noise"], self.st["Q_a"], self.st["Q_b"], self.D)

    # ---- columns, in the order As, Bs, Cs
    def update_A(self, S=None):
        S = S or self.statistics()
        st, pri = self.st, self.pri
        H = S["Sx1x"] - np.einsum("nkp,npj->nkj", st["B_mean"], S["Su1x"])
        st["qld_A"] = O._update_columns(st["A_mean"], st["A_cov"], pri["A_prior_mean"], pri["A_prior_prec"], self._Qbar(), S["Sxx_m"], H)

    def update_B(self, S=None):
        S = S or self.statistics()
        st, pri = self.st, self.pri
        H = S["Sxu"] - np.einsum("nkj,npj->nkp", st["A_mean"], S["Su1x"])
        st["qld_B"] = O._update_columns(st["B_mean"], st["B_cov"], pri["B_prior_mean"], pri["B_prior_prec"], self._Qbar(), S["Suu"], H)

    def update_C(self, S=None):
        O.update_C(self.st, self.pri, S or self.statistics())

    # ---- noise
    def _mean_parent_moments(self, S):
        """(E, HM): sum_t <pmu_t pmu_t^T> + sum_t <x_t x_t^T> and sum_t <x_t> <pmu_t>^T for pmu_t = A x_{t-1} + B u_t"""
        st = self.st
        E, HM = O._residual_second_moment(S["Sxx_p"], st["A_mean"], st["A_cov"], S["Sxx_m"], S["Sx1x"])
        cross = np.einsum("nkj,npj,nlp->nkl", st["A_mean"], S["Su1x"], st["B_mean"])
        E = E + O.outer_expect(st["B_mean"], st["B_cov"], S["Suu"]) + cross + np.swapaxes(cross, 1, 2)
        HM = HM + np.einsum("nkp,nlp->nkl", S["Sxu"], st["B_mean"])
        return E, HM

    def update_Q(self, S=None):
        S = S or self.statistics()
        st, pri, kind = self.st, self.pri, self.pri["noise"]
        E, HM = self._mean_parent_moments(S)
        if kind == "diagonal_gamma":
            st["Q_b"] = pri["Q_b0"][None] + 0.5 * np.einsum("nii->ni", E) - np.einsum("nii->ni", HM)
        else:
            st["Q_b"] = pri["Q_b0"] + 0.5 * np.einsum("nii->n", E) - np.einsum("nii->n", HM)
        st["Q_a"] = O._bcast_a(O.noise_a(kind, pri["Q_a0"], self.T - 1, self.D), st["Q_b"], kind)

    def update_R(self, S=None):
        O.update_R(self.st, self.pri, S or self.statistics(), self.T)

    # ---- bound
    def elbo_parts(self, bound="reference"):
        st, pri, T = self.st, self.pri, self.T
        S = self.statistics()
        exact = bound == "exact"
        out = (XR.elbo_parts_exact if exact else O.elbo_parts)(st, pri, S, T)
        # L_X: the second moment of the mean parent with the input's terms
        E0, HM0 = O._residual_second_moment(S["Sxx_p"], st["A_mean"], st["A_cov"], S["Sxx_m"], S["Sx1x"])
        E, HM = self._mean_parent_moments(S)
        out[:, 0] += -0.5 * np.einsum("nij,nji->n", self._Qbar(), (E - E0) - 2 * (HM - HM0))
        # the columns of B against their Constant parents (gaussian.py:141-147), into part 2
        M, Mcov, pm, pp = st["B_mean"], st["B_cov"], pri["B_prior_mean"], pri["B_prior_prec"]
        rows, LN2PI = self.D, _ln2pi(st["X"])
        for i in range(self.P):
            ex = np.einsum("nk,nl->nkl", M[:, :, i], M[:, :, i]) + Mcov[:, i] \
                + np.outer(pm[:, i], pm[:, i])[None] - 2 * np.einsum("nk,l->nkl", M[:, :, i], pm[:, i])
            out[:, 2] += -0.5 * rows * LN2PI + 0.5 * O._lndet_diag(pp[i]) - 0.5 * np.einsum("k,nkk->n", pp[i], ex)
            ent = XL.slogdet(Mcov[:, i])[1] if exact else st["qld_B"][:, i]
            out[:, 2] += 0.5 * rows * LN2PI + 0.5 * ent + 0.5 * rows
        return out

    def iterate(self, bound="reference"):
        """forward, backward, As, Bs, Cs, Q, R, bound: pyvb_lds_iterate on such a handle."""
        self.sweep("forward")
        self.sweep("backward")
        S = self.statistics()
        self.update_A(S)
        self.update_B(S)
        self.update_C(S)
        self.update_Q(S)
        self.update_R(S)
        return self.elbo_parts(bound)


def models(Y, U, st0, pri, lengths=None, cls=Model):
    """What LDSBatch.from_problem(Y, st0, pri, U=U, lengths=) was given, as a list of (rows, Model): one model of all N replicates
    where the chains have one length, one per replicate otherwise (rows past a chain's end are cut off)."""
    N, T = Y.shape[:2]
    if lengths is None or all(int(t) == T for t in lengths):
        return [(list(range(N)), cls(Y, U, st0, pri))]
    return [([n], cls(Y[n:n + 1, :Tn], U[n:n + 1, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st0.items()}, pri))
            for n, Tn in enumerate(int(t) for t in lengths)]


QUANTITIES = ("X", "Sigma", "A_mean", "A_colvar", "B_mean", "B_colvar", "C_mean", "C_colvar", "Q_b", "R_b")


def snapshot(ms, T):
    """What a trace records of a list of (rows, Model): arrays [N, ...] in the handle's layout (padding rows of X: 0)."""
    out = {}
    for k in ("Sigma", "A_mean", "B_mean", "C_mean"):
        out[k] = np.concatenate([m.st[k] for _, m in ms])
    out["X"] = np.concatenate([np.concatenate([m.st["X"], np.zeros((m.st["X"].shape[0], T - m.T, m.D), dtype=m.st["X"].dtype)], axis=1)
                               for _, m in ms])
    for w in "ABC":
        out[w + "_colvar"] = np.concatenate([np.einsum("nikk->nik", m.st[w + "_cov"]) for _, m in ms])
    for nm in ("Q_b", "R_b"):
        out[nm] = np.concatenate([np.broadcast_to(m.st[nm].reshape(m.st[nm].shape[0], -1), (m.st[nm].shape[0], m.D if nm == "Q_b" else m.K))
                                  for _, m in ms])
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# The cases the device is measured on (tests/test_inputs_gpu.py; tests/test_inputs_cpu.py checks the float64 comparator's own distance
# from the extended run on them): T, D, K, P, chain lengths or None, time split or None, iterations of the extended run.
# ----------------------------------------------------------------------------------------------------------------------------
CASES = {
    "t19_d6k4p2": (19, 6, 4, 2, None, None, 2),                 # smallest; one tile everywhere
    "t33_d5k15p1": (33, 5, 15, 1, None, None, 2),               # K + 2P = 17 crosses a tile; a single column of B
    "t77_d16k16p8": (77, 16, 16, 8, None, None, 2),             # K + 2P = 32
    "t40_d64k40p12": (40, 64, 40, 12, None, None, 1),           # K + 2P = 64 and D = 64 (a long-double iteration at this width takes seconds)
    "t700_d8k8p3_w4": (700, 8, 8, 3, None, 4, 2),               # segments that start from their warm-up, several wavefronts per chain
    "lengths_d16k10p3": (77, 16, 10, 3, (2, 3, 19, 60, 77), None, 2),   # shortest chain; the zeroed u_{t+1} at each chain's own end
}
SEEDS = {"t19_d6k4p2": 31400, "t33_d5k15p1": 31410, "t77_d16k16p8": 31420, "t40_d64k40p12": 31430, "t700_d8k8p3_w4": 31440,
         "lengths_d16k10p3": 31450}
ITERS = 2
BOUNDS = ("reference", "exact")
_cache = {}


def n_case(name):
    ln = CASES[name][4]
    return 2 if ln is None else len(ln)


def problem(name):
    """(Y, U, st0, pri, lengths) of a case; shared between the tests: do not write to the arrays."""
    if ("problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, P, ln = CASES[name][:5]
        Y, U, st0, pri = synth.make_input_problem(T, D, K, P, n_case(name), seed=SEEDS[name])
        if ln is not None:
            live = np.arange(T)[None, :] < np.asarray(ln)[:, None]
            Y, U = np.where(live[:, :, None], Y, 0.0), np.where(live[:, :, None], U, 0.0)
            st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
        for a in [Y, U] + list(st0.values()):
            a.setflags(write=False)
        _cache["problem", name] = (Y, U, st0, pri, None if ln is None else np.asarray(ln, dtype=np.int32))
    return _cache["problem", name]


# the stages of an iteration in the order pyvb_lds_iterate runs them, each with the quantities it produces
STAGES = (("forward", ("X",)), ("backward", ("X", "Sigma")), ("A", ("A_mean", "A_colvar")), ("B", ("B_mean", "B_colvar")),
          ("C", ("C_mean", "C_colvar")), ("Q", ("Q_b",)), ("R", ("R_b",)))


def run_stages(do, snap, bound, iters):
    """One trace function for the float64 comparator, its extended run and the handle, so that the three sequences line up by
    construction: do(stage) runs a stage, snap() returns the quantities, bound(mode) the parts [N, 6].  Returns a list of
    ((iteration, stage, quantity), array), every quantity after the stage that produces it, then ((iteration, "bound", mode), parts)."""
    out = []
    for it in range(iters):
        for stage, keys in STAGES:
            do(stage)
            s = snap()
            out += [((it, stage, k), np.array(s[k])) for k in keys]
        out += [((it, "bound", mode), np.array(bound(mode))) for mode in BOUNDS]
    return out


def do_stage(m, stage):
    """A stage on a Model."""
    if stage in ("forward", "backward"):
        m.sweep(stage)
    else:
        getattr(m, "update_" + stage)()


def trace(name, extended=False):
    """The comparator's stage-by-stage run of a case (run_stages), in float64 or (extended) np.longdouble: ITERS iterations in
    float64, the case's own number in long double.  Cached; shared between the tests."""
    key = ("trace", name, extended)
    if key not in _cache:
        Y, U, st0, pri, ln = problem(name)
        if extended:
            import extended_ref as ER
            Y, U, st0, pri = ER.to_long(Y), ER.to_long(U), ER.to_long(st0), ER.to_long(pri)
        ms = models(Y, U, st0, pri, ln)
        _cache[key] = run_stages(lambda stage: [do_stage(m, stage) for _, m in ms], lambda: snapshot(ms, CASES[name][0]),
                                 lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), CASES[name][6] if extended else ITERS)
    return _cache[key]


# ----------------------------------------------------------------------------------------------------------------------------
# Channel by channel (tests/test_input_channels_cpu.py, tests/test_input_channels_gpu.py; extended_ref.compare_channels).  The
# problems are synth.make_input_problem's with the channels of U replaced by named patterns -- channel p takes pattern p mod 8 --
# and with finite random values, not zeros, in row 0 of U (u_0 is never used) and in the padding rows t >= T_n of U and Y.
# X's padding stays zero.  T, D, K, P, chain lengths or None, time split or None, iterations of the extended run, big (small = 1 / big).
# ----------------------------------------------------------------------------------------------------------------------------
U_PATTERNS = ("as drawn", "x big", "x small", "impulse at t = 1", "impulse at t = T_n - 1", "dead: nonzero at t = 0 only", "constant 1",
              "as drawn")
CHANNEL_CASES = {
    "t48_d5k2p31": (48, 5, 2, 31, None, None, 2, 1e3),          # P = IN_PMAX, Kt = 64 at one state tile; two W tiles, CT = 4
    "t27_d17k3p17": (27, 17, 3, 17, None, None, 2, 1e3),        # one real column in W's second tile, read after V's first tile was
                                                                # stored over its padding; DT = 2 with one real row
    "t27_d33k32p16": (27, 33, 32, 16, None, None, 2, 1e3),      # P a full tile, Kt = 64, the gain columns start on an operand-tile edge
    "t48_d64k2p31": (48, 64, 2, 31, None, None, 1, 1e3),        # the cap at full state width (one long-double iteration)
    "t700_d8k8p5_w4": (700, 8, 8, 5, None, 4, 2, 1e3),          # the impulses at t = 1 and T - 1 in the first and last wavefront's part
    "lengths_d16k10p9": (77, 16, 10, 9, (2, 3, 19, 60, 77), None, 2, 30.0),    # every pattern in every chain, live padding in U and Y
}
# (chosen so that the float64 comparator is within extended_ref.CAP unit by unit, tests/test_input_channels_cpu.py; a draw over
# it is replaced, never tolerated)
CHANNEL_SEEDS = {"t48_d5k2p31": 33400, "t27_d17k3p17": 33410, "t27_d33k32p16": 33420, "t48_d64k2p31": 33430, "t700_d8k8p5_w4": 33440,
                 "lengths_d16k10p9": 33450}


def channel_lengths(name):
    """int [N]: the chain length of every replicate of a case of CHANNEL_CASES"""
    T, ln = CHANNEL_CASES[name][0], CHANNEL_CASES[name][4]
    return np.full(2, T, dtype=np.int32) if ln is None else np.asarray(ln, dtype=np.int32)


def pattern_inputs(U, lengths, big, rng):
    """(U with channel p of every replicate replaced by pattern p mod 8 of U_PATTERNS on the rows 1 .. T_n - 1 that are used, the
    label of every [replicate][channel]).  Row 0, which no chain uses, and the padding rows t >= T_n are drawn anew: finite, not zero
    (row 0 is the only nonzero row of a dead channel).  Where two patterns coincide (T_n = 2: t = 1 is T_n - 1) the label says so."""
    U = U.copy()
    N, T, P = U.shape
    labels = []
    for n, Tn in enumerate(int(t) for t in lengths):
        labels.append([])
        U[n, 0] = rng.standard_normal(P)
        for p in range(P):
            k, name = p % 8, U_PATTERNS[p % 8]
            u = U[n, 1:Tn, p]
            if k == 1:
                u *= big
            elif k == 2:
                u /= big
            elif k in (3, 4):
                u[:] = 0.0
                u[0 if k == 3 else Tn - 2] = 1.0
                if Tn == 2:
                    name = "impulse at t = 1 = T_n - 1"
            elif k == 5:
                u[:] = 0.0
                assert U[n, 0, p] != 0.0
            elif k == 6:
                u[:] = 1.0
            labels[-1].append(name)
        U[n, Tn:] = rng.standard_normal((T - Tn, P))
    return U, labels


def channel_problem(name):
    """(Y, U, st0, pri, lengths or None, the labels [replicate][channel] of U) of a case of CHANNEL_CASES; shared: do not write."""
    if ("channel problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, P, ln, _, _, big = CHANNEL_CASES[name]
        lengths = channel_lengths(name)
        Y, U, st0, pri = synth.make_input_problem(T, D, K, P, len(lengths), seed=CHANNEL_SEEDS[name])
        rng = np.random.default_rng(CHANNEL_SEEDS[name] + 1)
        U, labels = pattern_inputs(U, lengths, big, rng)
        live = (np.arange(T)[None, :] < lengths[:, None])[:, :, None]
        Y = np.where(live, Y, rng.standard_normal(Y.shape))
        st0["X"] = np.where(live, st0["X"], 0.0)
        for a in [Y, U] + list(st0.values()):
            a.setflags(write=False)
        _cache["channel problem", name] = (Y, U, st0, pri, None if ln is None else lengths, labels)
    return _cache["channel problem", name]


def channel_run(prob, extended=False, iters=ITERS, cls=Model):
    """run_stages of the comparator on a problem (Y, U, st0, pri, lengths, ...), in float64 or cast up to long double"""
    Y, U, st0, pri, ln = prob[:5]
    if extended:
        import extended_ref as ER
        Y, U, st0, pri = ER.to_long(Y), ER.to_long(U), ER.to_long(st0), ER.to_long(pri)
    ms = models(Y, U, st0, pri, ln, cls)
    return run_stages(lambda stage: [do_stage(m, stage) for _, m in ms], lambda: snapshot(ms, Y.shape[1]),
                      lambda mode: np.concatenate([m.elbo_parts(mode) for _, m in ms]), iters)


def channel_trace(name, extended=False):
    """trace() for a case of CHANNEL_CASES.  Cached; shared between the tests."""
    key = ("channel trace", name, extended)
    if key not in _cache:
        _cache[key] = channel_run(channel_problem(name), extended, CHANNEL_CASES[name][6] if extended else ITERS)
    return _cache[key]


def load_fixture(path):
    """tests/golden/inputs_*.npz -> (meta, Y [N, T, K], U [N, T, P], st0, pri, lengths, z)"""
    z = dict(np.load(path, allow_pickle=False))
    lengths = [int(t) for t in z["lengths"]]
    pri = {k[6:]: z[k].copy() for k in z if k.startswith("prior_")}
    pri["noise"] = str(z["noise"])
    if pri["noise"] == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(pri[k])
    st0 = {k[5:]: z[k].copy() for k in z if k.startswith("init_")}
    meta = {"lengths": lengths, "D": int(z["D"]), "K": int(z["K"]), "P": int(z["P"]), "noise": pri["noise"], "iters": [int(i) for i in z["iters"]]}
    return meta, z["Y"].copy(), z["U"].copy(), st0, pri, lengths, z
