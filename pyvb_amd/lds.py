"""LDSBatch: N independent replicates of the linear-dynamical-system graph of the
reference's examples/Linear_Dynamic_System.py:46-66, resident on one MI355X.

Consecutive replicates can share A, C, Q, R (models=, from_trials): several time series, one model.

Thin Python over the C ABI (include/pyvb_hip.h); every method is one or a few
kernel launches.  The node classes in pyvb_amd.nodes bind to an LDSBatch with
N = 1; bench.py and the parity tests drive it directly.
"""
import numpy as np

from . import _capi as C

__all__ = ["LDSBatch", "pad_series"]

_NOISE = {"diagonal_gamma": C.NOISE_DIAGONAL_GAMMA, "gamma": C.NOISE_GAMMA, "wishart": C.NOISE_WISHART}
_WHICH = {"A": 0, "C": 1}
_PARENT_ENTRIES = {"gamma": "column", "diagonal_gamma": "entry"}       # kind (_capi.PARENTS) -> the word in pyvb_*_{set,get,update}_*_precisions


def _f64(a, shape, name):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != tuple(shape):
        raise AssertionError("%s has shape %s, expected %s" % (name, a.shape, tuple(shape)))
    return a


_STATE_KEYS = ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b")
_ALPHA_KEYS = ("A_alpha_b", "C_alpha_b")        # [1, D] each: qb of the columns' Gamma parents, where a series' state carries them
_ENTRY_KEYS = ("A_entry_b", "C_entry_b")        # [1, D, rows] each: qb of the columns' DiagonalGamma parents, likewise
_INPUT_KEYS = ("B_mean", "B_colvar")            # [1, D, P], [1, P, D]: the input gain of a series with a known input, likewise
_REGRESSOR_KEYS = ("E_mean", "E_colvar")        # [1, K, Pv], [1, Pv, K]: the regressors' gain of a series with known regressors, likewise


def pad_series(series):
    """series: list of (Y_n[T_n, K], st0_n), st0_n as synth.initial_state(T_n, D, K, 1) gives it.  Returns (Y[N, T, K],
    st0, lengths) with T = max T_n: the inputs of a handle with chain lengths.  Rows t >= T_n of Y and of st0["X"] are
    padding (zeros here); no result depends on what they hold.  A_alpha_b / C_alpha_b (set_column_precisions) and A_entry_b /
    C_entry_b (set_entry_precisions) travel along where the states carry them."""
    N = len(series)
    if N == 0:
        raise ValueError("no series")
    lengths = np.array([np.shape(y)[0] for y, _ in series], dtype=np.int32)
    T, K = int(lengths.max()), np.shape(series[0][0])[1]
    D = np.shape(series[0][1]["X"])[-1]
    Y, X = np.zeros((N, T, K)), np.zeros((N, T, D))
    for n, (y, st) in enumerate(series):
        y = np.asarray(y, dtype=np.float64)
        x = np.asarray(st["X"], dtype=np.float64).reshape(-1, D)
        if y.shape != (lengths[n], K) or x.shape != (lengths[n], D):
            raise AssertionError("series %d: Y has shape %s and X %s, expected (%d, %d) and (%d, %d)"
                                 % (n, y.shape, x.shape, lengths[n], K, lengths[n], D))
        Y[n, :lengths[n]], X[n, :lengths[n]] = y, x
    st0 = {"X": X}
    for k in _STATE_KEYS[1:] + tuple(k for k in _ALPHA_KEYS + _ENTRY_KEYS + _INPUT_KEYS + _REGRESSOR_KEYS if k in series[0][1]):
        st0[k] = np.concatenate([np.asarray(st[k], dtype=np.float64) for _, st in series])       # each [1, ...]
    return Y, st0, lengths


class LDSBatch(object):
    ELBO_PARTS = ("X", "Y", "A", "C", "Q", "R")

    def __init__(self, N, T, D, K, noise="diagonal_gamma", device=0, lengths=None, models=None, inputs=0, regressors=0):
        """regressors: Pv >= 1 known regressors in the output equation, y_t = C x_t + E v_t (pyvb_lds_create_regressors):
        set_regressors gives V [N, T, Pv] (V = 1: an output offset), E [K, Pv] is a matrix of Gaussian columns like C (set_state /
        get_state: E_mean, E_colvar; set_priors: E_prior_mean, E_prior_prec; update_E).  Composes with inputs=; DiagonalGamma /
        Gamma noise and max(D, K + 2 P + Pv) <= 64; not with models=.  0: none.
        inputs: P >= 1 known inputs that drive the states, x_t = A x_{t-1} + B u_t (pyvb_lds_create_inputs): set_inputs gives
        U [N, T, P], B [D, P] is a matrix of Gaussian columns like A (set_state / get_state: B_mean, B_colvar; set_priors:
        B_prior_mean, B_prior_prec; update_B).  DiagonalGamma / Gamma noise and max(D, K + 2 P) <= 64; not with models=.  0: none.
        lengths: int [N], the chain length T_n of each replicate, 2 <= T_n <= T (pyvb_lds_create_lengths); None: all T.
        Arrays stay [N, T, ...]; rows t >= T_n of replicate n are padding: setters accept anything there, getters return
        0.0 in X and in the outputs.
        models: int [N], the model of each replicate (pyvb_lds_create_tied): consecutive replicates with the same id are the
        chains of one model and share A, C, Q, R -- several time series, one model.  Ids start at 0 and rise in steps of 0 or
        1.  None: every replicate is a model of its own.  Parameter arrays stay [N, ...]; set_state takes a model's
        parameters from the row of its first replicate, getters return them in every row of the model."""
        if noise not in _NOISE:
            raise NotImplementedError("noise precision %r has no HIP path (DiagonalGamma, Gamma and Wishart do)" % (noise,))
        self.N, self.T, self.D, self.K, self.noise, self.device = int(N), int(T), int(D), int(K), noise, int(device)
        self.P = int(inputs or 0)
        self.Pv = int(regressors or 0)
        self.bound = "reference"
        h = C.ctypes.c_void_p()
        if self.Pv and models is None:
            ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
            if ln is not None and ln.shape != (self.N,):
                raise AssertionError("lengths has shape %s, expected (%d,)" % (ln.shape, self.N))
            C.check(C.lib.pyvb_lds_create_regressors(C.ctypes.byref(h), self.device, self.N, self.T, self.D, self.K, self.P, self.Pv,
                                                     _NOISE[noise], None if ln is None else ln.ctypes.data_as(C._ip)))
            self.lengths = np.empty(self.N, dtype=np.int32)
            C.check(C.lib.pyvb_lds_get_lengths(h, self.lengths.ctypes.data_as(C._ip)))
        elif self.P or self.Pv:
            if models is not None:
                raise NotImplementedError("chains that share A, C, Q, R (models=) are not served together with %s"
                                          % ("inputs" if self.P else "regressors"))
            ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
            if ln is not None and ln.shape != (self.N,):
                raise AssertionError("lengths has shape %s, expected (%d,)" % (ln.shape, self.N))
            C.check(C.lib.pyvb_lds_create_inputs(C.ctypes.byref(h), self.device, self.N, self.T, self.D, self.K, self.P, _NOISE[noise],
                                                 None if ln is None else ln.ctypes.data_as(C._ip)))
            self.lengths = np.empty(self.N, dtype=np.int32)
            C.check(C.lib.pyvb_lds_get_lengths(h, self.lengths.ctypes.data_as(C._ip)))
        elif models is not None:
            ln = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.int32)
            md = np.ascontiguousarray(models, dtype=np.int32)
            for nm, a in (("lengths", ln), ("models", md)):
                if a is not None and a.shape != (self.N,):
                    raise AssertionError("%s has shape %s, expected (%d,)" % (nm, a.shape, self.N))
            C.check(C.lib.pyvb_lds_create_tied(C.ctypes.byref(h), self.device, self.N, self.T, self.D, self.K, _NOISE[noise],
                                               None if ln is None else ln.ctypes.data_as(C._ip), md.ctypes.data_as(C._ip)))
            self.lengths = np.empty(self.N, dtype=np.int32)
            C.check(C.lib.pyvb_lds_get_lengths(h, self.lengths.ctypes.data_as(C._ip)))
        elif lengths is None:
            C.check(C.lib.pyvb_lds_create(C.ctypes.byref(h), self.device, self.N, self.T, self.D, self.K, _NOISE[noise]))
            self.lengths = np.full(self.N, self.T, dtype=np.int32)
        else:
            ln = np.ascontiguousarray(lengths, dtype=np.int32)
            if ln.shape != (self.N,):
                raise AssertionError("lengths has shape %s, expected (%d,)" % (ln.shape, self.N))
            C.check(C.lib.pyvb_lds_create_lengths(C.ctypes.byref(h), self.device, self.N, self.T, self.D, self.K, _NOISE[noise],
                                                  ln.ctypes.data_as(C._ip)))
            self.lengths = np.empty(self.N, dtype=np.int32)
            C.check(C.lib.pyvb_lds_get_lengths(h, self.lengths.ctypes.data_as(C._ip)))
        self.models = np.empty(self.N, dtype=np.int32)
        C.check(C.lib.pyvb_lds_get_models(h, self.models.ctypes.data_as(C._ip)))
        self._h = h

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            C.lib.pyvb_lds_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs -----------------------------------------------------------------------------
    def set_priors(self, pri):
        """pri: dict as pyvb_amd.synth.default_priors (Constant parents of X_0 and of the
        columns, Gamma-family hyper-parameters).  Scalars are broadcast for the Gamma kind."""
        D, K = self.D, self.K
        arrs = [
            _f64(pri["x0_mean"], (D,), "x0_mean"), _f64(pri["x0_prec"], (D, D), "x0_prec"),
            _f64(pri["A_prior_mean"], (D, D), "A_prior_mean"), _f64(pri["A_prior_prec"], (D, D), "A_prior_prec"),
            _f64(pri["C_prior_mean"], (K, D), "C_prior_mean"), _f64(pri["C_prior_prec"], (D, K), "C_prior_prec"),
        ]
        if self.noise == "wishart":     # Wishart(dim, v0, w0): Q_a0 / R_a0 hold v0, Q_b0 / R_b0 the matrices w0
            self._check(C.lib.pyvb_lds_set_priors(self._h, *([C.dptr(a) for a in arrs] + [None] * 4)))
            qw0, rw0 = _f64(pri["Q_b0"], (D, D), "Q_w0"), _f64(pri["R_b0"], (K, K), "R_w0")
            self._check(C.lib.pyvb_lds_set_wishart_priors(self._h, float(pri["Q_a0"]), C.dptr(qw0), float(pri["R_a0"]), C.dptr(rw0)))
            return
        arrs += [C.broadcast(pri["Q_a0"], (D,)), C.broadcast(pri["Q_b0"], (D,)), C.broadcast(pri["R_a0"], (K,)), C.broadcast(pri["R_b0"], (K,))]
        self._check(C.lib.pyvb_lds_set_priors(self._h, *[C.dptr(a) for a in arrs]))       # (the columns have Constant parents again)
        if self.P:      # the Constant parents of the columns of B: B_prior_mean [D, P] (row, col), B_prior_prec [P, D] (column, entry)
            bm, bp = _f64(pri["B_prior_mean"], (D, self.P), "B_prior_mean"), _f64(pri["B_prior_prec"], (self.P, D), "B_prior_prec")
            self._check(C.lib.pyvb_lds_set_input_priors(self._h, C.dptr(bm), C.dptr(bp)))
        if self.Pv:     # those of the columns of E: E_prior_mean [K, Pv] (row, col), E_prior_prec [Pv, K] (column, entry)
            em, ep = _f64(pri["E_prior_mean"], (K, self.Pv), "E_prior_mean"), _f64(pri["E_prior_prec"], (self.Pv, K), "E_prior_prec")
            self._check(C.lib.pyvb_lds_set_regressor_priors(self._h, C.dptr(em), C.dptr(ep)))

    def set_inputs(self, U):
        """U[N,T,P]: row t drives x_t; row 0 and, with chain lengths, the rows t >= T_n are never read."""
        U = _f64(U, (self.N, self.T, self.P), "U")
        self._check(C.lib.pyvb_lds_set_inputs(self._h, C.dptr(U)))

    def get_inputs(self):
        U = np.empty((self.N, self.T, self.P))
        self._check(C.lib.pyvb_lds_get_inputs(self._h, C.dptr(U)))
        return U

    def set_regressors(self, V):
        """V[N,T,Pv]: row t enters y_t, row 0 included; with chain lengths, the rows t >= T_n are never read."""
        V = _f64(V, (self.N, self.T, self.Pv), "V")
        self._check(C.lib.pyvb_lds_set_regressors(self._h, C.dptr(V)))

    def get_regressors(self):
        V = np.empty((self.N, self.T, self.Pv))
        self._check(C.lib.pyvb_lds_get_regressors(self._h, C.dptr(V)))
        return V

    def set_observations(self, Y):
        """Y[N,T,K]; NaN = missing entry (the rows concerned become variational nodes: set_output_state, update_Y).
        With chain lengths, rows t >= T_n may hold anything; NaN in a row t < T_n is refused (E_UNSUPPORTED)."""
        Y = _f64(Y, (self.N, self.T, self.K), "Y")
        self._check(C.lib.pyvb_lds_set_observations(self._h, C.dptr(Y)))

    def set_output_state(self, Yq, Yrowvar):
        """Initial posterior of the outputs that are not fully observed: means [N,T,K], isotropic variances [N,T]."""
        q, v = _f64(Yq, (self.N, self.T, self.K), "Yq"), _f64(Yrowvar, (self.N, self.T), "Yrowvar")
        self._check(C.lib.pyvb_lds_set_output_state(self._h, C.dptr(q), C.dptr(v)))

    def update_Y(self):
        """[y.update() for y in Ys if not y.observed]"""
        self._check(C.lib.pyvb_lds_update_Y(self._h))

    def get_outputs(self, with_qld=False):
        """(posterior means [N,T,K], variances [N,T,K]) of the outputs; fully observed rows: (value, 0).
        with_qld: also q_ln_det [N,T] of the rows updated so far (NaN otherwise).  Padding rows (t >= T_n): 0, 0, NaN."""
        q, v = np.empty((self.N, self.T, self.K)), np.empty((self.N, self.T, self.K))
        ld = np.empty((self.N, self.T)) if with_qld else None
        self._check(C.lib.pyvb_lds_get_outputs(self._h, C.dptr(q), C.dptr(v), C.dptr(ld)))
        return (q, v, ld) if with_qld else (q, v)

    def set_state(self, X=None, A_mean=None, A_colvar=None, C_mean=None, C_colvar=None, Q_b=None, R_b=None, B_mean=None, B_colvar=None,
                  E_mean=None, E_colvar=None):
        """X[N,T,D] and the parameter posteriors; padding rows of X (t >= T_n) may hold anything.  On a handle with inputs also
        B_mean [N,D,P] and B_colvar [N,P,D], on one with regressors E_mean [N,K,Pv] and E_colvar [N,Pv,K]."""
        N, T, D, K = self.N, self.T, self.D, self.K
        if E_mean is not None or E_colvar is not None:
            em = None if E_mean is None else _f64(E_mean, (N, K, self.Pv), "E_mean")
            ev = None if E_colvar is None else _f64(E_colvar, (N, self.Pv, K), "E_colvar")
            self._check(C.lib.pyvb_lds_set_regressor_state(self._h, C.dptr(em), C.dptr(ev)))
        if B_mean is not None or B_colvar is not None:
            bm = None if B_mean is None else _f64(B_mean, (N, D, self.P), "B_mean")
            bv = None if B_colvar is None else _f64(B_colvar, (N, self.P, D), "B_colvar")
            self._check(C.lib.pyvb_lds_set_input_state(self._h, C.dptr(bm), C.dptr(bv)))
        shapes = [("X", X, (N, T, D)), ("A_mean", A_mean, (N, D, D)), ("A_colvar", A_colvar, (N, D, D)),
                  ("C_mean", C_mean, (N, K, D)), ("C_colvar", C_colvar, (N, D, K)), ("Q_b", Q_b, (N, D)), ("R_b", R_b, (N, K))]
        arrs = [None if a is None else _f64(a, s, nm) for nm, a, s in shapes]
        self._check(C.lib.pyvb_lds_set_state(self._h, *[C.dptr(a) for a in arrs]))

    def set_wishart_state(self, Q_w=None, R_w=None):
        """Posterior qw of the Wishart nodes, [N,D,D] and [N,K,K] (nodes_todo.py:216-217 draws a random rank-one one)."""
        q = None if Q_w is None else _f64(Q_w, (self.N, self.D, self.D), "Q_w")
        r = None if R_w is None else _f64(R_w, (self.N, self.K, self.K), "R_w")
        self._check(C.lib.pyvb_lds_set_wishart_state(self._h, C.dptr(q), C.dptr(r)))

    def get_wishart_state(self):
        N, D, K = self.N, self.D, self.K
        out = {"Q_v": np.empty(N), "Q_w": np.empty((N, D, D)), "R_v": np.empty(N), "R_w": np.empty((N, K, K))}
        self._check(C.lib.pyvb_lds_get_wishart_state(self._h, C.dptr(out["Q_v"]), C.dptr(out["Q_w"]), C.dptr(out["R_v"]), C.dptr(out["R_w"])))
        return out

    def set_column_cov(self, A_cov=None, C_cov=None):
        a = None if A_cov is None else _f64(A_cov, (self.N, self.D, self.D, self.D), "A_cov")
        c = None if C_cov is None else _f64(C_cov, (self.N, self.D, self.K, self.K), "C_cov")
        self._check(C.lib.pyvb_lds_set_column_cov(self._h, C.dptr(a), C.dptr(c)))

    def get_column_cov(self):
        """Dense posterior covariances of the columns of A ([N,D,D,D]) and C ([N,D,K,K]); Wishart noise only."""
        A, Cc = np.empty((self.N, self.D, self.D, self.D)), np.empty((self.N, self.D, self.K, self.K))
        self._check(C.lib.pyvb_lds_get_column_cov(self._h, C.dptr(A), C.dptr(Cc)))
        return A, Cc

    def set_column_observations(self, A_obs=None, C_obs=None):
        """Known entries of A ([D,D]) and C ([K,D]) as (row, col) arrays with NaN where unknown
        (As[i].observe(...), examples/LDS_knowns_in_A.py:73-74).  Call after set_state."""
        a = None if A_obs is None else _f64(A_obs, (self.D, self.D), "A_obs")
        c = None if C_obs is None else _f64(C_obs, (self.K, self.D), "C_obs")
        self._check(C.lib.pyvb_lds_set_column_observations(self._h, C.dptr(a), C.dptr(c)))

    # -- the precision parents of the columns: the handle knows which kind a matrix has (column_parents) ------------
    def _parent_shape(self, nm, kind):
        """of a0 and b0, and of one replicate's qb"""
        return (self.D,) if kind == "gamma" else (self.D, self.D if nm == "A" else self.K)

    def _parents_fn(self, verb, kind):
        return getattr(C.lib, "pyvb_lds_%s_%s_precisions" % (verb, _PARENT_ENTRIES[kind]))

    def _set_parents(self, kind, given):
        for nm, t in zip("AC", given):
            if t is not None:
                shape = self._parent_shape(nm, kind)
                arrs = [C.broadcast(v, s) for v, s in zip(t, (shape, shape, (self.N,) + shape))]        # a0, b0, qb
                self._check(self._parents_fn("set", kind)(self._h, _WHICH[nm], *[C.dptr(a) for a in arrs]))

    def _with_parents(self, kind):
        return [nm for nm, k in sorted(self.column_parents().items()) if k == kind]       # A first

    def _get_parents(self, kind):
        out = {}
        for nm in self._with_parents(kind):
            qa, qb = (np.empty((self.N,) + self._parent_shape(nm, kind)) for _ in "ab")
            self._check(self._parents_fn("get", kind)(self._h, _WHICH[nm], C.dptr(qa), C.dptr(qb)))
            out[nm] = (qa, qb)
        return out

    def _update_parents(self, kind, which):
        for w in (self._with_parents(kind) if which is None else [which]):
            self._check(self._parents_fn("update", kind)(self._h, _WHICH.get(w, w)))

    def column_parents(self):
        """{"A": kind, "C": kind}, each "constant", "gamma" or "diagonal_gamma": the kind of precision parent the columns of the
        matrix have (pyvb_lds_get_column_parents) -- the most recent setter's, "constant" after set_priors."""
        kind = (C.ctypes.c_int * 2)()
        self._check(C.lib.pyvb_lds_get_column_parents(self._h, kind))
        return {"A": C.PARENTS[kind[0]], "C": C.PARENTS[kind[1]]}

    def set_column_precisions(self, A=None, C=None):
        """Gamma precision parents for the columns of A and / or C (automatic relevance determination): each a tuple
        (a0[D], b0[D], qb[N, D]) -- alpha_i ~ Gamma(a0_i, b0_i) is the prior precision of column i, qb its initial posterior
        rate (the reference draws rand()).  Scalars are broadcast.  Call after set_priors, which returns the columns to
        Constant parents.  DiagonalGamma / Gamma noise and max(D, K) <= 64 only."""
        self._set_parents("gamma", (A, C))

    def column_precisions(self):
        """{"A": (qa[N, D], qb[N, D]), "C": ...} of the matrices that have Gamma parents; E[alpha] = qa / qb."""
        return self._get_parents("gamma")

    def update_column_precisions(self, which=None):
        """[al.update() for al in alphas] of the columns of which = "A" (or 0), "C" (or 1); None: of every matrix that has
        Gamma parents, A first."""
        self._update_parents("gamma", which)

    def set_entry_precisions(self, A=None, C=None):
        """DiagonalGamma precision parents for the columns of A and / or C, a precision of its own for every entry (sparse
        transition / loading matrices): each a tuple (a0[D, rows], b0[D, rows], qb[N, D, rows]) in [column][row] order as
        A_prior_prec is, rows = D for A and K for C -- alpha[i][k] ~ Gamma(a0[i][k], b0[i][k]) is the prior precision of entry
        (k, i), qb its initial posterior rate.  Scalars are broadcast.  Call after set_priors, which returns the columns to
        Constant parents; it replaces Gamma parents of the same matrix (set_column_precisions) and is replaced by them.
        DiagonalGamma / Gamma noise and max(D, K) <= 64 only."""
        self._set_parents("diagonal_gamma", (A, C))

    def entry_precisions(self):
        """{"A": (qa[N, D, D], qb[N, D, D]), "C": (qa[N, D, K], qb[N, D, K])} of the matrices that have DiagonalGamma parents, in
        [column][row] order; E[alpha] = qa / qb."""
        return self._get_parents("diagonal_gamma")

    def update_entry_precisions(self, which=None):
        """[dg.update() for dg in the DiagonalGamma parents] of the columns of which = "A" (or 0), "C" (or 1); None: of every
        matrix that has such parents, A first."""
        self._update_parents("diagonal_gamma", which)

    # -- outputs ----------------------------------------------------------------------------
    def get_state(self, what=("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b")):
        """Posterior means of the states and the parameter posteriors.  Padding rows of X (t >= T_n) read as 0.0; Q_a / R_a
        count the children of each replicate's own Q (T_n - 1) and R (T_n)."""
        N, T, D, K = self.N, self.T, self.D, self.K
        shapes = {"X": (N, T, D), "A_mean": (N, D, D), "A_colvar": (N, D, D), "C_mean": (N, K, D), "C_colvar": (N, D, K),
                  "Q_a": (N, D), "Q_b": (N, D), "R_a": (N, K), "R_b": (N, K)}
        order = ["X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b"]
        out = {k: np.empty(shapes[k]) for k in order if k in what}
        self._check(C.lib.pyvb_lds_get_state(self._h, *[C.dptr(out.get(k)) for k in order]))
        if self.P and ("A_mean" in what or "B_mean" in what):       # a handle with inputs: the third matrix beside the two
            out.update(self.get_input_state(("B_mean", "B_colvar")))
        if self.Pv and ("C_mean" in what or "E_mean" in what):      # a handle with regressors: their gain beside C
            out.update(self.get_regressor_state(("E_mean", "E_colvar")))
        return out

    def get_regressor_state(self, what=("E_mean", "E_colvar", "qld_E", "lnd_E")):
        """E_mean [N,K,Pv], E_colvar [N,Pv,K], and q_ln_det / ln det qcov of the columns of E [N,Pv] (NaN before their first update)."""
        shapes = {"E_mean": (self.N, self.K, self.Pv), "E_colvar": (self.N, self.Pv, self.K), "qld_E": (self.N, self.Pv), "lnd_E": (self.N, self.Pv)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in what}
        self._check(C.lib.pyvb_lds_get_regressor_state(self._h, *[C.dptr(out.get(k)) for k in shapes]))
        return out

    def get_input_state(self, what=("B_mean", "B_colvar", "qld_B", "lnd_B")):
        """B_mean [N,D,P], B_colvar [N,P,D], and q_ln_det / ln det qcov of the columns of B [N,P] (NaN before their first update)."""
        shapes = {"B_mean": (self.N, self.D, self.P), "B_colvar": (self.N, self.P, self.D), "qld_B": (self.N, self.P), "lnd_B": (self.N, self.P)}
        out = {k: np.empty(shapes[k]) for k in shapes if k in what}
        self._check(C.lib.pyvb_lds_get_input_state(self._h, *[C.dptr(out.get(k)) for k in shapes]))
        return out

    def get_posterior_classes(self):
        """(Sigma[N,3,D,D], q_ln_det[N,3]) of X_0, the interior X_t and X_{T-1} as of their last update (with chain lengths:
        of replicate n's X_0, its interior and its X_{T_n-1}; T_n = 2 has no interior)."""
        S = np.empty((self.N, 3, self.D, self.D))
        q = np.empty((self.N, 3))
        self._check(C.lib.pyvb_lds_get_posterior_classes(self._h, C.dptr(S), C.dptr(q)))
        return S, q

    def set_posterior_classes(self, Sigma, qld_x=None):
        """Initial covariances of X_0, the interior X_t and X_{T-1} ([N,3,D,D]); see include/pyvb_hip.h."""
        S = _f64(Sigma, (self.N, 3, self.D, self.D), "Sigma")
        q = None if qld_x is None else _f64(qld_x, (self.N, 3), "qld_x")
        self._check(C.lib.pyvb_lds_set_posterior_classes(self._h, C.dptr(S), C.dptr(q)))

    def get_column_qld(self):
        qa, qc = np.empty((self.N, self.D)), np.empty((self.N, self.D))
        self._check(C.lib.pyvb_lds_get_column_qld(self._h, C.dptr(qa), C.dptr(qc)))
        return qa, qc

    def get_logdets(self):
        """ln det qcov as the last updates left it: of the X_t classes [N,3], of the columns of A and C [N,D] each, and of
        the outputs with missing entries [N,T] (NaN where the q_ln_det getters give NaN).  Stored in both bound modes."""
        lx, la, lc = np.empty((self.N, 3)), np.empty((self.N, self.D)), np.empty((self.N, self.D))
        ly = np.empty((self.N, self.T))
        self._check(C.lib.pyvb_lds_get_logdets(self._h, C.dptr(lx), C.dptr(la), C.dptr(lc), C.dptr(ly)))
        return {"X": lx, "A": la, "C": lc, "Y": ly}

    def set_bound_mode(self, mode):
        """Which lower bound elbo(), elbo_total() and iterate() form: "reference" (the reference's, quirks included; the
        default) or "exact" (E_q[ln p] - E_q[ln q]).  The updates do not depend on it.  Changing it empties the history."""
        if mode not in C.BOUND_MODES:
            raise ValueError("bound mode must be 'reference' or 'exact', not %r" % (mode,))
        self._check(C.lib.pyvb_lds_set_bound_mode(self._h, C.BOUND_MODES[mode]))
        self.bound = mode

    def get_warmup(self):
        w = np.empty((self.N, 2), dtype=np.int32)
        self._check(C.lib.pyvb_lds_get_warmup(self._h, w.ctypes.data_as(C._ip)))
        return w

    def get_time_split(self):
        w = C.ctypes.c_int()
        self._check(C.lib.pyvb_lds_get_time_split(self._h, C.ctypes.byref(w)))
        return w.value

    def set_time_split(self, W):
        """Wavefronts per replicate in the sweeps (chosen by the library; tests force W = 1, the headline code path)."""
        self._check(C.lib.pyvb_lds_set_time_split(self._h, int(W)))

    # -- updates ----------------------------------------------------------------------------
    def sweep(self, direction="forward"):
        self._check(C.lib.pyvb_lds_sweep(self._h, C.FORWARD if direction == "forward" else C.BACKWARD))

    def update_x(self, t):
        """Xs[t].update() in every active replicate that has a node t (t < T_n)."""
        self._check(C.lib.pyvb_lds_update_x(self._h, int(t)))

    def update_A(self):
        self._check(C.lib.pyvb_lds_update_A(self._h))

    def update_C(self):
        self._check(C.lib.pyvb_lds_update_C(self._h))

    def update_B(self):
        """[b.update() for b in Bs]: the columns of the input gain (handles with inputs)."""
        self._check(C.lib.pyvb_lds_update_B(self._h))

    def update_E(self):
        """[e.update() for e in Es]: the columns of the regressors' gain (handles with regressors)."""
        self._check(C.lib.pyvb_lds_update_E(self._h))

    def update_columns(self, which, col_begin, col_end):
        """As[i].update() (which = "A") or Cs[i].update() ("C") for i in [col_begin, col_end), in order."""
        self._check(C.lib.pyvb_lds_update_columns(self._h, 0 if which == "A" else 1, int(col_begin), int(col_end)))

    def update_Q(self):
        self._check(C.lib.pyvb_lds_update_Q(self._h))

    def update_R(self):
        self._check(C.lib.pyvb_lds_update_R(self._h))

    def elbo(self):
        """Per-replicate lower-bound parts [N,6] (X, Y, A, C, Q, R) of the current bound mode (set_bound_mode)."""
        self._check(C.lib.pyvb_lds_elbo(self._h))
        out = np.empty((self.N, 6))
        self._check(C.lib.pyvb_lds_get_elbo(self._h, C.dptr(out)))
        return out

    def elbo_total(self):
        """Parts summed over replicates (and over ranks when a communicator is attached)."""
        out = np.empty(6)
        self._check(C.lib.pyvb_lds_elbo_total(self._h, C.dptr(out)))
        return out

    def iterate(self, niters=1):
        """niters x (forward sweep, backward sweep, A, [B on a handle with inputs,] C, [E on a handle with regressors,] Q, R, [the
        columns' Gamma / DiagonalGamma parents,] lower bound); asynchronous."""
        self._check(C.lib.pyvb_lds_iterate(self._h, int(niters)))

    def elbo_history(self, last=4096):
        """Lower-bound parts of the most recent iterate() iterations, [count, 6], summed over the replicates (and over
        the ranks when a communicator is attached); oldest first."""
        out = np.empty((int(last), 6))
        cnt = C.ctypes.c_int()
        self._check(C.lib.pyvb_lds_get_elbo_history(self._h, C.dptr(out), int(last), C.ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def reset_elbo_history(self):
        self._check(C.lib.pyvb_lds_reset_elbo_history(self._h))

    def sync(self):
        self._check(C.lib.pyvb_lds_sync(self._h))

    # -- per-replicate bookkeeping ----------------------------------------------------------
    FAIL_BITS = ((C.FAIL_STATES, "X_t"), (C.FAIL_COLUMNS, "columns of A / C"), (C.FAIL_NOISE, "Wishart Q / R"))

    def _check(self, rc):
        """C.check; a LinAlgError carries .replicates, the indices of the active replicates that failed."""
        try:
            C.check(rc)
        except np.linalg.LinAlgError as e:
            st = self.status()
            e.replicates = [int(n) for n in np.nonzero((st != 0) & self.active())[0]]
            e.status = st
            raise

    def status(self):
        """int [N]: C.FAIL_* bits per replicate -- which node family's posterior precision was not positive definite --
        pending on the device or reported by the most recent failed sync.  Never raises because of a flag."""
        st = np.zeros(self.N, dtype=np.int32)
        C.check(C.lib.pyvb_lds_get_status(self._h, st.ctypes.data_as(C._ip)))
        return st

    @classmethod
    def describe_status(cls, bits):
        """The node families named by the FAIL_* bits of one replicate."""
        return ", ".join(nm for b, nm in cls.FAIL_BITS if int(bits) & b) or "none"

    def set_active(self, mask):
        """bool [N]: replicates with False are switched off -- no update touches them, their state reads back as it was, the
        totals leave them out, their flags no longer raise.  The mask can only shrink (switching one on again: error)."""
        m = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8)
        if m.shape != (self.N,):
            raise AssertionError("mask has shape %s, expected (%d,)" % (m.shape, self.N))
        C.check(C.lib.pyvb_lds_set_active(self._h, m.ctypes.data_as(C._ucp)))

    def active(self):
        m = np.zeros(self.N, dtype=np.uint8)
        C.check(C.lib.pyvb_lds_get_active(self._h, m.ctypes.data_as(C._ucp)))
        return m.astype(bool)

    def iterate_until(self, max_iters, tol=1e-3, check_every=8):
        """iterate(), with Network.learn's stopping test (network.py:53: the bound improved by less than tol) applied by every
        replicate to itself on the device.  A replicate that converges is frozen for the life of the handle and stays in the
        totals at its final bound.  Returns the number of iterations launched: it ends when no replicate is left running
        (seen every check_every iterations) or after max_iters.  Synchronises."""
        n = C.ctypes.c_int()
        self._check(C.lib.pyvb_lds_iterate_until(self._h, int(max_iters), float(tol), int(check_every), C.ctypes.byref(n)))
        return n.value

    def convergence(self):
        """(iters int [N], converged bool [N], llb float [N]): the iterations each replicate has carried out under
        iterate_until, whether it has converged, and the last bound its test saw (NaN before the first)."""
        it, cv, llb = np.zeros(self.N, dtype=np.int32), np.zeros(self.N, dtype=np.uint8), np.empty(self.N)
        self._check(C.lib.pyvb_lds_get_convergence(self._h, it.ctypes.data_as(C._ip), cv.ctypes.data_as(C._ucp), C.dptr(llb)))
        return it, cv.astype(bool), llb

    def iterate_until_model(self, max_iters, tol=1e-3, check_every=8):
        """iterate_until() with the stopping test applied by every MODEL to the bound of its graph, the sum of its chains' parts
        (models=, from_trials): the chains of a model share A, C, Q, R and stop together.  A model that converges is frozen for
        the life of the handle and stays in the totals at its final bound.  Where every replicate is a model of its own this is
        iterate_until, bitwise.  Returns the number of iterations launched.  Synchronises."""
        n = C.ctypes.c_int()
        self._check(C.lib.pyvb_lds_iterate_until_model(self._h, int(max_iters), float(tol), int(check_every), C.ctypes.byref(n)))
        return n.value

    def model_convergence(self):
        """(iters int [M], converged bool [M], llb float [M]), one entry per model: the iterations it has carried out under
        iterate_until_model, whether it has converged, and the last bound its test saw (NaN before the first).  convergence()
        returns the same values replicated on every chain of the model."""
        M = int(self.models[-1]) + 1
        it, cv, llb = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.uint8), np.empty(M)
        self._check(C.lib.pyvb_lds_get_model_convergence(self._h, it.ctypes.data_as(C._ip), cv.ctypes.data_as(C._ucp), C.dptr(llb)))
        return it, cv.astype(bool), llb

    # -- measurement ------------------------------------------------------------------------
    def timing(self, on=True):
        self._check(C.lib.pyvb_lds_timing_enable(self._h, 1 if on else 0))
        self._check(C.lib.pyvb_lds_timing_reset(self._h))

    def kernel_times(self):
        names = {"prep": C.K_PREP, "sweep_fwd": C.K_SWEEP_FWD, "sweep_bwd": C.K_SWEEP_BWD, "stats": C.K_STATS,
                 "params": C.K_PARAMS, "elbo": C.K_ELBO, "step": C.K_STEP, "gy": C.K_GY, "inputs": C.K_INPUTS}
        if self.Pv:     # the kernels of k_regressors.hip, on the handles that launch them
            names["regressors"] = C.K_REGRESSORS
        out = {}
        for nm, k in names.items():
            ms, cnt = C.ctypes.c_double(), C.ctypes.c_int()
            self._check(C.lib.pyvb_lds_timing_get(self._h, k, C.ctypes.byref(ms), C.ctypes.byref(cnt)))
            out[nm] = (ms.value, cnt.value)
        return out

    # -- multi-GPU --------------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        buf = C.ctypes.create_string_buffer(128)
        C.check(C.lib.pyvb_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid, rank, world):
        self._check(C.lib.pyvb_lds_comm_init(self._h, uid, int(rank), int(world)))

    def comm_init_host(self, comm, rank, world):
        """The ELBO all-reduce through a host process group (pyvb_amd.dist) instead of RCCL: rehearsal of the sharded
        path with several ranks on one GPU (pyvb_lds_comm_init_host)."""
        from .dist import host_allreduce_callback
        self._host_cb = host_allreduce_callback(comm)          # kept alive with the handle
        self._check(C.lib.pyvb_lds_comm_init_host(self._h, self._host_cb, None, int(rank), int(world)))

    # -- convenience ------------------------------------------------------------------------
    def live_rows(self):
        """bool [N, T]: True where row t is a node of replicate n's chain (t < T_n)."""
        return np.arange(self.T)[None, :] < self.lengths[:, None]

    def has_missing_outputs(self, Y):
        """NaN in a row of Y that is an output of some graph (padding rows do not count)."""
        return bool(np.isnan(np.asarray(Y))[self.live_rows()].any())

    @classmethod
    def from_series(cls, series, pri, device=0, U=None, V=None):
        """One handle for time series of different lengths: series is a list of (Y_n[T_n, K], st0_n) with st0_n as
        synth.initial_state(T_n, D, K, 1) gives it; replicate n is the graph with T_n time steps (pad_series).
        U: a list of U_n[T_n, P], the known input of every series (st0_n then carries B_mean, B_colvar), padded as Y is.
        V: a list of V_n[T_n, Pv], the known regressors of every series' outputs (st0_n then carries E_mean, E_colvar), likewise."""
        Y, st0, lengths = pad_series(series)

        def padded(L, nm):
            if L is None:
                return None
            Lp = np.zeros(Y.shape[:2] + (np.shape(L[0])[1],))
            for n, u in enumerate(L):
                if np.shape(u) != (lengths[n], Lp.shape[2]):
                    raise AssertionError("series %d: %s has shape %s, expected (%d, %d)" % (n, nm, np.shape(u), lengths[n], Lp.shape[2]))
                Lp[n, :lengths[n]] = u
            return Lp
        return cls.from_problem(Y, st0, pri, device, lengths=lengths, U=padded(U, "U"), V=padded(V, "V"))

    @classmethod
    def from_trials(cls, trials, pri, device=0):
        """One model fitted to several recorded series (trials, sessions, subjects): trials is a list with one entry per model,
        each a list of (Y_n[T_n, K], st0_n) as from_series takes them.  The chains of a model share A, C, Q, R; their
        initial parameters are those of the model's first entry, every chain keeps its own initial states (pad_series)."""
        if not trials or any(len(t) == 0 for t in trials):
            raise ValueError("every model needs at least one series")
        Y, st0, lengths = pad_series([s for t in trials for s in t])
        models = np.repeat(np.arange(len(trials), dtype=np.int32), [len(t) for t in trials])
        return cls.from_problem(Y, st0, pri, device, lengths=lengths, models=models)

    @classmethod
    def from_problem(cls, Y, st0, pri, device=0, lengths=None, models=None, U=None, V=None):
        """U [N, T, P]: a known input that drives the states (synth.make_input_problem); st0 then carries B_mean and B_colvar, pri
        B_prior_mean and B_prior_prec.  V [N, T, Pv]: known regressors in the output equation (synth.make_regression_problem); st0
        then carries E_mean and E_colvar, pri E_prior_mean and E_prior_prec."""
        N, T, K = Y.shape
        D = st0["A_mean"].shape[1]
        b = cls(N, T, D, K, pri.get("noise", "diagonal_gamma"), device, lengths=lengths, models=models,
                inputs=0 if U is None else np.shape(U)[2], regressors=0 if V is None else np.shape(V)[2])
        b.set_priors(pri)
        b.set_observations(Y)
        if V is not None:
            b.set_regressors(V)
            b.set_state(E_mean=st0["E_mean"], E_colvar=st0["E_colvar"])
        if U is not None:
            b.set_inputs(U)
            b.set_state(B_mean=st0["B_mean"], B_colvar=st0["B_colvar"])
        if "Yq" in st0 and b.has_missing_outputs(Y):
            b.set_output_state(st0["Yq"], st0["Yrowvar"])
        if b.noise == "wishart":        # the compact initial state carries the diagonal of qw in Q_b / R_b
            b.set_state(**{k: st0[k] for k in ("X", "A_mean", "A_colvar", "C_mean", "C_colvar")})
            dense = lambda v: np.einsum("nd,de->nde", v, np.eye(v.shape[1])) if v.ndim == 2 else v
            b.set_wishart_state(dense(st0["Q_b"]), dense(st0["R_b"]))
        else:
            b.set_state(**{k: st0[k] for k in ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_b", "R_b")})
        if pri.get("A_obs") is not None or pri.get("C_obs") is not None:
            b.set_column_observations(pri.get("A_obs"), pri.get("C_obs"))
        # Gamma parents of the columns: priors in pri (A_alpha_a0, A_alpha_b0; the same for C), the state in st0 (A_alpha_b, C_alpha_b)
        ard = {w: (pri[w + "_alpha_a0"], pri[w + "_alpha_b0"], st0[w + "_alpha_b"]) for w in ("A", "C") if pri.get(w + "_alpha_a0") is not None}
        if ard:
            b.set_column_precisions(**ard)
        # DiagonalGamma parents, one precision per entry: A_entry_a0, A_entry_b0 in pri, A_entry_b in st0 (the same for C)
        ent = {w: (pri[w + "_entry_a0"], pri[w + "_entry_b0"], st0[w + "_entry_b"]) for w in ("A", "C") if pri.get(w + "_entry_a0") is not None}
        if ent:
            b.set_entry_precisions(**ent)
        return b
