"""TEST INFRASTRUCTURE: the oracles run in extended precision (np.longdouble, 64-bit significand), the yardstick that
measures the float64 oracle and the HIP kernels against that run, and the cases both are measured on.

The algorithm is not restated: oracle/lds_closed_form.py and oracle/pca_closed_form.py preserve the dtype of what they are
given, and their inversions / factorisations go through oracle/_xlinalg.py, which has a long-double version.  to_long()
casts a problem; *_trace() runs the example's loop stage by stage and records every compared quantity after the stage
that produces it.  The same trace function drives the float64 oracle, the extended run and (tests/test_envelope_gpu.py) the
handle, so the three sequences of (key, array) line up by construction.

Yardstick.  For a quantity q after a stage, with rel() the suite's max-norm relative error,
    e64   = rel(float64 oracle, extended run)          what LAPACK / einsum in float64 lose on this problem
    y     = max(e64, n 2^-52),  n = max(D, K, T)       (max(d, q, N) for PCA): never below one length-n float64 accumulation
    e_gpu = rel(handle, extended run) <= FACTOR y,     FACTOR = 16
and every case must have e64 <= CAP = 1e-11 on every quantity, so the bound never exceeds 1.6e-10.

The lower bound.  digamma and gammaln have a long-double version (oracle/_xspecial.py), so elbo_parts and
tests/exact_bound_ref.py: elbo_parts_exact run in extended precision too, and the traces yield the parts [N, 6] (PCA: [5])
after each iteration under the key (iteration, "bound", mode).  A part is measured in units of its replicate's
s_r = sum_p |part_p| of the extended run (the parity suite's convention for the parts):
    e64 = |p64 - pext| / s_r,   e_gpu = |pgpu - pext| / s_r <= FACTOR max(e64, n 2^-52),   e64 <= CAP
part by part and replicate by replicate (bound_errors, compare_bound).

Outputs with missing entries are also measured row by row (compare_rows): a row's missing entries in units of the row's largest
one, e_row <= FACTOR max(e64_row, n 2^-52) with e64_row <= CAP, its known entries bitwise -- on cases whose rows are named
patterns (_missing_rows), in the envelope's order and in orders of their own (lds_trace_order, rows_reference).

VB-PCA is measured row by row too (compare_pca_rows): X over a row's missing entries, Z over the row, X_rowvar, each in the row's own
unit and by the same rule, the observed entries of X bitwise the data -- on cases whose rows are named patterns aimed at the mask
words, tiles, blocks and halves of the sweeps (PCA_ROW_PATTERNS, PCA_ROW_CASES, pca_rows_reference).

The 128-wide LDS class is measured tile by tile (BIG_CASES, tile_errors, compare_tiles): the last two axes of every matrix
quantity cut into 16 x 16 tiles, the states into the 16-entry tile of each node, each tile in units of its own largest entry
of the extended run, e_tile <= FACTOR max(e64_tile, n 2^-52) with e64_tile <= CAP; a tile that is exactly zero in the extended
run is exactly zero on the handle, and the known entries of A and C are held bitwise (known_offenders).

Known inputs and regressors are measured chain by chain, channel by channel and end node by end node (channel_errors,
compare_channels; the cases are inputs_ref.CHANNEL_CASES and regressors_ref.CHANNEL_CASES): every quantity and every part of both
bounds of each replicate on its own, column p of B_mean / E_mean and row p of B_colvar / E_colvar, X at nodes 0, 1, T_n - 2 and
T_n - 1, each in units of its own largest entry of the extended run, e_unit <= FACTOR max(e64_unit, n 2^-52) with n = max(T_n, D, K)
of the chain's own length and e64_unit <= CAP; a unit that is exactly zero in the extended run is exactly zero on the handle.
"""
import functools
import importlib.util
import os

import numpy as np

import exact_bound_ref as XR
from oracle import lds_closed_form as O
from oracle import pca_closed_form as P
from pyvb_amd import synth

LD = np.longdouble
U64 = 2.0 ** -52
FACTOR = 16.0
CAP = 1e-11
HERE = os.path.dirname(os.path.abspath(__file__))


def require_extended():
    """The reference must carry at least 11 bits more than float64; a platform whose long double is float64 cannot run these
    tests, and that is a failure, not a skip."""
    eps = float(np.finfo(LD).eps)
    if eps > 2.0 ** -63:
        raise RuntimeError("np.longdouble has eps = %.3e > 2^-63 on this platform: no extended-precision reference, "
                           "the accuracy-envelope tests cannot run here" % eps)


def _cast(v):
    if isinstance(v, np.ndarray):
        return v.astype(LD) if v.dtype.kind == "f" else v.copy()
    if isinstance(v, (float, np.floating)):
        return LD(v)
    return v


def to_long(d):
    """A copy of a dict of states, priors or initial values -- or of one array -- with every floating-point entry cast to
    np.longdouble (exactly); masks, integers and strings stay."""
    require_extended()
    if isinstance(d, dict):
        return {k: _cast(v) for k, v in d.items()}
    return _cast(np.asarray(d))


def rel(a, b):
    """max |a - b| / max |b| (tests/test_gpu_parity.py: _rel), formed in long double."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), LD(1e-300)))


def yardstick(e64, n):
    return max(e64, n * U64)


BOUND_MODES = ("reference", "exact")
LDS_PARTS = ("L_X", "L_Y", "L_A", "L_C", "L_Q", "L_R")
PCA_PARTS = ("L_W", "L_Z", "L_X", "L_Mu", "L_Beta")


def bound_errors(got, ext):
    """The yardstick's unit for the parts of a bound.  got, ext: [N, P] (or [P]: one replicate).  Returns
    (|got - ext| / s_r, |got - ext| / |ext|) as float64 [N, P], s_r = sum_p |ext[r, p]|; the second is for the record only
    (a part that is exactly 0 in the extended run reports 0 or inf there)."""
    got, ext = np.atleast_2d(np.asarray(got, dtype=LD)), np.atleast_2d(np.asarray(ext, dtype=LD))
    assert got.shape == ext.shape, (got.shape, ext.shape)
    d = np.abs(got - ext)
    s = np.abs(ext).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(d == 0, LD(0), d / np.abs(ext))
    return (d / s).astype(float), own.astype(float)


def compare_bound(got, ext, e64, n):
    """[(replicate, part index, e64, e_gpu, e_gpu / y, error relative to the part itself)] for parts `got` [N, P] against the
    extended run's `ext`, with e64 [N, P] the float64 oracle's distance from it in the same unit."""
    e_gpu, own = bound_errors(got, ext)
    e64 = np.atleast_2d(e64)
    return [(r, p, float(e64[r, p]), float(e_gpu[r, p]), float(e_gpu[r, p] / yardstick(float(e64[r, p]), n)), float(own[r, p]))
            for r in range(e_gpu.shape[0]) for p in range(e_gpu.shape[1])]


# ----------------------------------------------------------------------------------------------------------------------------
# LDS cases (the smallest shapes that reach each kernel instantiation)
# ----------------------------------------------------------------------------------------------------------------------------
def _wishart_priors(pri, D, K, rng):
    """tests/test_gpu_parity.py: _wishart_priors with a generator -- proper priors: v0 > (dim - 1) / 2, dense w0"""
    pri["noise"] = "wishart"
    W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
    W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)


def _plain(T, D, K, N, seed, **kw):
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=seed)
    return dict(Y=Y, st0=st0, pri=pri, iters=2, **kw)


def _gamma(T, D, K, N, seed):
    c = _plain(T, D, K, N, seed)
    c["pri"]["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        c["pri"][k] = np.float64(1e-3)
    return c


def _hard(T, D, K, N, seed):
    """tests/test_gpu_parity.py: test_warmup_is_data_driven_and_exact_fallback -- F close to its spectral bound"""
    c = _plain(T, D, K, N, seed)
    c["st0"]["R_b"] = c["st0"]["R_b"] * 1e8
    c["st0"]["Q_b"] = c["st0"]["Q_b"] * 1e-6
    return c


def _wishart(T, D, K, N, seed, iters=2, known=False):
    c = _plain(T, D, K, N, seed)
    c["iters"] = iters
    _wishart_priors(c["pri"], D, K, np.random.default_rng(T))
    if known:           # tests/test_gpu_parity.py: test_known_matrix_entries_with_wishart_noise
        rng = np.random.default_rng(5)
        A_obs = np.full((D, D), np.nan); C_obs = np.full((K, D), np.nan)
        A_obs[0, 0] = 0.9; A_obs[min(3, D - 1), 2] = -0.25; A_obs[D - 1, 2] = 0.1
        A_obs[:, D - 1] = np.linspace(-0.2, 0.2, D)
        C_obs[rng.random((K, D)) < 0.15] = 0.5
        C_obs[:, 1] = np.arange(K) * 0.1 - 0.2
        C_obs[:, 0] = np.nan
        c["pri"]["A_obs"], c["pri"]["C_obs"] = A_obs, C_obs
    return c


def _missing(T, D, K, N, seed):
    """tests/test_gpu_parity.py: test_outputs_with_missing_entries"""
    c = _plain(T, D, K, N, seed)
    rng = np.random.default_rng(T + K)
    mask = rng.random((N, T, K)) < 0.15
    mask[:, 1] = True; mask[:, T // 2] = True; mask[:, 0, 0] = True; mask[:, 3] = False
    c["Y"] = np.where(mask, np.nan, c["Y"])
    c["st0"]["Yq"] = rng.standard_normal((N, T, K)); c["st0"]["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, T))
    return c


def _known(T, D, K, N, seed):
    """tests/test_gpu_parity.py: test_known_matrix_entries_vs_oracle"""
    c = _plain(T, D, K, N, seed)
    A_obs = np.full((D, D), np.nan); C_obs = np.full((K, D), np.nan)
    A_obs[0, 0] = 1.0; A_obs[1, 0] = 1e-2; A_obs[3, 2] = -0.5
    A_obs[:, 4] = np.linspace(-0.2, 0.2, D)
    C_obs[2, 1] = 3.0; C_obs[:, 3] = np.arange(K) - 2.0
    c["pri"]["A_obs"], c["pri"]["C_obs"] = A_obs, C_obs
    return c


def _lengths(lengths, D, K, seed):
    """tests/test_lengths_gpu.py: _problem -- one handle, a chain length per replicate, padding rows zero"""
    T, N = max(lengths), len(lengths)
    c = _plain(T, D, K, N, seed)
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    c["Y"] = np.where(live[:, :, None], c["Y"], 0.0)
    c["st0"]["X"] = np.where(live[:, :, None], c["st0"]["X"], 0.0)
    c["lengths"] = tuple(lengths)
    return c


ROW_PATTERNS = ("all", "one known, first", "one known, last", "one missing, first", "one missing, last", "a tile", "alternating",
                "upper half", "observed", "Bernoulli", "all")
ROW_PATTERNS_BIG = {5: "low half", 6: "high half", 7: "the seam"}      # K > 64: instead of the tile, alternating and upper half


def _missing_rows(T, K, rng):
    """(mask [T, K], true = missing; the name of each row's pattern).  Row t takes pattern t mod 11 of ROW_PATTERNS -- for K > 64
    the three of ROW_PATTERNS_BIG, which meet the kernels' second entry per lane (lane + 64), in place of indices 5..7 -- and the
    last row is then "all": rows 0 and T - 1 are unobserved nodes at the ends of the chain.  These are the pivot sets a
    Bernoulli mask meets only by luck: one known entry in a row, one missing entry in lane 0 or lane K - 1, exactly one
    8-wide tile, every second entry."""
    k = np.arange(K)
    mask, names = np.zeros((T, K), dtype=bool), []
    for t in range(T):
        p = 10 if t == T - 1 else t % 11
        name = ROW_PATTERNS_BIG.get(p, ROW_PATTERNS[p]) if K > 64 else ROW_PATTERNS[p]
        mask[t] = {"all": lambda: k >= 0, "one known, first": lambda: k != 0, "one known, last": lambda: k != K - 1,
                   "one missing, first": lambda: k == 0, "one missing, last": lambda: k == K - 1,
                   "a tile": lambda: k < min(8, K - 1), "alternating": lambda: k % 2 == 0, "upper half": lambda: k >= K // 2,
                   "observed": lambda: k < 0, "Bernoulli": lambda: rng.random(K) < 0.3,
                   "low half": lambda: k < 64, "high half": lambda: k >= 64, "the seam": lambda: (k == 63) | (k == 64)}[name]()
        names.append(name)
    return mask, names


def _rows(c, **kw):
    """The named row patterns on the outputs of a case: replicate 0 takes _missing_rows; a second replicate has exactly one
    missing entry (row 2, entry 1), so a replicate with almost nothing to do sits beside a full one.  Yq and Yrowvar as
    _missing draws them.  c["patterns"][n][t] names the pattern of row t of replicate n."""
    N, T, K = c["Y"].shape
    assert N in (1, 2)
    rng = np.random.default_rng(T + K)
    mask = np.zeros((N, T, K), dtype=bool)
    mask[0], names = _missing_rows(T, K, rng)
    c["patterns"] = [names]
    if N == 2:
        mask[1, 2, 1] = True
        c["patterns"].append(["one missing, alone" if t == 2 else "observed" for t in range(T)])
    c["Y"] = np.where(mask, np.nan, c["Y"])
    c["st0"]["Yq"] = rng.standard_normal((N, T, K)); c["st0"]["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, T))
    c.update(kw)
    return c


def _default_outputs(c, explicit):
    """A case of _rows with the initial outputs a handle gives itself when it is told none -- N(0, I) on every row that holds
    NaN -- either spelled out (explicit) or left out of the state."""
    if explicit:
        c["st0"]["Yq"] = np.where(np.isnan(c["Y"]).any(axis=2, keepdims=True), 0.0, np.nan_to_num(c["Y"]))
        c["st0"]["Yrowvar"] = np.ones(c["Y"].shape[:2])
    else:
        del c["st0"]["Yq"], c["st0"]["Yrowvar"]
    c["iters"] = 1
    return c


# name -> (builder, in the warm-up contract?)
LDS_CASES = {
    "t19_d6_k4":            (lambda: _plain(19, 6, 4, 2, 101), False),
    "t77_d16_k16":          (lambda: _plain(77, 16, 16, 2, 102), True),
    "t77_d33_k17_gamma":    (lambda: _gamma(77, 33, 17, 2, 103), False),
    "t40_d64_k64":          (lambda: _plain(40, 64, 64, 1, 104), True),
    "t700_d8_k8_split":     (lambda: _plain(700, 8, 8, 1, 105, split_chosen=True), True),
    "t2402_d64_k64_w1":     (lambda: dict(_plain(2402, 64, 64, 1, 106, W=1, headline=True), iters=1), True),
    "t400_d4_k4_hard":      (lambda: _hard(400, 4, 4, 2, 2), True),
    "t12_d72_k66_big":      (lambda: _plain(12, 72, 66, 1, 108), True),
    "t600_d72_k66_big_w3":  (lambda: dict(_plain(600, 72, 66, 1, 109, W=3), iters=1), True),
    "t40_d16_k16_wishart":  (lambda: _wishart(40, 16, 16, 2, 110), False),
    "t30_d33_k17_wishart":  (lambda: _wishart(30, 33, 17, 1, 111), False),
    "t30_d17_k9_wishart_known": (lambda: _wishart(30, 17, 9, 1, 112, known=True), False),
    "t6_d72_k9_wishart_big": (lambda: _wishart(6, 72, 9, 1, 113, iters=1), False),
    "t60_d5_k6_missing":    (lambda: _missing(60, 5, 6, 2, 114), False),
    "t80_d5_k6_known":      (lambda: _known(80, 5, 6, 2, 115), False),
    "lengths_3_19_60_77_d16_k16": (lambda: _lengths((3, 19, 60, 77), 16, 16, 116), True),
    # length 2 is the shortest chain a handle accepts: no interior class, nint = 0 in the bound (no recurrence matrices either,
    # so the case is not in the warm-up contract)
    "lengths_2_17_33_d16_k16": (lambda: _lengths((2, 17, 33), 16, 16, 117), False),
    # outputs with missing entries in named row patterns (_missing_rows), two iterations with update_Y in both.  Wishart noise:
    # k_impute_dense, whose every row exchanges on a pivot set of its own -- two replicates, one of them with a single missing
    # entry; K = 64, where no lane is idle and a row has 63 pivots (with this seed the float64 oracle stays at 5e-13 row by row
    # after the second update_Y too; a draw whose cov - gain cov^T cancellation puts the one-known rows over the cap is to be
    # replaced, tests/test_missing_rows_cpu.py decides); T = 3, where one of the kernel's four wavefronts owns no row; the
    # shortest chain; known columns of C beside dense <y y^T>.  Then the 128-wide class, whose lanes take entries lane and
    # lane + 64 (K <= 102: the float64 bound is finite, quirk Q2).  Seven
    # outputs of 72 states leave the Gamma case's second iteration close to the cap on the reference side (e64 5.6e-12 with
    # this seed, 2.2e-12 row-wise; of seeds 124, 127..130 the others are at 8e-12..2e-11 and over it row-wise).
    "t11_d5_k9_wishart_rows":   (lambda: _rows(_wishart(11, 5, 9, 2, 118)), False),
    "t11_d6_k64_wishart_rows":  (lambda: _rows(_wishart(11, 6, 64, 1, 119)), False),
    "t3_d17_k33_wishart_rows":  (lambda: _rows(_wishart(3, 17, 33, 1, 120)), False),
    "t2_d3_k2_wishart_rows":    (lambda: _rows(_wishart(2, 3, 2, 1, 121)), False),
    "t11_d17_k9_wishart_known_rows": (lambda: _rows(_wishart(11, 17, 9, 1, 122, known=True)), False),
    "t11_d12_k100_rows_big":    (lambda: _rows(_plain(11, 12, 100, 1, 123)), False),
    "t7_d72_k70_gamma_rows_big": (lambda: _rows(_gamma(7, 72, 70, 1, 128)), False),
}
# Cases of tests/test_missing_rows_gpu.py alone.  K = 128 is compared on the outputs only: with the default prior precision the
# float64 oracle's bound is inf there (quirk Q2), so the case forms no bound and is not in the envelope.
ROW_CASES = {
    "t7_d65_k128_rows_big":     lambda: _rows(_plain(7, 65, 128, 1, 125), outputs_only=True),
    # (seven rows stop at "low half": the high half and the seam with no lane idle in either half need eleven)
    "t11_d9_k128_rows_big":     lambda: _rows(_plain(11, 9, 128, 1, 126), outputs_only=True),
    "t11_d5_k9_wishart_rows_default":   lambda: _default_outputs(lds_case("t11_d5_k9_wishart_rows"), False),
    "t11_d5_k9_wishart_rows_explicit":  lambda: _default_outputs(lds_case("t11_d5_k9_wishart_rows"), True),
    "t11_d12_k100_rows_big_default":    lambda: _default_outputs(lds_case("t11_d12_k100_rows_big"), False),
    "t11_d12_k100_rows_big_explicit":   lambda: _default_outputs(lds_case("t11_d12_k100_rows_big"), True),
}
ROWS_ENVELOPE = [k for k in LDS_CASES if "_rows" in k]
WARMUP_CASES = [k for k, v in LDS_CASES.items() if v[1]]
# The exact bound needs a handle of its own (the mode is set before the first update); these two reach no
# other instantiation of the bound than t40_d64_k64 and t12_d72_k66_big do, so their long runs are not repeated.
EXACT_BOUND_CASES = [k for k in LDS_CASES if k not in ("t2402_d64_k64_w1", "t600_d72_k66_big_w3")]


# ----------------------------------------------------------------------------------------------------------------------------
# the 128-wide class, 64 < max(D, K) <= 128, at every tile count (tests/test_big_envelope_cpu.py, tests/test_big_envelope_gpu.py)
# ----------------------------------------------------------------------------------------------------------------------------
def _q2(c):
    """Where max(D, K) > 102 the column prior precisions are 1e-2: det(1e-3 I) underflows from 103 dimensions on and the float64
    oracle's bound is -inf (quirk Q2; tests/test_gpu_parity.py: test_stagewise_vs_oracle_beyond_64 does the same)."""
    D, K = c["st0"]["A_mean"].shape[1], c["Y"].shape[2]
    if max(D, K) > 102:
        c["pri"]["A_prior_prec"] = np.full_like(c["pri"]["A_prior_prec"], 1e-2)
        c["pri"]["C_prior_prec"] = np.full_like(c["pri"]["C_prior_prec"], 1e-2)
    return c


def _known_at_block_edges(T, D, K, seed):
    """_known (entries (0, 0), (1, 0), (3, 2) and the whole column 4 of A; entry (2, 1) and the whole column 3 of C; column 0 of C
    free) with known entries of both matrices on either side of the edges of k_cols_big's 16-column blocks: columns 15, 16, 17
    and 95, and column 96, the one column of the last block at D = 97; the last row of A and of C among them."""
    c = _known(T, D, K, 1, seed)
    assert D == 97
    A_obs, C_obs = c["pri"]["A_obs"], c["pri"]["C_obs"]
    for j, col in enumerate((15, 16, 17, 95, 96)):
        A_obs[[7 * j + 3, 16 * j + 15, 16 * j + 16], col] = (0.05 * (j + 1), -0.1, 0.02 * (j - 2))
        C_obs[[11 * j + 1, 16 * j + 31, 16 * j + 32], col] = (0.5 - 0.25 * j, 1.5, -0.75)
    # the last row of each.  Entry (last row, 96) stays free: it is a tile of its own, and a tile of known entries alone has no unit
    # -- the oracle conditions on them by formula and leaves a rounding residue where the handle has 0.0 (known_offenders holds that)
    A_obs[D - 1, 95] = 0.125; A_obs[D - 1, 16] = -0.0625
    C_obs[K - 1, 16] = 2.0; C_obs[K - 1, 95] = -1.0
    assert np.isnan(C_obs[:, 0]).all() and not np.isnan(A_obs[:, 4]).any() and np.isnan(A_obs[D - 1, 96]) and np.isnan(C_obs[K - 1, 96])
    return c


# name -> (builder, in the warm-up contract?).  Two iterations and N = 1 unless the name or the builder says otherwise.  What
# each is there for (pyvb_amd/csrc/k_big.hip, k_wishart_big.hip; tests/test_big_envelope_cpu.py holds the counts):
BIG_CASES = {
    # full width, nothing padded: eight real tiles in every kernel, every tile pair of k_stats_big; 33 interior nodes: Lseg = 3,
    # eleven live segment columns and five idle; statistics chunks of 12, 12 and 11 rows
    "t35_d128_k128":        (lambda: _q2(_plain(35, 128, 128, 1, 201)), True),
    # D & 3 != 0: the scalar stores of Sigma in k_prep_big; K odd: k_gy_big<false> and its clamped loads; one padded row in state
    # tile 7, one real row in output tile 7; chunks of 16 and 11 rows
    "t27_d127_k113":        (lambda: _q2(_plain(27, 127, 113, 1, 202)), True),
    # the smallest shape of the class, one real row in tile 4; two replicates: the strides of the gains block, scratch, trash
    "t27_d65_k65_n2":       (lambda: _q2(_plain(27, 65, 65, 2, 203)), True),
    # isotropic noise on the two-wavefront k_noise<2> / k_elbo<2>; one real row in state tile 7
    "t27_d113_k81_gamma":   (lambda: _q2(_gamma(27, 113, 81, 1, 204)), False),
    # k_cols_big for C with wavefronts 1..3 owning no row; K odd and below one tile pair
    "t27_d128_k17":         (lambda: _q2(_plain(27, 128, 17, 1, 205)), True),
    # D <= 64 < K: two column blocks against 128 rows, Syx row tiles up to 7 against state tiles 0 and 1
    "t27_d17_k128":         (lambda: _q2(_plain(27, 17, 128, 1, 206)), True),
    # known entries of A and C at the block edges of k_cols_big.  The seed: the reference's bound takes ln(det) of a partly known
    # column's covariance over its free entries (gaussian.py:150; 93 to 112 of them here), which float64 represents only between
    # 1e-308 and 1e308 -- the same hazard as quirk Q2.  With this draw the determinants are within 1e-225 .. 1e218 after both
    # iterations; with seeds 207, 209, 214, 215, 219 one underflows after the first and the float64 oracle's L_C is -inf.
    "t27_d97_k113_known":   (lambda: _q2(_known_at_block_edges(27, 97, 113, 218)), False),
    # gj_wg128 with 128 real pivots in k_wexpect_big and k_cols_wishart_big, covb_pos with RT = 16 -- on the Q side, then on the R side
    "t20_d128_k81_wishart": (lambda: _q2(_wishart(20, 128, 81, 1, 301, iters=1)), False),
    "t20_d97_k128_wishart": (lambda: _q2(_wishart(20, 97, 128, 1, 302, iters=1)), False),
    # columns that warm up from zero at full width; run at W = 1 and at W = 2 (parts of 304 and 294 nodes, Lseg = 19: the warm-up
    # crosses a part border, with the forward sweep's own c_t buffer) against this one reference
    "t600_d128_k128_warm":  (lambda: dict(_q2(_plain(600, 128, 128, 1, 208)), iters=1, splits=(1, 2)), True),
}
BIG_WARMUP_CASES = [k for k, v in BIG_CASES.items() if v[1]]
BIG_SPLITS = {"t600_d128_k128_warm": (1, 2)}        # the forced time splits a case is run at (its "splits")
BIG_EXACT_BOUND_CASES = ["t35_d128_k128", "t27_d127_k113"]      # the others reach no further instantiation of k_elbo<2>


def lds_case(name):
    if name in BIG_CASES:
        return BIG_CASES[name][0]()
    return ROW_CASES[name]() if name in ROW_CASES else LDS_CASES[name][0]()


class OracleLDS(object):
    """The stage calls of pyvb_amd.lds.LDSBatch on one oracle state, in the dtype of what it is given."""

    def __init__(self, Y, st0, pri):
        self.Y, self.pri, self.T = Y, pri, Y.shape[1]
        self.st = O.expand_state(st0, pri, self.T, Y)
        self.noise = pri["noise"]
        self.post = self.S = None
        self.recurrences = []

    def sweep(self, direction):
        if direction == "forward":
            self.post = O.state_posteriors(self.st, self.pri)
            if self.T > 2:      # the recurrence matrices of the segmented sweeps: F = Sigma_1 <Q><A>, B = Sigma_1 <A>^T<Q>
                S1, Qb, A = self.post["Sigma"][:, 1], self.post["Qbar"], self.st["A_mean"]
                self.recurrences.append((S1 @ (Qb @ A), S1 @ (np.swapaxes(A, -1, -2) @ Qb)))
        O.sweep(self.st, self.pri, self.Y, direction, self.post)

    def update_Y(self):
        O.update_Y(self.st, self.pri)

    def update_A(self):
        self.S = O.statistics(self.st, self.Y)
        O.update_A(self.st, self.pri, self.S)

    def update_C(self):
        O.update_C(self.st, self.pri, self.S)

    def update_Q(self):
        O.update_Q(self.st, self.pri, self.S, self.T)

    def update_R(self):
        O.update_R(self.st, self.pri, self.S, self.T)

    def elbo_parts(self, mode):
        """[N, 6] of the state as it is, from the statistics the parameter updates of this iteration read (O.iterate)."""
        fn = O.elbo_parts if mode == "reference" else XR.elbo_parts_exact
        return fn(self.st, self.pri, self.S, self.T)

    # readers, shaped as the handle's
    def read(self, name):
        st = self.st
        if name == "Sigma":
            return st["Sigma"]
        if name in ("A_colvar", "C_colvar"):
            return np.einsum("nikk->nik", st[name[0] + "_cov"])
        if name in ("Q_v", "R_v"):
            return st[name[0] + "_a"]
        if name in ("Q_w", "R_w"):
            return st[name[0] + "_b"]
        if name in ("Q_b", "R_b") and st[name].ndim == 1:       # Gamma: one scalar per replicate, the handle repeats it
            dim = st["A_mean"].shape[1] if name == "Q_b" else st["C_mean"].shape[1]
            return np.repeat(st[name][:, None], dim, axis=1)
        return st[name]


class HandleLDS(object):
    """The same calls and readers on an LDSBatch."""

    def __init__(self, b):
        self.b, self.noise, self.T = b, b.noise, b.T

    def __getattr__(self, name):
        return getattr(self.b, name)

    def elbo_parts(self, mode):
        assert self.b.bound == mode, "the handle forms the %s bound, not the %s one" % (self.b.bound, mode)
        return self.b.elbo()

    def read(self, name):
        b = self.b
        if name == "Sigma":
            return b.get_posterior_classes()[0]
        if name in ("Yq", "Yvar"):
            return b.get_outputs()[name == "Yvar"]
        if name in ("Q_v", "Q_w", "R_v", "R_w"):
            return b.get_wishart_state()[name]
        if name in ("A_cov", "C_cov"):
            return b.get_column_cov()[name == "C_cov"]
        return b.get_state((name,))[name]


def lds_trace(m, iters, missing, bounds=()):
    """Drive m (OracleLDS or HandleLDS) through `iters` passes of the example's loop; yields ((iteration, stage, name), array)
    after every stage for every quantity the envelope compares, and after each pass ((iteration, "bound", mode), parts [N, 6])
    for every mode in `bounds` (an oracle forms both on one state; a handle forms the one it was set to)."""
    wishart = m.noise == "wishart"
    for it in range(iters):
        m.sweep("forward")
        yield (it, "forward sweep", "X"), np.array(m.read("X"))
        m.sweep("backward")
        yield (it, "backward sweep", "X"), np.array(m.read("X"))
        yield (it, "backward sweep", "Sigma"), np.array(m.read("Sigma"))
        if missing:
            m.update_Y()
            yield (it, "update_Y", "Yq"), np.array(m.read("Yq"))
            yield (it, "update_Y", "Yvar"), np.array(m.read("Yvar"))
        m.update_A()
        yield (it, "update_A", "A_mean"), np.array(m.read("A_mean"))
        m.update_C()
        yield (it, "update_C", "C_mean"), np.array(m.read("C_mean"))
        m.update_Q()
        m.update_R()
        names = ["A_colvar", "C_colvar"] + (["Q_v", "Q_w", "R_v", "R_w", "A_cov", "C_cov"] if wishart else ["Q_b", "R_b"])
        for nm in names:
            yield (it, "update_R", nm), np.array(m.read(nm))
        for mode in bounds:
            yield (it, "bound", mode), np.array(m.elbo_parts(mode))


def _alone(c, n, Tn):
    """Replicate n of a case with chain lengths, as a problem of its own (tests/test_lengths_gpu.py: _alone)."""
    Y = c["Y"][n:n + 1, :Tn].copy()
    st0 = {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]).copy() for k, v in c["st0"].items()}
    return Y, st0


def _cut(key, arr, rows, T):
    """The part of a handle-shaped array that a reference run covers: all replicates, or replicate `rows` of a handle with
    chain lengths (its first T rows of X); of Sigma the classes that are alive (no interior class at T = 2)."""
    if rows is not None:
        arr = arr[rows:rows + 1]
        if key[2] == "X":
            arr = arr[:, :T]
    if key[2] == "Sigma" and T <= 2:
        arr = arr[:, [0, 2]]
    return arr


def is_bound(key):
    return key[1] == "bound"


def _problems(c):
    """[(rows, T, Y, st0)]: the whole batch of a case, or each replicate alone where the replicates have lengths of their own"""
    if c.get("lengths"):
        return [(n, Tn) + _alone(c, n, Tn) for n, Tn in enumerate(c["lengths"])]
    return [(None, c["Y"].shape[1], c["Y"], c["st0"])]


def lds_float64_bound(name):
    """[{(iteration, "bound", mode): parts [N, 6]}] of a fresh run of the float64 oracle, one dict per entry of
    lds_reference(name).  Not cached: tests/test_extended_ref_cpu.py runs it with parts of the oracle replaced by mutants."""
    c = lds_case(name)
    missing = bool(np.isnan(c["Y"]).any())
    out = []
    for rows, T, Y, st0 in _problems(c):
        m64 = OracleLDS(Y.copy(), {k: v.copy() for k, v in st0.items()}, c["pri"])
        out.append({k: a for k, a in lds_trace(m64, c["iters"], missing, BOUND_MODES) if is_bound(k)})
    return out


def lds_reference(name):
    """[(rows, T, n, ext, e64, recurrences, run)] for a case (see _lds_reference)."""
    return _lds_reference(name)[0]


def lds_bound_reference(name):
    """[{(iteration, "bound", mode): (ext [N, 6] long double, e64 [N, 6], the same relative to each part itself)}], one dict
    per entry of lds_reference(name), from the same two runs."""
    return _lds_reference(name)[1]


def lds_tile_reference(name):
    """[{key: e64 by tile (tile_errors of the float64 oracle)}], one dict per entry of lds_reference(name), from the same two
    runs; for the cases of BIG_CASES."""
    return _lds_reference(name)[2]


@functools.lru_cache(maxsize=None)
def _lds_reference(name):
    """([(rows, T, n, ext, e64, recurrences, run)], [bound records], [tile records]) for a case: one entry for the whole batch, or one per replicate when the
    replicates have lengths of their own.  ext: {key: long-double array}; e64: {key: distance of the float64 oracle from it};
    recurrences: per iteration (F, B) [N, D, D] of the extended run; run: the extended OracleLDS as the last stage left it.
    Computed once per process, never modified."""
    require_extended()
    c = lds_case(name)
    D, K = c["st0"]["A_mean"].shape[1], c["Y"].shape[2]
    missing = bool(np.isnan(c["Y"]).any())
    runs, bounds, tiles = [], [], []
    for rows, T, Y, st0 in _problems(c):
        m64 = OracleLDS(Y.copy(), {k: v.copy() for k, v in st0.items()}, c["pri"])
        mx = OracleLDS(to_long(Y), to_long(st0), to_long(c["pri"]))
        ext, e64, bnd, til = {}, {}, {}, {}
        for (k64, a64), (kx, ax) in zip(lds_trace(m64, c["iters"], missing, BOUND_MODES), lds_trace(mx, c["iters"], missing, BOUND_MODES)):
            assert k64 == kx and ax.dtype == LD, (k64, kx, ax.dtype)
            if is_bound(kx):
                ax.setflags(write=False)
                bnd[kx] = (ax,) + bound_errors(a64, ax)
                continue
            ext[kx] = _cut(kx, ax, None, T)
            e64[kx] = rel(_cut(k64, a64, None, T), ext[kx])
            ext[kx].setflags(write=False)
            if name in BIG_CASES and kx[2] in TILE_QUANTITIES:
                til[kx] = tile_errors(_cut(k64, a64, None, T), ext[kx], kx[2])
                til[kx].setflags(write=False)
        runs.append((rows, T, max(D, K, T), ext, e64, mx.recurrences, mx))
        bounds.append(bnd)
        tiles.append(til)
    return runs, bounds, tiles


def compare_with_reference(name, handle_trace):
    """Measure a handle's trace against lds_reference(name): [(run, key, e64, e_gpu, ratio = e_gpu / yardstick)]."""
    rows_out = []
    runs = lds_reference(name)
    for key, arr in handle_trace:
        if is_bound(key):
            continue
        for rows, T, n, ext, e64, _, _ in runs:
            got = _cut(key, arr, rows, T)
            assert np.all(np.isfinite(got)), "%s: non-finite values in %r" % (name, key)
            e_gpu = rel(got, ext[key])
            rows_out.append((rows, key, e64[key], e_gpu, e_gpu / yardstick(e64[key], n)))
    return rows_out


def compare_bound_with_reference(name, handle_trace):
    """The bound keys of a handle's trace against lds_bound_reference(name): [(key, replicate, part index, e64, e_gpu,
    e_gpu / yardstick, error relative to the part itself)]."""
    out = []
    for key, arr in handle_trace:
        if not is_bound(key):
            continue
        for (rows, T, n, _, _, _, _), bnd in zip(lds_reference(name), lds_bound_reference(name)):
            ext, e64, _ = bnd[key]
            got = arr if rows is None else arr[rows:rows + 1]       # (a non-finite part gives a NaN ratio, which no bound admits)
            out += [(key, row[0] if rows is None else rows) + row[1:] for row in compare_bound(got, ext, e64, n)]
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# outputs with missing entries, row by row
# ----------------------------------------------------------------------------------------------------------------------------
# rel() is max-abs over the whole array: a known entry that is no longer pinned (variance 1e-13 for 0.0) disappears under the
# variance of a fully missing row, and so does the one missing entry of an otherwise observed row being off by 1e-10 of itself.
# Here every row is measured in units of its own largest missing entry, and its known entries are held to the observation
# bitwise (the oracle pins them the same way, O.update_Y: "exact pins").
def lds_trace_order(m, updates, bounds=()):
    """lds_trace with update_Y only in the iterations whose entry of `updates` is true (iterate() does not update the outputs,
    as the reference's example loop does not), and the outputs read in the others too, under the stage "outputs kept".  With
    every entry true the keys and the calls are those of lds_trace(m, len(updates), True, bounds)."""
    wishart = m.noise == "wishart"
    for it, upd in enumerate(updates):
        m.sweep("forward")
        yield (it, "forward sweep", "X"), np.array(m.read("X"))
        m.sweep("backward")
        yield (it, "backward sweep", "X"), np.array(m.read("X"))
        yield (it, "backward sweep", "Sigma"), np.array(m.read("Sigma"))
        if upd:
            m.update_Y()
        yield (it, "update_Y" if upd else "outputs kept", "Yq"), np.array(m.read("Yq"))
        yield (it, "update_Y" if upd else "outputs kept", "Yvar"), np.array(m.read("Yvar"))
        m.update_A()
        yield (it, "update_A", "A_mean"), np.array(m.read("A_mean"))
        m.update_C()
        yield (it, "update_C", "C_mean"), np.array(m.read("C_mean"))
        m.update_Q()
        m.update_R()
        names = ["A_colvar", "C_colvar"] + (["Q_v", "Q_w", "R_v", "R_w", "A_cov", "C_cov"] if wishart else ["Q_b", "R_b"])
        for nm in names:
            yield (it, "update_R", nm), np.array(m.read(nm))
        for mode in bounds:
            yield (it, "bound", mode), np.array(m.elbo_parts(mode))


def row_errors(got, ext, miss):
    """[N, T]: per row, max over its missing entries of |got - ext| in units of the row's largest missing-entry magnitude in
    ext; NaN for a row without missing entries."""
    got, ext = np.asarray(got, dtype=LD), np.asarray(ext, dtype=LD)
    out = np.full(miss.shape[:2], np.nan)
    for n, t in zip(*np.nonzero(miss.any(axis=2))):
        u = miss[n, t]
        out[n, t] = float(np.abs(got[n, t, u] - ext[n, t, u]).max() / max(np.abs(ext[n, t, u]).max(), LD(1e-300)))
    return out


def is_rows_key(key):
    return key[1] == "update_Y" and key[2] in ("Yq", "Yvar")


def row_iterations(updates):
    """the iterations after whose update_Y the rows are compared: all that have one"""
    return tuple(it for it, upd in enumerate(updates) if upd)


def lds_float64_rows(name, make=None, updates=None):
    """[(key, array)] of a fresh run of the float64 oracle through lds_trace_order, without the bounds.  make(Y, st0, pri): the
    oracle to drive -- tests/test_missing_rows_cpu.py runs OracleLDS with a defect planted in update_Y."""
    c = lds_case(name)
    m = (make or OracleLDS)(c["Y"].copy(), {k: v.copy() for k, v in c["st0"].items()}, c["pri"])
    return list(lds_trace_order(m, updates or (True,) * c["iters"]))


@functools.lru_cache(maxsize=None)
def rows_reference(name, updates=None):
    """A case with missing outputs run by both oracles through lds_trace_order: a dict with n = max(D, K, T); updates; miss
    [N, T, K]; ext {key: long-double array} and e64 {key: the float64 oracle's distance from it} as lds_reference has them; rows
    {key: [N, T] of row_errors of the float64 oracle} for the outputs after each update_Y; bound {key: (ext [N, 6], e64, own)} as
    lds_bound_reference (empty for a case compared on its outputs only).  Computed once per process, never modified."""
    require_extended()
    c = lds_case(name)
    updates = tuple(updates or (True,) * c["iters"])
    Y, T = c["Y"], c["Y"].shape[1]
    D, K = c["st0"]["A_mean"].shape[1], Y.shape[2]
    miss = np.isnan(Y)
    modes = () if c.get("outputs_only") else BOUND_MODES
    m64 = OracleLDS(Y.copy(), {k: v.copy() for k, v in c["st0"].items()}, c["pri"])
    mx = OracleLDS(to_long(Y), to_long(c["st0"]), to_long(c["pri"]))
    ext, e64, rows, bnd = {}, {}, {}, {}
    with np.errstate(all="ignore"):         # (the bound before the first update_Y is NaN in both oracles)
        for (k64, a64), (kx, ax) in zip(lds_trace_order(m64, updates, modes), lds_trace_order(mx, updates, modes)):
            assert k64 == kx and ax.dtype == LD, (k64, kx, ax.dtype)
            if is_bound(kx):
                ax.setflags(write=False)
                bnd[kx] = (ax,) + bound_errors(a64, ax)
                continue
            ext[kx] = _cut(kx, ax, None, T)
            e64[kx] = rel(_cut(k64, a64, None, T), ext[kx])
            ext[kx].setflags(write=False)
            if is_rows_key(kx):
                rows[kx] = row_errors(a64, ax, miss)
    return dict(n=max(D, K, T), updates=updates, miss=miss, ext=ext, e64=e64, rows=rows, bound=bnd)


def compare_rows(name, trace, updates=None, tag=None):
    """The outputs of a trace (a handle's, or an oracle's) after each update_Y against rows_reference(name, updates), row by row.
    Returns [(key, replicate, row, pattern, e64_row, e_row, e_row / yardstick(e64_row, n), pinned)]: the distances are
    row_errors', over the row's missing entries (0 for a row that has none); pinned: the row's known entries -- of an observed
    row all of them -- are bitwise the observation in Yq, exactly 0.0 in Yvar.  A row is in order when its ratio is at most
    FACTOR and it is pinned (offending_rows).  Prints every row it measured."""
    c = lds_case(name)
    ref = rows_reference(name, None if updates is None else tuple(updates))
    Y, miss, n = c["Y"], ref["miss"], ref["n"]
    out = []
    for key, arr in trace:
        if not is_rows_key(key) or key[0] not in row_iterations(ref["updates"]):
            continue
        e_got = row_errors(arr, ref["ext"][key], miss)
        for r in range(Y.shape[0]):
            for t in range(Y.shape[1]):
                known = ~miss[r, t]
                if key[2] == "Yq":
                    pinned = np.array_equal(np.ascontiguousarray(arr[r, t, known], dtype=np.float64).view(np.int64), Y[r, t, known].view(np.int64))
                else:
                    pinned = bool(np.all(arr[r, t, known] == 0.0))
                e64r, e = (0.0, 0.0) if known.all() else (float(ref["rows"][key][r, t]), float(e_got[r, t]))
                ratio = e / yardstick(e64r, n)
                out.append((key, r, t, c["patterns"][r][t], e64r, e, ratio, pinned))
                print("%-32s r%d it%d %-4s row %2d %-19s e64 %.2e  e_row %.2e  e_row/y %6.2f%s%s"
                      % (tag or name, r, key[0], key[2], t, c["patterns"][r][t], e64r, e, ratio, "" if pinned else "  <-- known entries not pinned",
                         "" if ratio <= FACTOR else "  <-- over"))
    if out:
        print("%-32s SUMMARY rows  max e64 %.2e  max e_row %.2e  max e_row/y %.2f" % (tag or name, max(r[4] for r in out), max(r[5] for r in out), max(r[6] for r in out)))
    return out


def offending_rows(rows):
    return [r for r in rows if not (r[6] <= FACTOR and r[7])]


def compare_with_rows_reference(name, trace, updates=None, skip_bound=()):
    """compare_with_reference and compare_bound_with_reference against rows_reference(name, updates), for the orders lds_reference
    does not run: ([(None, key, e64, e_gpu, ratio)], [(key, replicate, part index, e64, e_gpu, ratio, own)]).  skip_bound: the
    iterations whose bound is not compared."""
    ref = rows_reference(name, None if updates is None else tuple(updates))
    T = lds_case(name)["Y"].shape[1]
    out, bnd = [], []
    for key, arr in trace:
        if is_bound(key):
            if key[0] not in skip_bound:
                ext, e64, _ = ref["bound"][key]
                bnd += [(key,) + row for row in compare_bound(arr, ext, e64, ref["n"])]
            continue
        got = _cut(key, arr, None, T)
        assert np.all(np.isfinite(got)), "%s: non-finite values in %r" % (name, key)
        e_gpu = rel(got, ref["ext"][key])
        out.append((None, key, ref["e64"][key], e_gpu, e_gpu / yardstick(ref["e64"][key], ref["n"])))
    return out, bnd


# ----------------------------------------------------------------------------------------------------------------------------
# the 128-wide class, tile by tile
# ----------------------------------------------------------------------------------------------------------------------------
# rel() is a maximum over a whole array.  An off-diagonal 16 x 16 tile of Sigma, or of a column-variance block, is small beside
# the diagonal, and the kernels of the 128-wide class deal their work out by such tiles: four wavefronts own two row tiles each of
# the recurrence matrices, k_stats_big forms every pair of the eight state tiles once and stores its mirror, the column pass runs
# over blocks of 16 columns.  One tile wrong by 1e-10 of itself does not move the max-norm.  Here every tile is measured in units
# of its own largest entry of the extended run.
TILE = 16
TILE_MATRICES = ("Sigma", "A_mean", "C_mean", "A_colvar", "C_colvar", "Q_w", "R_w", "A_cov", "C_cov")
TILE_QUANTITIES = TILE_MATRICES + ("X",)


def _tile_max(a, axes):
    """max |a| over 16-wide tiles of each of `axes` (the last one or two), a ragged last tile where the extent is no multiple of
    16: the padding is zero, which changes no maximum of absolute values"""
    a = np.abs(a)
    pad = [(0, 0)] * a.ndim
    for ax in axes:
        pad[ax] = (0, -a.shape[ax] % TILE)
    a = np.pad(a, pad)
    for ax in sorted((ax % a.ndim for ax in axes), reverse=True):      # from the last axis: the earlier positions stay
        a = a.reshape(a.shape[:ax] + (a.shape[ax] // TILE, TILE) + a.shape[ax + 1:]).max(axis=ax + 1)
    return a


def tile_errors(got, ext, name="matrix"):
    """float64 [..., ceil(R / 16), ceil(C / 16)] for a matrix quantity [..., R, C] ([..., T, ceil(D / 16)] for name "X" [..., T, D]):
    per tile max |got - ext| / max |ext|, both over the tile.  A tile that is exactly zero in the extended run measures 0.0 if it
    is exactly zero in `got` too and inf if it is not."""
    got, ext = np.asarray(got, dtype=LD), np.asarray(ext, dtype=LD)
    assert got.shape == ext.shape, (name, got.shape, ext.shape)
    axes = (-1,) if name == "X" else (-2, -1)
    d, u = _tile_max(got - ext, axes), _tile_max(ext, axes)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(u == 0, np.where(d == 0, LD(0), LD(np.inf)), d / u)
    return e.astype(float)


def compare_tiles(name, trace, tag=None):
    """The tiles of a trace (a handle's, or an oracle's) against lds_reference(name) / lds_tile_reference(name), for every quantity
    of TILE_QUANTITIES after every stage that yields it.  Returns [(run, key, e64 by tile, e by tile, e / yardstick(e64, n) by
    tile)], the three arrays shaped as tile_errors gives them; a tile is in order when its ratio is at most FACTOR
    (offending_tiles) -- a tile that is zero in the extended run and not in the trace has ratio inf.  Prints one line per key."""
    out = []
    for key, arr in trace:
        if is_bound(key) or key[2] not in TILE_QUANTITIES:
            continue
        for (rows, T, n, ext, _, _, _), til in zip(lds_reference(name), lds_tile_reference(name)):
            got = _cut(key, arr, rows, T)
            assert np.all(np.isfinite(got)), "%s: non-finite values in %r" % (name, key)
            e = tile_errors(got, ext[key], key[2])
            with np.errstate(invalid="ignore"):
                ratio = np.where(e == 0, 0.0, e / np.maximum(til[key], n * U64))
            out.append((rows, key, til[key], e, ratio))
            w = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
            print("%-28s %-4s it%d %-15s %-9s TILES %6d  max e64 %.2e  max e_tile %.2e  max e_tile/y %6.2f at %r%s"
                  % (tag or name, "" if rows is None else "r%d" % rows, key[0], key[1], key[2], e.size, til[key].max(), e.max(), ratio[w],
                     tuple(int(i) for i in w), "" if ratio[w] <= FACTOR else "  <-- %d over" % int((~(ratio <= FACTOR)).sum())))
    return out


def offending_tiles(rows):
    """[(run, key, tile index, e64, e, ratio)] of the tiles of compare_tiles' result that are beyond FACTOR x yardstick"""
    return [(r, key, tuple(int(i) for i in idx), float(e64[idx]), float(e[idx]), float(ratio[idx]))
            for r, key, e64, e, ratio in rows for idx in zip(*np.nonzero(~(ratio <= FACTOR)))]


def known_offenders(which, mean, colvar, obs):
    """[(which, replicate, row, column, what)] of the known entries of A or C (obs [rows, D], NaN = not known) that are not held:
    the mean [N, rows, D] bitwise the given value, the variance (colvar [N, D, rows], column first) exactly 0.0."""
    known = ~np.isnan(obs)
    mean, colvar = np.ascontiguousarray(mean, dtype=np.float64), np.asarray(colvar, dtype=np.float64)
    bad = []
    for n in range(mean.shape[0]):
        same = mean[n].view(np.int64) == np.ascontiguousarray(obs, dtype=np.float64).view(np.int64)
        bad += [(which, n, int(i), int(j), "mean") for i, j in zip(*np.nonzero(known & ~same))]
        bad += [(which, n, int(i), int(j), "variance") for i, j in zip(*np.nonzero(known & ~(colvar[n].T == 0.0)))]
    return bad


class PinnedHandleLDS(HandleLDS):
    """HandleLDS that checks the known entries of A and C after every update_A / update_C: self.pins collects known_offenders'
    findings, self.pin_checks counts the entries looked at."""

    def __init__(self, b, pri):
        HandleLDS.__init__(self, b)
        self.obs = {w: pri.get(w + "_obs") for w in ("A", "C")}
        self.pins, self.pin_checks = [], 0

    def _check(self, w):
        """(a partly known column is conditioned at its own update, not before: each matrix is looked at after its own)"""
        obs = self.obs[w]
        if obs is not None:
            g = self.b.get_state((w + "_mean", w + "_colvar"))
            self.pins += known_offenders(w, g[w + "_mean"], g[w + "_colvar"], obs)
            self.pin_checks += int((~np.isnan(obs)).sum()) * self.b.N

    def update_A(self):
        self.b.update_A()
        self._check("A")

    def update_C(self):
        self.b.update_C()
        self._check("C")


# ----------------------------------------------------------------------------------------------------------------------------
# the warm-up rule of k_prep.hip / k_big.hip, in NumPy
# ----------------------------------------------------------------------------------------------------------------------------
LN_TOL = float(np.log(LD(1e-18)))


def induced_norm(M, which):
    """inf: max row sum; 1: max column sum"""
    return float(np.abs(M).sum(axis=-1 if which == "inf" else -2).max())


def warmup_rule(M, which):
    """J*: the smallest J = 4a + 8b + 16c + 32d (a, b, c in {0, 1}, d <= 16) whose bound n_2^a n_3^b n_4^c n_5^d on ||M^J||,
    n_k = ||M^(2^k)||, is at most 1e-18; 1 << 30 if there is none.

    This is the device's documented rule (pyvb_amd/csrc/k_prep.hip, k_big.hip) restated, not an independent optimum: J <= J* + 4
    shows that a kernel follows its own rule on the right matrices and norms, no more.  The independent evidence that a
    warm-up is long enough is power_norm(): ||M^J|| itself, taken in long double."""
    l, Pw = {}, M
    for k in range(1, 6):
        Pw = Pw @ Pw
        if k >= 2:
            nrm = induced_norm(Pw, which)
            l[k] = (np.log(nrm) if nrm > 0.0 else -1e300) if nrm < 1.0 else None
    best = 1 << 30
    for d in range(17):
        for abc in range(8):
            use = {2: abc & 1, 3: (abc >> 1) & 1, 4: abc >> 2, 5: d}
            if any(use[k] and l[k] is None for k in use):
                continue
            bound = sum(use[k] * l[k] for k in use if use[k])
            J = 4 * use[2] + 8 * use[3] + 16 * use[4] + 32 * d
            if J > 0 and bound <= LN_TOL and J < best:
                best = J
    return best


def power_norm(M, J, which):
    """||M^J|| in long double"""
    return induced_norm(np.linalg.matrix_power(M, int(J)), which)


# ----------------------------------------------------------------------------------------------------------------------------
# the arguments the bounds give digamma and gammaln (and the edges of the kernels' digamma around them)
# ----------------------------------------------------------------------------------------------------------------------------
DIGAMMA_ROOT = 1.4616321449683623


def special_grid():
    """float64 [<= 256]: 1e-8, the Gamma priors' 1e-3 and 1e-3 + k / 2 (a0 + T / 2), the Wishart arguments v - i / 2 down to 0.5,
    the root of digamma, 9.999 / 10 / 10.001 where the kernels go over to the series, half-integers up to 5e3, 7.5e4, 1e5, 1e8,
    and negative non-integers on both sides of -64, below which the kernels use the reflection formula."""
    g = [1e-8, 1e-3, 0.5, 1.0, 1.5, 2.0, DIGAMMA_ROOT, 9.999, 10.0, 10.001]
    g += [1e-3 + 0.5 * k for k in range(1, 73)]
    g += [k + 0.5 for k in range(41)] + [float(k) for k in range(3, 41)]
    g += [float(int(1.09 ** k)) + 0.5 for k in range(44, 99)] + [4999.5, 5000.0]
    g += [7.5e4, 1e5, 1e8]
    g += [-0.5, -63.5, -64.5, -1000.25]
    g = np.array(sorted(set(g)))
    assert g.size <= 256
    return g


# ----------------------------------------------------------------------------------------------------------------------------
# VB-PCA with missing data
# ----------------------------------------------------------------------------------------------------------------------------
PCA_CASES = [(300, 20, 4), (77, 33, 17), (17, 250, 31), (600, 250, 16)]
# beta_a0 + d N / 2 = 0.501 < 10 at the smallest shape a handle accepts: the recurrence branch of the host's digamma (and the
# lower bound of a graph none of whose data is observed: pca_problem always hides entry (0, 0))
PCA_SMALL = (1, 1, 1)
PCA_BOUND_CASES = PCA_CASES + [PCA_SMALL]
PCA_NAMES = ("W_mean", "W_var", "Z", "Z_cov", "X", "Mu_mean", "Mu_var", "beta_a", "beta_b")


def pca_problem(N, d, q):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec); spec.loader.exec_module(G)
    return G.pca_problem(N, d, q, seed=1000 + N + d)


class OraclePCA(object):
    def __init__(self, init, pri, N, d, q):
        self.st, self.pri, self.N = P.make_state(init, pri, N, d, q), pri, N

    def update_W(self): P.update_W(self.st, self.pri)
    def update_Z(self): P.update_Z(self.st, self.pri)
    def update_X(self, lo, hi): P.update_X(self.st, self.pri, lo, hi)
    def update_Mu(self): P.update_Mu(self.st, self.pri)
    def update_Beta(self): P.update_Beta(self.st, self.pri)
    def get_state(self): return self.st

    def elbo_parts(self, mode):
        return P.elbo_parts(self.st, self.pri) if mode == "reference" else XR.pca_elbo_parts_exact(self.st, self.pri)


def pca_handle_parts(b):
    """elbo_parts(mode) for a PCABatch, as OraclePCA has it"""
    def parts(mode):
        assert b.bound == mode, "the handle forms the %s bound, not the %s one" % (b.bound, mode)
        return b.elbo()
    return parts


def _pca_rowvar(g):
    """[N]: the variance a row's missing entries carry -- a handle's X_rowvar, the largest entry of the row in an oracle's X_var
    (0 where the row is observed, tests/test_pca_gpu.py: _compare)"""
    return g["X_rowvar"] if "X_rowvar" in g else g["X_var"].max(1)


def pca_trace(m, N, iters=2, stage_reads=True, bounds=(), parts=None, rowvar=False):
    """The stages of tests/test_pca_gpu.py: test_stagewise_vs_oracle on m (OraclePCA or a PCABatch).  stage_reads=False reads
    only at the end of each iteration: a read between update_Z and update_X(1, N) makes a handle carry the Z update out on its
    own, and the fused sweep over the rows (pyvb_amd/csrc/k_pca.hip: the "columns" / "pairs" kinds of PCABatch.set_sweep) is then never run.
    rowvar: X_rowvar [N] is yielded wherever X is, from the same read (the row-wise comparison, compare_pca_rows)."""
    for it in range(iters):
        m.update_W()
        if stage_reads:
            yield (it, "update_W", "W_mean"), np.array(m.get_state()["W_mean"])
        m.update_Z()
        if stage_reads:
            yield (it, "update_Z", "Z"), np.array(m.get_state()["Z"])
        m.update_X(0, 1)
        m.update_Mu()
        if stage_reads:
            yield (it, "update_Mu", "Mu_mean"), np.array(m.get_state()["Mu_mean"])
        m.update_X(1, N)
        if stage_reads:
            g = m.get_state()
            yield (it, "update_X", "X"), np.array(g["X"])
            if rowvar:
                yield (it, "update_X", "X_rowvar"), np.array(_pca_rowvar(g))
        m.update_Beta()
        g = m.get_state()
        for nm in PCA_NAMES:
            yield (it, "update_Beta", nm), np.array(g[nm])
        if rowvar:
            yield (it, "update_Beta", "X_rowvar"), np.array(_pca_rowvar(g))
        for mode in bounds:     # the parts [5] of the bound after the iteration (parts: pca_handle_parts(m) for a handle)
            yield (it, "bound", mode), np.array((parts or m.elbo_parts)(mode))


def pca_reference(N, d, q):
    """(n, ext, e64, extended state) as lds_reference."""
    return _pca_reference(N, d, q)[:4]


def pca_bound_reference(N, d, q):
    """{(iteration, "bound", mode): (ext [1, 5], e64 [1, 5], the same relative to each part itself)} as lds_bound_reference."""
    return _pca_reference(N, d, q)[4]


@functools.lru_cache(maxsize=None)
def _pca_reference(N, d, q):
    require_extended()
    init, pri = pca_problem(N, d, q)
    m64 = OraclePCA(init, pri, N, d, q)
    mx = OraclePCA(to_long(init), to_long(pri), N, d, q)
    ext, e64, bnd = {}, {}, {}
    for (k64, a64), (kx, ax) in zip(pca_trace(m64, N, bounds=BOUND_MODES), pca_trace(mx, N, bounds=BOUND_MODES)):
        assert k64 == kx and ax.dtype == LD, (k64, kx, ax.dtype)
        if is_bound(kx):
            ax = ax[None]
            ax.setflags(write=False)
            bnd[kx] = (ax,) + bound_errors(a64, ax)
            continue
        ext[kx] = ax
        e64[kx] = rel(a64, ax)
        ax.setflags(write=False)
    return max(d, q, N), ext, e64, mx.st, bnd


# ----------------------------------------------------------------------------------------------------------------------------
# VB-PCA, row by row
# ----------------------------------------------------------------------------------------------------------------------------
# rel() over the whole [N, d] array loses an observed entry overwritten by its prediction (which differs from the data by the
# noise) and the one missing entry of an otherwise observed row being off by 1e-10 of itself.  Here every row is a named
# pattern, its missing entries are measured in units of the row's largest one, its z in units of the row's largest latent, its
# variance relative to itself, and its observed entries are held bitwise to the data (P.update_X pins them the same way).
#
# What the patterns are aimed at (pyvb_amd/csrc/k_pca.hip): the mask is read one 32-bit word per lane, four entries at a
# time; a wavefront owns 32-column blocks of two 16-column tiles; a pair of k_pca_pairs splits the row at column 128.
# Row n takes pattern n mod 16; index 0 is a partly observed one because row 0 is the row the crawl order updates alone,
# before Mu (its other variants are an argument of pca_rows_problem).
PCA_ROW_PATTERNS = ("Bernoulli", "all", "one known, first", "one known, last", "one missing, first", "one missing, last",
                    "a byte of a word", "a word", "a tile", "a block", "alternating", "upper half", "low half", "the seam",
                    "the last tile", "observed")


def pca_pattern_mask(name, d, rng=None):
    """[d] bool, true = missing, of a named pattern at width d; None where the pattern is empty or degenerate there: nothing
    missing (but for "observed"), everything missing (but for "all"), or a seam without both its columns.  A pattern that
    reaches beyond d is cut off at d.  rng: for "Bernoulli" (0.3, redrawn in one entry so that the row is partly observed)."""
    k = np.arange(d)
    if name == "Bernoulli":
        if d < 2:
            return None
        m = (rng if rng is not None else np.random.default_rng(d)).random(d) < 0.3
        if not m.any():
            m[d // 2] = True
        if m.all():
            m[d // 2] = False
        return m
    m = {"all": lambda: k >= 0, "one known, first": lambda: k != 0, "one known, last": lambda: k != d - 1,
         "one missing, first": lambda: k == 0, "one missing, last": lambda: k == d - 1,
         "a byte of a word": lambda: k == 5, "a word": lambda: (k >= 4) & (k < 8), "a tile": lambda: (k >= 16) & (k < 32),
         "a block": lambda: (k >= 32) & (k < 64), "alternating": lambda: k % 2 == 0, "upper half": lambda: k >= d // 2,
         "low half": lambda: k < 128, "the seam": lambda: (k == 127) | (k == 128),
         "the last tile": lambda: k >= 16 * ((d - 1) // 16), "observed": lambda: k < 0}[name]()
    if (name != "all" and m.all()) or (name != "observed" and not m.any()) or (name == "the seam" and m.sum() != 2):
        return None
    return m


def _pca_row_patterns(N, d, rng):
    """(miss [N, d], the label of every row).  A pattern that is degenerate at d is replaced by the nearest one in
    PCA_ROW_PATTERNS that is not (the lower index first), and the label says so: "all (for a block)"."""
    L = len(PCA_ROW_PATTERNS)
    miss, names = np.zeros((N, d), dtype=bool), []
    for n in range(N):
        p = n % L
        for off in range(L):
            m, name = None, None
            for cand in (p - off, p + off):
                if 0 <= cand < L and m is None:
                    name = PCA_ROW_PATTERNS[cand]
                    m = pca_pattern_mask(name, d, rng)
            if m is not None:
                break
        miss[n] = m
        names.append(name if off == 0 else "%s (for %s)" % (name, PCA_ROW_PATTERNS[p]))
    return miss, names


def pca_has_column_patterns(N, d):
    """where N and d allow, two column patterns lie over the rows: column d // 3 is missing in every row, and column 2 is
    observed by row 8 only"""
    return N > 8 and d >= 3 and d // 3 != 2


def pca_rows_problem(N, d, q, row0="partial", unpinned=False):
    """(init, pri, labels): pca_problem(N, d, q) -- its data, its initial W, Z, Z_cov, Mu, beta_b, its priors -- with the mask
    replaced by the named row patterns and the two column patterns (pca_has_column_patterns).  The data are the complete
    matrix pca_problem draws before it hides entries; the initial means of the missing entries are standard normal, as there.
    row0: "partial" (its pattern, the default), "missing" or "observed" -- the X_0 step with something, everything or nothing
    to impute; an observed row 0 is exempt from the column patterns (it then is the one row that observes column d // 3).
    unpinned: init["X_full"] [N, d] standard normal and init["X_var0"] [N] positive -- rows that are not fully observed carry
    that mean at ALL entries until their first update (P.make_state, PCABatch.from_problem read both)."""
    assert row0 in ("partial", "missing", "observed")
    init, pri = pca_problem(N, d, q)
    # the complete data: the first draws of make_golden.pca_problem, replayed (held to its observed entries below)
    g = np.random.default_rng(1000 + N + d)
    W = g.standard_normal((d, q)); Z = g.standard_normal((N, q)); mean = g.standard_normal(d)
    X = Z @ W.T + mean + g.standard_normal((N, d)) * np.sqrt(1.0 / 20.0)
    assert np.array_equal(X[init["obs"]], init["X"][init["obs"]])
    rng = np.random.default_rng(7000 + 3 * N + d)
    miss, names = _pca_row_patterns(N, d, rng)
    if row0 == "missing":
        miss[0], names[0] = True, "all (row 0)"
    elif row0 == "observed":
        miss[0], names[0] = False, "observed (row 0)"
    if pca_has_column_patterns(N, d):
        keep = miss[0].copy()
        miss[:, d // 3] = True
        miss[:, 2] = True
        miss[8, 2] = False
        if row0 == "observed":
            miss[0] = keep
    init["obs"] = ~miss
    init["X"] = np.where(miss, rng.standard_normal((N, d)), X)
    if unpinned:
        init["X_full"] = rng.standard_normal((N, d))
        init["X_var0"] = 1.0 / rng.uniform(0.2, 1.0, N)
    return init, pri, names


def _rows_case(N, d, q, sweeps, **kw):
    c = dict(N=N, d=d, q=q, sweeps=tuple(sweeps), row0="partial", unpinned=False, iters=2, schedules=(True, False), bounds=True)
    c.update(kw)
    return c


_LONG = dict(iters=1, schedules=(False,))       # one iteration, read at its end only
# name -> the case; N of the long ones is a function of the device's CU count (256 on MI355X, and in the CPU tests).
# sweeps: the kinds of PCABatch.set_sweep the case runs under; schedules: stage_reads of pca_trace (True: a read after every
# stage, so pass 1 and pass 2 run apart; False: a read at the end of the iteration, which lets the fused sweeps run lazily and
# makes the read go through k_pca_materialize).  What each reaches in k_pca.hip:
PCA_ROW_CASES = {
    # pairs<true> without padding; the seam with both halves full; a ragged last tile (6 rows) in a chunk of its own
    "n70_d256_q16":     _rows_case(70, 256, 16, ("store", "columns", "pairs")),
    # pairs<true> with 15 padded columns in tile 15; 5 rows in the last tile
    "n37_d241_q16":     _rows_case(37, 241, 16, ("columns", "pairs")),
    # pairs<false>, DT = 15: the j < DT test inside half 1's last block; padded latent indices
    "n70_d240_q7":      _rows_case(70, 240, 7, ("columns", "pairs")),
    # DT = 9: half 1 owns one real column; pass12 with five wavefronts, the last with one tile
    "n40_d129_q16":     _rows_case(40, 129, 16, ("store", "columns", "pairs")),
    # DT = 8: half 1 owns nothing and still exchanges its partial
    "n33_d128_q5":      _rows_case(33, 128, 5, ("columns", "pairs")),
    "n20_d17_q1":       _rows_case(20, 17, 1, ("store", "columns", "pairs")),       # DT = 2, q = 1
    "n16_d64_q16":      _rows_case(16, 64, 16, ("store", "columns")),               # exactly one full tile
    "n15_d1_q1":        _rows_case(15, 1, 1, ("store", "columns")),                 # d = 1: the patterns degenerate to all / observed
    # QT = 2 (no lazy sweep): the two sides of the DT >= 13 chunk rule; pass1<2>, pass2<2, false>, pass12<2, false>
    "n35_d208_q17":     _rows_case(35, 208, 17, ("store",)),
    "n37_d209_q32":     _rows_case(37, 209, 32, ("store",)),
    # (d = 208 and 209 are DT = 13 and 14, both on the upper side of the rule; DT = 12 is d = 192.  At these N the tile count
    # caps the chunks on either side, so the rule shows in the partition only; tests/test_pca_rows_cpu.py holds that)
    "n35_d192_q17":     _rows_case(35, 192, 17, ("store",)),
    # rows that wait for their first update: pass2<1, true>, pass12<1, true>, pass2<2, true>, pass12<2, true>
    "n40_d129_q16_unpinned": _rows_case(40, 129, 16, ("store",), unpinned=True),
    "n35_d208_q17_unpinned": _rows_case(35, 208, 17, ("store",), unpinned=True),
    # the X_0 step and keep_z0 with nothing, or everything, to impute
    "n70_d256_q16_row0_missing":  _rows_case(70, 256, 16, ("columns", "pairs"), row0="missing"),
    "n70_d256_q16_row0_observed": _rows_case(70, 256, 16, ("columns", "pairs"), row0="observed"),
    # several tiles a chunk: a pair of k_pca_pairs goes on to a second tile (the ring of register sets and the flag counters
    # across tiles), k_pca_pass12 takes three steps of two tiles; a ragged last chunk
    "long_d256_q16":    _rows_case(lambda ncu: 80 * ncu + 24, 256, 16, ("columns", "pairs"), **_LONG),
    # pairs<false>: pair 0 does three tiles, so the three-ahead ring wraps entirely inside it
    "long_d32_q16":     _rows_case(lambda ncu: 144 * ncu + 8, 32, 16, ("pairs",), **_LONG),
    # (81 and 145 rows a CU round up to six and ten tiles a chunk.)  24 rows below 80 a CU it is FIVE: k_pca_pass12 ends on a step
    # with one tile of its two, pair 0 of k_pca_pairs has a second tile and its three neighbours have none.  Rows and quantities
    # only: the bound of this size is the case above's, and half the time of a long reference goes into its four evaluations.
    "long_d256_q16_five_tiles": _rows_case(lambda ncu: 80 * ncu - 24, 256, 16, ("columns", "pairs"), bounds=False, **_LONG),
}
PCA_ROW_QUANTITIES = ("X", "Z", "X_rowvar")


@functools.lru_cache(maxsize=None)
def pca_rows_case(name, ncu=256):
    """The case with its problem: N resolved, init, pri, patterns (the label of every row), miss [N, d], has (rows with a
    missing entry).  Computed once per process; the arrays are read-only."""
    c = dict(PCA_ROW_CASES[name])
    c["name"] = name
    if callable(c["N"]):
        c["N"] = int(c["N"](ncu))
    c["init"], c["pri"], c["patterns"] = pca_rows_problem(c["N"], c["d"], c["q"], row0=c["row0"], unpinned=c["unpinned"])
    c["miss"] = ~c["init"]["obs"]
    c["has"] = c["miss"].any(axis=1)
    c["n"] = max(c["d"], c["q"], c["N"])
    for v in list(c["init"].values()) + list(c["pri"].values()) + [c["miss"], c["has"]]:
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def is_pca_rows_key(key):
    return key[2] in PCA_ROW_QUANTITIES


def pca_row_errors(name, got, ext, miss):
    """[N] of a row quantity against the extended run's, each row in its own unit.  X: max over the row's missing entries of
    |got - ext| over the largest missing-entry magnitude of ext (row_errors, for all rows at once); NaN for a row without
    missing entries.  Z: max |z - z_ext| over max |z_ext| of the row.  X_rowvar: |v - v_ext| / |v_ext|, NaN for a row without
    missing entries."""
    got, ext = np.asarray(got, dtype=LD), np.asarray(ext, dtype=LD)
    tiny = LD(1e-300)
    if name == "X":
        e = np.where(miss, np.abs(got - ext), LD(0)).max(axis=1) / np.maximum(np.where(miss, np.abs(ext), LD(0)).max(axis=1), tiny)
        return np.where(miss.any(axis=1), e, np.nan).astype(float)
    if name == "Z":
        return (np.abs(got - ext).max(axis=1) / np.maximum(np.abs(ext).max(axis=1), tiny)).astype(float)
    assert name == "X_rowvar"
    return np.where(miss.any(axis=1), np.abs(got - ext) / np.maximum(np.abs(ext), tiny), np.nan).astype(float)


def _pca_oracle(c, long, make=None):
    init = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c["init"].items()}
    pri = dict(c["pri"])
    return (make or OraclePCA)(to_long(init) if long else init, to_long(pri) if long else pri, c["N"], c["d"], c["q"])


def pca_float64_rows(name, make=None, ncu=256):
    """[(key, array)] of a fresh run of the float64 oracle through the case's trace, read after every stage where the case has
    that schedule, without the bounds.  make(init, pri, N, d, q): the oracle to drive -- tests/test_pca_rows_cpu.py runs OraclePCA
    with a defect planted in update_X."""
    c = pca_rows_case(name, ncu)
    return list(pca_trace(_pca_oracle(c, False, make), c["N"], iters=c["iters"], stage_reads=True in c["schedules"], rowvar=True))


@functools.lru_cache(maxsize=None)
def pca_rows_reference(name, ncu=256):
    """A case of PCA_ROW_CASES run by both oracles: a dict with n = max(d, q, N); ext {key: long-double array} and e64 {key: the
    float64 oracle's distance from it} as pca_reference has them (X_rowvar among the quantities); rows {key: [N] of pca_row_errors
    of the float64 oracle} for X, Z and X_rowvar wherever the trace reads them; bound {key: (ext [1, 5], e64, own)} as
    pca_bound_reference, both modes (empty for a case without bounds).  The oracles are read after every stage where the case has that schedule: a read changes
    nothing in an oracle, so the keys of the end-of-iteration schedule are among these with the same values.  Computed once
    per process, never modified."""
    require_extended()
    c = pca_rows_case(name, ncu)
    kw = dict(iters=c["iters"], stage_reads=True in c["schedules"], bounds=BOUND_MODES if c["bounds"] else (), rowvar=True)
    m64, mx = _pca_oracle(c, False), _pca_oracle(c, True)
    ext, e64, rows, bnd = {}, {}, {}, {}
    for (k64, a64), (kx, ax) in zip(pca_trace(m64, c["N"], **kw), pca_trace(mx, c["N"], **kw)):
        assert k64 == kx and ax.dtype == LD, (k64, kx, ax.dtype)
        if is_bound(kx):
            ax = ax[None]
            ax.setflags(write=False)
            bnd[kx] = (ax,) + bound_errors(a64, ax)
            continue
        ext[kx] = ax
        if kx[2] == "X_rowvar":         # (zero on the observed rows: measured where a row has a missing entry)
            e64[kx] = rel(a64[c["has"]], ax[c["has"]]) if c["has"].any() else 0.0
        else:
            e64[kx] = rel(a64, ax)
        ax.setflags(write=False)
        if is_pca_rows_key(kx):
            rows[kx] = pca_row_errors(kx[2], a64, ax, c["miss"])
    return dict(n=c["n"], ext=ext, e64=e64, rows=rows, bound=bnd)


def compare_pca_rows(name, trace, tag=None, ncu=256):
    """X, Z and X_rowvar of a trace (a handle's, or an oracle's; pca_trace with rowvar=True) against pca_rows_reference(name), row
    by row wherever the trace reads them.  Returns [(key, 0, row, pattern, e64_row, e_row, e_row / yardstick(e64_row, n), pinned)],
    the layout of compare_rows, so that offending_rows() picks the rows that are out of order: the distances are
    pca_row_errors' (0 for X and X_rowvar of a row without missing entries); pinned: the observed entries of the row of X -- all
    of a fully observed row -- are bitwise the data (true for Z and X_rowvar, which have no pin).  Every X the trace reads
    comes after an update of all rows, so rows that start unpinned have been conditioned by then.
    Prints every row that is out of order and one line that names the worst row: every row of every read would be some
    600 000 lines for the whole of tests/test_pca_rows_gpu.py."""
    c = pca_rows_case(name, ncu)
    ref = pca_rows_reference(name, ncu)
    tag = tag or name
    miss, n, pats, data = c["miss"], c["n"], c["patterns"], c["init"]["X"]
    out = []
    for key, arr in trace:
        if is_bound(key) or not is_pca_rows_key(key):
            continue
        assert np.all(np.isfinite(arr)), "%s: non-finite values in %r" % (tag, key)
        e64r = np.nan_to_num(ref["rows"][key], nan=0.0)
        e = np.where(np.isnan(ref["rows"][key]), 0.0, pca_row_errors(key[2], arr, ref["ext"][key], miss))
        ratio = e / np.maximum(e64r, n * U64)
        if key[2] == "X":
            same = np.ascontiguousarray(arr, dtype=np.float64).view(np.int64) == np.ascontiguousarray(data).view(np.int64)
            pinned = (same | miss).all(axis=1)
        else:
            pinned = np.ones(c["N"], dtype=bool)
        out += [(key, 0, r, pats[r], float(e64r[r]), float(e[r]), float(ratio[r]), bool(pinned[r])) for r in range(c["N"])]
    bad = offending_rows(out)
    for r in bad:
        print("%-44s it%d %-11s %-8s row %5d %-30s e64 %.2e  e_row %.2e  e_row/y %6.2f%s%s"
              % (tag, r[0][0], r[0][1], r[0][2], r[2], r[3], r[4], r[5], r[6], "" if r[7] else "  <-- observed entries not pinned", "" if r[6] <= FACTOR else "  <-- over"))
    if out:
        w = max(out, key=lambda r: r[6] if r[6] == r[6] else np.inf)
        print("%-44s ROWS N %d, %d reads  max e64 %.2e  max e_row %.2e  max e_row/y %.2f (it%d %s %s row %d, %s)  pins lost %d"
              % (tag, c["N"], len(out) // c["N"], max(r[4] for r in out), max(r[5] for r in out), w[6], w[0][0], w[0][1], w[0][2], w[2], w[3], sum(not r[7] for r in out)))
    return out


def compare_pca_with_rows_reference(name, trace, ncu=256):
    """The whole-array quantities and the parts of the bound of a trace against pca_rows_reference(name):
    ([(None, key, e64, e_gpu, ratio)], [(key, 0, part index, e64, e_gpu, ratio, own)]) as compare_with_rows_reference."""
    c = pca_rows_case(name, ncu)
    ref = pca_rows_reference(name, ncu)
    out, bnd = [], []
    for key, arr in trace:
        if is_bound(key):
            ext, e64, _ = ref["bound"][key]
            bnd += [(key,) + row for row in compare_bound(arr, ext, e64, ref["n"])]
            continue
        assert np.all(np.isfinite(arr)), "%s: non-finite values in %r" % (name, key)
        if key[2] == "X_rowvar":
            arr, ext = arr[c["has"]], ref["ext"][key][c["has"]]
            e_gpu = rel(arr, ext) if arr.size else 0.0
        else:
            e_gpu = rel(arr, ref["ext"][key])
        out.append((None, key, ref["e64"][key], e_gpu, e_gpu / yardstick(ref["e64"][key], ref["n"])))
    return out, bnd


# ----------------------------------------------------------------------------------------------------------------------------
# known inputs and regressors, channel by channel
# ----------------------------------------------------------------------------------------------------------------------------
# rel() is a maximum over [N, ...] with the replicates stacked.  A chain of 2 nodes beside one of 77, the column of B under an
# input a thousand times its neighbour's (the column is a thousandth of the neighbour's), the two nodes of X that the boundary
# terms -<A>^T<Q> e_1 and <Q> e_{T-1} are added to: each is a small part of such an array, and off by 1e-10 of itself it does not
# move the max-norm.  Here the units are
#   chain     every quantity of a trace and every part of both bounds, replicate by replicate (a part in units of its replicate's
#             s_r, as bound_errors has it);
#   channel   column p of B_mean / E_mean and row p of B_colvar / E_colvar of each replicate;
#   node      X at nodes 0, 1, T_n - 2 and T_n - 1 of each replicate, each on its own, the rest of the chain together, and the
#             padding rows t >= T_n, which are zero in the reference
# each in units of its own largest entry of the extended run, e_unit <= FACTOR max(e64_unit, n 2^-52) with n = max(T_n, D, K) of
# the chain's own length and e64_unit <= CAP (on the cases of regressors_ref.KAPPA_CASES the yardstick also admits one rounding of
# the cancelling sum behind R_b, measured on the reference side and capped at CAP: the kappa-clause of DESIGN.md section 17); a unit that is exactly zero in the extended run (the mean column of a dead channel
# with prior mean 0) is exactly zero or it is out of order.  inputs_ref.CHANNEL_CASES and regressors_ref.CHANNEL_CASES are the
# cases; R below is either module.
CHANNEL_QUANTITIES = ("B_mean", "B_colvar", "E_mean", "E_colvar")
CHANNEL_KINDS = ("chain", "channel", "node")


def _unit_error(got, ext):
    d, u = np.abs(got - ext).max(), np.abs(ext).max()
    if u == 0:
        return 0.0 if d == 0 else np.inf
    return float(d / u)


def end_nodes(Tn):
    """the nodes of a chain of Tn that are units of their own: 0, 1, T_n - 2, T_n - 1"""
    return sorted({0, 1, Tn - 2, Tn - 1})


def channel_errors(got, ext, key, lengths):
    """{(kind, replicate, index): max |got - ext| / max |ext| over the unit} for the array of a trace key against the extended
    run's, both in the handle's layout [N, ...].  index: "" for a chain unit (a part's name for a bound key), the channel for a
    channel unit, the node, "rest" or "padding" for a node unit.  A unit that is exactly zero in ext measures 0.0 if it is exactly
    zero in got too and inf if it is not."""
    got, ext = np.asarray(got, dtype=LD), np.asarray(ext, dtype=LD)
    assert got.shape == ext.shape, (key, got.shape, ext.shape)
    out = {}
    if is_bound(key):
        e = bound_errors(got, ext)[0]
        return {("chain", r, LDS_PARTS[p]): float(e[r, p]) for r in range(e.shape[0]) for p in range(e.shape[1])}
    q = key[2]
    for r, Tn in enumerate(int(t) for t in lengths):
        g, x = got[r], ext[r]
        if q == "X":
            T = x.shape[0]
            for t in end_nodes(Tn):
                out["node", r, t] = _unit_error(g[t], x[t])
            if Tn > 4:
                out["node", r, "rest"] = _unit_error(g[2:Tn - 2], x[2:Tn - 2])
            if Tn < T:
                out["node", r, "padding"] = _unit_error(g[Tn:], x[Tn:])
            g, x = g[:Tn], x[:Tn]
        elif q == "Sigma" and Tn <= 2:
            g, x = g[[0, 2]], x[[0, 2]]
        elif q in CHANNEL_QUANTITIES:
            for p in range(x.shape[1] if q.endswith("_mean") else x.shape[0]):
                out["channel", r, p] = _unit_error(g[:, p], x[:, p]) if q.endswith("_mean") else _unit_error(g[p], x[p])
        out["chain", r, ""] = _unit_error(g, x)
    return out


def _channel_record(R, prob, f64, ext):
    """prob: (Y, U, st0, pri, lengths, ...) of inputs_ref or (Y, U, V, st0, pri, lengths, ...) of regressors_ref"""
    Y = prob[0]
    i = [isinstance(v, dict) for v in prob].index(True)
    st0, ln = prob[i], prob[i + 2]
    lengths = np.full(Y.shape[0], Y.shape[1], dtype=np.int32) if ln is None else np.asarray(ln, dtype=np.int32)
    assert [k for k, _ in ext] == [k for k, _ in f64][:len(ext)] and all(a.dtype == LD for _, a in ext)
    for _, a in f64 + ext:
        a.setflags(write=False)
    return dict(lengths=lengths, D=st0["A_mean"].shape[1], K=Y.shape[2], keys=[k for k, _ in f64], f64=[a for _, a in f64],
                ext=[a for _, a in ext], e64=[channel_errors(a, x, k, lengths) for (k, a), (_, x) in zip(f64, ext)])


def channel_reference_of(R, prob, iters, ext_iters=None):
    """The two runs of R.channel_run (R: inputs_ref or regressors_ref) on a problem as R.channel_problem gives it: a dict with
    lengths [N], D, K, keys, ext [the extended run's arrays, in the order of keys], e64 [channel_errors of the float64 comparator],
    f64 [its arrays; iters iterations, the extended run ext_iters of them]."""
    require_extended()
    return _channel_record(R, prob, R.channel_run(prob, False, iters), R.channel_run(prob, True, iters if ext_iters is None else ext_iters))


@functools.lru_cache(maxsize=None)
def channel_reference(R, name):
    """channel_reference_of for a case of R.CHANNEL_CASES, from R.channel_trace's cached runs.  Computed once per process, never
    modified."""
    require_extended()
    ref = _channel_record(R, R.channel_problem(name), R.channel_trace(name), R.channel_trace(name, extended=True))
    if name in getattr(R, "KAPPA_CASES", ()):       # the kappa-clause: what one rounding of a cancelling sum does to every unit
        runs = R.kappa_allowance(name)
        assert all([k for k, _ in run] == ref["keys"][:len(ref["ext"])] for run in runs)
        cond = []
        for i, (key, x) in enumerate(zip(ref["keys"], ref["ext"])):
            es = [channel_errors(run[i][1], x, key, ref["lengths"]) for run in runs]
            cond.append({u: min(max(e[u] for e in es), CAP) for u in es[0]})
        ref["cond"] = cond
    return ref


def compare_channels(ref, trace, tag):
    """The units of a trace (a handle's, or a comparator's: [(key, array)] as run_stages gives it) against a reference of
    channel_reference / channel_reference_of, for every key of the trace that the extended run has.  Returns [(key, kind, replicate, index,
    e64_unit, e_unit, e_unit / yardstick(e64_unit, n))], n = max(T_n, D, K) of the replicate's own chain; a unit is in order when
    its ratio is at most FACTOR (offending_units) -- a unit that is zero in the extended run and not in the trace has ratio inf.
    Prints every unit that is out of order and the worst unit of each quantity and kind."""
    out = []
    index = {k: i for i, k in enumerate(ref["keys"])}
    assert trace and all(k in index for k, _ in trace), "the trace's keys are not the reference's"
    for key, arr in trace:
        if index[key] >= len(ref["ext"]):
            continue
        ext, e64 = ref["ext"][index[key]], ref["e64"][index[key]]
        cond = ref["cond"][index[key]] if "cond" in ref else {}
        assert np.all(np.isfinite(arr)), "%s: non-finite values in %r" % (tag, key)
        for (kind, r, idx), e in channel_errors(arr, ext, key, ref["lengths"]).items():
            n = max(int(ref["lengths"][r]), ref["D"], ref["K"])
            y = max(yardstick(e64[kind, r, idx], n), cond.get((kind, r, idx), 0.0))
            out.append((key, kind, r, idx, e64[kind, r, idx], e, 0.0 if e == 0 else e / y))
    line = "%-34s it%d %-8s %-9s %-7s r%d %-9s e64 %.2e  e_unit %.2e  e_unit/y %6.2f%s"
    for row in offending_units(out):
        print(line % ((tag, row[0][0]) + row[0][1:] + row[1:] + ("  <-- over",)))
    worst = {}
    for row in out:
        k = (row[0][2] if not is_bound(row[0]) else "bound " + row[0][2], row[1])
        if k not in worst or not row[6] <= worst[k][6]:
            worst[k] = row
    for k in sorted(worst):
        row = worst[k]
        print(line % ((tag + " WORST", row[0][0]) + row[0][1:] + row[1:] + ("",)))
    for kind in CHANNEL_KINDS:
        for what, sel in (("", lambda row: not is_bound(row[0])), (" of the bound", lambda row: is_bound(row[0]))):
            rows = [row for row in out if row[1] == kind and sel(row)]
            if rows:
                print("%-34s SUMMARY by %-7s%-13s units %5d  max e64 %.2e  max e_unit %.2e  max e_unit/y %.2f"
                      % (tag, kind, what, len(rows), max(r[4] for r in rows), max(r[5] for r in rows), max(r[6] for r in rows)))
    return out


def offending_units(rows):
    return [row for row in rows if not row[6] <= FACTOR]
