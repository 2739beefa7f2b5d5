"""GPU parity: the HIP path (through the C ABI) against the golden fixtures produced by the
reference and against the oracle on seeded inputs.  Run with `-m gpu` on an MI355X.

Tolerances (north_star): posterior means/covariances 1e-8 relative (max-norm), lower bound 1e-8
relative.  q_ln_det is compared through s = 0.5/q_ln_det (see tests/test_oracle_golden.py).
"""
import numpy as np
import pytest

from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-8


def _rel(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _close(a, b, what, rtol=RTOL):
    assert np.all(np.isfinite(a)), what + ": non-finite values"
    err = _rel(a, b)
    assert err <= rtol, "%s: rel err %.3e" % (what, err)


def _close_qld(a, b, what):
    sa, sb = 0.5 / np.asarray(a, dtype=float), 0.5 / np.asarray(b, dtype=float)
    ok = np.isfinite(sb)            # never-updated (fully observed) columns have no q_ln_det
    assert np.all(np.abs(sa - sb)[ok] <= 1e-9 * np.maximum(1.0, np.abs(sb[ok]))), what


def _batch(Y, st0, pri):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri)


def _compare_params(b, st, tag):
    g = b.get_state()
    _close(g["A_mean"], st["A_mean"], tag + "A_mean")
    _close(g["C_mean"], st["C_mean"], tag + "C_mean")
    _close(g["A_colvar"], np.einsum("nikk->nik", st["A_cov"]), tag + "A_colvar")
    _close(g["C_colvar"], np.einsum("nikk->nik", st["C_cov"]), tag + "C_colvar")
    if b.noise == "wishart":
        w = b.get_wishart_state()
        for nm, key in (("Q_v", "Q_a"), ("Q_w", "Q_b"), ("R_v", "R_a"), ("R_w", "R_b")):
            _close(w[nm], st[key], tag + nm)
        Ac, Cc = b.get_column_cov()
        _close(Ac, st["A_cov"], tag + "A_cov (dense)")
        _close(Cc, st["C_cov"], tag + "C_cov (dense)")
    else:
        for nm in ("Q_a", "Q_b", "R_a", "R_b"):
            ref = st[nm] if st[nm].ndim == 2 else np.repeat(st[nm][:, None], g[nm].shape[1], axis=1)
            _close(g[nm], ref, tag + nm)
    qa, qc = b.get_column_qld()
    _close_qld(qa, st["qld_A"], tag + "qld_A")
    _close_qld(qc, st["qld_C"], tag + "qld_C")


def _stagewise(Y, st0, pri, iters):
    """Run the example's loop on the GPU and in the oracle, comparing after every stage."""
    N, T, K = Y.shape
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T, Y)
    missing = bool(np.isnan(Y).any())
    for it in range(iters):
        tag = "it%d " % it
        post = O.state_posteriors(st, pri)
        O.sweep(st, pri, Y, "forward", post)
        b.sweep("forward")
        _close(b.get_state(("X",))["X"], st["X"], tag + "X after forward sweep")
        O.sweep(st, pri, Y, "backward", post)
        b.sweep("backward")
        _close(b.get_state(("X",))["X"], st["X"], tag + "X after backward sweep")
        Sig, qld = b.get_posterior_classes()
        cls = [0, 1, 2] if T > 2 else [0, 2]
        _close(Sig[:, cls], st["Sigma"][:, cls], tag + "Sigma")
        _close_qld(qld[:, cls], st["qld_x"][:, cls], tag + "qld_x")
        if missing:
            O.update_Y(st, pri); b.update_Y()
            q, v = b.get_outputs()
            _close(q, st["Yq"], tag + "Yq after update_Y")
            _close(v, st["Yvar"], tag + "Yvar after update_Y")
        S = O.statistics(st, Y)
        O.update_A(st, pri, S); b.update_A()
        _close(b.get_state(("A_mean",))["A_mean"], st["A_mean"], tag + "A_mean after update_A")
        O.update_C(st, pri, S); b.update_C()
        _close(b.get_state(("C_mean",))["C_mean"], st["C_mean"], tag + "C_mean after update_C")
        O.update_Q(st, pri, S, T); b.update_Q()
        O.update_R(st, pri, S, T); b.update_R()
        _compare_params(b, st, tag)
        parts = O.elbo_parts(st, pri, S, T)
        got = b.elbo()
        scale = np.abs(parts).sum(axis=1, keepdims=True)
        assert np.all(np.abs(got - parts) <= RTOL * scale), tag + "elbo parts\n%r\n%r" % (got, parts)
        _close(got.sum(1), parts.sum(1), tag + "elbo total")
    b.close()
    return st


def test_golden_fixtures(golden):
    """The reference's own outputs (tests/golden/*.npz), reproduced by the HIP path."""
    meta, Y, st0, pri, z = golden
    T = meta["T"]
    missing = bool(np.isnan(Y).any())
    b = _batch(Y, st0, pri)
    b.sweep("forward")
    _close(b.get_state(("X",))["X"][0], z["it1_fwd_X"], "forward sweep vs reference")
    b.sweep("backward")
    for it in range(1, max(meta["iters"]) + 1):
        if it > 1:
            b.sweep("forward"); b.sweep("backward")
        if missing:
            b.update_Y()
        b.update_A(); b.update_C(); b.update_Q(); b.update_R()
        if it in meta["iters"]:
            tag = "it%d_" % it
            g = b.get_state()
            _close(g["X"][0], z[tag + "X"], tag + "X")
            Sig, qld = b.get_posterior_classes()
            cls = [0, 1, 2] if T > 2 else [0, 2]
            _close(Sig[0][cls], z[tag + "Sigma"][cls], tag + "Sigma")
            _close_qld(qld[0][cls], z[tag + "qld_x"][cls], tag + "qld_x")
            _close(g["A_mean"][0], z[tag + "A_mean"], tag + "A_mean")
            _close(g["C_mean"][0], z[tag + "C_mean"], tag + "C_mean")
            for nm in ("A", "C"):
                ref = z[tag + nm + "_colvar"] if tag + nm + "_colvar" in z else np.einsum("ikk->ik", z[tag + nm + "_cov"])
                _close(g[nm + "_colvar"][0], ref, tag + nm + "_colvar")
            if meta["noise"] == "wishart":      # qv, qw after the first update (the valid parity target); the
                w = b.get_wishart_state()       # reference has no lower bound with Wishart parents (Q8)
                for nm, key in (("Q_v", "Q_a"), ("Q_w", "Q_b"), ("R_v", "R_a"), ("R_w", "R_b")):
                    _close(w[nm][0], z[tag + key], tag + nm)
                Ac, Cc = b.get_column_cov()
                _close(Ac[0], z[tag + "A_cov"], tag + "A_cov (dense)")
                _close(Cc[0], z[tag + "C_cov"], tag + "C_cov (dense)")
                if missing:
                    q, v = b.get_outputs()
                    _close(q[0], z[tag + "Yq"], tag + "Yq")
                    _close(v[0], z[tag + "Yvar"], tag + "Yvar")
                # The lower bound with Wishart parents is PARITY UNPINNED against the reference (it raises there):
                # what pins the device's six class sums -- known entries of A / C, outputs with NaN and the ln det of their
                # missing blocks included -- is the oracle's derivation (oracle/lds_closed_form.py), run here on the fixture's
                # inputs through the same first iteration
                st = O.expand_state(st0, pri, T, Y)
                post = O.state_posteriors(st, pri)
                O.sweep(st, pri, Y, "forward", post); O.sweep(st, pri, Y, "backward", post)
                if missing:
                    O.update_Y(st, pri)
                S = O.statistics(st, Y)
                O.update_A(st, pri, S); O.update_C(st, pri, S); O.update_Q(st, pri, S, T); O.update_R(st, pri, S, T)
                want = O.elbo_parts(st, pri, S, T)[0]
                got = b.elbo()[0]
                assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= RTOL * np.abs(want).sum()), (got, want)
                continue
            for nm in ("Q_a", "Q_b", "R_a", "R_b"):
                _close(g[nm][0], np.broadcast_to(z[tag + nm], g[nm][0].shape), tag + nm)
            if missing:
                q, v = b.get_outputs()
                _close(q[0], z[tag + "Yq"], tag + "Yq")
                _close(v[0], z[tag + "Yvar"], tag + "Yvar")
            parts = b.elbo()[0]
            ref = z[tag + "elbo_parts"]
            assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), "%s elbo parts %r vs %r" % (tag, parts, ref)
            assert abs(parts.sum() - ref.sum()) <= RTOL * abs(ref.sum())
    b.close()


@pytest.mark.parametrize("T,D,K,N", [
    (300, 16, 16, 3), (120, 64, 64, 2), (1000, 5, 3, 2), (77, 33, 17, 2), (64, 20, 40, 2), (50, 64, 7, 1), (40, 2, 64, 2)])
def test_stagewise_vs_oracle(T, D, K, N):
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=100 + T + D)
    _stagewise(Y, st0, pri, iters=3)


@pytest.mark.parametrize("T,D,K,N,kind", [(70, 96, 96, 2, "diagonal_gamma"), (12, 128, 128, 1, "diagonal_gamma"), (45, 65, 70, 2, "diagonal_gamma"),
                                          (33, 70, 20, 2, "gamma"), (20, 12, 100, 1, "diagonal_gamma"), (3, 80, 80, 1, "diagonal_gamma"),
                                          (2, 100, 66, 2, "diagonal_gamma")])
def test_stagewise_vs_oracle_beyond_64(T, D, K, N, kind):
    """The second shape class of the fused path, 64 < max(D, K) <= 128 (pyvb_amd/csrc/k_big.hip: a workgroup per replicate),
    stage by stage against the oracle; the reference itself is pinned at D = K = 80 by the fixture lds_d80k80_t3."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=900 + T + D)
    if kind == "gamma":
        pri["noise"] = "gamma"
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    if max(D, K) > 102:
        # quirk Q2: the reference takes ln det of the prior precision through np.linalg.det, and det(1e-3 I) underflows to 0
        # from 103 dimensions on: its lower bound is -inf there.  The device sums logs and stays finite; the
        # comparison uses a prior precision whose determinant is representable (1e-2: 1e-256 at 128 dimensions)
        pri["A_prior_prec"] = np.full_like(pri["A_prior_prec"], 1e-2)
        pri["C_prior_prec"] = np.full_like(pri["C_prior_prec"], 1e-2)
    _stagewise(Y, st0, pri, iters=3)


def test_column_ranges_on_the_128_wide_class():
    """As[i].update() / Cs[i].update() for a RANGE of columns (pyvb_lds_update_columns) on the blocked column kernel of the 128-wide
    class (k_cols_big: blocks of 16 columns): ranges that start and end inside a block, span several, are a single column, are the
    last column; some entries of A and C known.  Against the oracle's column loop over the same ranges, then Q and R from the result."""
    T, D, K, N = 12, 100, 70, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=57)
    rng = np.random.default_rng(3)
    pri["A_obs"] = np.where(rng.random((D, D)) < 0.05, rng.standard_normal((D, D)) * 0.2, np.nan)
    pri["C_obs"] = np.where(rng.random((K, D)) < 0.05, rng.standard_normal((K, D)), np.nan)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    O.sweep(st, pri, Y, "forward"); b.sweep("forward")
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")
    S = O.statistics(st, Y)
    for which, lo, hi in [("A", 5, 77), ("C", 0, 1), ("A", 99, 100), ("C", 17, 33), ("A", 0, 100), ("C", 30, 100), ("A", 15, 17), ("C", 0, 100)]:
        (O.update_A if which == "A" else O.update_C)(st, pri, S, cols=(lo, hi))
        b.update_columns(which, lo, hi)
        g = b.get_state()
        _close(g["A_mean"], st["A_mean"], "A_mean after %s[%d:%d]" % (which, lo, hi)); _close(g["C_mean"], st["C_mean"], "C_mean after %s[%d:%d]" % (which, lo, hi))
    O.update_Q(st, pri, S, T); b.update_Q()
    O.update_R(st, pri, S, T); b.update_R()
    _compare_params(b, st, "after the column ranges: ")
    b.close()


@pytest.mark.parametrize("T,D,K,N,kind", [(25, 40, 100, 2, "diagonal_gamma"), (20, 72, 66, 1, "gamma")])
def test_outputs_with_missing_entries_beyond_64(T, D, K, N, kind):
    """Y with NaN (gaussian.py:90-96) where K (or D) exceeds 64: the output kernels handle two entries per lane."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=710 + T)
    rng = np.random.default_rng(T + K)
    mask = rng.random((N, T, K)) < 0.15
    mask[:, 1] = True; mask[:, T // 2] = True; mask[:, 0, 0] = True; mask[:, 3] = False
    Y = np.where(mask, np.nan, Y)
    st0["Yq"] = rng.standard_normal((N, T, K)); st0["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, T))
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    _stagewise(Y, st0, pri, iters=3)


def test_known_matrix_entries_beyond_64():
    """Known entries of A and C (LDS_knowns_in_A.py) on the 128-wide kernels: partially known, fully known and free columns."""
    T, D, K, N = 30, 70, 90, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=43)
    rng = np.random.default_rng(2)
    A_obs = np.where(rng.random((D, D)) < 0.1, rng.standard_normal((D, D)) * 0.2, np.nan)
    C_obs = np.where(rng.random((K, D)) < 0.1, rng.standard_normal((K, D)), np.nan)
    A_obs[:, 3] = np.linspace(-0.1, 0.1, D); C_obs[:, 0] = np.nan; C_obs[:, 69] = rng.standard_normal(K)
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    _stagewise(Y, st0, pri, iters=3)


def test_beyond_64_iterate_matches_the_staged_calls_and_single_updates():
    """pyvb_lds_iterate on the 128-wide kernels equals the separate calls; a sweep spelled as T single X_t.update() calls
    (pyvb_lds_update_x: the time-0 class, interior nodes, the last node) equals the oracle's; Wishart noise above 64
    dimensions is refused at creation."""
    from pyvb_amd import _capi
    from pyvb_amd.lds import LDSBatch
    T, D, K, N = 40, 72, 90, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=31)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.iterate(2)
    for _ in range(2):
        b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.allclose(a.elbo(), b.elbo(), rtol=1e-12)
    hist = a.elbo_history(2)
    assert np.allclose(hist[-1], a.elbo().sum(0), rtol=1e-12)
    a.close(); b.close()
    c = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    O.sweep(st, pri, Y, "forward"); c.sweep("forward")
    O.sweep(st, pri, Y, "backward"); c.sweep("backward")
    S = O.statistics(st, Y); O.update_A(st, pri, S); c.update_A()
    for t in list(range(T)) + [T - 1, 5, 0]:
        O.update_x(st, pri, Y, t); c.update_x(t)
    _close(c.get_state(("X",))["X"], st["X"], "X after single updates of every node")
    c.close()
    # Wishart noise is served up to 128 dimensions since round 4 (k_wishart_big.hip) -- alone: with known entries of A / C or
    # with outputs that hold NaN it stops at 64, and says so
    wb = LDSBatch(1, 10, 65, 4, "wishart")
    with pytest.raises(_capi.PyvbHipError, match="64"):
        wb.set_column_observations(np.full((65, 65), np.nan), np.full((4, 65), np.nan))
    with pytest.raises(_capi.PyvbHipError, match="64"):
        wb.set_observations(np.full((1, 10, 4), np.nan))
    wb.close()
    with pytest.raises(_capi.PyvbHipError):
        LDSBatch(1, 10, 129, 4, "wishart")


@pytest.mark.parametrize("T", [2, 3, 4, 5, 16, 17, 18, 19, 33, 34, 129])
def test_short_and_ragged_chains(T):
    """Segment bookkeeping: chains shorter than, equal to and just above multiples of 16 interior nodes."""
    Y, st0, pri = synth.make_problem(T, 6, 4, 2, seed=500 + T)
    _stagewise(Y, st0, pri, iters=2)


def test_gamma_noise():
    Y, st0, pri = synth.make_problem(90, 7, 9, 2, seed=77)
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)
    _stagewise(Y, st0, pri, iters=3)


def _wishart_priors(pri, D, K, rng=None):
    pri["noise"] = "wishart"
    if rng is None:
        pri["Q_a0"], pri["Q_b0"] = np.float64(1e-3), np.eye(D) * 1e-3
        pri["R_a0"], pri["R_b0"] = np.float64(1e-3), np.eye(K) * 1e-3
    else:       # proper priors: v0 > (dim - 1) / 2, dense w0
        W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
        W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)


@pytest.mark.parametrize("T,D,K,N,proper", [(40, 3, 4, 2, False), (120, 16, 16, 2, True), (90, 33, 17, 2, True), (30, 64, 64, 1, False),
                                            (6, 96, 96, 2, True), (3, 128, 128, 1, False), (20, 70, 9, 2, True), (12, 5, 100, 1, True)])
def test_wishart_noise_vs_oracle(T, D, K, N, proper):
    """Wishart Q and R (Linear_Dynamic_System.py:55-56; nodes_todo.py:205-234): dense expected precisions, dense
    column covariances; three iterations stage by stage against the oracle, which is pinned to the reference for
    the first one (fixture lds_wishart_d3k4_t40) and follows the deviations listed in k_wishart.hip afterwards.
    The lower bound with Wishart parents does not exist in the reference: both sides use the derived one.
    From 65 dimensions on the kernels are those of k_wishart_big.hip (fixtures lds_wishart_d66k3_t3, lds_wishart_d3k70_t3)."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=300 + T + D)
    _wishart_priors(pri, D, K, np.random.default_rng(T) if proper else None)
    if max(D, K) > 102:         # det(1e-3 I) underflows from 103 dimensions on (quirk Q2: the reference's bound is -inf there)
        pri["A_prior_prec"] = np.full_like(pri["A_prior_prec"], 1e-2); pri["C_prior_prec"] = np.full_like(pri["C_prior_prec"], 1e-2)
    _stagewise(Y, st0, pri, iters=3)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
    _close(b.get_state(("X",))["X"], st["X"], "X after iterate (Wishart)")
    _close(b.elbo().sum(1), parts.sum(1), "elbo after iterate (Wishart)")
    b.close()


@pytest.mark.parametrize("T,D,K,N,kind", [(60, 5, 6, 2, "diagonal_gamma"), (300, 16, 16, 2, "diagonal_gamma"), (40, 64, 33, 1, "gamma"), (1200, 8, 64, 2, "diagonal_gamma")])
def test_outputs_with_missing_entries(T, D, K, N, kind):
    """Y with NaN (gaussian.py:90-96): partially observed and unobserved outputs are variational nodes; stage by stage
    against the oracle (pinned to the reference by lds_missing_*.npz), then iterate() interleaved with update_Y."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=700 + T)
    rng = np.random.default_rng(T + K)
    mask = rng.random((N, T, K)) < 0.15
    mask[:, 1] = True; mask[:, T // 2] = True; mask[:, 0, 0] = True; mask[:, 3] = False
    Y = np.where(mask, np.nan, Y)
    st0["Yq"] = rng.standard_normal((N, T, K)); st0["Yrowvar"] = 1.0 / rng.uniform(0.5, 1.5, size=(N, T))
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    _stagewise(Y, st0, pri, iters=3)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T, Y)
    for it in range(2):
        O.iterate(st, pri, Y)           # the example's loop does not update the outputs ...
        b.iterate(1)
        O.update_Y(st, pri); b.update_Y()       # ... a script that does, between iterations
    parts = O.iterate(st, pri, Y)
    b.iterate(1)
    _close(b.get_state(("X",))["X"], st["X"], "X, iterate + update_Y")
    got = b.elbo()
    assert np.all(np.abs(got - parts) <= RTOL * np.abs(parts).sum(axis=1, keepdims=True)), (got, parts)
    b.close()


@pytest.mark.parametrize("T,D,K,N,frac", [(30, 3, 4, 2, 0.3), (50, 6, 17, 1, 0.15), (24, 20, 64, 1, 0.1)])
def test_missing_outputs_with_wishart_noise(T, D, K, N, frac):
    """Outputs with NaN under Wishart noise (round 2 refused the combination): a row's missing entries are correlated and
    regress on its known ones -- qcov_uu = inv(<R>_uu), gaussian.py:117-134 with a dense precision -- so <y y^T> carries a
    dense covariance sum into R's Wishart update and the bound's partial-observation terms read ln det qcov_uu.  Partially
    observed, completely missing and fully observed rows side by side; stage by stage against the oracle, which applies the
    reference's conditioning formula row by row."""
    rng = np.random.default_rng(T + K)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=60 + K)
    _wishart_priors(pri, D, K, np.random.default_rng(K))
    Y[rng.random(Y.shape) < frac] = np.nan
    Y[0, 3] = np.nan                                    # a row without any known entry
    Y[0, 5] = np.nan_to_num(Y[0, 5])                    # and a fully observed one
    st0["Yq"] = np.where(np.isnan(Y), rng.standard_normal(Y.shape), Y)
    st0["Yrowvar"] = rng.uniform(0.5, 2.0, size=Y.shape[:2])
    _stagewise(Y, st0, pri, iters=3)


def test_nondefault_priors():
    """Non-zero prior means and non-trivial prior precisions for X_0 and the columns."""
    T, D, K, N = 60, 5, 6, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=31)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((D, D))
    pri["x0_prec"] = W @ W.T + D * np.eye(D)
    pri["x0_mean"] = rng.standard_normal(D)
    pri["A_prior_mean"] = 0.3 * rng.standard_normal((D, D))
    pri["C_prior_mean"] = 0.3 * rng.standard_normal((K, D))
    pri["A_prior_prec"] = 0.01 + rng.random((D, D))
    pri["C_prior_prec"] = 0.01 + rng.random((D, K))
    pri["Q_a0"], pri["Q_b0"] = 0.1 + rng.random(D), 0.1 + rng.random(D)
    pri["R_a0"], pri["R_b0"] = 0.1 + rng.random(K), 0.1 + rng.random(K)
    _stagewise(Y, st0, pri, iters=2)


def test_single_updates_equal_sweep():
    """[x.update() for x in Xs] node by node == the fused sweep (both directions)."""
    T, D, K, N = 37, 8, 5, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=9)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.sweep("forward")
    for t in range(T):
        b.update_x(t)
    _close(b.get_state(("X",))["X"], a.get_state(("X",))["X"], "stepwise forward", 1e-12)
    a.sweep("backward")
    for t in range(T - 1, -1, -1):
        b.update_x(t)
    _close(b.get_state(("X",))["X"], a.get_state(("X",))["X"], "stepwise backward", 1e-12)
    a.update_A(); b.update_A()
    _close(b.get_state(("A_mean",))["A_mean"], a.get_state(("A_mean",))["A_mean"], "A after stepwise", 1e-12)
    a.close(); b.close()


def test_backward_sweep_without_forward():
    """A backward sweep that does not follow a forward sweep under the same parameters cannot reuse
    the forward sweep's G y_t and must compute it itself."""
    T, D, K, N = 90, 16, 16, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=17)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")
    _close(b.get_state(("X",))["X"], st["X"], "backward sweep first")
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")
    _close(b.get_state(("X",))["X"], st["X"], "backward sweep twice")
    S = O.statistics(st, Y)
    O.update_A(st, pri, S); b.update_A()
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")      # parameters changed: again no cached G y_t
    _close(b.get_state(("X",))["X"], st["X"], "backward sweep after a parameter update")
    O.sweep(st, pri, Y, "forward"); b.sweep("forward")
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")
    _close(b.get_state(("X",))["X"], st["X"], "forward then backward")
    b.close()


def test_partial_state_updates_are_refused():
    """Statistics while only some X_t were updated under new parameters: the three-class
    covariance structure does not hold, the library must say so (PYVB_E_STALE)."""
    from pyvb_amd import _capi
    Y, st0, pri = synth.make_problem(20, 4, 4, 1, seed=3)
    b = _batch(Y, st0, pri)
    b.iterate(1)
    b.update_x(3)
    with pytest.raises(_capi.PyvbHipError) as e:
        b.update_A()
    assert e.value.code == _capi.E_STALE
    b.close()


def test_parameters_before_any_sweep():
    """A fresh handle has no covariances for the X_t (the reference draws an individual one per node): the library says so
    (PYVB_E_STALE) instead of using zeros; with per-class initial covariances supplied it matches the oracle."""
    from pyvb_amd import _capi
    T, D, K, N = 30, 4, 5, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=8)
    b = _batch(Y, st0, pri)
    for call in (b.update_A, b.update_Q, b.elbo):
        with pytest.raises(_capi.PyvbHipError) as e:
            call()
        assert e.value.code == _capi.E_STALE
    rng = np.random.default_rng(1)
    Sig = np.stack([np.eye(D) / u for u in rng.random(N * 3)]).reshape(N, 3, D, D)
    b.set_posterior_classes(Sig)
    st = O.expand_state(st0, pri, T)
    st["Sigma"], st["qld_x"] = Sig, np.zeros((N, 3))
    S = O.statistics(st, Y)
    O.update_A(st, pri, S); b.update_A()
    O.update_C(st, pri, S); b.update_C()
    O.update_Q(st, pri, S, T); b.update_Q()
    O.update_R(st, pri, S, T); b.update_R()
    _compare_params(b, st, "before any sweep ")
    b.close()


def test_not_positive_definite_raises():
    Y, st0, pri = synth.make_problem(20, 4, 4, 1, seed=3)
    st0["Q_b"] = -np.abs(st0["Q_b"]) * 1e-9        # hugely negative expected precision
    b = _batch(Y, st0, pri)
    b.sweep("forward")
    with pytest.raises(np.linalg.LinAlgError):
        b.sync()
    b.close()


def test_iterate_equals_individual_calls_and_is_deterministic():
    T, D, K, N = 200, 16, 16, 5
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=12)
    a, b, c = _batch(Y, st0, pri), _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.iterate(3)
    c.iterate(3)
    for _ in range(3):
        b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    ea, eb, ec = a.elbo(), b.elbo(), c.elbo()
    assert np.array_equal(ea, eb) and np.array_equal(ea, ec)
    assert np.array_equal(a.get_state(("X",))["X"], c.get_state(("X",))["X"])
    tot = a.elbo_total()
    assert np.allclose(tot, ea.sum(0), rtol=1e-13)
    for x in (a, b, c):
        x.close()


def test_replicates_are_independent():
    """Replicate r of a batch gives bit-identical results to the same problem run alone."""
    T, D, K, N = 150, 16, 8, 4
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=21)
    full = _batch(Y, st0, pri)
    full.iterate(2)
    Xf, ef = full.get_state(("X",))["X"], full.elbo()
    for r in (0, 3):
        one = _batch(Y[r:r + 1], {k: v[r:r + 1] for k, v in st0.items()}, pri)
        one.iterate(2)
        assert np.array_equal(one.get_state(("X",))["X"][0], Xf[r])
        assert np.array_equal(one.elbo()[0], ef[r])
        one.close()
    full.close()


def test_warmup_is_data_driven_and_exact_fallback():
    """Slowly contracting recurrences must lengthen the warm-up: the length k_prep derives from the norms of F^4 .. F^32 is
    compared between a well-conditioned problem and one pushed towards the spectral bound (the recurrence matrix of a valid
    posterior has spectral radius <= 1/2, so k_prep's no-contraction value -- 1 << 30, 'run sequentially' -- needs a
    pathologically non-normal F and is not reachable from data; what IS reachable is a warm-up longer than a segment, which is
    the same code path: every segment then starts from the true boundary state).  Both are checked against the oracle stage by
    stage, the second also on a chain so short that every segment's warm-up reaches the boundary."""
    T, D, K, N = 400, 4, 4, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=2)
    b0 = _batch(Y, st0, pri)
    b0.sweep("forward")
    w_easy = b0.get_warmup()
    b0.close()
    # tiny observation precision and huge process precision => F close to its spectral bound
    st0["R_b"] = st0["R_b"] * 1e8
    st0["Q_b"] = st0["Q_b"] * 1e-6
    _stagewise(Y, st0, pri, iters=1)
    b = _batch(Y, st0, pri)
    b.sweep("forward")
    w = b.get_warmup()
    b.close()
    assert np.all(w >= 8) and np.all(w < (1 << 30))
    assert w[:, 0].min() > w_easy[:, 0].max(), (w, w_easy)          # the forward recurrence: longer than on the easy problem
    Lseg = (T - 2 + 15) // 16
    # a chain whose segments (2 interior nodes each) are all shorter than the warm-up: the sweep degenerates to the
    # sequential chain, exactly
    Ts = 34
    Ys, st0s, pris = synth.make_problem(Ts, D, K, N, seed=3)
    st0s["R_b"] = st0s["R_b"] * 1e8
    st0s["Q_b"] = st0s["Q_b"] * 1e-6
    _stagewise(Ys, st0s, pris, iters=2)
    bs = _batch(Ys, st0s, pris)
    bs.sweep("forward")
    assert bs.get_warmup().min() > (Ts - 2 + 15) // 16
    bs.close()


def test_headline_shape_against_oracle():
    """BASELINE config 3 shape (T = 10^4, D = K = 64) on a few replicates: one full iteration
    against the oracle, plus the size-independent checks at N = 64."""
    T, D, K = 10000, 64, 64
    Y, st0, pri = synth.make_problem(T, D, K, 2, seed=4242)
    st = O.expand_state(st0, pri, T)
    parts = O.iterate(st, pri, Y)
    b = _batch(Y, st0, pri)
    b.iterate(1)
    got = b.elbo()
    _close(b.get_state(("X",))["X"], st["X"], "X (T=10^4, D=64)")
    _compare_params(b, st, "headline ")
    _close(got.sum(1), parts.sum(1), "elbo (T=10^4, D=64)")
    b.close()
    # N = 64 replicas of the two problems: every copy must agree bitwise with the first
    rep = 32
    Yb = np.concatenate([Y] * rep)
    stb = {k: np.concatenate([v] * rep) for k, v in st0.items()}
    big = _batch(Yb, stb, pri)
    big.iterate(1)
    e = big.elbo()
    assert np.array_equal(e[0::2], np.repeat(e[0:1], rep, 0)) and np.array_equal(e[1::2], np.repeat(e[1:2], rep, 0))
    # a different batch size may split the time axis of the statistics kernel differently:
    # same values up to summation order
    assert np.all(np.abs(e[:2] - got) <= 1e-12 * np.abs(got).sum(axis=1, keepdims=True))
    big.close()


def test_headline_instantiation_one_wavefront_per_replicate_warmup():
    """The instantiation bench.py times -- k_sweep<4,4,true,{1,2},SPLIT=false>: one wavefront per replicate, 16
    segments of Lseg nodes that warm up J < Lseg steps from zero -- forced on a handful of replicates
    (pyvb_lds_set_time_split) and compared with the oracle over two full iterations."""
    T, D, K, N = 2402, 64, 64, 3
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=777)
    b = _batch(Y, st0, pri)
    b.set_time_split(1)
    assert b.get_time_split() == 1
    st = O.expand_state(st0, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
        w = b.get_warmup()
        assert np.all(w > 0) and np.all(w < (T - 2) // 16), "warm-up path not exercised: J = %r, Lseg = %d" % (w, (T - 2) // 16)
        _close(b.get_state(("X",))["X"], st["X"], "X (W = 1, iteration %d)" % it)
        got = b.elbo()
        assert np.all(np.abs(got - parts) <= RTOL * np.abs(parts).sum(axis=1, keepdims=True)), "elbo parts (W = 1)"
    _compare_params(b, st, "W = 1 ")
    Sig, qld = b.get_posterior_classes()
    _close(Sig, st["Sigma"], "Sigma (W = 1)")
    # stage by stage as well (MODE 0 backward sweep, separate statistics with Sxx from k_stats)
    b.close()
    b = _batch(Y, st0, pri)
    b.set_time_split(1)
    st = O.expand_state(st0, pri, T)
    post = O.state_posteriors(st, pri)
    O.sweep(st, pri, Y, "backward", post); b.sweep("backward")
    _close(b.get_state(("X",))["X"], st["X"], "backward sweep alone (W = 1)")
    O.sweep(st, pri, Y, "forward", post); b.sweep("forward")
    _close(b.get_state(("X",))["X"], st["X"], "forward sweep with stored states (W = 1)")
    b.close()


def test_time_split_of_the_128_wide_class():
    """Few replicates at 64 < D <= 128: the interior time range is dealt out to W workgroups per replicate (k_sweep_big, as SPLIT
    in k_sweep.hip; round 3 ran one chain as ONE workgroup).  The library's own choice of W, two iterations stage by stage
    against the oracle; W = 1 and W = 3 forced on the same problem end at the same states (to rounding: the parts warm up
    across their borders)."""
    T, D, K, N = 1500, 100, 70, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4242)
    b = _batch(Y, st0, pri)
    W = b.get_time_split()
    assert W > 1, W
    b.close()
    _stagewise(Y, st0, pri, iters=2)
    out = {}
    for w in (1, 3, W):
        b = _batch(Y, st0, pri)
        b.set_time_split(w)
        assert b.get_time_split() == w
        b.iterate(2)
        out[w] = (b.get_state(), b.elbo())
        b.close()
    for w in (3, W):
        for k in ("X", "A_mean", "C_mean", "Q_b", "R_b"):
            _close(out[w][0][k], out[1][0][k], "W = %d against W = 1: %s" % (w, k), 1e-11)
        assert np.all(np.abs(out[w][1] - out[1][1]) <= 1e-10 * np.abs(out[1][1]).sum(axis=1, keepdims=True))
    # Wishart noise on the split sweep (dense boundary nodes in every part that can reach them)
    _wishart_priors(pri, D, K, np.random.default_rng(3))
    _stagewise(Y[:, :400], {k: (v[:, :400] if k == "X" else v) for k, v in st0.items()}, pri, iters=1)


def test_time_split_of_the_128_wide_class_with_a_part_without_nodes():
    """T = 51 forced into three parts: 49 interior nodes in parts of 32, so the third workgroup of a replicate owns no node.  Two
    iterations against the oracle."""
    T, D, K, N = 51, 100, 70, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4243)
    b = _batch(Y, st0, pri)
    b.set_time_split(3)
    assert b.get_time_split() == 3
    st = O.expand_state(st0, pri, T)
    for _ in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
    _compare_params(b, st, "T = 51, set_time_split(3): ")
    _close(b.get_state(("X",))["X"], st["X"], "X, T = 51, set_time_split(3)")
    _close(b.elbo().sum(1), parts.sum(1), "elbo, T = 51, set_time_split(3)")
    b.close()


def test_headline_batch_1024_replicates():
    """BASELINE configs[2] as bench.py runs it: N = 1024 replicates (the library itself chooses one wavefront per
    replicate), T = 10^4, D = K = 64.  Two distinct problems tiled 512 times: replicates 0 and 1 against the oracle,
    every copy bitwise equal to the first."""
    T, D, K, N = 10000, 64, 64, 1024
    Y2, st2, pri = synth.make_problem(T, D, K, 2, seed=4243)
    rep = N // 2
    Y = np.concatenate([Y2] * rep)
    st0 = {k: np.concatenate([v] * rep) for k, v in st2.items()}
    b = _batch(Y, st0, pri)
    del Y
    assert b.get_time_split() == 1
    st = O.expand_state(st2, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y2)
        b.iterate(1)
    w = b.get_warmup()
    assert np.all(w > 0) and np.all(w < (T - 2) // 16)
    e = b.elbo()
    assert np.all(np.abs(e[:2] - parts) <= RTOL * np.abs(parts).sum(axis=1, keepdims=True)), "elbo parts (N = 1024)"
    _close(e[:2].sum(1), parts.sum(1), "elbo (N = 1024)")
    assert np.array_equal(e[0::2], np.repeat(e[0:1], rep, 0)) and np.array_equal(e[1::2], np.repeat(e[1:2], rep, 0))
    g = b.get_state(("A_mean", "C_mean", "Q_b", "R_b"))
    _close(g["A_mean"][:2], st["A_mean"], "A_mean (N = 1024)")
    _close(g["C_mean"][:2], st["C_mean"], "C_mean (N = 1024)")
    _close(g["Q_b"][:2], st["Q_b"], "Q_b (N = 1024)")
    _close(g["R_b"][:2], st["R_b"], "R_b (N = 1024)")
    X = b.get_state(("X",))["X"]
    _close(X[:2], st["X"], "X (N = 1024)")
    assert np.array_equal(X[2:4], X[:2]) and np.array_equal(X[-2:], X[:2])
    b.close()


def test_baseline_config2_single_long_chain():
    """BASELINE configs[1]: T = 10^4, D = K = 16, one replicate, three full iterations against the oracle
    (the segmented sweeps run with 624 interior nodes per segment and a data-driven warm-up)."""
    T, D, K = 10000, 16, 16
    Y, st0, pri = synth.make_problem(T, D, K, 1, seed=2)
    st = O.expand_state(st0, pri, T)
    b = _batch(Y, st0, pri)
    for it in range(3):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
        _close(b.get_state(("X",))["X"], st["X"], "X (config 2, iteration %d)" % it)
        _close(b.elbo().sum(1), parts.sum(1), "elbo (config 2, iteration %d)" % it)
    _compare_params(b, st, "config 2 ")
    b.close()


@pytest.mark.parametrize("T,D,K,N", [(600, 6, 4, 1), (777, 16, 16, 2), (1030, 33, 17, 3), (4099, 8, 8, 5), (2050, 64, 64, 1)])
def test_time_split_over_wavefronts(T, D, K, N):
    """Few replicates and a long chain: the sweeps deal the time axis out to several wavefronts per replicate
    (ragged parts, parts without nodes, warm-up across part borders)."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=900 + T)
    _stagewise(Y, st0, pri, iters=2)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
    _close(b.get_state(("X",))["X"], st["X"], "X after iterate (time split)")
    _close(b.elbo().sum(1), parts.sum(1), "elbo after iterate (time split)")
    b.close()


def test_rccl_communicator_single_rank():
    """The RCCL leg of pyvb_lds_elbo_total (dlopen of librccl, unique id, communicator, all-reduce on
    the handle's stream) with a one-rank communicator: the sum over ranks is the local sum."""
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri = synth.make_problem(50, 8, 8, 3, seed=5)
    b = _batch(Y, st0, pri)
    b.iterate(1)
    local = b.elbo().sum(0)
    uid = LDSBatch.comm_unique_id()
    assert len(uid) == 128
    b.comm_init(uid, 0, 1)
    tot = b.elbo_total()
    assert np.allclose(tot, local, rtol=1e-13)
    b.close()


def test_known_matrix_entries_vs_oracle():
    """Observed entries of A and C (LDS_knowns_in_A.py): partially and fully known columns."""
    T, D, K, N = 80, 5, 6, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=41)
    A_obs = np.full((D, D), np.nan); C_obs = np.full((K, D), np.nan)
    A_obs[0, 0] = 1.0; A_obs[1, 0] = 1e-2; A_obs[3, 2] = -0.5
    A_obs[:, 4] = np.linspace(-0.2, 0.2, D)
    C_obs[2, 1] = 3.0; C_obs[:, 3] = np.arange(K) - 2.0
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    _stagewise(Y, st0, pri, iters=3)


@pytest.mark.parametrize("T,D,K,N", [(60, 5, 6, 2), (40, 17, 9, 1), (30, 64, 64, 1)])
def test_known_matrix_entries_with_wishart_noise(T, D, K, N):
    """Known entries of A and C together with Wishart noise (gaussian.py:125-134 on dense column covariances): the column kernel
    conditions on them by exchanging the known pivots back after the inversion (gj_wave_subset); partially known, fully
    known and free columns side by side, three iterations stage by stage against the oracle (which applies the reference's
    conditioning formula to the dense covariance), the lower bound's partial-observation branch (:148-150) included."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=70 + D)
    _wishart_priors(pri, D, K, np.random.default_rng(D))
    rng = np.random.default_rng(5)
    A_obs = np.full((D, D), np.nan); C_obs = np.full((K, D), np.nan)
    A_obs[0, 0] = 0.9; A_obs[min(3, D - 1), 2] = -0.25; A_obs[D - 1, 2] = 0.1
    A_obs[:, D - 1] = np.linspace(-0.2, 0.2, D)                 # a fully known column
    C_obs[rng.random((K, D)) < 0.15] = 0.5
    C_obs[:, 1] = np.arange(K) * 0.1 - 0.2                      # another
    C_obs[:, 0] = np.nan                                         # and a free one
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    _stagewise(Y, st0, pri, iters=3)
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
    _close(b.get_state(("A_mean",))["A_mean"], st["A_mean"], "A after iterate (Wishart, known entries)")
    _close(b.elbo().sum(1), parts.sum(1), "elbo after iterate (Wishart, known entries)")
    b.close()


def test_wishart_column_covariances_round_trip():
    """pyvb_lds_set_column_cov / get_column_cov / get_wishart_state: what goes in comes out, the diagonals follow."""
    T, D, K, N = 12, 5, 3, 4
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=2)
    _wishart_priors(pri, D, K)
    b = _batch(Y, st0, pri)
    rng = np.random.default_rng(0)
    A = rng.standard_normal((N, D, D, D)); A = A @ np.swapaxes(A, -1, -2) + np.eye(D)
    Cc = rng.standard_normal((N, D, K, K)); Cc = Cc @ np.swapaxes(Cc, -1, -2) + np.eye(K)
    b.set_column_cov(A, Cc)
    A2, C2 = b.get_column_cov()
    assert np.array_equal(A, A2) and np.array_equal(Cc, C2)
    g = b.get_state(("A_colvar", "C_colvar"))
    assert np.array_equal(g["A_colvar"], np.einsum("nikk->nik", A)) and np.array_equal(g["C_colvar"], np.einsum("nikk->nik", Cc))
    w = b.get_wishart_state()
    assert np.allclose(w["Q_v"], 1e-3 + 0.5 * (T - 1)) and np.allclose(w["R_v"], 1e-3 + 0.5 * T)
    b.close()
