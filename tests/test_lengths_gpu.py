"""GPU: one LDS handle whose replicates have chain lengths of their own (include/pyvb_hip.h: pyvb_lds_create_lengths).

Replicate n of such a handle is the graph of examples/Linear_Dynamic_System.py:46-66 with T_n time steps.  The comparator for it
is always the same model on its own: the reference's recorded run (tests/golden/lds_*d4k5*.npz) or the oracle
(oracle/lds_closed_form.py) with N = 1 and T = T_n.  Tolerances are those of tests/test_gpu_parity.py: RTOL = 1e-8 max-norm for
states and parameters, the lower bound as in its _stagewise, 1e-12 where that file uses 1e-12.

"Bitwise" is justified as in tests/test_status_mask_gpu.py: replicates share no arithmetic, and two handles of the same
N, T, D, K, lengths and time split run the same instructions in the same order on the rows both compute.
"""
import glob
import os

import numpy as np
import pytest

import exact_bound_ref as XR
from conftest import GOLDEN_DIR, load_golden
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
    ok = np.isfinite(sb)
    assert np.all(np.abs(sa - sb)[ok] <= 1e-9 * np.maximum(1.0, np.abs(sb[ok]))), what


def _gamma(pri):
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)


def _problem(T, D, K, lengths, seed, kind="diagonal_gamma", fill=0.0):
    """A handle's inputs: N = len(lengths) simulated series, the first T_n steps of each, padding rows filled with `fill`."""
    N = len(lengths)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=seed)
    if kind == "gamma":
        _gamma(pri)
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    Y = np.where(live[:, :, None], Y, fill)
    st0["X"] = np.where(live[:, :, None], st0["X"], fill)
    return Y, st0, pri


def _alone(Y, st0, pri, n, Tn):
    """Replicate n on its own, as the oracle takes it: (Y[1, T_n, K], dense state)."""
    Yn = Y[n:n + 1, :Tn].copy()
    sn = {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]).copy() for k, v in st0.items()}
    return Yn, O.expand_state(sn, pri, Tn, Yn)


def _batch(Y, st0, pri, lengths):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=np.asarray(lengths, dtype=np.int32))


def _cls(Tn):
    return [0, 1, 2] if Tn > 2 else [0, 2]


def _compare_x(b, sts, lengths, tag):
    X = b.get_state(("X",))["X"]
    for n, Tn in enumerate(lengths):
        _close(X[n, :Tn], sts[n]["X"][0], "%sX of replicate %d (T_n = %d)" % (tag, n, Tn))
        assert np.array_equal(X[n, Tn:], np.zeros_like(X[n, Tn:])), "%spadding rows of X, replicate %d" % (tag, n)


def _compare_params(b, sts, tag):
    g = b.get_state()
    qa, qc = b.get_column_qld()
    for n, st in enumerate(sts):
        t = "%sreplicate %d " % (tag, n)
        _close(g["A_mean"][n], st["A_mean"][0], t + "A_mean")
        _close(g["C_mean"][n], st["C_mean"][0], t + "C_mean")
        _close(g["A_colvar"][n], np.einsum("ikk->ik", st["A_cov"][0]), t + "A_colvar")
        _close(g["C_colvar"][n], np.einsum("ikk->ik", st["C_cov"][0]), t + "C_colvar")
        for nm in ("Q_a", "Q_b", "R_a", "R_b"):
            _close(g[nm][n], np.broadcast_to(st[nm][0], g[nm][n].shape), t + nm)
        _close_qld(qa[n], st["qld_A"][0], t + "qld_A")
        _close_qld(qc[n], st["qld_C"][0], t + "qld_C")


def _compare_elbo(got, sts, Ys, pri, lengths, tag, parts_fn=None):
    for n, Tn in enumerate(lengths):
        S = O.statistics(sts[n], Ys[n])
        want = (parts_fn or O.elbo_parts)(sts[n], pri, S, Tn)[0]
        assert np.all(np.isfinite(got[n])), tag
        assert np.all(np.abs(got[n] - want) <= RTOL * np.abs(want).sum()), "%selbo parts of replicate %d\n%r\n%r" % (tag, n, got[n], want)
        assert abs(got[n].sum() - want.sum()) <= RTOL * abs(want.sum()), "%selbo total of replicate %d" % (tag, n)


def _stagewise(Y, st0, pri, lengths, iters, W=None):
    """The example's loop on the handle and, replicate by replicate, in the oracle; compared after every stage."""
    b = _batch(Y, st0, pri, lengths)
    if W is not None:
        b.set_time_split(W)
    alone = [_alone(Y, st0, pri, n, Tn) for n, Tn in enumerate(lengths)]
    Ys, sts = [a[0] for a in alone], [a[1] for a in alone]
    assert np.array_equal(b.lengths, np.asarray(lengths))
    for it in range(iters):
        tag = "it%d " % it
        posts = [O.state_posteriors(st, pri) for st in sts]
        for direction in ("forward", "backward"):
            for st, Yn, post in zip(sts, Ys, posts):
                O.sweep(st, pri, Yn, direction, post)
            b.sweep(direction)
            _compare_x(b, sts, lengths, tag + direction + " sweep: ")
        Sig, qld = b.get_posterior_classes()
        for n, Tn in enumerate(lengths):
            _close(Sig[n][_cls(Tn)], sts[n]["Sigma"][0][_cls(Tn)], tag + "Sigma of replicate %d" % n)
            _close_qld(qld[n][_cls(Tn)], sts[n]["qld_x"][0][_cls(Tn)], tag + "qld_x of replicate %d" % n)
        Ss = [O.statistics(st, Yn) for st, Yn in zip(sts, Ys)]
        for st, S in zip(sts, Ss):
            O.update_A(st, pri, S)
        b.update_A()
        for n, st in enumerate(sts):
            _close(b.get_state(("A_mean",))["A_mean"][n], st["A_mean"][0], tag + "A_mean after update_A, replicate %d" % n)
        for st, S in zip(sts, Ss):
            O.update_C(st, pri, S)
        b.update_C()
        for n, st in enumerate(sts):
            _close(b.get_state(("C_mean",))["C_mean"][n], st["C_mean"][0], tag + "C_mean after update_C, replicate %d" % n)
        for st, S, Tn in zip(sts, Ss, lengths):
            O.update_Q(st, pri, S, Tn); O.update_R(st, pri, S, Tn)
        b.update_Q(); b.update_R()
        _compare_params(b, sts, tag)
        _compare_elbo(b.elbo(), sts, Ys, pri, lengths, tag)
    b.close()


# ---- 1. the reference side by side ------------------------------------------------------------------------------------------
def test_four_reference_runs_of_different_lengths_on_one_handle():
    """The reference's own runs at T = 3, 19, 60 and 200 (D = 4, K = 5) as the four replicates of one handle of T = 200:
    after each recorded iteration every replicate reproduces its fixture, to the tolerances of test_golden_fixtures."""
    paths = sorted(glob.glob(os.path.join(GOLDEN_DIR, "lds_*d4k5*.npz")))
    cases = [load_golden(p) for p in paths if "gamma" not in os.path.basename(p)]
    lengths = [c[0]["T"] for c in cases]
    assert sorted(lengths) == [3, 19, 60, 200], paths
    iters = cases[0][0]["iters"]
    assert all(list(c[0]["iters"]) == list(iters) and c[0]["noise"] == "diagonal_gamma" for c in cases)
    from pyvb_amd.lds import LDSBatch
    pri = cases[0][3]
    for c in cases[1:]:
        for k in pri:
            assert np.array_equal(np.asarray(pri[k]), np.asarray(c[3][k])), "the fixtures share their priors: " + k
    b = LDSBatch.from_series([(c[1][0], c[2]) for c in cases], pri)
    assert b.T == 200 and list(b.lengths) == lengths
    b.sweep("forward")
    X = b.get_state(("X",))["X"]
    for n, c in enumerate(cases):
        _close(X[n, :lengths[n]], c[4]["it1_fwd_X"], "forward sweep vs reference, replicate %d" % n)
    b.sweep("backward")
    for it in range(1, max(iters) + 1):
        if it > 1:
            b.sweep("forward"); b.sweep("backward")
        b.update_A(); b.update_C(); b.update_Q(); b.update_R()
        if it not in iters:
            continue
        g = b.get_state()
        Sig, qld = b.get_posterior_classes()
        parts = b.elbo()
        for n, (c, Tn) in enumerate(zip(cases, lengths)):
            z, tag = c[4], "it%d_" % it
            what = "replicate %d (T_n = %d) %s" % (n, Tn, tag)
            _close(g["X"][n, :Tn], z[tag + "X"], what + "X")
            _close(Sig[n][_cls(Tn)], z[tag + "Sigma"][_cls(Tn)], what + "Sigma")
            _close_qld(qld[n][_cls(Tn)], z[tag + "qld_x"][_cls(Tn)], what + "qld_x")
            _close(g["A_mean"][n], z[tag + "A_mean"], what + "A_mean")
            _close(g["C_mean"][n], z[tag + "C_mean"], what + "C_mean")
            for nm in ("A", "C"):
                ref = z[tag + nm + "_colvar"] if tag + nm + "_colvar" in z else np.einsum("ikk->ik", z[tag + nm + "_cov"])
                _close(g[nm + "_colvar"][n], ref, what + nm + "_colvar")
            for nm in ("Q_a", "Q_b", "R_a", "R_b"):
                _close(g[nm][n], np.broadcast_to(z[tag + nm], g[nm][n].shape), what + nm)
            ref = z[tag + "elbo_parts"]
            assert np.all(np.abs(parts[n] - ref) <= RTOL * np.abs(ref).sum()), "%s elbo parts %r vs %r" % (what, parts[n], ref)
            assert abs(parts[n].sum() - ref.sum()) <= RTOL * abs(ref.sum()), what + "elbo total"
    b.close()


# ---- 2. stage by stage against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
@pytest.mark.parametrize("D,K,T", [(6, 4, 77), (16, 16, 77), (33, 17, 77), (64, 64, 40)])
def test_stagewise_vs_oracle(D, K, T, kind):
    lengths = [2, 3, 4, 18, 19, 34, T]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7000 + D + K, kind=kind)
    _stagewise(Y, st0, pri, lengths, iters=2)


# ---- 3. padding is never read -----------------------------------------------------------------------------------------------
def _everything(b):
    out = dict(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["qld_A"], out["qld_C"] = b.get_column_qld()
    for k, v in b.get_logdets().items():
        out["lnd_" + k] = v
    out["Yq"], out["Yvar"], out["Yqld"] = b.get_outputs(with_qld=True)
    out["elbo"] = b.elbo()
    return out


@pytest.mark.parametrize("T,D,K,W", [(77, 6, 4, None), (40, 64, 64, None), (700, 8, 8, 4)])
def test_padding_is_never_read(T, D, K, W):
    lengths = [2, 3, 4, 18, 19, 34, T] if T < 100 else [T, 500, 300, 40, 3, 2]
    outs = []
    for fill in (0.0, np.nan):
        Y, st0, pri = _problem(T, D, K, lengths, seed=7100 + D, fill=fill)
        b = _batch(Y, st0, pri, lengths)
        if W is not None:
            b.set_time_split(W)
        b.iterate(3)
        outs.append(_everything(b))
        outs[-1]["history"] = b.elbo_history()
        b.close()
    zero, nan = outs
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    for k in zero:
        assert np.array_equal(zero[k], nan[k], equal_nan=True), k          # every getter pads alike, so whole arrays compare
    assert np.all(np.isfinite(zero["X"])) and np.all(np.isfinite(zero["elbo"])) and np.all(np.isfinite(zero["history"]))
    for out in outs:
        assert np.all(out["X"][~live] == 0.0) and np.all(out["Yq"][~live] == 0.0) and np.all(out["Yvar"][~live] == 0.0)
        assert np.all(np.isnan(out["Yqld"][~live])) and np.all(np.isnan(out["lnd_Y"][~live]))
        assert np.array_equal(out["Yq"][live], Y[live])


# ---- 4. equal lengths change nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,K,N", [(120, 16, 16, 3), (600, 8, 6, 5)])
def test_equal_lengths_change_nothing(T, D, K, N):
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7200 + T)
    a, b = LDSBatch.from_problem(Y, st0, pri), LDSBatch.from_problem(Y, st0, pri, lengths=np.full(N, T))
    assert np.array_equal(a.lengths, b.lengths) and a.get_time_split() == b.get_time_split()
    a.iterate(3); b.iterate(3)
    ea, eb = _everything(a), _everything(b)
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), k
    assert np.array_equal(a.elbo_history(), b.elbo_history())
    a.close(); b.close()


# ---- 5. the time split ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 4, None])
def test_time_split(W):
    """Chains much shorter than the handle's T leave whole parts of the time axis without nodes: the sum of mu mu^T that the
    backward sweep forms per part must not pick up a part that was never written."""
    T, D, K = 2050, 8, 8
    lengths = [2050, 1500, 300, 40, 3, 2]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7300)
    b = _batch(Y, st0, pri, lengths)
    if W is not None:
        b.set_time_split(W)
    print("time split:", b.get_time_split())
    b.iterate(2)
    alone = [_alone(Y, st0, pri, n, Tn) for n, Tn in enumerate(lengths)]
    Ys, sts = [a[0] for a in alone], [a[1] for a in alone]
    for st, Yn in zip(sts, Ys):
        O.iterate(st, pri, Yn, with_elbo=False); O.iterate(st, pri, Yn, with_elbo=False)
    _compare_x(b, sts, lengths, "W = %r: " % (W,))
    _compare_params(b, sts, "W = %r: " % (W,))
    _compare_elbo(b.elbo(), sts, Ys, pri, lengths, "W = %r: " % (W,))
    # the same through the staged calls, where the statistics kernel forms Sxx itself
    c = _batch(Y, st0, pri, lengths)
    if W is not None:
        c.set_time_split(W)
    for _ in range(2):
        c.sweep("forward"); c.sweep("backward"); c.update_A(); c.update_C(); c.update_Q(); c.update_R()
    _compare_x(c, sts, lengths, "staged, W = %r: " % (W,))
    _compare_params(c, sts, "staged, W = %r: " % (W,))
    b.close(); c.close()


# ---- 6. calling orders and modes --------------------------------------------------------------------------------------------
def test_iterate_equals_the_staged_calls_and_the_history_sums_the_replicates():
    T, D, K = 90, 7, 9
    lengths = [90, 2, 33, 3, 61]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7400)
    a, b = _batch(Y, st0, pri, lengths), _batch(Y, st0, pri, lengths)
    a.iterate(2)
    for _ in range(2):
        b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()
    ga, gb = a.get_state(), b.get_state()
    for k in ga:
        assert np.array_equal(ga[k], gb[k]), k
    assert np.allclose(a.elbo(), b.elbo(), rtol=1e-12)
    hist = a.elbo_history(2)
    assert hist.shape == (2, 6)
    assert np.allclose(hist[-1], a.elbo().sum(0), rtol=1e-12)
    assert np.allclose(a.elbo_total(), a.elbo().sum(0), rtol=1e-12)
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_single_updates_in_both_directions_equal_the_sweeps(kind):
    """pyvb_lds_update_x(t) for t = 0..T-1 and back: Xs_n[t].update() where replicate n has a node t, nothing elsewhere; node
    T_n - 1 is the last node of its own chain."""
    T, D, K = 40, 5, 6
    lengths = [40, 2, 3, 17, 39]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7500, kind=kind)
    a, b = _batch(Y, st0, pri, lengths), _batch(Y, st0, pri, lengths)
    for it in range(2):
        a.sweep("forward")
        for t in range(T):
            b.update_x(t)
        assert np.allclose(a.get_state(("X",))["X"], b.get_state(("X",))["X"], rtol=1e-12, atol=0), "forward, iteration %d" % it
        a.sweep("backward")
        for t in reversed(range(T)):
            b.update_x(t)
        assert np.allclose(a.get_state(("X",))["X"], b.get_state(("X",))["X"], rtol=1e-12, atol=0), "backward, iteration %d" % it
        for h in (a, b):
            h.update_A(); h.update_C(); h.update_Q(); h.update_R()
        assert np.allclose(a.elbo(), b.elbo(), rtol=1e-12)
    # and against the oracle's single updates, replicate by replicate
    alone = [_alone(Y, st0, pri, n, Tn) for n, Tn in enumerate(lengths)]
    c = _batch(Y, st0, pri, lengths)
    order = list(range(T)) + [T - 1, 5, 0, 2, 1]
    for t in order:
        c.update_x(t)
    for (Yn, st), Tn in zip(alone, lengths):
        post = O.state_posteriors(st, pri)
        for t in order:
            if t < Tn:
                O.update_x(st, pri, Yn, t, post)
    _compare_x(c, [s for _, s in alone], lengths, "single updates: ")
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("kind", ["diagonal_gamma", "gamma"])
def test_exact_bound_per_replicate(kind):
    T, D, K = 50, 5, 6
    lengths = [50, 2, 3, 20, 35]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7600, kind=kind)
    b = _batch(Y, st0, pri, lengths)
    b.set_bound_mode("exact")
    alone = [_alone(Y, st0, pri, n, Tn) for n, Tn in enumerate(lengths)]
    Ys, sts = [a[0] for a in alone], [a[1] for a in alone]
    for it in range(2):
        b.iterate(1)
        want = np.concatenate([XR.iterate_exact(st, pri, Yn) for st, Yn in zip(sts, Ys)])
        got = b.elbo()
        assert np.all(np.isfinite(got))
        assert np.all(np.abs(got - want) <= RTOL * np.maximum(np.abs(want), 1.0)), "iteration %d\n%r\n%r" % (it, got, want)
        assert np.allclose(b.elbo_history()[-1], got.sum(0), rtol=1e-12)
    ld = b.get_logdets()
    for n, st in enumerate(sts):
        _close(ld["X"][n][_cls(lengths[n])], np.linalg.slogdet(st["Sigma"][0])[1][_cls(lengths[n])], "ln det Sigma, replicate %d" % n)
    b.close()


def test_known_entries_of_A_and_C():
    T, D, K = 60, 6, 7
    lengths = [60, 2, 3, 19, 44]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7700)
    rng = np.random.default_rng(D)
    A_obs = np.where(rng.random((D, D)) < 0.2, 0.3 * rng.standard_normal((D, D)), np.nan)
    C_obs = np.where(rng.random((K, D)) < 0.2, rng.standard_normal((K, D)), np.nan)
    A_obs[:, 1] = 0.1
    C_obs[:, 0] = np.nan
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    _stagewise(Y, st0, pri, lengths, iters=2)


# ---- 7. the other handle-wide features --------------------------------------------------------------------------------------
def test_activity_mask_on_a_mixed_length_handle():
    """One short and one long replicate switched off mid-run: they stand still, the others end where they end without it."""
    T, D, K = 600, 8, 6
    lengths = [600, 3, 450, 40, 2, 77]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7800)
    b, twin = _batch(Y, st0, pri, lengths), _batch(Y, st0, pri, lengths)
    try:
        assert b.get_time_split() == twin.get_time_split()
        b.iterate(2); twin.iterate(2)
        before = _everything(b)
        mask = np.ones(len(lengths), dtype=bool); mask[[1, 2]] = False
        b.set_active(mask)
        for h in (b, twin):
            h.iterate(1)
            h.sweep("forward"); h.sweep("backward")
            h.update_x(0); h.update_x(2); h.update_x(T - 1)
            h.update_A(); h.update_C(); h.update_Q(); h.update_R()
            h.iterate(2)
            h.sweep("forward")
        after, ref = _everything(b), _everything(twin)
        for k in after:
            assert np.array_equal(after[k][~mask], before[k][~mask], equal_nan=True), ("switched-off rows", k)
            assert np.array_equal(after[k][mask], ref[k][mask], equal_nan=True), ("active rows", k)
        tot = b.elbo_total()
        assert np.all(np.abs(tot - after["elbo"][mask].sum(0)) <= len(lengths) * 2.0 ** -52 * np.abs(after["elbo"][mask]).sum(0))
    finally:
        b.close(); twin.close()


@pytest.mark.parametrize("r", [1, 3])
def test_one_ill_posed_replicate_fails_alone(r):
    T, D, K = 120, 5, 7
    lengths = [120, 3, 50, 120, 2]
    Y, st0, pri = _problem(T, D, K, lengths, seed=7900)
    bad = {k: v.copy() for k, v in st0.items()}
    bad["Q_b"][r] = -np.abs(bad["Q_b"][r]) * 1e-9       # as tests/test_gpu_parity.py::test_not_positive_definite_raises
    b, twin = _batch(Y, bad, pri, lengths), _batch(Y, st0, pri, lengths)
    try:
        b.sweep("forward"); twin.sweep("forward")
        with pytest.raises(np.linalg.LinAlgError) as ei:
            b.sync()
        assert ei.value.replicates == [r], ei.value.replicates
        assert "replicate %d" % r in str(ei.value)
        twin.sync()
        mask = np.ones(len(lengths), dtype=bool); mask[r] = False
        b.set_active(mask)
        b.iterate(3); twin.iterate(3)
        b.sync()
        assert not b.status().any()
        eb, et = _everything(b), _everything(twin)
        for k in eb:
            assert np.array_equal(eb[k][mask], et[k][mask], equal_nan=True), k
    finally:
        b.close(); twin.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_nan_in_a_live_row_is_refused_and_nan_in_padding_is_not():
    from pyvb_amd import _capi
    T, D, K = 30, 4, 5
    lengths = [30, 7, 2]
    Y, st0, pri = _problem(T, D, K, lengths, seed=8000, fill=np.nan)
    b = _batch(Y, st0, pri, lengths)                    # NaN in padding only: accepted
    b.iterate(1)
    assert np.all(np.isfinite(b.elbo()))
    Ybad = Y.copy()
    Ybad[1, 6, 2] = np.nan                              # the last live row of replicate 1
    with pytest.raises(_capi.PyvbHipError) as ei:
        b.set_observations(Ybad)
    assert ei.value.code == _capi.E_UNSUPPORTED and "replicate 1" in str(ei.value), str(ei.value)
    Yok = Y.copy()
    Yok[1, 7, 2] = 5.0; Yok[2, 2:] = np.nan             # its first padding row, and replicate 2's padding
    b.set_observations(Yok)
    b.iterate(1)
    assert np.all(np.isfinite(b.elbo()))
    b.close()
