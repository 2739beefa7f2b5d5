"""The parameter tail of an iteration (k_moments, k_cols: columns of A and C, residuals, noise update) on the smallest shapes
that reach each branch of the 64-wide column kernel: full tiles, padded rows with the trace over the wavefront, a single
partial tile, known entries, column ranges that start and end inside a block of 16, a switched-off replicate, and the
handles that reduce their moments over chunks, parts of the time axis or the chains of a model.

Every case is compared with oracle/lds_closed_form.py stage by stage at the suite's RTOL (tests/test_gpu_parity.py), and the
fused launch of iterate() with the stage-wise update_A / update_C / update_Q / update_R.

The warm-up lengths that get_warmup() reports are held to the rule itself on the inputs of the
accuracy envelope: J is what tests/extended_ref.py: warmup_rule gives for the recurrence matrices of the reference run."""
import numpy as np
import pytest

import extended_ref as E
import test_envelope_gpu as EV
import test_gpu_parity as P
import test_tied_gpu as TG
from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu

KEYS = ("X", "A_mean", "C_mean", "A_colvar", "C_colvar", "Q_a", "Q_b", "R_a", "R_b")


def _staged(b, iters):
    for _ in range(iters):
        b.sweep("forward"); b.sweep("backward"); b.update_A(); b.update_C(); b.update_Q(); b.update_R()


def _iterate_equals_staged(Y, st0, pri, iters=2, prepare=None):
    """iterate() (columns, residuals and noise of A / Q and C / R in one launch) against the staged calls: the same
    arithmetic in the same order, so bit for bit."""
    a, b = P._batch(Y, st0, pri), P._batch(Y, st0, pri)
    try:
        if prepare:
            prepare(a); prepare(b)
        a.iterate(iters)
        _staged(b, iters)
        ga, gb = a.get_state(), b.get_state()
        for k in KEYS:
            assert np.array_equal(ga[k], gb[k]), k
        for x, y in zip(a.get_column_qld(), b.get_column_qld()):
            assert np.array_equal(x, y, equal_nan=True)
        assert np.array_equal(a.elbo(), b.elbo())
    finally:
        a.close(); b.close()


def _gamma(pri):
    pri["noise"] = "gamma"
    for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
        pri[k] = np.float64(1e-3)


@pytest.mark.parametrize("T,D,K,N,kind", [(40, 64, 64, 3, "diagonal_gamma"),     # full tiles
                                          (30, 33, 17, 2, "gamma"),              # padded rows and columns, wave_sum
                                          (19, 6, 4, 2, "diagonal_gamma")])      # one partial tile
def test_shapes_vs_oracle_and_iterate(T, D, K, N, kind):
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7100 + D)
    if kind == "gamma":
        _gamma(pri)
    P._stagewise(Y, st0, pri, iters=2)
    _iterate_equals_staged(Y, st0, pri)


def test_known_entries_and_a_fully_known_column():
    T, D, K, N = 24, 20, 9, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7201)
    A_obs = np.full((D, D), np.nan); C_obs = np.full((K, D), np.nan)
    A_obs[0, 0] = 1.0; A_obs[3, 2] = -0.5; A_obs[19, 15] = 0.25; A_obs[7, 16] = 1e-2      # both sides of a block border
    A_obs[:, 17] = np.linspace(-0.2, 0.2, D)                                                # a column that is never updated
    C_obs[2, 1] = 3.0; C_obs[:, 18] = np.arange(K) - 2.0
    pri["A_obs"], pri["C_obs"] = A_obs, C_obs
    P._stagewise(Y, st0, pri, iters=2)
    _iterate_equals_staged(Y, st0, pri)


def test_column_ranges_inside_and_across_blocks():
    """pyvb_lds_update_columns on (5, 23) -- starts and ends inside a block -- and (16, 32) -- exactly one block -- against
    the oracle's column loop over the same ranges; then Q and R from the result."""
    T, D, K, N = 20, 40, 33, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7301)
    b = P._batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    O.sweep(st, pri, Y, "forward"); b.sweep("forward")
    O.sweep(st, pri, Y, "backward"); b.sweep("backward")
    S = O.statistics(st, Y)
    for which, lo, hi in [("A", 5, 23), ("C", 16, 32), ("C", 5, 23), ("A", 16, 32)]:
        (O.update_A if which == "A" else O.update_C)(st, pri, S, cols=(lo, hi))
        b.update_columns(which, lo, hi)
        g = b.get_state()
        P._close(g["A_mean"], st["A_mean"], "A_mean after %s[%d:%d]" % (which, lo, hi))
        P._close(g["C_mean"], st["C_mean"], "C_mean after %s[%d:%d]" % (which, lo, hi))
        P._close(g["A_colvar"], np.einsum("nikk->nik", st["A_cov"]), "A_colvar after %s[%d:%d]" % (which, lo, hi))
        P._close(g["C_colvar"], np.einsum("nikk->nik", st["C_cov"]), "C_colvar after %s[%d:%d]" % (which, lo, hi))
    O.update_Q(st, pri, S, T); b.update_Q()
    O.update_R(st, pri, S, T); b.update_R()
    P._compare_params(b, st, "after the column ranges: ")
    b.close()


def test_a_switched_off_replicate_keeps_its_rows():
    T, D, K, N = 30, 33, 17, 3
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7401)
    b, twin = P._batch(Y, st0, pri), P._batch(Y, st0, pri)
    try:
        b.iterate(1); twin.iterate(1)
        before = b.get_state()
        qld_before = b.get_column_qld()
        mask = np.array([True, False, True])
        b.set_active(mask)
        b.iterate(1); _staged(b, 1)
        twin.iterate(1); _staged(twin, 1)
        after, ref = b.get_state(), twin.get_state()
        for k in KEYS:
            assert np.array_equal(after[k][~mask], before[k][~mask]), "switched-off row changed: " + k
            assert np.array_equal(after[k][mask], ref[k][mask]), "active rows differ from the unmasked twin: " + k
        for x, y in zip(b.get_column_qld(), qld_before):
            assert np.array_equal(x[~mask], y[~mask])
    finally:
        b.close(); twin.close()


def test_a_tied_handle_of_two_chains():
    lengths, models = [30, 17], [0, 0]
    Y, st0, pri = TG._problem(7501, lengths=lengths, T=30, D=33, K=17)
    TG._stagewise(Y, st0, pri, lengths, models, iters=2)
    a, b = TG._batch(Y, st0, pri, lengths, models), TG._batch(Y, st0, pri, lengths, models)
    try:
        a.iterate(2)
        _staged(b, 2)
        ga, gb = a.get_state(), b.get_state()
        for k in KEYS:
            assert np.array_equal(ga[k], gb[k]), k
        for x, y in zip(a.get_column_qld(), b.get_column_qld()):
            assert np.array_equal(x, y, equal_nan=True)
        assert np.array_equal(a.elbo(), b.elbo())
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("T,D,K,N", [(100, 64, 33, 2),
                                     (51, 33, 17, 2)])      # 49 interior nodes in parts of 32: the third part holds no node
def test_time_split_into_three_parts(T, D, K, N):
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7601)

    def split(b):
        b.set_time_split(3)
        assert b.get_time_split() == 3

    b = P._batch(Y, st0, pri)
    split(b)
    st = O.expand_state(st0, pri, T)
    for it in range(2):
        parts = O.iterate(st, pri, Y)
        b.iterate(1)
    P._compare_params(b, st, "set_time_split(3): ")
    P._close(b.elbo().sum(1), parts.sum(1), "elbo after iterate, set_time_split(3)")
    b.close()
    _iterate_equals_staged(Y, st0, pri, prepare=split)


def test_default_time_split_matches_the_recorded_table():
    """The time split a handle picks for itself is the one tests/test_geometry_cpu.py holds geometry.h to: the same literal table
    (the shapes up to T = 4099; no data is needed to ask)."""
    from test_geometry_cpu import LDS_TABLE
    from pyvb_amd.lds import LDSBatch
    got = {}
    for (N, T, D, K) in LDS_TABLE:
        if T <= 4099:
            b = LDSBatch(N, T, D, K)
            got[(N, T, D, K)] = b.get_time_split()
            b.close()
    assert len(got) == 16 and got == {s: LDS_TABLE[s][1] for s in got}


def test_moments_reduced_over_chunks():
    """N = 2, T = 700: the statistics come in several chunks per replicate, which k_moments adds up."""
    T, D, K, N = 700, 16, 16, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=7701)
    P._stagewise(Y, st0, pri, iters=1)
    _iterate_equals_staged(Y, st0, pri)



@pytest.mark.parametrize("name", E.WARMUP_CASES)
def test_warmup_lengths_follow_the_rule(name):
    """J of get_warmup() after every iteration's sweeps equals warmup_rule() of the recurrence matrices F (inf-norm,
    forward) and B (1-norm, backward) of the envelope's reference run of the case (the handle's run and the reference are the
    envelope's own, shared with tests/test_envelope_gpu.py)."""
    _, warm = EV._run_handle(name)
    runs = E.lds_reference(name)
    per_replicate = runs[0][0] is not None
    bad = []
    for it, w in enumerate(warm):
        for n in range(w.shape[0]):
            F, B = (m[0] for m in runs[n][5][it]) if per_replicate else (m[n] for m in runs[0][5][it])
            for M, which, J, what in ((F, "inf", int(w[n, 0]), "forward"), (B, "1", int(w[n, 1]), "backward")):
                Jstar = E.warmup_rule(M, which)
                print("%-28s it%d replicate %d %-8s J %4d  rule %4d%s" % (name, it, n, what, J, Jstar, "" if J == Jstar else "  <-- differs"))
                if J != Jstar:
                    bad.append((it, n, what, J, Jstar))
    assert not bad, "%s: (iteration, replicate, sweep, J, rule) %r" % (name, bad)
