"""GPU: the two boundary nodes of a sweep, X_0 and X_{T-1} (pyvb_amd/csrc/k_sweep.hip: boundary_update).

Their three matrix-vector chains fetch the matrix in blocks of 16 rows from clamped places, with zero selected outside D / K,
and get the wave-uniform factors (the neighbour's mean, y, the noise diagonals) through LDS.  The shapes below are the smallest
at which the clamping, the padding of a block, the skipping of whole blocks and the hand-off can go wrong: D = K = 1, one
dimension padded and the other not, K > D and D > K, every tile count, no interior node, the opening boundary computed by
several wavefronts.  The comparator is the oracle (oracle/lds_closed_form.py) after a forward and after a backward
pyvb_lds_sweep: rows 0 and T - 1 on their own, then the whole state; the tolerance is the state tolerance of
tests/test_gpu_parity.py.  Replicates share no arithmetic and a handle's launches are deterministic, so where two calls run the
same instructions on the same inputs the comparison is np.array_equal.
"""
import numpy as np
import pytest

from oracle import lds_closed_form as O
from pyvb_amd import synth
from test_gpu_parity import RTOL, _close, _wishart_priors

pytestmark = pytest.mark.gpu


def _batch(Y, st0, pri, lengths=None):
    from pyvb_amd.lds import LDSBatch
    return LDSBatch.from_problem(Y, st0, pri, lengths=None if lengths is None else np.asarray(lengths, dtype=np.int32))


def _both_sweeps(Y, st0, pri, tag):
    """Forward then backward on the handle and in the oracle; the boundary rows and the state after each."""
    T = Y.shape[1]
    b = _batch(Y, st0, pri)
    st = O.expand_state(st0, pri, T)
    post = O.state_posteriors(st, pri)
    for direction in ("forward", "backward"):
        O.sweep(st, pri, Y, direction, post)
        b.sweep(direction)
        X = b.get_state(("X",))["X"]
        what = "%s, %s sweep: " % (tag, direction)
        _close(X[:, 0], st["X"][:, 0], what + "row 0", RTOL)
        _close(X[:, T - 1], st["X"][:, T - 1], what + "row T - 1", RTOL)
        _close(X, st["X"], what + "X", RTOL)
    return b


@pytest.mark.parametrize("T,D,K,N", [(2, 3, 2, 2), (3, 1, 1, 1), (5, 17, 33, 2), (6, 64, 64, 2), (9, 48, 16, 3), (20, 64, 33, 1),
                                     (600, 6, 4, 1)])
def test_boundary_rows_vs_oracle(T, D, K, N):
    """No interior node; D = K = 1; padding in both dimensions with K > D; no padding; padding with whole blocks past D;
    padding with D > K; the time axis split over several wavefronts (the opening boundary is computed by more than one
    wavefront and stored by the first)."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4100 + T + D)
    b = _both_sweeps(Y, st0, pri, "T=%d D=%d K=%d" % (T, D, K))
    if T == 600:
        assert b.get_time_split() > 1, b.get_time_split()
    b.close()


@pytest.mark.parametrize("T,D,K,N,proper", [(6, 5, 6, 2, False), (8, 33, 17, 1, True)])
def test_boundary_rows_with_wishart_noise(T, D, K, N, proper):
    """The dense branch: <Q><A> and <R><C> take the place of the scaled rows of <A> and <C>."""
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4300 + T + D)
    _wishart_priors(pri, D, K, np.random.default_rng(T) if proper else None)
    _both_sweeps(Y, st0, pri, "Wishart T=%d D=%d K=%d" % (T, D, K)).close()


def test_boundary_rows_with_chain_lengths():
    """T_n = 2, 3 and T on one handle: the closing boundary of replicate n sits at T_n - 1.  Every replicate against the same
    model on its own in the oracle."""
    T, D, K, lengths = 12, 17, 9, [2, 3, 12]
    N = len(lengths)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4500)
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    Y = np.where(live[:, :, None], Y, 0.0)
    st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
    b = _batch(Y, st0, pri, lengths)
    sts = []
    for n, Tn in enumerate(lengths):
        sn = {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]).copy() for k, v in st0.items()}
        sts.append(O.expand_state(sn, pri, Tn))
    for direction in ("forward", "backward"):
        b.sweep(direction)
        X = b.get_state(("X",))["X"]
        for n, Tn in enumerate(lengths):
            O.sweep(sts[n], pri, Y[n:n + 1, :Tn], direction)
            what = "replicate %d (T_n = %d), %s sweep: " % (n, Tn, direction)
            _close(X[n, 0], sts[n]["X"][0, 0], what + "row 0", RTOL)
            _close(X[n, Tn - 1], sts[n]["X"][0, Tn - 1], what + "row T_n - 1", RTOL)
            _close(X[n, :Tn], sts[n]["X"][0], what + "X", RTOL)
            assert np.array_equal(X[n, Tn:], np.zeros_like(X[n, Tn:])), what + "padding rows"
    b.close()


def test_switched_off_replicate_keeps_its_boundary_rows():
    T, D, K, N = 5, 17, 33, 3
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4600)
    b = _batch(Y, st0, pri)
    b.sweep("forward")
    before = b.get_state(("X",))["X"].copy()
    b.set_active(np.array([True, False, True]))
    for direction in ("backward", "forward"):
        b.sweep(direction)
        X = b.get_state(("X",))["X"]
        assert np.array_equal(X[1, 0], before[1, 0]) and np.array_equal(X[1, T - 1], before[1, T - 1]), direction
        assert np.array_equal(X[1], before[1]), direction
        assert not np.array_equal(X[0], before[0]) and not np.array_equal(X[2], before[2]), direction      # the others did move
    b.close()


def test_single_boundary_updates_equal_the_sweep_bitwise():
    """update_x(0) and update_x(T - 1) (k_step) run the chains of the sweep's boundary nodes: the same bits, given the
    neighbour the sweep saw -- the old one at the opening boundary, the sweep's own new one at the closing boundary."""
    T, D, K, N = 5, 17, 33, 2
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=4700)
    a, b = _batch(Y, st0, pri), _batch(Y, st0, pri)
    a.sweep("forward")
    Xa = a.get_state(("X",))["X"]
    b.update_x(0)                           # neighbour: the initial X_1, as in the sweep
    assert np.array_equal(b.get_state(("X",))["X"][:, 0], Xa[:, 0])
    b.set_state(X=Xa)
    b.update_x(T - 1)                       # neighbour: the sweep's new X_{T-2}
    assert np.array_equal(b.get_state(("X",))["X"], Xa)
    a.sweep("backward")
    Xb = a.get_state(("X",))["X"]
    b.update_x(T - 1)                       # neighbour: X_{T-2} of the forward sweep
    assert np.array_equal(b.get_state(("X",))["X"][:, T - 1], Xb[:, T - 1])
    b.set_state(X=Xb)
    b.update_x(0)
    assert np.array_equal(b.get_state(("X",))["X"], Xb)
    a.close(); b.close()
