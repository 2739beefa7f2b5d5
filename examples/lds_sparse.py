#!/usr/bin/env python3
"""Sparse transition matrices on one MI355X: which state drives which, inferred from the recording.  In the reference this is
examples/Linear_Dynamic_System.py with a DiagonalGamma node as the precision parent of every column of A,
`Gaussian(D, pmu, DiagonalGamma(D, a0, b0))` (gaussian.py:55-61; nodes_todo.py:159-204): entry (k, i) of A has the prior
N(0, alpha[i][k]^-1) with a precision of its own, and an entry the data do not need is driven to zero while its <alpha> grows --
a Gamma node per column (examples/lds_ard.py) can only switch whole columns off.  Here the handle takes the hyperpriors with the
other priors (LDSBatch.from_problem: A_entry_a0, A_entry_b0 in pri, [column][row] as A_prior_prec is, and the initial A_entry_b in
the state), and iterate() updates the precision nodes after Q and R.

A system whose A is banded (every state is driven by itself and its two neighbours) is recorded through an identity-like C and
fitted.  Pruning is slow: expect <alpha> of the entries off the band to grow by orders of magnitude over a few hundred iterations,
not in thirty.

    python examples/lds_sparse.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

T, D, d = 200, 5, 8                                  # time steps, states, observed dimension


def make_inputs():
    """(Y [1, T, d], st0, pri, the true A): a banded system, broad Gamma priors on every entry's precision, qb as rand()."""
    rng = np.random.default_rng(70)
    A = np.zeros((D, D))
    for k in range(D):
        for i in range(max(0, k - 1), min(D, k + 2)):
            A[k, i] = 0.6 if i == k else 0.25 * (1 if i > k else -1)
    C = np.vstack([np.eye(D), 0.5 * rng.standard_normal((d - D, D))])
    Y = np.empty((1, T, d))
    x = rng.standard_normal(D)
    for t in range(T):
        if t > 0:
            x = A @ x + np.sqrt(0.1) * rng.standard_normal(D)
        Y[0, t] = C @ x + np.sqrt(0.05) * rng.standard_normal(d)
    pri = synth.default_priors(D, d)
    st0 = synth.initial_state(T, D, d, 1, seed=71)
    pri["A_entry_a0"], pri["A_entry_b0"] = np.full((D, D), 1e-3), np.full((D, D), 1e-3)
    st0["A_entry_b"] = 0.5 + rng.random((1, D, D))
    return Y, st0, pri, A


if __name__ == "__main__":
    niters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    Y, st0, pri, A_true = make_inputs()
    b = LDSBatch.from_problem(Y, st0, pri)
    b.iterate(niters)                                # forward, backward, A, C, Q, R, the precisions of A's entries, lower bound
    parts = b.elbo()
    A_mean = b.get_state(("A_mean",))["A_mean"][0]
    qa, qb = b.entry_precisions()["A"]
    b.close()

    print("fitted %d states to %d time steps of a banded system, %d iterations  lower bound %.15g" % (D, T, niters, parts.sum()))
    E = (qa / qb)[0].T                               # [row][column], as A is read
    for k in range(D):
        print("<alpha> row %d:" % k, " ".join("%.6e" % v for v in E[k]))
    for k in range(D):
        print("<A> row %d    :" % k, " ".join("% .6e" % v for v in A_mean[k]))
    print("band of the true A (up to a relabelling of the states):")
    for k in range(D):
        print("              ", " ".join("x" if A_true[k, i] != 0.0 else "." for i in range(D)))
