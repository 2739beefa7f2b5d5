#!/usr/bin/env python3
"""Automatic relevance determination on one MI355X: the state dimension of a linear dynamical system inferred, not guessed.  In
the reference this is examples/Linear_Dynamic_System.py with a Gamma node as the precision parent of every column of A and C,
`Gaussian(q, pmu, Gamma(q, a0, b0))` (gaussian.py:55-61): column i has the prior N(0, alpha_i^-1 I), and a column the data do not
need is driven to zero while its <alpha_i> grows.  Here the handle takes the hyperpriors with the other priors
(LDSBatch.from_problem: A_alpha_a0, A_alpha_b0, C_alpha_a0, C_alpha_b0 in pri, the initial A_alpha_b, C_alpha_b in the state), and
iterate() updates the alpha nodes after Q and R.

A system with 2 states is recorded and fitted with a generous D = 5.  Pruning is slow: expect the superfluous columns of C to
shrink by orders of magnitude over a few hundred iterations, not to vanish in thirty.

    python examples/lds_ard.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 120
T, q_true, D, d = 150, 2, 5, 5                       # time steps, true and fitted latent dimension, observed dimension

system = synth.simulate_lds(T, q_true, d, 1, seed=60)        # Y [1, T, d] of a 2-state system
Y = system["Y"]
pri = synth.default_priors(D, d)
st0 = synth.initial_state(T, D, d, 1, seed=61)
rng = np.random.default_rng(62)
for w in ("A", "C"):                                  # broad Gamma priors on every column's precision; qb as the reference's rand()
    pri[w + "_alpha_a0"], pri[w + "_alpha_b0"] = np.full(D, 1e-3), np.full(D, 1e-3)
    st0[w + "_alpha_b"] = 0.5 + rng.random((1, D))

b = LDSBatch.from_problem(Y, st0, pri)
b.iterate(niters)                                    # forward, backward, A, C, Q, R, alpha_A, alpha_C, lower bound
parts = b.elbo()
state = b.get_state(("A_mean", "C_mean"))
alpha = b.column_precisions()
b.close()

print("fitted D = %d to %d time steps of a %d-state system, %d iterations  lower bound %.15g" % (D, T, q_true, niters, parts.sum()))
for w, M in (("A", state["A_mean"][0]), ("C", state["C_mean"][0])):
    qa, qb = alpha[w]
    print("<alpha_%s>       :" % w, " ".join("%.6e" % v for v in (qa / qb)[0]))
    print("column norms of %s:" % w, " ".join("%.6e" % v for v in np.sqrt((M ** 2).sum(0))))
