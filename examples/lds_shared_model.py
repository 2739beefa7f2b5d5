#!/usr/bin/env python3
"""One linear dynamical system fitted to several recorded series (trials, sessions, subjects) on one MI355X.  In the reference
this is examples/Linear_Dynamic_System.py with `As, A, Cs, C, Q, R` built once and the loop of :58-66 run once per series,
each with its own X_0.  Here every series is a chain of one handle, and the chains of a model share A, C, Q, R
(LDSBatch.from_trials): before the parameters are updated the statistics of a model's chains are summed on the device.

Two systems are recorded, five trials of different lengths of the first and three of the second; each system gets one model.

    python examples/lds_shared_model.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
q, d = 2, 5                                          # latent and observed dimension
TRIALS = ((120, 75, 40, 12, 3), (90, 60, 2))         # lengths of the trials of the two systems


def record(system, T, rng):
    """One trial of T steps of a system (Linear_Dynamic_System.py:40-44)."""
    A, C, Q, R = (system[k][0] for k in ("A", "C", "Q", "R"))
    x, Y = rng.standard_normal(q), np.empty((T, d))
    for t in range(T):
        if t > 0:
            x = A @ x + np.sqrt(Q) * rng.standard_normal(q)
        Y[t] = C @ x + np.sqrt(R) * rng.standard_normal(d)
    return Y


systems = [synth.simulate_lds(2, q, d, 1, seed=80 + m) for m in range(len(TRIALS))]      # (only their parameters are used)
rng = np.random.default_rng(90)
trials = [[(record(systems[m], T, rng), synth.initial_state(T, q, d, 1, seed=100 + 10 * m + n)) for n, T in enumerate(Ts)]
          for m, Ts in enumerate(TRIALS)]

b = LDSBatch.from_trials(trials, synth.default_priors(q, d))     # pads to the longest trial; a model's parameters start as its first trial's
b.iterate(niters)                                    # sweeps per chain, A, C, Q, R per model, lower bound
parts = b.elbo()                                     # [chains, 6]: the rows of a model add up to the bound of its graph
state = b.get_state(("R_a", "R_b"))
b.close()

print("storage: %d chains x %d time steps; chain lengths %s; models %s" % (b.N, b.T, b.lengths.tolist(), b.models.tolist()))
for m, Ts in enumerate(TRIALS):
    rows = np.nonzero(b.models == m)[0]
    print("model %d: %d trials, %3d time steps in all  lower bound %.15g" % (m, len(Ts), sum(Ts), parts[rows].sum()))
    first = rows[0]                                  # every row of a model holds the model's parameters
    print("model %d, observation noise precision, learnt :" % m, np.round(state["R_a"][first] / state["R_b"][first], 1))
    print("model %d, observation noise precision, true   :" % m, np.round(1.0 / systems[m]["R"][0], 1))
