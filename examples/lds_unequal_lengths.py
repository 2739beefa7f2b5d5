#!/usr/bin/env python3
"""Time series of different lengths learnt side by side on one MI355X: every series is its own linear dynamical system (the
graph of the reference's examples/Linear_Dynamic_System.py:46-66 with its own number of time steps), and all of them share one
handle, so an iteration over the whole collection is a handful of kernel launches.

    python examples/lds_unequal_lengths.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 30
q, d = 2, 5                                          # latent and observed dimension
LENGTHS = (200, 120, 75, 40, 12)

# one simulated recording per length, each with its own random initial posterior
sims = [synth.simulate_lds(T, q, d, 1, seed=30 + n) for n, T in enumerate(LENGTHS)]
series = [(sim["Y"][0], synth.initial_state(T, q, d, 1, seed=60 + n)) for n, (sim, T) in enumerate(zip(sims, LENGTHS))]

b = LDSBatch.from_series(series, synth.default_priors(q, d))     # pads to the longest, remembers every length
b.iterate(niters)                                    # forward sweep, backward sweep, A, C, Q, R, lower bound: all series at once
bound = b.elbo().sum(axis=1)
state = b.get_state(("C_mean", "R_a", "R_b"))
b.close()

print("storage: %d series x %d time steps; chain lengths %s" % (b.N, b.T, list(b.lengths)))
for n, T in enumerate(LENGTHS):
    print("series %d: T = %3d  lower bound %.15g" % (n, T, bound[n]))
n = 0
print("series 0, observation noise precision, learnt :", np.round(state["R_a"][n] / state["R_b"][n], 1))
print("series 0, observation noise precision, true   :", np.round(1.0 / sims[n]["R"][0], 1))
