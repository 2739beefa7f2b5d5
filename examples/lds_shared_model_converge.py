#!/usr/bin/env python3
"""Several models learnt side by side on one MI355X, each fitted to its own handful of recorded series and each stopping on its
own.  A model is the graph of the reference's examples/Linear_Dynamic_System.py with `As, A, Cs, C, Q, R` built once and the loop
of :58-66 run once per series (examples/lds_shared_model.py); Network.learn's stopping test (network.py:53: the lower bound
improved by less than tol) is applied on the device to the bound of every model's graph, the sum over its series.  The series of
a model share A, C, Q, R, so they stop together; a model that has converged costs nothing from then on, and the call returns when
none is left running (examples/lds_converge_each.py does the same for models of one series each).

Four models: one with a single series, one with three, two with two, of different lengths.

    python examples/lds_shared_model_converge.py [tol [max_iters]]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

tol = float(sys.argv[1]) if len(sys.argv) > 1 else 8.0
max_iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
T, q, d = 60, 4, 5                                   # longest series, latent and observed dimension
TRIALS = ((19,), (60, 2, 33), (3, 17), (41, 25))     # lengths of the series of the four models

N = sum(len(Ts) for Ts in TRIALS)
Y, st0, pri = synth.make_problem(T, q, d, N, seed=9300)          # N simulated recordings, each with its own initial posterior
trials, n = [], 0
for Ts in TRIALS:                                    # series n, cut to its length: (Y_n[T_n, d], its initial state)
    trials.append([(Y[n + i, :Tn], {k: (v[n + i:n + i + 1, :Tn] if k == "X" else v[n + i:n + i + 1]) for k, v in st0.items()})
                   for i, Tn in enumerate(Ts)])
    n += len(Ts)

b = LDSBatch.from_trials(trials, pri)                # a model's parameters start as its first series'
iters_run = b.iterate_until_model(max_iters, tol)    # sweeps per series, A, C, Q, R per model, lower bound, stopping test per model
iters, converged, bound = b.model_convergence()      # one entry per model
chain_iters = b.convergence()[0]                     # the same, on every series of the model
total = b.elbo_total().sum()                         # the converged models count at their final bound
models = b.models                                    # int [N]: the model of every series
b.close()

print("%d series in %d models, tol = %g: %d iterations launched" % (N, len(TRIALS), tol, iters_run))
for m, Ts in enumerate(TRIALS):
    assert np.all(chain_iters[models == m] == iters[m])
    print("model %d (%d series, %3d time steps): %2d iterations, %s, lower bound %.15g"
          % (m, len(Ts), sum(Ts), iters[m], "converged" if converged[m] else "still running", bound[m]))
print("sum of the lower bounds %.15g (per model: %.15g)" % (total, np.sum(bound)))
