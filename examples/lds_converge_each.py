#!/usr/bin/env python3
"""Several data sets learnt side by side on one MI355X, each stopping on its own: every replicate of the handle is its own
linear dynamical system (the graph of the reference's examples/Linear_Dynamic_System.py:46-66) and applies Network.learn's
stopping test (network.py:53: the lower bound improved by less than tol) to itself, on the device.  A data set that has
converged costs nothing from then on; the call returns when none is left running.

    python examples/lds_converge_each.py [tol [max_iters]]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

tol = float(sys.argv[1]) if len(sys.argv) > 1 else 2.0
max_iters = int(sys.argv[2]) if len(sys.argv) > 2 else 40
T, q, d, N = 30, 4, 5, 6                             # time steps, latent and observed dimension, data sets

Y, st0, pri = synth.make_problem(T, q, d, N, seed=8100)          # N simulated recordings, each with its own initial posterior
b = LDSBatch.from_problem(Y, st0, pri)
iters_run = b.iterate_until(max_iters, tol)          # forward sweep, backward sweep, A, C, Q, R, lower bound, stopping test
iters, converged, bound = b.convergence()
total = b.elbo_total().sum()                         # the converged data sets count at their final bound
b.close()

print("%d data sets, tol = %g: %d iterations launched" % (N, tol, iters_run))
for n in range(N):
    print("data set %d: %2d iterations, %s, lower bound %.15g"
          % (n, iters[n], "converged" if converged[n] else "still running", bound[n]))
print("sum of the lower bounds %.15g (per data set: %.15g)" % (total, np.sum(bound)))
