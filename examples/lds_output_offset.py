#!/usr/bin/env python3
"""Recordings that are not zero-mean, on one MI355X: an output offset as a known regressor.  In the reference this is
examples/Linear_Dynamic_System.py with a constant in the output equation,

    Es = [Gaussian(d, zeros, eye * 1e-3)];  E = hstack(Es)
    Ys.append(Gaussian(d, C * Xs[-1] + E * Constant(ones((1, 1))), R))

-- an Addition of two Multiplications as the mean parent of Y_t.  Here the handle is created with the number of regressors
(LDSBatch.from_problem(..., V=V): E_prior_mean, E_prior_prec in pri, the initial E_mean, E_colvar in the state), and iterate()
updates the columns of E behind those of C: forward, backward, As, Cs, Es, Q, R, lower bound.

Three series of 400 steps from 2-state systems are recorded with an offset of its own on each of the 4 channels and fitted twice:
with regressors=1 and V = 1, and as they are, without.  Pre-centring the data would bias the bound; the regressor does not.  The
column of E, started at the channel means, is printed beside the true offsets, and the lower bound of each series beside that of
the fit without the regressor, which has to explain the offset through the states.

    python examples/lds_output_offset.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 60
T, q, d, n = 400, 2, 4, 3                            # time steps, latent and observed dimension, series

offset = 20.0 * np.random.default_rng(80).standard_normal((n, d))         # the mean of every channel of every series
Y = synth.simulate_lds(T, q, d, n, seed=81)["Y"] + offset[:, None, :]
V = np.ones((n, T, 1))
_, _, _, st0, pri = synth.make_regression_problem(T, q, d, 0, 1, n, seed=82)    # priors of the example, an initial state drawn as the constructors do
# ... but for E, which starts at the channel means: from a random E the states, updated first, take the offset for a slow mode of
# theirs (the fixed point that pre-centring avoids and the regressor, started there, does not enter)
st0["E_mean"] = Y.mean(axis=1)[:, :, None]

b = LDSBatch.from_problem(Y, st0, pri, V=V)
b.iterate(niters)                                    # forward, backward, A, C, E, Q, R, lower bound
with_offset = b.elbo().sum(1)
E = b.get_regressor_state(("E_mean",))["E_mean"][:, :, 0]
b.close()

plain = LDSBatch.from_problem(Y, {k: v for k, v in st0.items() if not k.startswith("E_")}, pri)
plain.iterate(niters)
without = plain.elbo().sum(1)
plain.close()

print("fitted %d series of %d time steps, %d iterations" % (n, T, niters))
for i in range(n):
    print("series %d offset fitted:" % i, " ".join("%.6e" % v for v in E[i]))
    print("series %d offset true  :" % i, " ".join("%.6e" % v for v in offset[i]))
    print("series %d lower bound with the regressor %.15g without %.15g" % (i, with_offset[i], without[i]))
print("largest error of an offset %.3e of the largest offset" % (np.abs(E - offset).max() / np.abs(offset).max()))
