#!/usr/bin/env python3
"""A driven linear dynamical system on one MI355X: a plant with an actuator log.  In the reference this is
examples/Linear_Dynamic_System.py with a known input in the state equation,

    Bs = [Gaussian(q, zeros, eye * 1e-3) for i in range(p)];  B = hstack(Bs)
    Xs.append(Gaussian(q, A * Xs[-1] + B * Constant(u[t]), Q))

-- an Addition of two Multiplications as the mean parent of X_t.  Here the handle is created with the number of inputs
(LDSBatch.from_problem(..., U=U): B_prior_mean, B_prior_prec in pri, the initial B_mean, B_colvar in the state), and iterate()
updates the columns of B between those of A and C: forward, backward, As, Bs, Cs, Q, R, lower bound.

A 2-state system driven through 2 channels is recorded for 200 steps and fitted.  The states are identified up to a change of
basis, so B itself is not comparable with the simulator's; what the input does to the outputs is: the Markov parameters C B (the
response one step after a pulse) and C A B (two steps after) are printed beside the true ones; a hundred iterations bring both
within about a percent.

    python examples/lds_inputs.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 100
T, q, d, p = 200, 2, 4, 2                            # time steps, latent, observed and input dimension

system = synth.simulate_driven_lds(T, q, d, p, 1, seed=70)       # Y [1, T, d], U [1, T, p] and the true A, B, C
Y, U = system["Y"], system["U"]
_, _, st0, pri = synth.make_input_problem(T, q, d, p, 1, seed=71)    # priors of the example, an initial state drawn as the constructors do

b = LDSBatch.from_problem(Y, st0, pri, U=U)
b.iterate(niters)                                    # forward, backward, A, B, C, Q, R, lower bound
parts = b.elbo()
st = b.get_state(("A_mean", "C_mean"))
b.close()

A, B, C = st["A_mean"][0], st["B_mean"][0], st["C_mean"][0]
print("fitted %d states, %d inputs to %d time steps, %d iterations  lower bound %.15g" % (q, p, T, niters, parts.sum()))
for name, got, true in (("C B", C @ B, system["C"][0] @ system["B"][0]), ("C A B", C @ A @ B, system["C"][0] @ system["A"][0] @ system["B"][0])):
    print("%-5s fitted:" % name, " ".join("%.6e" % v for v in got.ravel()))
    print("%-5s true  :" % name, " ".join("%.6e" % v for v in true.ravel()))
    print("%-5s relative error %.3e" % (name, np.abs(got - true).max() / np.abs(true).max()))
