#!/usr/bin/env python3
"""Automatic relevance determination for VB-PCA on one MI355X: the latent dimension inferred, not guessed (Bishop's variational
PCA).  In the reference this is examples/PCA_missing_data.py with a Gamma node as the precision parent of every column of W,
`Ws = [Gaussian(d, zeros, Gamma(d, a0, b0)) for i in range(q)]` (gaussian.py:55-61): column i has the prior N(0, alpha_i^-1 I),
and a column the data do not need is driven to zero while its <alpha_i> grows.  Here the handle takes the hyperpriors with the
other priors (PCABatch.from_problem: pri["W_alpha"] = (a0, b0, qb)) and iterate() updates the alpha nodes in every pass.

Rank-2 data in d = 10 dimensions, a tenth of the entries missing, fitted with a generous q = 6.  Pruning takes a few hundred
iterations, and how many of the four spare columns have reached norm 0 by then depends on the seed; the others are still shrinking.

    python examples/pca_ard.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd.pca import PCABatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
N, d, q_true, q = 200, 10, 2, 6                      # rows, observed dimension, true and fitted latent dimension

rng = np.random.default_rng(70)
X = rng.standard_normal((N, q_true)) @ rng.standard_normal((d, q_true)).T + rng.standard_normal(d) \
    + rng.standard_normal((N, d)) / np.sqrt(50.0)
obs = rng.random((N, d)) > 0.1
init = {"obs": obs, "X": np.where(obs, X, 0.0),     # data; the missing entries start at 0
        "W_mean": rng.standard_normal((d, q)), "Z": rng.standard_normal((N, q)), "Z_cov": np.eye(q),
        "Mu_mean": np.zeros(d), "beta_b": 1.0}
pri = {"W_prior_mean": np.zeros((d, q)), "W_prior_prec": np.ones((q, d)),       # the precisions are replaced by <alpha_i>
       "Mu_prior_mean": np.zeros(d), "Mu_prior_prec": np.full(d, 1e-3), "beta_a0": 1e-3, "beta_b0": 1e-3,
       # broad Gamma priors on every column's precision; qb as the reference's rand()
       "W_alpha": (1e-3, 1e-3, 0.5 + rng.random(q))}

b = PCABatch.from_problem(init, pri)
b.iterate(niters)                                    # W, Z, alpha, X_0, Mu, X_1.., Beta, lower bound
parts = b.elbo()
state = b.get_state()
qa, qb = b.column_precisions()
b.close()

print("fitted q = %d to %d rows of rank-%d data in d = %d, %d iterations  lower bound %.15g" % (q, N, q_true, d, niters, parts.sum()))
print("<alpha>         :", " ".join("%.6e" % v for v in qa / qb))
print("column norms of W:", " ".join("%.6e" % v for v in np.sqrt((state["W_mean"] ** 2).sum(0))))
print("noise precision  : %.6g (true: 50)" % (state["beta_a"] / state["beta_b"]))
