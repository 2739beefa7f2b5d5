#!/usr/bin/env python3
"""Sparse loadings for VB-PCA on one MI355X: a precision for every entry of W (sparse Bayesian PCA / sparse factor analysis).
In the reference this is examples/PCA_missing_data.py with a DiagonalGamma node as the precision parent of every column of W,
`Ws = [Gaussian(d, zeros, DiagonalGamma(d, a0, b0)) for i in range(q)]` (gaussian.py:55-61, nodes_todo.py:159-204): entry
W[k][i] has the prior N(0, 1 / gamma_ik), and an entry the data do not need is driven to zero while its <gamma_ik> grows.  Here
the handle takes the hyperpriors with the other priors (PCABatch.from_problem: pri["W_entry"] = (a0, b0, qb)) and iterate()
updates the parents in every pass.

Data in d = 12 dimensions from q = 3 factors, each of which loads on four of the dimensions only; a tenth of the entries missing.
The likelihood does not tell a set of loadings from a rotation of it; the prior on the entries does, and it works slowly:
pruning takes hundreds of iterations, and how far the entries outside the true support have shrunk by then depends on the seed.
The script prints the loadings it found and the share of their squared weight that lies on the true support.

    python examples/pca_sparse.py [iterations]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyvb_amd.pca import PCABatch

niters = int(sys.argv[1]) if len(sys.argv) > 1 else 300
N, d, q = 300, 12, 3                                 # rows, observed dimension, factors

rng = np.random.default_rng(71)
support = np.zeros((d, q), dtype=bool)
for i in range(q):
    support[4 * i:4 * i + 4, i] = True               # factor i loads on dimensions 4 i .. 4 i + 3
W_true = np.where(support, rng.uniform(1.0, 2.0, (d, q)) * rng.choice([-1.0, 1.0], (d, q)), 0.0)
X = rng.standard_normal((N, q)) @ W_true.T + rng.standard_normal(d) + rng.standard_normal((N, d)) / np.sqrt(50.0)
obs = rng.random((N, d)) > 0.1
init = {"obs": obs, "X": np.where(obs, X, 0.0),     # data; the missing entries start at 0
        "W_mean": rng.standard_normal((d, q)), "Z": rng.standard_normal((N, q)), "Z_cov": np.eye(q),
        "Mu_mean": np.zeros(d), "beta_b": 1.0}
pri = {"W_prior_mean": np.zeros((d, q)), "W_prior_prec": np.ones((q, d)),       # the precisions are replaced by <gamma_ik>
       "Mu_prior_mean": np.zeros(d), "Mu_prior_prec": np.full(d, 1e-3), "beta_a0": 1e-3, "beta_b0": 1e-3,
       # broad Gamma priors on every entry's precision; qb as the reference's rand()
       "W_entry": (1e-3, 1e-3, 0.5 + rng.random((q, d)))}

b = PCABatch.from_problem(init, pri)
b.iterate(niters)                                    # W, Z, the parents, X_0, Mu, X_1.., Beta, lower bound
parts = b.elbo()
state = b.get_state()
qa, qb = b.entry_precisions()
b.close()

W = state["W_mean"]
print("fitted %d factors to %d rows in d = %d, %d iterations  lower bound %.15g" % (q, N, d, niters, parts.sum()))
print("loadings <W> (rows = dimensions):")
for k in range(d):
    print("   " + " ".join("% .4f" % v for v in W[k]))
# which fitted column is which factor is not identified: match every fitted column to the factor it overlaps most
sq = W ** 2
owner = [int(np.argmax([sq[support[:, j], i].sum() for j in range(q)])) for i in range(q)]
on = sum(sq[support[:, owner[i]], i].sum() for i in range(q))
print("squared loadings   :", " ".join("%.6e" % v for v in sq.sum(0)))
print("<gamma> range      : %.6e %.6e" % ((qa / qb).min(), (qa / qb).max()))
print("weight on support  : %.6f of the squared loadings lie on their factor's four dimensions" % (on / sq.sum()))
print("noise precision    : %.6g (true: 50)" % (state["beta_a"] / state["beta_b"]))
