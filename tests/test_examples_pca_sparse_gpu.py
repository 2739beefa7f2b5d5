"""examples/pca_sparse.py runs, and what it prints -- the lower bound, the columns' squared loadings and the range of <gamma> -- is
what tests/pca_entry_ref.py composes from the oracle on the same inputs (pinned against the reference by
tests/test_pca_entry_cpu.py), to the tolerance of tests/test_pca_gpu.py.  Every <gamma> is finite and positive; nothing is
asserted about how many entries are pruned (that varies with the seed and the number of iterations)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pca_entry_ref as PR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_pca_sparse_example():
    niters = 4
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "pca_sparse.py"), str(niters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    N, d, q = 300, 12, 3                                # the script's inputs, rebuilt the way it builds them
    rng = np.random.default_rng(71)
    support = np.zeros((d, q), dtype=bool)
    for i in range(q):
        support[4 * i:4 * i + 4, i] = True
    W_true = np.where(support, rng.uniform(1.0, 2.0, (d, q)) * rng.choice([-1.0, 1.0], (d, q)), 0.0)
    X = rng.standard_normal((N, q)) @ W_true.T + rng.standard_normal(d) + rng.standard_normal((N, d)) / np.sqrt(50.0)
    obs = rng.random((N, d)) > 0.1
    init = {"obs": obs, "X": np.where(obs, X, 0.0), "W_mean": rng.standard_normal((d, q)), "Z": rng.standard_normal((N, q)),
            "Z_cov": np.eye(q), "Mu_mean": np.zeros(d), "beta_b": 1.0}
    pri = {"W_prior_mean": np.zeros((d, q)), "Mu_prior_mean": np.zeros(d), "Mu_prior_prec": np.full(d, 1e-3), "beta_a0": 1e-3,
           "beta_b0": 1e-3, "W_entry_a0": np.full((q, d), 1e-3), "W_entry_b0": np.full((q, d), 1e-3)}
    init["W_entry_b"] = 0.5 + rng.random((q, d))
    st = PR.make_state(init, pri, N, d, q)
    for _ in range(niters):
        parts = PR.iterate(st, pri)
    llb = float(re.search(r"lower bound (\S+)", r.stdout).group(1))
    print("printed %.15g, comparator %.15g" % (llb, parts.sum()))
    assert np.isfinite(llb) and abs(llb - parts.sum()) <= RTOL * np.abs(parts).sum()
    sq = np.array([float(v) for v in re.search(r"squared loadings +:((?: \S+)+)", r.stdout).group(1).split()])
    lo, hi = [float(v) for v in re.search(r"<gamma> range +:((?: \S+)+)", r.stdout).group(1).split()]
    assert sq.shape == (q,) and np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi
    want = st["W_entry_a"] / st["W_entry_b"]
    want_sq = (st["W_mean"] ** 2).sum(0)
    # the script prints seven significant digits
    assert abs(lo - want.min()) <= 1e-6 * want.min() and abs(hi - want.max()) <= 1e-6 * want.max(), (lo, hi, want.min(), want.max())
    assert np.abs(sq - want_sq).max() <= 1e-6 * np.abs(want_sq).max(), (sq, want_sq)
    assert len(re.findall(r"^   [ -]\d+\.\d{4}(?: [ -]\d+\.\d{4}){2}$", r.stdout, re.M)) == d          # the loadings, a row per dimension
