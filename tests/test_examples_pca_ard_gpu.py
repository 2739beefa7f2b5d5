"""examples/pca_ard.py runs, and what it prints -- the lower bound, <alpha> and the column norms of W -- is what
tests/pca_ard_ref.py composes from the oracle on the same inputs (pinned against the reference by tests/test_pca_ard_cpu.py), to
the tolerance of tests/test_pca_gpu.py.  Every <alpha> is finite and positive; nothing is asserted about how many columns are
pruned (the count varies with the seed)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pca_ard_ref as PR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_pca_ard_example():
    niters = 4
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "pca_ard.py"), str(niters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    N, d, q_true, q = 200, 10, 2, 6                     # the script's inputs, rebuilt the way it builds them
    rng = np.random.default_rng(70)
    X = rng.standard_normal((N, q_true)) @ rng.standard_normal((d, q_true)).T + rng.standard_normal(d) \
        + rng.standard_normal((N, d)) / np.sqrt(50.0)
    obs = rng.random((N, d)) > 0.1
    init = {"obs": obs, "X": np.where(obs, X, 0.0), "W_mean": rng.standard_normal((d, q)), "Z": rng.standard_normal((N, q)),
            "Z_cov": np.eye(q), "Mu_mean": np.zeros(d), "beta_b": 1.0}
    pri = {"W_prior_mean": np.zeros((d, q)), "Mu_prior_mean": np.zeros(d), "Mu_prior_prec": np.full(d, 1e-3), "beta_a0": 1e-3,
           "beta_b0": 1e-3, "W_alpha_a0": np.full(q, 1e-3), "W_alpha_b0": np.full(q, 1e-3)}
    init["W_alpha_b"] = 0.5 + rng.random(q)
    st = PR.make_state(init, pri, N, d, q)
    for _ in range(niters):
        parts = PR.iterate(st, pri)
    llb = float(re.search(r"lower bound (\S+)", r.stdout).group(1))
    print("printed %.15g, comparator %.15g" % (llb, parts.sum()))
    assert np.isfinite(llb) and abs(llb - parts.sum()) <= RTOL * np.abs(parts).sum()
    alpha = np.array([float(v) for v in re.search(r"<alpha> +:((?: \S+)+)", r.stdout).group(1).split()])
    norms = np.array([float(v) for v in re.search(r"column norms of W:((?: \S+)+)", r.stdout).group(1).split()])
    assert alpha.shape == norms.shape == (q,)
    assert np.all(np.isfinite(alpha)) and np.all(alpha > 0.0), alpha
    want_alpha = st["W_alpha_a"] / st["W_alpha_b"]
    want_norms = np.sqrt((st["W_mean"] ** 2).sum(0))
    # the script prints seven significant digits
    assert np.abs(alpha - want_alpha).max() <= 1e-6 * np.abs(want_alpha).max(), (alpha, want_alpha)
    assert np.abs(norms - want_norms).max() <= 1e-6 * np.abs(want_norms).max(), (norms, want_norms)
