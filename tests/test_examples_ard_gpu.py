"""examples/lds_ard.py runs, and what it prints -- the lower bound, <alpha> and the column norms of A and C -- is what
tests/ard_ref.py composes from the oracle on the same inputs (pinned against the reference by tests/test_ard_cpu.py), to the
tolerance of tests/test_gpu_parity.py.  Every <alpha> is finite and positive; nothing is asserted about how many columns are pruned."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ard_ref as AR
from pyvb_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_lds_ard_example():
    niters = 4
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "lds_ard.py"), str(niters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    T, q_true, D, d = 150, 2, 5, 5                      # the script's inputs, rebuilt the way it builds them
    Y = synth.simulate_lds(T, q_true, d, 1, seed=60)["Y"]
    pri, st0 = synth.default_priors(D, d), synth.initial_state(T, D, d, 1, seed=61)
    rng = np.random.default_rng(62)
    for w in ("A", "C"):
        pri[w + "_alpha_a0"], pri[w + "_alpha_b0"] = np.full(D, 1e-3), np.full(D, 1e-3)
        st0[w + "_alpha_b"] = 0.5 + rng.random((1, D))
    (_, m), = AR.models(Y, st0, pri)
    for _ in range(niters):
        parts = m.iterate()
    llb = float(re.search(r"lower bound (\S+)", r.stdout).group(1))
    print("printed %.15g, comparator %.15g" % (llb, parts.sum()))
    assert np.isfinite(llb) and abs(llb - parts.sum()) <= RTOL * np.abs(parts).sum()
    for w in ("A", "C"):
        alpha = np.array([float(v) for v in re.search(r"<alpha_%s> +:((?: \S+)+)" % w, r.stdout).group(1).split()])
        norms = np.array([float(v) for v in re.search(r"column norms of %s:((?: \S+)+)" % w, r.stdout).group(1).split()])
        assert alpha.shape == norms.shape == (D,)
        assert np.all(np.isfinite(alpha)) and np.all(alpha > 0.0), alpha
        want_alpha = m.expectation(w)
        want_norms = np.sqrt((m.chains[0][w + "_mean"][0] ** 2).sum(0))
        # the script prints seven significant digits
        assert np.abs(alpha - want_alpha).max() <= 1e-6 * np.abs(want_alpha).max(), (w, alpha, want_alpha)
        assert np.abs(norms - want_norms).max() <= 1e-6 * np.abs(want_norms).max(), (w, norms, want_norms)
