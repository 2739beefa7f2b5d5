"""examples/lds_shared_model.py runs, and the lower bound it prints for each model is that of the shared-parameter graph as
tests/tied_ref.py composes it from the oracle (pinned against the reference by tests/test_tied_cpu.py), to the tolerance of
tests/test_gpu_parity.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tied_ref as TR
from pyvb_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def _record(system, T, rng, q, d):
    A, C, Q, R = (system[k][0] for k in ("A", "C", "Q", "R"))
    x, Y = rng.standard_normal(q), np.empty((T, d))
    for t in range(T):
        if t > 0:
            x = A @ x + np.sqrt(Q) * rng.standard_normal(q)
        Y[t] = C @ x + np.sqrt(R) * rng.standard_normal(d)
    return Y


def test_lds_shared_model_example():
    niters = 6
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "lds_shared_model.py"), str(niters)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {int(m): (int(c), int(t), float(v))
           for m, c, t, v in re.findall(r"model (\d+): (\d+) trials, +(\d+) time steps in all  lower bound (\S+)", r.stdout)}
    trials = ((120, 75, 40, 12, 3), (90, 60, 2))        # the script's inputs, rebuilt the way it builds them
    assert sorted(got) == [0, 1], r.stdout
    assert "models [0, 0, 0, 0, 0, 1, 1, 1]" in r.stdout, r.stdout
    q, d = 2, 5
    pri = synth.default_priors(q, d)
    systems = [synth.simulate_lds(2, q, d, 1, seed=80 + m) for m in range(len(trials))]
    rng = np.random.default_rng(90)
    for m, Ts in enumerate(trials):
        Ys = [_record(systems[m], T, rng, q, d)[None] for T in Ts]
        st0s = [synth.initial_state(T, q, d, 1, seed=100 + 10 * m + n) for n, T in enumerate(Ts)]
        chains = TR.make_model(Ys, st0s, pri)
        for _ in range(niters):
            parts = TR.iterate(chains, pri, Ys)
        assert got[m][:2] == (len(Ts), sum(Ts))
        print("model %d: printed %.15g, comparator %.15g" % (m, got[m][2], parts.sum()))
        assert np.isfinite(got[m][2]) and abs(got[m][2] - parts.sum()) <= RTOL * np.abs(parts).sum(), (m, got[m][2], parts.sum())
