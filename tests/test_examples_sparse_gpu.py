"""examples/lds_sparse.py runs under its fixed seed, and what it prints -- the lower bound, <alpha> of every entry of A and the
posterior mean of A -- is what tests/entry_ref.py composes from the oracle on the same inputs (pinned against the reference by
tests/test_entry_cpu.py), to the tolerance of tests/test_gpu_parity.py.  Every <alpha> is finite and positive; nothing is asserted
about how many entries are pruned."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import entry_ref as NR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(REPO, "examples", "lds_sparse.py")
RTOL = 1e-8


def _rows(out, label, D):
    rows = [[float(v) for v in m.group(1).split()] for m in re.finditer(r"%s row \d+ *:((?: +\S+)+)" % re.escape(label), out)]
    a = np.array(rows)
    assert a.shape == (D, D), (label, a.shape)
    return a


def test_lds_sparse_example():
    niters = 4
    r = subprocess.run([sys.executable, SCRIPT, str(niters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    spec = importlib.util.spec_from_file_location("lds_sparse_example", SCRIPT)      # the script's inputs, built by its own function
    ex = importlib.util.module_from_spec(spec); spec.loader.exec_module(ex)
    Y, st0, pri, A_true = ex.make_inputs()
    D = ex.D
    (_, m), = NR.models(Y, st0, pri)
    for _ in range(niters):
        parts = m.iterate()
    llb = float(re.search(r"lower bound (\S+)", r.stdout).group(1))
    print("printed %.15g, comparator %.15g" % (llb, parts.sum()))
    assert np.isfinite(llb) and abs(llb - parts.sum()) <= RTOL * np.abs(parts).sum()
    alpha, A_mean = _rows(r.stdout, "<alpha>", D), _rows(r.stdout, "<A>", D)
    assert np.all(np.isfinite(alpha)) and np.all(alpha > 0.0), alpha
    want_alpha, want_A = m.expectation("A").T, m.chains[0]["A_mean"][0]
    # the script prints seven significant digits
    assert np.abs(alpha - want_alpha).max() <= 1e-6 * np.abs(want_alpha).max(), (alpha, want_alpha)
    assert np.abs(A_mean - want_A).max() <= 1e-6 * np.abs(want_A).max(), (A_mean, want_A)
