"""examples/lds_output_offset.py runs, and what it prints -- the column of E and the lower bound of every series, with the regressor
and without -- is what tests/regressors_ref.py and the oracle compose on the same inputs (pinned against the reference by
tests/test_regressors_cpu.py), to the tolerance of tests/test_gpu_parity.py.  The offsets are recovered in E: within a tenth of the
largest one (the mean of C x_t over 400 steps of a system with |C x| of about 7 and a correlation time of at most ten steps has a
standard deviation of about 1.1, three of which over twelve channels are 7 % of the largest offset, 51; the CPU run this was written
from has 4.5 %).  Every series reaches a higher bound with the regressor than the same handle without it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import regressors_ref as RR
from oracle import lds_closed_form as O
from pyvb_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_lds_output_offset_example():
    niters = 60
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "lds_output_offset.py"), str(niters)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    T, q, d, n = 400, 2, 4, 3                            # the script's inputs, rebuilt the way it builds them
    offset = 20.0 * np.random.default_rng(80).standard_normal((n, d))
    Y = synth.simulate_lds(T, q, d, n, seed=81)["Y"] + offset[:, None, :]
    V = np.ones((n, T, 1))
    _, _, _, st0, pri = synth.make_regression_problem(T, q, d, 0, 1, n, seed=82)
    st0["E_mean"] = Y.mean(axis=1)[:, :, None]
    m = RR.Model(Y, None, V, st0, pri)
    st = O.expand_state(RR.split_regressors(st0)[0], pri, T)
    for _ in range(niters):
        parts = m.iterate()
        plain = O.iterate(st, pri, Y)
    for i in range(n):
        got = np.array([float(v) for v in re.search(r"series %d offset fitted:((?: \S+)+)" % i, r.stdout).group(1).split()])
        true = np.array([float(v) for v in re.search(r"series %d offset true  :((?: \S+)+)" % i, r.stdout).group(1).split()])
        want = m.st["E_mean"][i, :, 0]
        # the script prints seven significant digits
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max(), (i, got, want)
        assert np.abs(true - offset[i]).max() <= 1e-6 * np.abs(offset).max()
        w, wo = (float(v) for v in re.search(r"series %d lower bound with the regressor (\S+) without (\S+)" % i, r.stdout).groups())
        print("series %d: with %.15g (comparator %.15g), without %.15g (oracle %.15g)" % (i, w, parts[i].sum(), wo, plain[i].sum()))
        assert abs(w - parts[i].sum()) <= RTOL * np.abs(parts[i]).sum() and abs(wo - plain[i].sum()) <= RTOL * np.abs(plain[i]).sum()
        assert w > wo
        err = np.abs(got - offset[i]).max() / np.abs(offset).max()
        print("series %d: error of the offsets %.3e of the largest" % (i, err))
        assert err <= 0.1, (i, err)
