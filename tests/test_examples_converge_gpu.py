"""examples/lds_converge_each.py runs, and every data set stops where the oracle run alone on it stops (tests/converge_ref.py,
case A: the script's inputs), with the oracle's lower bound to the tolerance of tests/test_gpu_parity.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import converge_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_lds_converge_each_example():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "lds_converge_each.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    got = re.findall(r"data set (\d+): +(\d+) iterations, (converged|still running), lower bound (\S+)", r.stdout)
    runs = R.alone("A")
    assert [int(g[0]) for g in got] == list(range(len(runs))), r.stdout
    assert "40 iterations launched" in r.stdout
    for g, run in zip(got, runs):
        want = run["trace"][-1]
        assert (int(g[1]), g[2] == "converged") == (run["iters"], run["converged"]), (g, run["iters"])
        assert abs(float(g[3]) - want.sum()) <= RTOL * np.abs(want).sum(), (g, want.sum())
