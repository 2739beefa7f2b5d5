"""examples/lds_shared_model_converge.py runs, and every model stops where the comparator run alone on it stops
(tests/model_converge_ref.py, case "reference": the script's inputs), with the comparator's lower bound to the tolerance of
tests/test_tied_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import model_converge_ref as MR

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-8


def test_lds_shared_model_converge_example():
    r = subprocess.run([sys.executable, os.path.join(REPO, "examples", "lds_shared_model_converge.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    got = re.findall(r"model (\d+) \((\d+) series, +(\d+) time steps\): +(\d+) iterations, (converged|still running), lower bound (\S+)", r.stdout)
    runs = MR.alone("reference")
    assert [int(g[0]) for g in got] == list(range(len(runs))), r.stdout
    assert [int(g[1]) for g in got] == [len(run["rows"]) for run in runs]
    assert "24 iterations launched" in r.stdout           # the last stop is at 19, seen at the next multiple of check_every = 8
    for g, run in zip(got, runs):
        want = run["trace"][-1]
        assert (int(g[3]), g[4] == "converged") == (run["iters"], run["converged"]), (g, run["iters"])
        assert abs(float(g[5]) - want.sum()) <= RTOL * abs(want.sum()), (g, want.sum())
