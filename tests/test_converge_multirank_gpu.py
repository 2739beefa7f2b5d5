"""pyvb_lds_iterate_until with a communicator attached: the replicates of a case sharded over two ranks on the ONE GPU of the box
(host transport, as tests/test_multirank_gpu.py), against the single-rank run.  The stop is collective: the running count rides
through the all-reduce, so both ranks launch the same number of iterations -- also the rank whose own replicates are all done."""
import os
import subprocess
import sys

import numpy as np
import pytest

import converge_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "converge_multirank_worker.py")
STATE = ("X", "A_mean", "A_colvar", "C_mean", "C_colvar", "Q_a", "Q_b", "R_a", "R_b", "Sigma", "qld_x", "elbo", "llb")


def _run(name, check_every, world, tmp_path, port):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    prefix = str(tmp_path / ("%s_w%d" % (name, world)))
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), prefix, name, str(check_every)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=120)         # each process under its own limit: a rank that waits alone ends the test
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)[-3000:]
    return [dict(np.load(prefix + "_%d.npz" % r)) for r in range(world)]


# case A: one replicate never stops, both ranks run out together.  Case F with a check after every iteration: rank 1's
# replicates are done after 3 iterations, rank 0's after 4 -- rank 1 has to go on into the fourth all-reduce.
@pytest.mark.parametrize("name,check_every,port", [("A", 8, 29830), ("F", 1, 29840)])
def test_both_ranks_stop_in_the_same_iteration(name, check_every, port, tmp_path):
    one = _run(name, check_every, 1, tmp_path, port)[0]
    many = _run(name, check_every, 2, tmp_path, port + 2)
    runs = R.alone(name)
    assert [tuple(m["rows"]) for m in many] == [(0, 3), (3, 6)]
    assert int(many[0]["iters_run"]) == int(many[1]["iters_run"]) == int(one["iters_run"])
    if name == "F":
        assert int(one["iters_run"]) == 4 and max(many[1]["iters"]) == 3
    assert list(np.concatenate([m["iters"] for m in many])) == list(one["iters"]) == [r["iters"] for r in runs]
    assert list(np.concatenate([m["converged"] for m in many])) == list(one["converged"])
    for k in STATE:                                     # replicates are independent: bitwise
        np.testing.assert_array_equal(np.concatenate([m[k] for m in many]), one[k], err_msg=k)
    scale = np.abs(one["history"]).max()
    for m in many:
        assert m["history"].shape == one["history"].shape
        assert np.abs(m["history"] - one["history"]).max() <= 1e-12 * scale
        assert np.abs(m["elbo_total"] - one["elbo_total"]).max() <= 1e-12 * scale
    assert np.array_equal(many[0]["history"], many[1]["history"])
