"""One rank of tests/test_converge_multirank_gpu.py: the replicates of a case of tests/converge_ref.py sharded over the ranks on
ONE GPU, the collectives of pyvb_lds_iterate_until (six parts and the running count, seven doubles) through the host transport
(tests/multirank_worker.py does the same for pyvb_lds_iterate).

    python tests/converge_multirank_worker.py RANK WORLD OUT_PREFIX CASE CHECK_EVERY

A rank that waits alone ends itself: the transport's own time limit, and an alarm for the whole process.
"""
import os
import signal
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from pyvb_amd import dist                                     # noqa: E402
import converge_ref as R                                      # noqa: E402

LIMIT = 90          # seconds for the whole process


def main(rank, world, prefix, name, check_every):
    from pyvb_amd.lds import LDSBatch
    signal.alarm(LIMIT)
    comm = dist.SocketComm(world, rank, timeout=60.0) if world > 1 else dist.LocalComm()
    c = R.CASES[name]
    Y, st0, pri, _ = R.problem(name)
    lo, hi = dist.shard_range(Y.shape[0], rank, world)
    sl = slice(lo, hi)
    b = LDSBatch.from_problem(Y[sl], {k: v[sl] for k, v in st0.items()}, pri, device=0)
    if world > 1:
        b.comm_init_host(comm, rank, world)
    out = {"iters_run": np.array(b.iterate_until(c["max_iters"], c["tol"], check_every)), "rows": np.array([lo, hi])}
    out["iters"], out["converged"], out["llb"] = b.convergence()
    out["history"], out["elbo_total"] = b.elbo_history(), b.elbo_total()
    out.update(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["elbo"] = b.elbo()
    b.close()
    np.savez(prefix + "_%d.npz" % rank, **out)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]))
