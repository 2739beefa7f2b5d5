"""One rank of the two-rank rehearsal of pyvb_lds_iterate_until_model (tests/test_model_converge_gpu.py): the base case of
tests/model_converge_ref.py cut between models -- a model never spans ranks, every rank numbers its own models from 0 -- on ONE
GPU, the collectives (six parts and the number of running chains, seven doubles) through the host transport, as
tests/converge_multirank_worker.py does it for the per-replicate entry.

    python tests/model_converge_multirank_worker.py RANK WORLD OUT_PREFIX

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
import model_converge_ref as MR                               # noqa: E402

LIMIT = 90          # seconds for the whole process
NAME = "reference"
CUTS = {1: [0, 8], 2: [0, 4, 8]}        # rank r of a world holds replicates CUTS[world][r] .. CUTS[world][r + 1] - 1


def main(rank, world, prefix):
    from pyvb_amd.lds import LDSBatch
    signal.alarm(LIMIT)
    comm = dist.SocketComm(world, rank, timeout=60.0) if world > 1 else dist.LocalComm()
    c = MR.CASES[NAME]
    Y, st0, pri, lengths, models = MR.problem(NAME)
    lo, hi = CUTS[world][rank], CUTS[world][rank + 1]
    sl = slice(lo, hi)
    b = LDSBatch.from_problem(Y[sl], {k: v[sl] for k, v in st0.items()}, pri, device=0, lengths=lengths[sl], models=models[sl] - models[lo])
    if world > 1:
        b.comm_init_host(comm, rank, world)
    out = {"iters_run": np.array(b.iterate_until_model(c["max_iters"], c["tol"], 1)), "rows": np.array([lo, hi])}
    out["iters"], out["converged"], out["llb"] = b.model_convergence()
    out["chain_iters"] = b.convergence()[0]
    out["history"], out["elbo_total"] = b.elbo_history(), b.elbo_total()
    out.update(b.get_state())
    out["Sigma"], out["qld_x"] = b.get_posterior_classes()
    out["elbo"] = b.elbo()
    b.close()
    np.savez(prefix + "_%d.npz" % rank, **out)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
