"""One rank of the multi-rank rehearsal of a VB-PCA handle with DiagonalGamma parents on the columns of W, on ONE GPU
(tests/test_pca_entry_gpu.py; the pattern of tests/multirank_worker.py): the rows are sharded, the collectives travel through the host
transport, and the update of the parents is a local launch on every rank.

    python tests/pca_entry_multirank_worker.py RANK WORLD OUT_PREFIX
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from pyvb_amd import dist                              # noqa: E402
import pca_entry_ref as PR                               # noqa: E402

SHAPE = (41, 40, 5)
ITERS = 3


def rank_run(rank, world, comm):
    from pyvb_amd.pca import PCABatch
    N, d, q = SHAPE
    init, pri = PR.handle_problem(*PR.problem(N, d, q))
    lo, hi = dist.shard_range(N, rank, world)
    b = PCABatch(hi - lo, d, q, device=0, N_total=N, row_offset=lo)
    if world > 1:
        b.comm_init_host(comm, rank, world)
    b.set_priors(pri)
    b.set_entry_precisions(*pri["W_entry"])
    b.set_data(np.where(init["obs"], init["X"], np.nan)[lo:hi])
    b.set_state(X_missing=init["X"][lo:hi], W_mean=init["W_mean"], Z=init["Z"][lo:hi], Z_cov=init["Z_cov"],
                Mu_mean=init["Mu_mean"], beta_b=float(init["beta_b"]))
    b.iterate(ITERS)
    st = b.get_state()
    st["elbo"] = b.elbo()
    st["entry_a"], st["entry_b"] = b.entry_precisions()
    st["rows"] = np.array([lo, hi])
    b.close()
    return st


if __name__ == "__main__":
    rank, world, prefix = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    comm = dist.SocketComm(world, rank) if world > 1 else dist.LocalComm()
    res = rank_run(rank, world, comm)
    np.savez(prefix + "_%d.npz" % rank, **res)
    comm.barrier()
    comm.close()
