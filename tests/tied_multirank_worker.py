"""One rank of the two-rank rehearsal of a handle whose chains share A, C, Q, R (tests/test_tied_gpu.py), on ONE GPU through the
host transport, as tests/multirank_worker.py does it.  The replicates are cut between models -- a model never spans ranks -- and
every rank numbers its own models from 0.

    python tests/tied_multirank_worker.py RANK WORLD OUT_PREFIX
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pyvb_amd import dist, synth                              # noqa: E402

T, D, K, SEED, ITERS = 60, 4, 5, 9200, 3
LENGTHS = np.array([19, 60, 2, 33, 3, 17], dtype=np.int32)
MODELS = np.array([0, 1, 1, 1, 2, 2], dtype=np.int32)
CUTS = {1: [0, 6], 2: [0, 4, 6]}        # rank r of a world holds replicates CUTS[world][r] .. CUTS[world][r + 1] - 1


def run(rank, world, comm):
    from pyvb_amd.lds import LDSBatch
    Y, st0, pri = synth.make_problem(T, D, K, len(LENGTHS), seed=SEED)
    lo, hi = CUTS[world][rank], CUTS[world][rank + 1]
    sl = slice(lo, hi)
    b = LDSBatch.from_problem(Y[sl], {k: v[sl] for k, v in st0.items()}, pri, device=0, lengths=LENGTHS[sl],
                              models=MODELS[sl] - MODELS[lo])
    if world > 1:
        b.comm_init_host(comm, rank, world)
    b.iterate(ITERS)
    out = {k: v for k, v in b.get_state().items() if k in ("X", "A_mean", "C_mean", "Q_b", "R_b")}
    out.update(elbo=b.elbo(), elbo_total=b.elbo_total(), history=b.elbo_history(), rows=np.array([lo, hi]))
    b.close()
    return out


if __name__ == "__main__":
    rank, world, prefix = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    comm = dist.SocketComm(world, rank) if world > 1 else dist.LocalComm()
    np.savez(prefix + "_%d.npz" % rank, **run(rank, world, comm))
    comm.barrier()
    comm.close()
