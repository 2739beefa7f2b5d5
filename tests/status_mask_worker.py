"""One rank of tests/test_status_mask_gpu.py::test_a_switched_off_row_does_not_reach_the_other_ranks: two ranks on ONE GPU,
the ELBO all-reduce through the host transport (tests/multirank_worker.py does the same for the healthy case).

    python tests/status_mask_worker.py RANK WORLD OUT_PREFIX

Rank 0's replicate 1 is ill posed (Q_b negative, as tests/test_gpu_parity.py::test_not_positive_definite_raises makes it).
Both ranks issue the same collectives: iterate(ITERS) and elbo_total().
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pyvb_amd import dist, synth                              # noqa: E402

T, D, K, N, ITERS = 300, 8, 6, 3, 3


def main(rank, world, prefix):
    from pyvb_amd.lds import LDSBatch
    comm = dist.SocketComm(world, rank) if world > 1 else dist.LocalComm()
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=70 + rank)
    if rank == 0:
        st0["Q_b"][1] = -np.abs(st0["Q_b"][1]) * 1e-9
    b = LDSBatch.from_problem(Y, st0, pri, device=0)
    if world > 1:
        b.comm_init_host(comm, rank, world)
    b.sweep("forward")
    failed = []
    try:
        rows = b.elbo()                     # (no collective) the rows as they are before anything is switched off
    except np.linalg.LinAlgError as e:
        failed = e.replicates
        rows = b.elbo()                     # the flags were reported and cleared: the same rows, garbage included
    mask = np.ones(N, dtype=bool)
    mask[failed] = False
    b.set_active(mask)
    b.iterate(ITERS)
    out = {"failed": np.array(failed, dtype=int), "elbo_rows": rows, "elbo_total": b.elbo_total(),
           "elbo_local": b.elbo()[mask].sum(0), "history": b.elbo_history()}
    b.close()
    np.savez(prefix + "_%d.npz" % rank, **out)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]), sys.argv[3])
