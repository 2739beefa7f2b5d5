"""Dumps what a build computes on the problems of tests/test_column_parents_gpu.py, for the bit-for-bit comparison of two builds
(profiles/column_parents_refactor.txt, item 4):

    python profiles/column_parents_dump.py --tree CHECKOUT --out DIR

CHECKOUT is a built checkout whose pyvb_amd is imported (this one by default; the parent commit's for the other side); only calls
that both have are used.  Four handles -- the LDS handle taken through A: Gamma, DiagonalGamma, Gamma and C: DiagonalGamma,
set_priors, DiagonalGamma; the VB-PCA handle taken through Gamma, DiagonalGamma, set_priors, Gamma; a plain handle of each kind
without parents -- and for each, after three iterations in the reference and three more in the exact bound mode, every array of
get_state(), of the parents' getters and the parts of the bound as DIR/<handle>_<mode>_<name>.npy.  `cmp` the two directories' files.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=REPO)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import numpy as np
    import pyvb_amd
    import test_column_parents_gpu as P
    from pyvb_amd.lds import LDSBatch
    from pyvb_amd.pca import PCABatch
    print("pyvb_amd from", os.path.dirname(pyvb_amd.__file__), "library version", pyvb_amd._capi.lib.pyvb_version(), flush=True)
    os.makedirs(args.out, exist_ok=True)

    Y, st0, pri, models, hyper = P.lds_problem()
    other = {k: {w: tuple(v + 0.5 for v in t) for w, t in d.items()} for k, d in hyper.items()}
    lds = LDSBatch.from_problem(Y, st0, pri, models=models)
    lds.set_entry_precisions(C=other["diagonal_gamma"]["C"])
    lds.set_priors(pri)
    lds.set_column_precisions(A=other["gamma"]["A"])
    lds.set_entry_precisions(A=other["diagonal_gamma"]["A"])
    lds.set_entry_precisions(C=hyper["diagonal_gamma"]["C"])
    lds.set_column_precisions(A=hyper["gamma"]["A"])
    init, ppri, phyper = P.pca_problem()
    pca = PCABatch.from_problem(init, ppri)
    pca.set_column_precisions(*[v + 0.5 for v in phyper["gamma"]])
    pca.set_entry_precisions(*phyper["diagonal_gamma"])
    pca.set_priors(ppri)
    pca.set_column_precisions(*phyper["gamma"])
    handles = [("lds_parents", lds, P.lds_outputs), ("lds_plain", LDSBatch.from_problem(Y, st0, pri, models=models), P.lds_outputs),
               ("pca_parents", pca, lambda b: P.pca_outputs(b, "gamma")),
               ("pca_plain", PCABatch.from_problem(init, ppri), lambda b: P.pca_outputs(b, "constant"))]
    count = 0
    for name, b, outputs in handles:
        for mode in P.MODES:
            b.set_bound_mode(mode)
            b.iterate(3)
            for k, v in sorted(outputs(b).items()):
                np.save(os.path.join(args.out, "%s_%s_%s.npy" % (name, mode, k)), np.asarray(v))
                count += 1
        b.close()
    print("wrote %d arrays to %s" % (count, args.out))


if __name__ == "__main__":
    main()
