"""Launch counts per kernel id after every call of one fixed scripted sequence per noise kind (setters, single update_x, partial
column ranges, update_Q / R, elbo, iterate, set_active), with pyvb_lds_timing_enable on.  Two builds of the library launch the
same kernels exactly when their outputs are equal line by line:
    PYVB_HIP_LIB=<one build> python profiles/launch_counts.py > a.txt;  PYVB_HIP_LIB=<other> python profiles/launch_counts.py > b.txt;  cmp a.txt b.txt
`python profiles/launch_counts.py pca` runs one fixed stage-wise VB-PCA sequence instead (no timers on that handle: run it under
rocprofv3 --kernel-trace --stats and take the call count per kernel name)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pyvb_amd import synth
from pyvb_amd.lds import LDSBatch
from pyvb_amd.pca import PCABatch


def lds_sequence(kind, D, K, T, N, seed):
    rng = np.random.default_rng(seed)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=seed)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    if kind == "wishart":
        W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
        W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)
    if max(D, K) > 102:
        pri["A_prior_prec"] = np.full_like(pri["A_prior_prec"], 1e-2); pri["C_prior_prec"] = np.full_like(pri["C_prior_prec"], 1e-2)
    b = LDSBatch.from_problem(Y, st0, pri)
    b.timing(True)
    ops = ["fwd", "bwd", "A", "Q", "fwd", "bwd", "elbo", "Ccols", "R", "elbo", "xs", "Acols", "Q", "R", "elbo", "iterate", "elbo",
           "set_state_X", "fwd", "bwd", "C", "elbo", "set_priors", "elbo", "iterate", "set_active", "iterate", "Acols", "Q", "elbo",
           "bwd", "fwd", "A", "C", "Q", "R", "elbo", "set_state_A", "iterate", "iterate", "elbo"]
    mask = np.ones(N, dtype=bool)
    for i, op in enumerate(ops):
        if op == "fwd": b.sweep("forward")
        elif op == "bwd": b.sweep("backward")
        elif op == "xs":
            for t in range(T):
                b.update_x(t)
        elif op in ("A", "C"): b.update_columns(op, 0, D)
        elif op in ("Acols", "Ccols"):
            c0 = int(rng.integers(0, D)); b.update_columns(op[0], c0, int(rng.integers(c0 + 1, D + 1)))
        elif op == "Q": b.update_Q()
        elif op == "R": b.update_R()
        elif op == "elbo": b.elbo()
        elif op == "iterate": b.iterate(2)
        elif op == "set_state_X": b.set_state(X=b.get_state(("X",))["X"])
        elif op == "set_state_A": b.set_state(A_mean=b.get_state(("A_mean",))["A_mean"])
        elif op == "set_priors": b.set_priors(pri)
        elif op == "set_active":
            mask[N // 2] = False; b.set_active(mask)
        b.sync()
        kt = b.kernel_times()
        print("%-14s D=%3d %2d %-12s %s" % (kind, D, i, op, " ".join("%s=%d" % (k, kt[k][1]) for k in sorted(kt))), flush=True)
    b.close()


def pca_sequence():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden"))
    import make_golden as G
    for sweep, N in (("columns", 3000), ("pairs", 3000)):
        init, pri = G.pca_problem(N, 250, 16, seed=77)
        b = PCABatch.from_problem(init, pri)
        b.set_sweep(sweep)
        b.iterate(3); b.update_W(); b.update_Z(); b.update_X(0, 1); b.update_Mu(); b.update_X(1, N); b.update_Beta(); b.elbo()
        b.iterate(1); b.update_X(100, 900); b.iterate(1); b.get_state()
        b.update_Z(); b.update_X(0, N); b.update_X0(); b.update_Mu(); b.iterate(2); b.elbo()
        if len(sys.argv) > 2 and sys.argv[2] == "advice":      # row 0 is read while its imputed entries are unstored
            b.update_Z(); b.update_X(0, N); b.iterate(1)
        b.get_state(); b.close()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pca":
        pca_sequence()
    else:
        for kind in ("diagonal_gamma", "gamma", "wishart"):
            for shape in ((12, 9, 40, 4, 11), (128, 128, 40, 4, 12)):
                try:
                    lds_sequence(kind, *shape)
                except Exception as e:          # (a sequence that ends early ends at the same line in both builds)
                    print("%-14s D=%3d stopped: %s" % (kind, shape[0], str(e)[:160]), flush=True)
