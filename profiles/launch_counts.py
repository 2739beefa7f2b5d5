"""Launch counts per kernel id after every call of one fixed scripted sequence per noise kind (setters, single update_x, partial
column ranges, update_Q / R, elbo, iterate, set_active), with pyvb_lds_timing_enable on.  Two builds of the library launch the
same kernels exactly when their outputs are equal line by line:
    PYVB_HIP_LIB=<one build> python profiles/launch_counts.py > a.txt;  PYVB_HIP_LIB=<other> python profiles/launch_counts.py > b.txt;  cmp a.txt b.txt
`python profiles/launch_counts.py pca` runs one fixed stage-wise VB-PCA sequence instead (no timers on that handle: run it under
rocprofv3 --kernel-trace --stats and take the call count per kernel name).
`python profiles/launch_counts.py flow` runs one scripted sequence each for the classes of handle whose branches the update flow
(pyvb_amd/csrc/lds_flow.h) has beside the three noise kinds -- a handle with inputs, Gamma parents on A with DiagonalGamma parents
on C, outputs with NaN under both noise families, a tied handle with unequal lengths, iterate_until with replicates that stop --
the same way, and ends each in the bytes of get_state() and elbo()."""
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


def _wishart(pri, D, K, rng):
    pri["noise"] = "wishart"
    W = rng.standard_normal((D, D)); pri["Q_b0"] = 0.05 * (W @ W.T + D * np.eye(D)); pri["Q_a0"] = np.float64(0.5 * D + 1.0)
    W = rng.standard_normal((K, K)); pri["R_b0"] = 0.05 * (W @ W.T + K * np.eye(K)); pri["R_a0"] = np.float64(0.5 * K + 0.5)


def scripted(tag, b, ops, pri, seed):
    """ops on a handle, the launch counts after each, then the bytes of get_state() and elbo()"""
    rng = np.random.default_rng(seed)
    b.timing(True)
    mask = np.ones(b.N, dtype=bool)
    for i, op in enumerate(ops):
        note = ""
        if op == "fwd": b.sweep("forward")
        elif op == "bwd": b.sweep("backward")
        elif op == "xs":
            for t in range(b.T):
                b.update_x(t)
        elif op == "x_some":
            for t in (0, b.T - 1, 1):
                b.update_x(t)
        elif op in ("A", "C"): b.update_columns(op, 0, b.D)
        elif op in ("Acols", "Ccols"):
            c0 = int(rng.integers(0, b.D)); b.update_columns(op[0], c0, int(rng.integers(c0 + 1, b.D + 1)))
        elif op == "B": b.update_B()
        elif op == "Q": b.update_Q()
        elif op == "R": b.update_R()
        elif op == "Y": b.update_Y()
        elif op == "alpha": b.update_column_precisions()
        elif op == "entry": b.update_entry_precisions()
        elif op == "elbo": b.elbo()
        elif op == "iterate": b.iterate(2)
        elif op == "exact": b.set_bound_mode("exact")
        elif op == "until":
            note = " ran %d converged %s" % (b.iterate_until(4, 2.0, 1), "".join(str(int(c)) for c in b.convergence()[1]))
        elif op == "until_model":
            note = " ran %d converged %s" % (b.iterate_until_model(3, 2.0, 1), "".join(str(int(c)) for c in b.model_convergence()[1]))
        elif op == "get_X": b.get_state(("X",))
        elif op == "set_state_X": b.set_state(X=b.get_state(("X",))["X"])
        elif op == "set_state_A": b.set_state(A_mean=b.get_state(("A_mean",))["A_mean"])
        elif op == "set_state_B": b.set_state(B_mean=b.get_input_state(("B_mean",))["B_mean"])
        elif op == "set_classes": b.set_posterior_classes(*b.get_posterior_classes())
        elif op == "set_priors": b.set_priors(pri)
        elif op == "set_active":
            mask[b.N - 1] = False; b.set_active(mask)
        else: raise ValueError(op)
        b.sync()
        kt = b.kernel_times()
        print("%-14s %2d %-12s %s%s" % (tag, i, op, " ".join("%s=%d" % (k, kt[k][1]) for k in sorted(kt)), note), flush=True)
    st = b.get_state()
    for k in sorted(st):
        print("%-14s %s %s" % (tag, k, np.ascontiguousarray(st[k]).tobytes().hex()), flush=True)
    print("%-14s elbo %s" % (tag, np.ascontiguousarray(b.elbo()).tobytes().hex()), flush=True)
    b.close()


def flow_sequences():
    # a handle with inputs: t19_d6k4p2 of tests/inputs_ref.py
    Y, U, st0, pri = synth.make_input_problem(19, 6, 4, 2, 2, seed=31400)
    scripted("inputs", LDSBatch.from_problem(Y, st0, pri, U=U),
             ["fwd", "bwd", "A", "B", "C", "Q", "R", "elbo", "iterate", "Acols", "Q", "elbo", "B", "elbo", "xs", "A", "Q", "R", "elbo", "set_state_B",
              "elbo", "iterate", "exact", "iterate", "set_classes", "elbo", "set_active", "iterate", "fwd", "B", "Q", "elbo", "get_X", "iterate"], pri, 1)
    # Gamma parents on A, DiagonalGamma parents on C
    D, K, T, N = 3, 4, 12, 3
    rng = np.random.default_rng(2)
    Y, st0, pri = synth.make_problem(T, D, K, N, seed=41)
    b = LDSBatch.from_problem(Y, st0, pri)
    b.set_column_precisions(A=(1.5, 0.7, 0.5 + rng.random((N, D))))
    b.set_entry_precisions(C=(1.2, 0.9, 0.5 + rng.random((N, D, K))))
    scripted("parents", b, ["fwd", "bwd", "A", "alpha", "C", "entry", "Q", "R", "elbo", "iterate", "elbo", "x_some", "fwd", "bwd", "Ccols", "entry",
                            "R", "elbo", "exact", "iterate", "set_priors", "iterate", "elbo"], pri, 2)
    # outputs with NaN under both noise families
    D, K, T, N = 4, 5, 10, 3
    for kind in ("diagonal_gamma", "wishart"):
        rng = np.random.default_rng(3)
        Y, st0, pri = synth.make_problem(T, D, K, N, seed=42)
        if kind == "wishart":
            _wishart(pri, D, K, rng)
        Y[rng.random(Y.shape) < 0.15] = np.nan
        Y[:, 3] = np.nan
        st0["Yq"] = rng.standard_normal(Y.shape); st0["Yrowvar"] = 0.5 + rng.random(Y.shape[:2])
        scripted("nan_" + kind, LDSBatch.from_problem(Y, st0, pri),
                 ["fwd", "bwd", "Y", "A", "C", "Q", "R", "Y", "elbo", "iterate", "Y", "elbo", "Acols", "Q", "elbo", "Ccols", "Y", "R", "elbo", "exact",
                  "iterate", "Y", "elbo", "set_active", "Y", "iterate", "get_X", "Y", "elbo"], pri, 3)
    # three chains in two models, unequal lengths
    D, K, T = 3, 4, 10
    Y0, s0, pri = synth.make_problem(T, D, K, 3, seed=43)
    series = [(Y0[n, :ln], dict(synth.initial_state(ln, D, K, 1, 430 + n))) for n, ln in enumerate((10, 7, 9))]
    scripted("tied", LDSBatch.from_trials([series[:2], series[2:]], pri),
             ["fwd", "bwd", "A", "C", "Q", "R", "elbo", "iterate", "elbo", "xs", "Acols", "Q", "elbo", "exact", "iterate", "until_model", "get_X",
              "iterate", "set_active", "iterate", "elbo"], pri, 4)
    # iterate_until with replicates that stop (case A of tests/converge_ref.py)
    Y, st0, pri = synth.make_problem(30, 4, 5, 6, seed=8100)
    scripted("until", LDSBatch.from_problem(Y, st0, pri),
             ["until", "get_X", "fwd", "bwd", "elbo", "until", "set_state_X", "iterate", "until", "A", "Q", "elbo", "until", "get_X", "until", "until",
              "iterate", "elbo"], pri, 5)


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
    elif len(sys.argv) > 1 and sys.argv[1] == "flow":
        flow_sequences()
    else:
        for kind in ("diagonal_gamma", "gamma", "wishart"):
            for shape in ((12, 9, 40, 4, 11), (128, 128, 40, 4, 12)):
                try:
                    lds_sequence(kind, *shape)
                except Exception as e:          # (a sequence that ends early ends at the same line in both builds)
                    print("%-14s D=%3d stopped: %s" % (kind, shape[0], str(e)[:160]), flush=True)
