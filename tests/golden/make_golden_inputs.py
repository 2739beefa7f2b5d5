#!/usr/bin/env python3
"""Generate tests/golden/inputs_*.npz by running the REFERENCE on input-driven LDS graphs:

    X_t = Gaussian(q, A * X_{t-1} + B * Constant(u_t), Q),    B = hstack(Bs),    t = 1 .. T-1

The graph is examples/Linear_Dynamic_System.py:46-66 with the mean parent of X_t an Addition of two Multiplications (node.py:52-129,
:182-276); the columns of B are Gaussians with Constant parents like those of A.  The reference is loaded as make_golden.py loads it
(a lib2to3-translated scratch copy that never enters the repository); what is committed is this script and the .npz it writes.

One iteration is the example's loop body with the new columns in their place: forward over the chain, backward, As, Bs, Cs, Q, R.
A fixture with several chain lengths holds independent graphs, one per chain (each its own A, B, C, Q, R): one handle with lengths.
Recorded: the inputs, the explicit initial state, the states after the first forward sweep alone, and after the listed iterations the
states and covariance classes, the three matrices with their variances and q_ln_det, qa / qb of Q and R, and the six parts of the
bound (the columns of B inside part 2).

    python tests/golden/make_golden_inputs.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)


def build_graph(nodes, Y, U, pri, st0):
    """make_golden.build_graph with the input: st0 holds one replicate ([1, ...] arrays)."""
    T, K = Y.shape
    D, P, kind = st0["A_mean"].shape[1], U.shape[1], pri["noise"]
    As = [nodes.Gaussian(D, pri["A_prior_mean"][:, [i]].copy(), np.diag(pri["A_prior_prec"][i])) for i in range(D)]
    A = nodes.hstack(As)
    Bs = [nodes.Gaussian(D, pri["B_prior_mean"][:, [i]].copy(), np.diag(pri["B_prior_prec"][i])) for i in range(P)]
    B = nodes.hstack(Bs)
    Cs = [nodes.Gaussian(K, pri["C_prior_mean"][:, [i]].copy(), np.diag(pri["C_prior_prec"][i])) for i in range(D)]
    C = nodes.hstack(Cs)
    if kind == "diagonal_gamma":
        Q = nodes.DiagonalGamma(D, pri["Q_a0"].copy(), pri["Q_b0"].copy())
        R = nodes.DiagonalGamma(K, pri["R_a0"].copy(), pri["R_b0"].copy())
    else:
        Q = nodes.Gamma(D, float(pri["Q_a0"]), float(pri["Q_b0"]))
        R = nodes.Gamma(K, float(pri["R_a0"]), float(pri["R_b0"]))
    X0 = nodes.Gaussian(D, pri["x0_mean"].reshape(D, 1).copy(), pri["x0_prec"].copy())
    Y0 = nodes.Gaussian(K, C * X0, R)
    Y0.observe(Y[0].reshape(K, 1).copy())
    Xs, Ys = [X0], [Y0]
    for t in range(1, T):
        Xs.append(nodes.Gaussian(D, A * Xs[-1] + B * nodes.Constant(U[t].reshape(P, 1).copy()), Q))
        Ys.append(nodes.Gaussian(K, C * Xs[-1], R))
        Ys[-1].observe(Y[t].reshape(K, 1).copy())
    for t, x in enumerate(Xs):
        x.qmu = st0["X"][0, t].reshape(D, 1).copy()
    for cols, mk, vk, rows in ((As, "A_mean", "A_colvar", D), (Bs, "B_mean", "B_colvar", D), (Cs, "C_mean", "C_colvar", K)):
        for i, col in enumerate(cols):
            col.qmu = st0[mk][0, :, [i]].reshape(rows, 1).copy()
            col.qcov = np.diag(st0[vk][0, i])
            col.qprec = np.linalg.inv(col.qcov)
    if kind == "diagonal_gamma":
        Q.qb, R.qb = st0["Q_b"][0].copy(), st0["R_b"][0].copy()
    else:
        Q.qb, R.qb = float(st0["Q_b"][0, 0]), float(st0["R_b"][0, 0])
    return dict(As=As, Bs=Bs, Cs=Cs, Q=Q, R=R, Xs=Xs, Ys=Ys)


def snapshot(gs, out, tag, T):
    """Every chain's graph: arrays [N, ...]; padding rows of X are 0."""
    D = len(gs[0]["As"])
    N = len(gs)
    X = np.zeros((N, T, D))
    rec = {k: [] for k in ("Sigma", "qld_x", "A_mean", "B_mean", "C_mean", "A_colvar", "B_colvar", "C_colvar", "qld_A", "qld_B", "qld_C",
                           "Q_a", "Q_b", "R_a", "R_b", "elbo_parts")}
    offdiag = 0.0
    for n, g in enumerate(gs):
        Xs = g["Xs"]
        Tn = len(Xs)
        X[n, :Tn] = np.hstack([x.qmu for x in Xs]).T
        cls = [0, 1 if Tn > 2 else 0, Tn - 1]
        rec["Sigma"].append(np.stack([Xs[t].qcov for t in cls]))
        rec["qld_x"].append(np.array([Xs[t].q_ln_det for t in cls]))
        for nm in "ABC":
            cols = g[nm + "s"]
            rec[nm + "_mean"].append(np.hstack([c.qmu for c in cols]))
            cov = np.stack([c.qcov for c in cols])
            rec[nm + "_colvar"].append(np.stack([np.diag(c) for c in cov]))
            offdiag = max(offdiag, np.max([np.abs(c - np.diag(np.diag(c))).max() for c in cov]))
            rec["qld_" + nm].append(np.array([c.q_ln_det for c in cols]))
        for nm in "QR":
            rec[nm + "_a"].append(np.array(g[nm].qa, dtype=float))
            rec[nm + "_b"].append(np.array(g[nm].qb, dtype=float))
        parts = [np.sum([float(nd.log_lower_bound()) for nd in grp]) for grp in (Xs, g["Ys"], g["As"] + g["Bs"], g["Cs"])]
        parts += [float(g["Q"].log_lower_bound()), float(g["R"].log_lower_bound())]
        rec["elbo_parts"].append(np.array(parts))
    out[tag + "X"] = X
    out[tag + "cov_offdiag_max"] = offdiag
    for k, v in rec.items():
        out[tag + k] = np.stack(v)


def run_case(ref, name, lengths, D, K, P, kind, iters, seed):
    from pyvb_amd import synth
    N, T = len(lengths), max(lengths)
    Y, U, st0, pri = synth.make_input_problem(T, D, K, P, N, seed)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
    Y, U = np.where(live[:, :, None], Y, 0.0), np.where(live[:, :, None], U, 0.0)
    st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
    out = {"lengths": np.asarray(lengths, dtype=np.int32), "T": T, "D": D, "K": K, "P": P, "noise": kind, "Y": Y, "U": U}
    for k, v in st0.items():
        out["init_" + k] = v
    for k, v in pri.items():
        if k != "noise":
            out["prior_" + k] = v
    gs = [build_graph(ref.nodes, Y[n, :Tn], U[n, :Tn], pri, {k: v[n:n + 1] for k, v in st0.items()}) for n, Tn in enumerate(lengths)]
    for it in range(1, max(iters) + 1):
        for g in gs:
            [x.update() for x in g["Xs"]]
        if it == 1:
            fwd = np.zeros((N, T, D))
            for n, g in enumerate(gs):
                fwd[n, :len(g["Xs"])] = np.hstack([x.qmu for x in g["Xs"]]).T
            out["it1_fwd_X"] = fwd
        for g in gs:
            [x.update() for x in reversed(g["Xs"])]
            [a.update() for a in g["As"]]
            [b.update() for b in g["Bs"]]
            [c.update() for c in g["Cs"]]
            g["Q"].update()
            g["R"].update()
        if it in iters:
            snapshot(gs, out, "it%d_" % it, T)
        print(name, "iteration", it, flush=True)
    out["iters"] = np.array(sorted(iters))
    path = os.path.join(HERE, "inputs_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


CASES = [
    # name, chain lengths, D, K, P, noise, checkpoints, seed
    ("d2k5p1_t50", (50,), 2, 5, 1, "diagonal_gamma", (1, 2, 5), 31300),
    ("gamma_d3k4p2_t20", (20,), 3, 4, 2, "gamma", (1, 2, 5), 31310),
    ("lengths_d4k5p3", (2, 7, 20), 4, 5, 3, "diagonal_gamma", (1, 2, 5), 31320),
]


if __name__ == "__main__":
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = MG.load_reference()
    for c in CASES:
        run_case(ref, *c)
