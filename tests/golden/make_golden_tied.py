#!/usr/bin/env python3
"""Generate tests/golden/tied_*.npz by running the REFERENCE on a graph whose chains share A, C, Q, R.

The graph is examples/Linear_Dynamic_System.py:46-66 with `As, A, Cs, C, Q, R` built once and the loop of :58-66 run once per
recorded series, each with its own X_0: several time series, one model.  hstack, Gamma and DiagonalGamma count their children
whoever they belong to (nodes_todo.py:43-62, :125-128, :183-186).  The reference is loaded as make_golden.py loads it (a
lib2to3-translated scratch copy that never enters the repository); what is committed is this script and the .npz it writes.

One iteration is the example's loop body (:69-77) with the two sweeps run over every chain: forward over all X of chain 0,
1, ..., backward likewise, then As, Cs, Q, R.  Recorded: inputs, the explicit initial state, and after the listed iterations the
states and the three covariance classes of every chain, the shared parameters, qa / qb and the six parts of the bound.

    python tests/golden/make_golden_tied.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)


def build_tied_graph(nodes, Ys_data, pri, st0):
    """Ys_data: list of [T_n, K]; st0: compact initial state with one row per chain (the parameters are those of row 0)."""
    D, K, kind = st0["A_mean"].shape[1], Ys_data[0].shape[1], pri["noise"]
    As = [nodes.Gaussian(D, pri["A_prior_mean"][:, [i]].copy(), np.diag(pri["A_prior_prec"][i])) for i in range(D)]
    A = nodes.hstack(As)
    Cs = [nodes.Gaussian(K, pri["C_prior_mean"][:, [i]].copy(), np.diag(pri["C_prior_prec"][i])) for i in range(D)]
    C = nodes.hstack(Cs)
    if kind == "diagonal_gamma":
        Q = nodes.DiagonalGamma(D, pri["Q_a0"].copy(), pri["Q_b0"].copy())
        R = nodes.DiagonalGamma(K, pri["R_a0"].copy(), pri["R_b0"].copy())
    else:
        Q = nodes.Gamma(D, float(pri["Q_a0"]), float(pri["Q_b0"]))
        R = nodes.Gamma(K, float(pri["R_a0"]), float(pri["R_b0"]))
    chains = []
    for n, Y in enumerate(Ys_data):
        X0 = nodes.Gaussian(D, pri["x0_mean"].reshape(D, 1).copy(), pri["x0_prec"].copy())
        Y0 = nodes.Gaussian(K, C * X0, R)
        Y0.observe(Y[0].reshape(K, 1).copy())
        Xs, Ys = [X0], [Y0]
        for t in range(1, Y.shape[0]):
            Xs.append(nodes.Gaussian(D, A * Xs[-1], Q))
            Ys.append(nodes.Gaussian(K, C * Xs[-1], R))
            Ys[-1].observe(Y[t].reshape(K, 1).copy())
        for t, x in enumerate(Xs):
            x.qmu = st0["X"][n, t].reshape(D, 1).copy()
        chains.append((Xs, Ys))
    for i in range(D):
        for col, mk, vk, rows in ((As[i], "A_mean", "A_colvar", D), (Cs[i], "C_mean", "C_colvar", K)):
            col.qmu = st0[mk][0, :, [i]].reshape(rows, 1).copy()
            col.qcov = np.diag(st0[vk][0, i])
            col.qprec = np.linalg.inv(col.qcov)
    if kind == "diagonal_gamma":
        Q.qb, R.qb = st0["Q_b"][0].copy(), st0["R_b"][0].copy()
    else:
        Q.qb, R.qb = float(st0["Q_b"][0, 0]), float(st0["R_b"][0, 0])
    return dict(As=As, Cs=Cs, A=A, C=C, Q=Q, R=R, chains=chains)


def snapshot(g, out, tag, T):
    As, Cs, Q, R, chains = g["As"], g["Cs"], g["Q"], g["R"], g["chains"]
    D = len(As)
    X = np.zeros((len(chains), T, D))
    Sig, qld = [], []
    for n, (Xs, _) in enumerate(chains):
        Tn = len(Xs)
        X[n, :Tn] = np.hstack([x.qmu for x in Xs]).T
        cls = [0, 1 if Tn > 2 else 0, Tn - 1]
        Sig.append(np.stack([Xs[t].qcov for t in cls]))
        qld.append(np.array([Xs[t].q_ln_det for t in cls]))
    out[tag + "X"], out[tag + "Sigma"], out[tag + "qld_x"] = X, np.stack(Sig), np.stack(qld)
    out[tag + "A_mean"] = np.hstack([a.qmu for a in As])
    out[tag + "C_mean"] = np.hstack([c.qmu for c in Cs])
    for nm, cols in (("A", As), ("C", Cs)):
        cov = np.stack([c.qcov for c in cols])
        out[tag + nm + "_colvar"] = np.stack([np.diag(c) for c in cov])
        out[tag + nm + "_cov_offdiag_max"] = np.max([np.abs(c - np.diag(np.diag(c))).max() for c in cov])
        out[tag + "qld_" + nm] = np.array([c.q_ln_det for c in cols])
    out[tag + "Q_a"], out[tag + "Q_b"] = np.array(Q.qa, dtype=float), np.array(Q.qb, dtype=float)
    out[tag + "R_a"], out[tag + "R_b"] = np.array(R.qa, dtype=float), np.array(R.qb, dtype=float)
    allX = [x for Xs, _ in chains for x in Xs]
    allY = [y for _, Ys in chains for y in Ys]
    parts = [np.sum([float(n.log_lower_bound()) for n in grp]) for grp in (allX, allY, As, Cs)]
    parts += [float(Q.log_lower_bound()), float(R.log_lower_bound())]
    out[tag + "elbo_parts"] = np.array(parts)


def run_case(ref, name, lengths, D, K, kind, iters, seed):
    from pyvb_amd import synth
    from pyvb_amd.lds import pad_series
    N, T = len(lengths), max(lengths)
    Yall, st_all, pri = synth.make_problem(T, D, K, N, seed)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    series = [(Yall[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st_all.items()})
              for n, Tn in enumerate(lengths)]
    Y, st0, ln = pad_series(series)
    out = {"lengths": ln, "T": T, "D": D, "K": K, "noise": kind, "Y": Y, "init_X": st0["X"]}
    for k, v in st0.items():
        if k != "X":
            out["init_" + k] = v[0]             # the model's parameters: those of its first chain
    for k, v in pri.items():
        if k != "noise":
            out["prior_" + k] = v
    g = build_tied_graph(ref.nodes, [Y[n, :Tn] for n, Tn in enumerate(lengths)], pri, st0)
    for it in range(1, max(iters) + 1):
        for Xs, _ in g["chains"]:
            [x.update() for x in Xs]
        if it == 1:
            fwd = np.zeros((N, T, D))
            for n, (Xs, _) in enumerate(g["chains"]):
                fwd[n, :len(Xs)] = np.hstack([x.qmu for x in Xs]).T
            out["it1_fwd_X"] = fwd
        for Xs, _ in g["chains"]:
            [x.update() for x in reversed(Xs)]
        [a.update() for a in g["As"]]
        [c.update() for c in g["Cs"]]
        g["Q"].update()
        g["R"].update()
        if it in iters:
            snapshot(g, out, "it%d_" % it, T)
        print(name, "iteration", it, flush=True)
    out["iters"] = np.array(sorted(iters))
    path = os.path.join(HERE, "tied_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


CASES = [
    # name, chain lengths, D, K, noise, checkpoints, seed
    ("d4k5_t19_60_3", (19, 60, 3), 4, 5, "diagonal_gamma", (1, 2, 5), 20280),
    ("gamma_d3k2_t7_4", (7, 4), 3, 2, "gamma", (1, 2, 5), 20281),
]


if __name__ == "__main__":
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = MG.load_reference()
    for c in CASES:
        run_case(ref, *c)
