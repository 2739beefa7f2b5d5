#!/usr/bin/env python3
"""Generate tests/golden/regressors_*.npz by running the REFERENCE on LDS graphs with known regressors in the output equation:

    Y_t = Gaussian(K, C * X_t + E * Constant(v_t), R),    E = hstack(Es),    t = 0 .. T-1

and, where P > 0, the known input of make_golden_inputs.py in the state equation.  The mean parent of Y_t is an Addition of two
Multiplications (node.py:52-129, :182-276); the columns of E are Gaussians with Constant parents like those of C.  The reference is
loaded as make_golden.py loads it (a lib2to3-translated scratch copy that never enters the repository); what is committed is this
script and the .npz it writes.

One iteration is the example's loop body with the new columns in their place: forward over the chain, backward, As, [Bs], Cs, Es, Q,
R.  A fixture with several chain lengths holds independent graphs, one per chain: one handle with lengths.  Recorded: the inputs, the
explicit initial state, the states after the first forward sweep alone, and after the listed iterations the states and covariance
classes, the matrices with their variances and q_ln_det, qa / qb of Q and R, and the six parts of the bound (the columns of B inside
part 2, those of E inside part 3).

    python tests/golden/make_golden_regressors.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)


def build_graph(nodes, Y, U, V, pri, st0):
    """make_golden_inputs.build_graph with the regressors: st0 holds one replicate ([1, ...] arrays); U None: no input."""
    T, K = Y.shape
    D, P, Pv, kind = st0["A_mean"].shape[1], 0 if U is None else U.shape[1], V.shape[1], pri["noise"]
    As = [nodes.Gaussian(D, pri["A_prior_mean"][:, [i]].copy(), np.diag(pri["A_prior_prec"][i])) for i in range(D)]
    A = nodes.hstack(As)
    Bs = [nodes.Gaussian(D, pri["B_prior_mean"][:, [i]].copy(), np.diag(pri["B_prior_prec"][i])) for i in range(P)]
    B = nodes.hstack(Bs) if P else None
    Cs = [nodes.Gaussian(K, pri["C_prior_mean"][:, [i]].copy(), np.diag(pri["C_prior_prec"][i])) for i in range(D)]
    C = nodes.hstack(Cs)
    Es = [nodes.Gaussian(K, pri["E_prior_mean"][:, [i]].copy(), np.diag(pri["E_prior_prec"][i])) for i in range(Pv)]
    E = nodes.hstack(Es)
    if kind == "diagonal_gamma":
        Q = nodes.DiagonalGamma(D, pri["Q_a0"].copy(), pri["Q_b0"].copy())
        R = nodes.DiagonalGamma(K, pri["R_a0"].copy(), pri["R_b0"].copy())
    else:
        Q = nodes.Gamma(D, float(pri["Q_a0"]), float(pri["Q_b0"]))
        R = nodes.Gamma(K, float(pri["R_a0"]), float(pri["R_b0"]))
    Xs, Ys = [], []
    for t in range(T):
        if t == 0:
            Xs.append(nodes.Gaussian(D, pri["x0_mean"].reshape(D, 1).copy(), pri["x0_prec"].copy()))
        elif P:
            Xs.append(nodes.Gaussian(D, A * Xs[-1] + B * nodes.Constant(U[t].reshape(P, 1).copy()), Q))
        else:
            Xs.append(nodes.Gaussian(D, A * Xs[-1], Q))
        Ys.append(nodes.Gaussian(K, C * Xs[-1] + E * nodes.Constant(V[t].reshape(Pv, 1).copy()), R))
        Ys[-1].observe(Y[t].reshape(K, 1).copy())
    for t, x in enumerate(Xs):
        x.qmu = st0["X"][0, t].reshape(D, 1).copy()
    for cols, mk, vk, rows in ((As, "A_mean", "A_colvar", D), (Bs, "B_mean", "B_colvar", D), (Cs, "C_mean", "C_colvar", K),
                               (Es, "E_mean", "E_colvar", K)):
        for i, col in enumerate(cols):
            col.qmu = st0[mk][0, :, [i]].reshape(rows, 1).copy()
            col.qcov = np.diag(st0[vk][0, i])
            col.qprec = np.linalg.inv(col.qcov)
    if kind == "diagonal_gamma":
        Q.qb, R.qb = st0["Q_b"][0].copy(), st0["R_b"][0].copy()
    else:
        Q.qb, R.qb = float(st0["Q_b"][0, 0]), float(st0["R_b"][0, 0])
    return dict(As=As, Bs=Bs, Cs=Cs, Es=Es, Q=Q, R=R, Xs=Xs, Ys=Ys)


def snapshot(gs, out, tag, T):
    """Every chain's graph: arrays [N, ...]; padding rows of X are 0."""
    D = len(gs[0]["As"])
    N = len(gs)
    names = "ABCE" if gs[0]["Bs"] else "ACE"
    X = np.zeros((N, T, D))
    rec = {k: [] for k in ["Sigma", "qld_x", "Q_a", "Q_b", "R_a", "R_b", "elbo_parts"] + [nm + s for nm in names for s in ("_mean", "_colvar")]
           + ["qld_" + nm for nm in names]}
    offdiag = 0.0
    for n, g in enumerate(gs):
        Xs = g["Xs"]
        Tn = len(Xs)
        X[n, :Tn] = np.hstack([x.qmu for x in Xs]).T
        cls = [0, 1 if Tn > 2 else 0, Tn - 1]
        rec["Sigma"].append(np.stack([Xs[t].qcov for t in cls]))
        rec["qld_x"].append(np.array([Xs[t].q_ln_det for t in cls]))
        for nm in names:
            cols = g[nm + "s"]
            rec[nm + "_mean"].append(np.hstack([c.qmu for c in cols]))
            cov = np.stack([c.qcov for c in cols])
            rec[nm + "_colvar"].append(np.stack([np.diag(c) for c in cov]))
            offdiag = max(offdiag, np.max([np.abs(c - np.diag(np.diag(c))).max() for c in cov]))
            rec["qld_" + nm].append(np.array([c.q_ln_det for c in cols]))
        for nm in "QR":
            rec[nm + "_a"].append(np.array(g[nm].qa, dtype=float))
            rec[nm + "_b"].append(np.array(g[nm].qb, dtype=float))
        parts = [np.sum([float(nd.log_lower_bound()) for nd in grp]) for grp in (Xs, g["Ys"], g["As"] + g["Bs"], g["Cs"] + g["Es"])]
        parts += [float(g["Q"].log_lower_bound()), float(g["R"].log_lower_bound())]
        rec["elbo_parts"].append(np.array(parts))
    out[tag + "X"] = X
    out[tag + "cov_offdiag_max"] = offdiag
    for k, v in rec.items():
        out[tag + k] = np.stack(v)


def run_case(ref, name, lengths, D, K, P, Pv, kind, iters, seed):
    from pyvb_amd import synth
    N, T = len(lengths), max(lengths)
    Y, U, V, st0, pri = synth.make_regression_problem(T, D, K, P, Pv, N, seed)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    live = (np.arange(T)[None, :] < np.asarray(lengths)[:, None])[:, :, None]
    Y, V = np.where(live, Y, 0.0), np.where(live, V, 0.0)
    U = None if U is None else np.where(live, U, 0.0)
    st0["X"] = np.where(live, st0["X"], 0.0)
    out = {"lengths": np.asarray(lengths, dtype=np.int32), "T": T, "D": D, "K": K, "P": P, "Pv": Pv, "noise": kind, "Y": Y, "V": V}
    if P:
        out["U"] = U
    for k, v in st0.items():
        out["init_" + k] = v
    for k, v in pri.items():
        if k != "noise":
            out["prior_" + k] = v
    gs = [build_graph(ref.nodes, Y[n, :Tn], None if U is None else U[n, :Tn], V[n, :Tn], pri, {k: v[n:n + 1] for k, v in st0.items()})
          for n, Tn in enumerate(lengths)]
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
            [e.update() for e in g["Es"]]
            g["Q"].update()
            g["R"].update()
        if it in iters:
            snapshot(gs, out, "it%d_" % it, T)
        print(name, "iteration", it, flush=True)
    out["iters"] = np.array(sorted(iters))
    path = os.path.join(HERE, "regressors_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


CASES = [
    # name, chain lengths, D, K, P, Pv, noise, checkpoints, seed
    ("p0_d2k5v2_t30", (30,), 2, 5, 0, 2, "diagonal_gamma", (1, 2, 5), 32300),
    ("gamma_d3k4p2v1_t20", (20,), 3, 4, 2, 1, "gamma", (1, 2, 5), 32310),
    ("lengths_d4k5p1v2", (2, 7, 20), 4, 5, 1, 2, "diagonal_gamma", (1, 2, 5), 32320),
]


if __name__ == "__main__":
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = MG.load_reference()
    for c in CASES:
        run_case(ref, *c)
