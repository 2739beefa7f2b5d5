#!/usr/bin/env python3
"""Generate tests/golden/wentry_*.npz by running the REFERENCE on VB-PCA graphs whose W columns have DiagonalGamma precision
parents, a Gamma per entry of W: sparse Bayesian PCA / sparse factor loadings.

The graph is examples/PCA_missing_data.py:31-42 with `Gaussian(d, pmu_i, DiagonalGamma(d, a0_i, b0_i))` for column i of W in place
of the Constant precision (gaussian.py:55-61 accepts the node; nodes_todo.py:159-204 is its class).  The reference is loaded as
make_golden.py loads it (a lib2to3-translated scratch copy that never enters the repository); what is committed is this script
and the .npz it writes.

One iteration is Network.learn's loop body (network.py:46-48) over the nodes fetch_network finds from [W], in the order it finds
them; that order is recorded ("D<i>" = the DiagonalGamma parent of column i).  Recorded besides: the inputs, the explicit initial
state (qb of the parents included), and after the listed iterations the state, qa / qb of Beta and of every parent ([q][d]), and
the five class sums of log_lower_bound() with the parents' terms inside part 0 (W).

build_graph takes the module that supplies `nodes` and `Network`: the reference here, pyvb_amd in
tests/test_nodes_pca_parents_gpu.py (kind="gamma" builds the graph of make_golden_pca_ard.py the same way).

    python tests/golden/make_golden_pca_entry.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def build_graph(mod, init, pri, explicit_x, kind="entry"):
    """make_golden.pca_build_graph with a precision parent on every column of W: kind "entry" DiagonalGamma (pri W_entry_a0,
    W_entry_b0 [q][d], init W_entry_b [q][d]), kind "gamma" Gamma (pri W_alpha_a0, W_alpha_b0 [q], init W_alpha_b [q])."""
    nodes = mod.nodes
    N, d = init["X"].shape
    q = init["Z"].shape[1]
    if kind == "entry":
        parents = [nodes.DiagonalGamma(d, np.array(pri["W_entry_a0"][i], dtype=float), np.array(pri["W_entry_b0"][i], dtype=float))
                   for i in range(q)]
    else:
        parents = [nodes.Gamma(d, float(pri["W_alpha_a0"][i]), float(pri["W_alpha_b0"][i])) for i in range(q)]
    Ws = [nodes.Gaussian(d, pri["W_prior_mean"][:, [i]].copy(), parents[i]) for i in range(q)]
    W = nodes.hstack(Ws)
    Mu = nodes.Gaussian(d, pri["Mu_prior_mean"].reshape(d, 1).copy(), np.diag(pri["Mu_prior_prec"]))
    Beta = nodes.Gamma(d, float(pri["beta_a0"]), float(pri["beta_b0"]))
    Zs = [nodes.Gaussian(q, np.zeros((q, 1)), np.eye(q)) for n in range(N)]
    Xs = [nodes.Gaussian(d, W * z + Mu, Beta) for z in Zs]
    data = np.where(init["obs"], init["X"], np.nan)
    [xn.observe(row.reshape(d, 1).copy()) for xn, row in zip(Xs, data)]
    for i, w in enumerate(Ws):
        w.qmu = init["W_mean"][:, [i]].copy()
        w.qcov = np.diag(init["W_var"][i])          # read by the parent's update only if it came before the column's own
    for i, p in enumerate(parents):
        p.qb = np.array(init["W_entry_b"][i], dtype=float) if kind == "entry" else float(init["W_alpha_b"][i])
    for n, z in enumerate(Zs):
        z.qmu = init["Z"][n].reshape(q, 1).copy()
        z.qcov = init["Z_cov"].copy()
    for n, x in enumerate(Xs):
        if not x.observed and explicit_x:
            x.qmu = init["X"][n].reshape(d, 1).copy()
    if not explicit_x:
        init["X_full"] = np.hstack([np.asarray(x.qmu, dtype=float) for x in Xs]).T.copy()
        init["X_var0"] = np.array([float(x.qcov[0, 0]) for x in Xs])
    Mu.qmu = init["Mu_mean"].reshape(d, 1).copy()
    Beta.qb = float(init["beta_b"])
    net = mod.Network()
    net.addnode(W)
    net.fetch_network()
    return dict(Ws=Ws, parents=parents, W=W, Mu=Mu, Beta=Beta, Zs=Zs, Xs=Xs, net=net)


def labels(g, parent_prefix="D"):
    lab = {}
    for key, pre in (("Ws", "W"), ("Zs", "Z"), ("Xs", "X"), ("parents", parent_prefix)):
        for i, n in enumerate(g[key]):
            lab[id(n)] = "%s%d" % (pre, i)
    lab[id(g["Mu"])], lab[id(g["Beta"])] = "Mu", "Beta"
    return lab


def run_case(MG, ref, name, N, d, q, iters, seed, per_entry, explicit_x):
    init, pri = MG.pca_problem(N, d, q, seed)
    rng = np.random.default_rng(seed + 1)
    del pri["W_prior_prec"]
    if per_entry:
        pri["W_prior_mean"] = 0.3 * rng.standard_normal((d, q))
        pri["W_entry_a0"], pri["W_entry_b0"] = rng.uniform(1.0, 3.0, (q, d)), rng.uniform(0.5, 1.5, (q, d))
    else:                   # broad hyperpriors on every entry
        pri["W_entry_a0"], pri["W_entry_b0"] = np.full((q, d), 1e-3), np.full((q, d), 1e-3)
    init["W_entry_b"] = rng.uniform(0.5, 1.5, (q, d))
    init["W_var"] = np.zeros((q, d))
    np.random.seed(seed)                    # the constructors draw from the global generator
    g = build_graph(ref, init, pri, explicit_x)
    net = g["net"]
    net.find_iterable()
    lab = labels(g)
    out = {"N": N, "d": d, "q": q, "order": np.array([lab[id(n)] for n in net.iterable_nodes])}
    for k, v in init.items():
        out["init_" + k] = v
    for k, v in pri.items():
        out["prior_" + k] = v
    groups = (g["Ws"] + g["parents"], g["Zs"], g["Xs"], [g["Mu"]], [g["Beta"]])
    for it in range(1, max(iters) + 1):
        for n in net.iterable_nodes:            # network.py:46-48
            n.update()
        if it in iters:
            tag = "it%d_" % it
            out[tag + "W_mean"] = np.hstack([w.qmu for w in g["Ws"]])
            out[tag + "W_var"] = np.stack([np.diag(w.qcov) for w in g["Ws"]])
            out[tag + "W_cov_offdiag_max"] = np.max([np.abs(w.qcov - np.diag(np.diag(w.qcov))).max() for w in g["Ws"]])
            out[tag + "Z"] = np.hstack([z.qmu for z in g["Zs"]]).T
            out[tag + "Z_cov"] = g["Zs"][0].qcov
            out[tag + "Z_cov_spread"] = np.max([np.abs(z.qcov - g["Zs"][0].qcov).max() for z in g["Zs"]])
            out[tag + "X"] = np.hstack([x.qmu for x in g["Xs"]]).T
            out[tag + "X_var"] = np.stack([np.diag(x.qcov) for x in g["Xs"]])
            out[tag + "Mu_mean"] = g["Mu"].qmu.reshape(-1)
            out[tag + "Mu_var"] = np.diag(g["Mu"].qcov)
            out[tag + "beta_a"], out[tag + "beta_b"] = np.float64(g["Beta"].qa), np.float64(g["Beta"].qb)
            out[tag + "W_entry_a"] = np.stack([np.asarray(p.qa, dtype=float).reshape(d) for p in g["parents"]])
            out[tag + "W_entry_b"] = np.stack([np.asarray(p.qb, dtype=float).reshape(d) for p in g["parents"]])
            out[tag + "elbo_parts"] = np.array([np.sum([float(n.log_lower_bound()) for n in grp]) for grp in groups])
        print(name, "iteration", it, flush=True)
    out["iters"] = np.array(sorted(iters))
    path = os.path.join(HERE, "wentry_%s.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


CASES = [
    # name, N, d, q, checkpoints, seed, non-zero prior means and per-entry (a0, b0), explicit initial X
    ("broad_n20_d5_q2", 20, 5, 2, (1, 2, 5), 24100, False, True),
    ("means_n12_d7_q3", 12, 7, 3, (1, 2, 5), 24110, True, True),
    ("default_init_n15_d4_q2", 15, 4, 2, (1, 2, 5), 24120, True, False),
]


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import make_golden as MG  # (puts the repository root on sys.path)
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = MG.load_reference()
    for c in CASES:
        run_case(MG, ref, *c)
