#!/usr/bin/env python3
"""Generate tests/golden/entry_*.npz by running the REFERENCE on LDS graphs whose columns of A and / or C have DiagonalGamma
precision parents: a precision of its own for every entry of the matrix (sparse transition / loading matrices).

The graph is that of make_golden_ard.py with `Gaussian(rows, pmu, DiagonalGamma(rows, a0_i, b0_i))` for column i of the matrices
named in `entry` (gaussian.py:55-61 accepts the node; nodes_todo.py:159-204 is its class) and, in the mixed case, `Gamma(rows, a0_i,
b0_i)` for those named in `gamma`.  The reference is loaded as make_golden.py loads it (a lib2to3-translated scratch copy that
never enters the repository); what is committed is this script and the .npz it writes.

One iteration: forward over every chain, backward likewise, As, Cs, Q, R, then [p.update() for p in parents] of A and of C.
Recorded: what make_golden_ard.py records, with qa / qb of the DiagonalGamma nodes as A_entry_a / A_entry_b [D][rows] (the same
for C) and their log_lower_bound() inside parts 2 (A) and 3 (C); packed as tests/ard_ref.py: pack does.

    python tests/golden/make_golden_entry.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (puts the repository root on sys.path)
import make_golden_tied as MT  # noqa: E402


def build_graph(nodes, Ys_data, pri, st0, entry, gamma):
    """make_golden_ard.build_graph with DiagonalGamma parents on the columns of the matrices named in `entry` and Gamma parents on
    those named in `gamma`."""
    D, K, kind = st0["A_mean"].shape[1], Ys_data[0].shape[1], pri["noise"]
    parents, kinds = {}, {}
    for w, rows in (("A", D), ("C", K)):
        if w in entry:
            parents[w] = [nodes.DiagonalGamma(rows, pri[w + "_entry_a0"][i].copy(), pri[w + "_entry_b0"][i].copy()) for i in range(D)]
            kinds[w] = "entry"
        elif w in gamma:
            parents[w] = [nodes.Gamma(rows, float(pri[w + "_alpha_a0"][i]), float(pri[w + "_alpha_b0"][i])) for i in range(D)]
            kinds[w] = "alpha"
    prec = lambda w, i: parents[w][i] if w in parents else np.diag(pri[w + "_prior_prec"][i])
    As = [nodes.Gaussian(D, pri["A_prior_mean"][:, [i]].copy(), prec("A", i)) for i in range(D)]
    A = nodes.hstack(As)
    Cs = [nodes.Gaussian(K, pri["C_prior_mean"][:, [i]].copy(), prec("C", i)) for i in range(D)]
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
    for cols, key in ((As, "A_obs"), (Cs, "C_obs")):        # known entries (examples/LDS_knowns_in_A.py:73-74): NaN = unknown
        if pri.get(key) is not None:
            for i, col in enumerate(cols):
                col.observe(pri[key][:, [i]].copy())
    for i in range(D):
        for col, mk, vk, rows in ((As[i], "A_mean", "A_colvar", D), (Cs[i], "C_mean", "C_colvar", K)):
            if col.observed:            # a fully known column keeps its observation
                continue
            col.qmu = st0[mk][0, :, [i]].reshape(rows, 1).copy()
            col.qcov = np.diag(st0[vk][0, i])
            col.qprec = np.linalg.inv(col.qcov)
    if kind == "diagonal_gamma":
        Q.qb, R.qb = st0["Q_b"][0].copy(), st0["R_b"][0].copy()
    else:
        Q.qb, R.qb = float(st0["Q_b"][0, 0]), float(st0["R_b"][0, 0])
    for w, ps in parents.items():
        for i, p in enumerate(ps):
            p.qb = st0[w + "_entry_b"][0, i].copy() if kinds[w] == "entry" else float(st0[w + "_alpha_b"][0, i])
    return dict(As=As, Cs=Cs, A=A, C=C, Q=Q, R=R, chains=chains, parents=parents, kinds=kinds)


def snapshot(g, out, tag, T):
    """make_golden_tied.snapshot (a fully known column has no q_ln_det: NaN), then the precision parents."""
    for c in g["As"] + g["Cs"]:
        if c.observed:
            c.q_ln_det = np.nan
    MT.snapshot(g, out, tag, T)
    parts = out[tag + "elbo_parts"]
    for w, p in (("A", 2), ("C", 3)):
        if w in g["parents"]:
            ps, key = g["parents"][w], "_" + g["kinds"][w] + "_"
            out[tag + w + key + "a"] = np.array([np.array(q.qa, dtype=float) for q in ps])
            out[tag + w + key + "b"] = np.array([np.array(q.qb, dtype=float) for q in ps])
            parts[p] += np.sum([float(q.log_lower_bound()) for q in ps])


def run_case(ref, name, lengths, D, K, kind, entry, gamma, knowns, iters, seed):
    from pyvb_amd import synth
    from pyvb_amd.lds import pad_series
    sys.path.insert(0, os.path.join(MG.REPO, "tests"))
    import ard_ref
    import entry_ref
    N, T = len(lengths), max(lengths)
    Yall, st_all, pri = synth.make_problem(T, D, K, N, seed)
    pri["noise"] = kind
    if kind == "gamma":
        for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
            pri[k] = np.float64(1e-3)
    if knowns:      # column 0 of A fully known, one entry of column 1
        A_obs = np.full((D, D), np.nan)
        A_obs[:, 0] = [0.9, 0.05, -0.1][:D]
        A_obs[2, 1] = -0.3
        pri["A_obs"] = A_obs
    series = [(Yall[n, :Tn], {k: (v[n:n + 1, :Tn] if k == "X" else v[n:n + 1]) for k, v in st_all.items()})
              for n, Tn in enumerate(lengths)]
    Y, st0, ln = pad_series(series)
    entry_ref.add_entry_priors(st0, pri, entry, seed + 1)
    ard_ref.add_hyperpriors(st0, pri, gamma, seed + 2)
    out = {"lengths": ln, "T": T, "D": D, "K": K, "noise": kind, "which": entry, "gamma": gamma, "Y": Y, "init_X": st0["X"]}
    for k, v in st0.items():
        if k != "X":
            out["init_" + k] = v[0]             # the model's parameters: those of its first chain
    for k, v in pri.items():
        if k != "noise":
            out["prior_" + k] = v
    g = build_graph(ref.nodes, [Y[n, :Tn] for n, Tn in enumerate(lengths)], pri, st0, entry, gamma)
    for it in range(1, max(iters) + 1):
        for Xs, _ in g["chains"]:
            [x.update() for x in Xs]
        for Xs, _ in g["chains"]:
            [x.update() for x in reversed(Xs)]
        [a.update() for a in g["As"]]
        [c.update() for c in g["Cs"]]
        g["Q"].update()
        g["R"].update()
        for w in ("A", "C"):
            [p.update() for p in g["parents"].get(w, [])]
        if it in iters:
            snapshot(g, out, "it%d_" % it, T)
        print(name, "iteration", it, flush=True)
    out["iters"] = np.array(sorted(iters))
    # one entry per quantity, the checkpoints stacked along a new first axis (an .npz entry costs more than these arrays hold)
    for k in [k[4:] for k in out if k.startswith("it%d_" % min(iters))]:
        out["snap_" + k] = np.stack([out.pop("it%d_%s" % (it, k)) for it in sorted(iters)])
    path = os.path.join(HERE, "entry_%s.npz" % name)
    np.savez_compressed(path, **ard_ref.pack(out))
    print("wrote", path, os.path.getsize(path), "bytes")


CASES = [
    # name, chain lengths, D, K, noise, matrices with DiagonalGamma parents, with Gamma parents, known entries in A, checkpoints, seed
    ("d3k4_t12", (12,), 3, 4, "diagonal_gamma", "AC", "", False, (1, 2, 5), 31300),
    ("mixed_d2k5_t20", (20,), 2, 5, "gamma", "C", "A", False, (1, 2, 5), 31310),
    ("knowns_d3k4_t15", (15,), 3, 4, "diagonal_gamma", "AC", "", True, (1, 2, 5), 31320),
    ("tied_d3k4", (9, 5), 3, 4, "diagonal_gamma", "AC", "", False, (1, 2, 5), 31330),
]


if __name__ == "__main__":
    warnings.simplefilter("ignore", DeprecationWarning)
    ref = MG.load_reference()
    for c in CASES:
        run_case(ref, *c)
