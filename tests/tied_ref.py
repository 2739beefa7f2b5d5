"""Comparator (test infrastructure) for LDS handles whose chains share A, C, Q, R (pyvb_lds_create_tied): the functions of
oracle/lds_closed_form.py composed as the shared-parameter graph composes the node updates.

A MODEL is a list of chains.  Every chain is an oracle state with N = 1 of its own length T_n (its X, and after a sweep its
Sigma / qld_x); the parameter entries (A_mean, A_cov, C_mean, C_cov, Q_a, Q_b, R_a, R_b, qld_A, qld_C) are shared by all its
chains: after every parameter update they are the same objects in every chain's dictionary.

  sweeps, statistics       per chain                       (the X_t of one chain see only their own neighbours and outputs)
  update_A / update_C      on the SUM of the chains' statistics    (hstack.pass_up_m1_m2 sums over its children, nodes_todo.py:43-62)
  update_Q / update_R      on the sum, with sum (T_n - 1) and sum T_n children    (nodes_todo.py:125-138, :183-190)
  lower bound              parts 0-1 (X, Y) summed over the chains, parts 2-5 (A, C, Q, R) taken once

tests/test_tied_cpu.py pins this composition against the reference's own run of such a graph (tests/golden/tied_*.npz).
"""
import numpy as np

from oracle import lds_closed_form as O

SHARED = ("A_mean", "A_cov", "C_mean", "C_cov", "Q_a", "Q_b", "R_a", "R_b", "qld_A", "qld_C")


def _share(chains):
    for st in chains[1:]:
        for k in SHARED:
            st[k] = chains[0][k]


def make_model(Ys, st0s, pri):
    """Ys: list of [1, T_n, K]; st0s: list of compact initial states (synth.initial_state form, one row each); the parameters
    are those of the first.  Returns the list of chain states."""
    chains = [O.expand_state(s, pri, Y.shape[1], Y) for Y, s in zip(Ys, st0s)]
    _share(chains)
    first = chains[0]
    D, K, kind = first["A_mean"].shape[1], first["C_mean"].shape[1], pri["noise"]
    nq, nr = sum(Y.shape[1] - 1 for Y in Ys), sum(Y.shape[1] for Y in Ys)
    first["Q_a"] = O._bcast_a(O.noise_a(kind, pri["Q_a0"], nq, D), first["Q_b"], kind)
    first["R_a"] = O._bcast_a(O.noise_a(kind, pri["R_a0"], nr, K), first["R_b"], kind)
    _share(chains)
    return chains


def sweep(chains, pri, Ys, direction):
    post = O.state_posteriors(chains[0], pri)           # of the shared parameters: the same three classes in every chain
    for st, Y in zip(chains, Ys):
        O.sweep(st, pri, Y, direction, post)


def update_x(chains, pri, Ys, t):
    post = O.state_posteriors(chains[0], pri)
    for st, Y in zip(chains, Ys):
        if t < Y.shape[1]:
            O.update_x(st, pri, Y, t, post)


def update_Y(chains, pri):
    for st in chains:
        if "Yobs" in st:
            O.update_Y(st, pri)


def statistics(chains, Ys):
    """(per-chain statistics, their sum)"""
    per = [O.statistics(st, Y) for st, Y in zip(chains, Ys)]
    return per, {k: sum(S[k] for S in per) for k in per[0]}


def update_A(chains, pri, pooled, cols=None):
    O.update_A(chains[0], pri, pooled, cols)
    _share(chains)


def update_C(chains, pri, pooled, cols=None):
    O.update_C(chains[0], pri, pooled, cols)
    _share(chains)


def update_Q(chains, pri, pooled, Ys):
    O.update_Q(chains[0], pri, pooled, sum(Y.shape[1] - 1 for Y in Ys) + 1)        # update_Q counts T - 1 children
    _share(chains)


def update_R(chains, pri, pooled, Ys):
    O.update_R(chains[0], pri, pooled, sum(Y.shape[1] for Y in Ys))
    _share(chains)


def elbo_parts(chains, pri, Ys, parts_fn=None):
    """The six parts of the model's graph, [6].  parts_fn: O.elbo_parts (default) or exact_bound_ref.elbo_parts_exact."""
    fn = parts_fn or O.elbo_parts
    per, _ = statistics(chains, Ys)
    rows = [fn(st, pri, S, Y.shape[1])[0] for st, S, Y in zip(chains, per, Ys)]
    out = np.array(rows[0], copy=True)
    for r in rows[1:]:
        out[:2] += r[:2]
    return out


def iterate(chains, pri, Ys, update_outputs=False, parts_fn=None):
    """One pass of the example's loop body over the model, then its lower bound."""
    sweep(chains, pri, Ys, "forward")
    sweep(chains, pri, Ys, "backward")
    if update_outputs:
        update_Y(chains, pri)
    _, pooled = statistics(chains, Ys)
    update_A(chains, pri, pooled)
    update_C(chains, pri, pooled)
    update_Q(chains, pri, pooled, Ys)
    update_R(chains, pri, pooled, Ys)
    return elbo_parts(chains, pri, Ys, parts_fn)


def load_tied(path):
    """tests/golden/tied_*.npz -> (meta, Ys, st0s, pri, raw): Ys / st0s per chain as make_model takes them."""
    import os
    z = dict(np.load(path, allow_pickle=False))
    lengths = [int(t) for t in z["lengths"]]
    pri = {k[6:]: z[k].copy() for k in z if k.startswith("prior_")}
    pri["noise"] = str(z["noise"])
    par = {k[5:]: z[k][None].copy() for k in z if k.startswith("init_") and k != "init_X"}
    Ys = [z["Y"][n:n + 1, :Tn].copy() for n, Tn in enumerate(lengths)]
    st0s = [dict(par, X=z["init_X"][n:n + 1, :Tn].copy()) for n, Tn in enumerate(lengths)]
    meta = {"lengths": lengths, "D": int(z["D"]), "K": int(z["K"]), "noise": pri["noise"],
            "iters": [int(i) for i in z["iters"]], "name": os.path.basename(path)[5:-4]}
    return meta, Ys, st0s, pri, z
