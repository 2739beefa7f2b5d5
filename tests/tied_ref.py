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


# ----------------------------------------------------------------------------------------------------------------------------
# The cases on which k_tie.hip is held to the accuracy envelope of DESIGN.md section 17 (tests/test_tied_gpu.py:
# test_parity_and_envelope; tests/test_tied_cpu.py measures the float64 comparator's own distance from its long-double run on them).
#
# k_tie sums the moment block (3 D^2 + K D + D doubles, an odd count exactly when D and K are both odd) and Syy (K doubles) over
# the chains of a model, 16 bytes per thread (k_tie<d2>) where the count is even and 8 (k_tie<double>) where it is odd.  A model of
# c chains takes its first chain, then (c - 1) // 4 turns of a body that loads four chains, then a tail of (c - 1) % 4 single loads;
# a model of one chain returns at once.  Which case reaches which path:
#
#   k_tie<double> on both buffers                    d3k3 (27 + 9 + 3 = 39 and 3 doubles), d33k17 (3861 and 17)
#   k_tie<d2> on both buffers                        d4k4 (68 and 4 doubles)
#   k_tie<d2> on the moments, <double> on Syy        d4k5_13 (72 and 5 doubles)
#   more than one block along the elements           d33k17: 3861 elements in 16 blocks of 256, the last one partly outside
#   the early return of a model of one chain         d3k3 (first model), d4k4 (second model)
#   no turn of the unrolled body, tails 1 and 3      d3k3: 2 and 4 chains; d4k4: 4 -- 4 is the largest model that never enters the
#                                                    body (a tail of 2 without a turn: the three-chain models of the older tests)
#   one turn, tails 0, 1, 2, 3                       d3k3: 5, 6, 7, 8 chains; d4k4: 5 (tail 0); d33k17: 6 (tail 1)
#   two turns, tail 0                                d3k3 and d4k4: 9 chains
#   three turns, tail 0                              d4k5_13: 13 chains, a model alone on its handle
#   a singleton between two tied models              d4k4: (5, 1, 9, 4) -- the early return sits between two models that do work
#   the second turn of the gridDim.y loop            none of these: test_more_models_than_the_grid_has_rows (65 537 models)
#
# T = 12 (20 at D = 33, K = 17; the long-double runs of all four cases together take about three seconds); every handle has a
# chain of full length, one of length 2 (no interior class) and one of length 3, the others are drawn from [2, T]; DiagonalGamma and
# Gamma noise.
# ----------------------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (T, D, K, chains per model, noise, seed)
    "d3k3": (12, 3, 3, (1, 2, 4, 5, 6, 7, 8, 9), "diagonal_gamma", 9200),
    "d4k4": (12, 4, 4, (5, 1, 9, 4), "gamma", 9201),
    "d33k17": (20, 33, 17, (6,), "diagonal_gamma", 9202),
    "d4k5_13": (12, 4, 5, (13,), "diagonal_gamma", 9203),
}
ITERS = 2
BOUNDS = ("reference", "exact")
PARAMS = ("A_mean", "C_mean", "A_colvar", "C_colvar", "Q_b", "R_b")
_cache = {}


def rows_of(models):
    """The rows of every model: ids start at 0 and rise in steps of 0 or 1, so a model is a run of consecutive rows."""
    models = np.asarray(models)
    return [r.tolist() for r in np.split(np.arange(models.size), np.flatnonzero(np.diff(models)) + 1)]


def live_classes(Tn):
    """The posterior classes of a chain of Tn nodes: first, interior, last; no interior one at Tn = 2."""
    return [0, 1, 2] if Tn > 2 else [0, 2]


def problem(name):
    """(Y [N, T, K], st0, pri, lengths int32 [N], models int32 [N]) of a case, the padding rows zero.  Shared between the tests: the
    arrays are read-only."""
    if ("problem", name) not in _cache:
        from pyvb_amd import synth
        T, D, K, sizes, kind, seed = CASES[name]
        N = sum(sizes)
        Y, st0, pri = synth.make_problem(T, D, K, N, seed=seed)
        if kind == "gamma":
            pri["noise"] = "gamma"
            for k in ("Q_a0", "Q_b0", "R_a0", "R_b0"):
                pri[k] = np.float64(1e-3)
        lengths = np.random.default_rng(seed + 1).integers(2, T + 1, size=N)
        lengths[:3] = (T, 2, 3)
        live = np.arange(T)[None, :] < lengths[:, None]
        Y = np.where(live[:, :, None], Y, 0.0)
        st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
        lengths = lengths.astype(np.int32)
        models = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        for a in [Y, lengths, models] + list(st0.values()):
            a.setflags(write=False)
        _cache["problem", name] = (Y, st0, pri, lengths, models)
    return _cache["problem", name]


def build_models(Y, st0, pri, lengths, models, only=None):
    """What LDSBatch.from_problem(Y, st0, pri, lengths=, models=) was given, as the comparator sees it: per model (rows, chain
    states, outputs per chain), in the dtype of Y / st0 / pri.  A model's parameters are those of its first row.  lengths None:
    every chain has T nodes.  only: the model indices to build (the others are left out of the list)."""
    out = []
    for m, rows in enumerate(rows_of(models)):
        if only is not None and m not in only:
            continue
        f = rows[0]
        Tn = [Y.shape[1] if lengths is None else int(lengths[n]) for n in rows]
        Ys = [Y[n:n + 1, :t].copy() for n, t in zip(rows, Tn)]
        st0s = [{k: (v[n:n + 1, :t] if k in ("X", "Yq", "Yrowvar") else v[f:f + 1]).copy() for k, v in st0.items()} for n, t in zip(rows, Tn)]
        out.append((rows, make_model(Ys, st0s, pri), Ys))
    return out


def snapshot(chains, pri, Ys):
    """What the envelope compares of one model, in the handle's vocabulary: X and the live classes of Sigma per chain, the
    parameters once (Q_b / R_b repeated over the dimension as the handle returns them under Gamma noise), the six parts of both
    bound modes."""
    import exact_bound_ref as XR
    st = chains[0]
    D, K = st["A_mean"].shape[1], st["C_mean"].shape[1]
    out = {"X": [np.array(ch["X"][0]) for ch in chains],
           "Sigma": [np.array(ch["Sigma"][0][live_classes(ch["X"].shape[1])]) for ch in chains],
           "A_mean": np.array(st["A_mean"][0]), "C_mean": np.array(st["C_mean"][0]),
           "A_colvar": np.einsum("ikk->ik", st["A_cov"][0]).copy(), "C_colvar": np.einsum("ikk->ik", st["C_cov"][0]).copy(),
           "Q_b": np.broadcast_to(st["Q_b"][0], (D,)).copy(), "R_b": np.broadcast_to(st["R_b"][0], (K,)).copy()}
    out["parts"] = {"reference": elbo_parts(chains, pri, Ys), "exact": elbo_parts(chains, pri, Ys, XR.elbo_parts_exact)}
    return out


def run(ms, pri, iters=ITERS):
    """`iters` passes of iterate() over the models of build_models(): per iteration a list, model by model, of snapshot()."""
    out = []
    for _ in range(iters):
        for rows, chains, Ys in ms:
            iterate(chains, pri, Ys)
        out.append([snapshot(chains, pri, Ys) for rows, chains, Ys in ms])
    return out


def trace(name, extended=False):
    """(models, run(models)) of a case in float64 or (extended) np.longdouble; the models are as the last iteration left them.
    Cached and shared between the tests: do not write to it."""
    key = ("trace", name, extended)
    if key not in _cache:
        Y, st0, pri, lengths, models = problem(name)
        if extended:
            import extended_ref as ER
            Y, st0, pri = ER.to_long(Y), ER.to_long(st0), ER.to_long(pri)
        ms = build_models(Y, st0, pri, lengths, models)
        _cache[key] = (ms, run(ms, pri))
    return _cache[key]


def accumulation_length(chains):
    """n of the envelope's floor n 2^-52 for a quantity of a tied model: max(D, K, sum of T_c).  The statistics behind every
    parameter of the model are one accumulation over the nodes of all its chains, and X, Sigma and the parts are formed from
    those parameters; for a model of one chain this is max(D, K, T)."""
    st = chains[0]
    return max(st["A_mean"].shape[1], st["C_mean"].shape[1], sum(ch["X"].shape[1] for ch in chains))


def envelope(got, s64, sx, n):
    """The rule of DESIGN.md section 17 on one model after one iteration: got, s64, sx are snapshot()s of whatever is measured (a
    handle's readout, or a float64 run with an error planted), of the float64 comparator and of its long-double run.  Returns
    [(what, e64, e, e / yardstick(e64, n))], e64 = rel(s64, sx) and e = rel(got, sx) quantity by quantity -- X per chain over its
    own length, Sigma per chain on its live classes -- and part by part in units of sum |parts| of the long-double run."""
    import extended_ref as ER
    out = []

    def one(what, a, b64, bx):
        assert bx.dtype == ER.LD and np.all(np.isfinite(np.asarray(a, dtype=float))), what
        e64, e = ER.rel(b64, bx), ER.rel(a, bx)
        out.append((what, e64, e, e / ER.yardstick(e64, n)))

    for k in ("X", "Sigma"):
        for c, (a, b64, bx) in enumerate(zip(got[k], s64[k], sx[k])):
            one("%s chain %d" % (k, c), a, b64, bx)
    for k in PARAMS:
        one(k, got[k], s64[k], sx[k])
    for mode in BOUNDS:
        px = sx["parts"][mode]
        e64 = ER.bound_errors(s64["parts"][mode], px)[0]
        for r, p, e6, e, ratio, own in ER.compare_bound(got["parts"][mode], px, e64, n):
            out.append(("%s %s" % (mode, ER.LDS_PARTS[p]), e6, e, ratio))
    return out


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
