"""The comparator of per-model convergence (include/pyvb_hip.h: pyvb_lds_iterate_until_model): every model of a handle run alone
in tests/tied_ref.py -- the oracle composed as the shared-parameter graph composes the node updates -- with Network.learn's
stopping test (network.py:40-56, the test is on line 53) applied on the host to the bound of the model's graph, the six parts
summed over its chains.  The parts are XR.elbo_parts_exact in exact mode, O.elbo_parts otherwise.

Which inputs may be compared: as in tests/converge_ref.py.  A test may assert equal stop iterations only where the reference's own
decision is not a rounding matter: every delta llb - old a run meets must lie at least GUARD * max(1, |llb|) from tol.  alone()
and resumed() assert that before they return anything to compare with, so a badly chosen case fails on the CPU.

Outputs that hold NaN: pyvb_lds_iterate's loop body never updates the outputs (include/pyvb_hip.h: "call pyvb_lds_update_Y where
the script does"), and neither does the loop of the entry under test, so the comparator updates them once, before the first
iteration (the bound is undefined before; the tests call update_Y() on the handle where this does), and learn_model's
update_outputs stays False for a run that is compared with the device.
"""
import copy
import functools

import numpy as np

import converge_ref as R
import exact_bound_ref as XR
import tied_ref as TR
from pyvb_amd import synth

GUARD = R.GUARD

BASE = dict(T=60, D=4, K=5, N=8, seed=9300, lengths=(19, 60, 2, 33, 3, 17, 41, 25), models=(0, 1, 1, 1, 2, 2, 3, 3))
# name -> the handle (shape, seed, noise, lengths, models, outputs with NaN) and the run (bound mode, tol, max_iters)
CASES = {
    "reference": dict(BASE, bound="reference", tol=8.0, max_iters=30),
    "exact": dict(BASE, noise="gamma", bound="exact", tol=2.5, max_iters=30),
    # D = 33, K = 17: the copy extents T * DP and 3 D^2 of the freeze; tol = None: wide_tol() takes it from the trace
    "wide": dict(T=20, D=33, K=17, N=4, seed=9310, models=(0, 0, 1, 1), bound="reference", tol=None, max_iters=8),
    # the problem of converge_ref's case "nan" (same NaN pattern), its three chains in two models
    "nan": dict(R.CASES["nan"], models=(0, 0, 1), like="nan", tol=5.0, max_iters=30),
    # models of 5, 1 and 9 chains, a singleton between them: k_converge's sum over the chains of a model runs over more than three,
    # k_tie through its unrolled body.  tol from the float64 comparator's deltas in exact mode (they fall monotonically): the
    # singleton meets 1.757, 1.314 in iterations 10, 11, the five chains 1.827, 1.325 in 11, 12, the nine 1.491, 1.279 in 16, 17
    "sizes_5_1_9": dict(T=12, D=4, K=5, N=15, seed=9322, lengths=(12, 2, 3, 9, 7, 5, 11, 4, 12, 2, 8, 6, 10, 3, 12),
                        models=(0,) * 5 + (1,) + (2,) * 9, bound="exact", tol=1.4, max_iters=25),
    # converge_ref's case D, every chain a model of its own: the comparator must reproduce converge_ref.learn_alone
    "singletons": dict(R.CASES["D"], models=(0, 1, 2, 3), like="D"),
}


@functools.lru_cache(maxsize=None)
def problem(name):
    """(Y, st0, pri, lengths or None, models) of a case; the arrays are shared between the tests and must not be written to."""
    c = CASES[name]
    models = np.asarray(c["models"], dtype=np.int32)
    if "like" in c:
        return R.problem(c["like"]) + (models,)
    T, D, K = c["T"], c["D"], c["K"]
    Y, st0, pri = synth.make_problem(T, D, K, c["N"], seed=c["seed"])
    if c.get("noise") == "gamma":
        R._gamma(pri)
    lengths = c.get("lengths")
    if lengths is not None:         # padding zeroed as tests/test_tied_gpu.py::_problem does
        live = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
        Y = np.where(live[:, :, None], Y, 0.0)
        st0["X"] = np.where(live[:, :, None], st0["X"], 0.0)
    for a in [Y] + list(st0.values()):
        a.setflags(write=False)
    return Y, st0, pri, (None if lengths is None else np.asarray(lengths, dtype=np.int32)), models


def rows_of(models):
    models = np.asarray(models)
    return [[int(n) for n in np.nonzero(models == m)[0]] for m in range(int(models.max()) + 1)]


def start(name):
    """Per model (rows, chain states, outputs per chain): the comparator's view of what the handle was given, the outputs with
    NaN updated once."""
    Y, st0, pri, lengths, models = problem(name)
    out = []
    for rows in rows_of(models):
        f = rows[0]
        Tn = [Y.shape[1] if lengths is None else int(lengths[n]) for n in rows]
        Ys = [Y[n:n + 1, :t].copy() for n, t in zip(rows, Tn)]
        st0s = [{k: (v[n:n + 1, :t] if k in ("X", "Yq", "Yrowvar") else v[f:f + 1]).copy() for k, v in st0.items()} for n, t in zip(rows, Tn)]
        chains = TR.make_model(Ys, st0s, pri)
        if CASES[name].get("nan"):
            TR.update_Y(chains, pri)
        out.append((rows, chains, Ys))
    return out


def parts_fn(bound):
    return XR.elbo_parts_exact if bound == "exact" else None


def learn_model(chains, pri, Ys, bound, tol, max_iters, update_outputs=False):
    """converge_ref.learn (Network.learn's loop, network.py:46-56) on one model, its chains updated in place."""
    return R.learn(lambda: TR.iterate(chains, pri, Ys, update_outputs=update_outputs, parts_fn=parts_fn(bound)), tol, max_iters)


@functools.lru_cache(maxsize=None)
def wide_tol():
    """The tol of case "wide": between the smallest deltas the two models meet in max_iters iterations, so that exactly one of
    them stops (alone() asserts the guard for it like for any other)."""
    c, pri = CASES["wide"], problem("wide")[2]
    dmin = []
    for rows, chains, Ys in start("wide"):
        trace = learn_model(chains, pri, Ys, c["bound"], -np.inf, c["max_iters"])[2]
        dmin.append(np.diff(trace.sum(1)).min())
    return float(0.5 * (dmin[0] + dmin[1]))


def _tol(name, tol):
    if tol is not None:
        return tol
    return wide_tol() if name == "wide" else CASES[name]["tol"]


@functools.lru_cache(maxsize=None)
def alone(name, tol=None, max_iters=None):
    """Every model of a case run to its own stop: a list of dicts with rows, iters, converged, trace [iters, 6], margin, chains
    (the comparator's state where the model stopped; shared: do not write to it) and Ys.  Asserts the guard on every model."""
    c = CASES[name]
    tol = _tol(name, tol)
    max_iters = c["max_iters"] if max_iters is None else max_iters
    pri = problem(name)[2]
    out = []
    for m, (rows, chains, Ys) in enumerate(start(name)):
        iters, converged, trace, margin = R.guarded(learn_model(chains, pri, Ys, c["bound"], tol, max_iters), tol, "case %s, model %d" % (name, m))
        out.append(dict(rows=rows, iters=iters, converged=converged, trace=trace, margin=margin, chains=chains, Ys=Ys))
    return out


@functools.lru_cache(maxsize=None)
def resumed(name, first_max_iters, tol, max_iters):
    """A second call on the same handle after alone(name, None, first_max_iters): the models that have not converged go on from
    where they are, with old = -inf again; the others stay.  Same dicts, iters summed over both calls, trace of the second call
    alone (cf. converge_ref.resumed)."""
    c, pri = CASES[name], problem(name)[2]
    out = []
    for m, r in enumerate(alone(name, None, first_max_iters)):
        if r["converged"]:
            out.append(dict(r, trace=r["trace"][-1:], moved=False))
            continue
        chains = copy.deepcopy(r["chains"])
        TR._share(chains)
        iters, converged, trace, margin = R.guarded(learn_model(chains, pri, r["Ys"], c["bound"], tol, max_iters), tol,
                                                    "case %s resumed, model %d" % (name, m))
        out.append(dict(r, iters=r["iters"] + iters, converged=converged, trace=trace, margin=margin, chains=chains, moved=True))
    return out


def continued(run):
    """A copy of a model's chains that a test may go on updating (the shared parameters shared again)."""
    chains = copy.deepcopy(run["chains"])
    TR._share(chains)
    return chains


totals = R.totals       # the history: per launched iteration the parts summed over the models, converged ones held at their last row
