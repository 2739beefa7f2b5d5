"""GPU: precision parents on the columns of W, reached from the node API (pyvb_amd.nodes, Network) -- Bishop's variational PCA
(a Gamma per column, tests/golden/ward_*.npz) and sparse loadings (a DiagonalGamma per column, tests/golden/wentry_*.npz).

Every fixture's graph is built by its generator's own build_graph, given pyvb_amd's `nodes` and `Network` in place of the
reference's; nothing of the reference is needed at run time.  The graph must bind to the fused plan (_recognise.PCAPlan), list its
nodes in the reference's crawl order, and reproduce the reference's recorded run at RTOL = 1e-8 through Network.learn's loop
body: the states, qb of every parent read through the node attribute, and the five class sums of the per-node
log_lower_bound().  Update orders the fused kernels do not serve and assignments while bound are held to a twin that runs node
by node (GenericPlan) from the start.
"""
import glob
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
RTOL = 1e-8
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "ward_*.npz"))) + sorted(glob.glob(os.path.join(GOLDEN_DIR, "wentry_*.npz")))
_ids = lambda p: os.path.basename(p)[:-4]


def _generator(path):
    name = "make_golden_pca_ard" if os.path.basename(path).startswith("ward_") else "make_golden_pca_entry"
    spec = importlib.util.spec_from_file_location(name, os.path.join(GOLDEN_DIR, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _rel(a, b):
    return np.abs(np.asarray(a, dtype=float) - np.asarray(b, dtype=float)).max() / max(np.abs(np.asarray(b, dtype=float)).max(), 1e-300)


def _graph(path):
    """(graph, fixture, the key of the parents' qb in it, the parents' label prefix)"""
    import pyvb_amd
    import pca_ard_ref as AR
    G = _generator(path)
    N, d, q, init, pri, z = AR.load_fixture(path)
    stem = os.path.basename(path)[:-4].split("_", 1)[1]
    case = [c for c in G.CASES if c[0] == stem][0]
    np.random.seed(case[5])                 # the generator's seed: the constructors draw from the global generator
    g = G.build_graph(pyvb_amd, dict(init), pri, case[7])
    if "alphas" in g:
        g["parents"] = g["alphas"]
    kind = ("W_alpha_b", "A") if os.path.basename(path).startswith("ward_") else ("W_entry_b", "D")
    return g, z, kind[0], kind[1]


def _labels(g, prefix):
    lab = {}
    for key, pre in (("Ws", "W"), ("Zs", "Z"), ("Xs", "X"), ("parents", prefix)):
        for i, n in enumerate(g[key]):
            lab[id(n)] = "%s%d" % (pre, i)
    lab[id(g["Mu"])], lab[id(g["Beta"])] = "Mu", "Beta"
    return lab


def _qb(g):
    return np.stack([np.asarray(p.qb, dtype=float) for p in g["parents"]])


def _snapshot(g):
    return [np.hstack([w.qmu for w in g["Ws"]]), np.stack([np.diag(w.qcov) for w in g["Ws"]]), np.hstack([z.qmu for z in g["Zs"]]).T,
            np.hstack([x.qmu for x in g["Xs"]]).T, g["Mu"].qmu.reshape(-1), np.array(float(g["Beta"].qb)), _qb(g)]


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_the_graph_binds_to_the_fused_plan_in_the_crawl_order(path):
    from pyvb_amd import nodes, _recognise
    g, z, key, prefix = _graph(path)
    plan = nodes._plan_of(g["W"])
    assert isinstance(plan, _recognise.PCAPlan), type(plan)
    assert all(p._plan is plan for p in g["parents"]) and plan.n_random_nodes == len(z["order"])
    net = g["net"]
    net.find_iterable()
    lab = _labels(g, prefix)
    assert [lab[id(n)] for n in net.iterable_nodes] == [str(s) for s in z["order"]]
    # before any update the parents read back what the graph was built with
    assert _rel(_qb(g), z["init_" + key]) == 0.0
    plan.release()


@pytest.mark.parametrize("path", FIXTURES, ids=_ids)
def test_the_learn_loop_reproduces_the_reference(path):
    from pyvb_amd import _recognise
    g, z, key, prefix = _graph(path)
    net = g["net"]
    net.find_iterable()
    groups = (g["Ws"] + g["parents"], g["Zs"], g["Xs"], [g["Mu"]], [g["Beta"]])
    for it in range(1, int(max(z["iters"])) + 1):
        for n in net.iterable_nodes:            # network.py:46-48
            n.update()
        if it not in z["iters"]:
            continue
        tag = "it%d_" % it
        assert isinstance(g["W"]._plan, _recognise.PCAPlan)
        got = {"W_mean": np.hstack([w.qmu for w in g["Ws"]]), "W_var": np.stack([np.diag(w.qcov) for w in g["Ws"]]),
               "Z": np.hstack([zz.qmu for zz in g["Zs"]]).T, "Z_cov": g["Zs"][1].qcov, "X": np.hstack([x.qmu for x in g["Xs"]]).T,
               "X_var": np.stack([np.diag(x.qcov) for x in g["Xs"]]), "Mu_mean": g["Mu"].qmu.reshape(-1),
               "Mu_var": np.diag(g["Mu"].qcov), "beta_b": float(g["Beta"].qb), key: _qb(g),
               key[:-1] + "a": np.stack([np.asarray(p.qa, dtype=float) for p in g["parents"]])}
        for k, v in got.items():
            e = _rel(v, z[tag + k])
            print("%s %s%s rel err %.2e" % (os.path.basename(path), tag, k, e))
            assert e <= RTOL, (tag + k, e)
        parts = np.array([np.sum([float(n.log_lower_bound()) for n in grp]) for grp in groups])
        ref = z[tag + "elbo_parts"]
        print("%s %sparts" % (os.path.basename(path), tag), parts, ref)
        assert np.all(np.abs(parts - ref) <= RTOL * np.abs(ref).sum()), (parts, ref)
        assert isinstance(g["W"]._plan, _recognise.PCAPlan)        # the single terms came from a mirror: the graph stayed
    # and Network.learn itself over the same list: the bound is the sum of the class parts on the device
    net.learn(1, tol=-np.inf, verbose=False)
    assert isinstance(g["W"]._plan, _recognise.PCAPlan) and np.isfinite(net.llb)
    total = np.sum([float(n.log_lower_bound()) for grp in groups for n in grp])
    assert abs(net.llb - total) <= RTOL * np.abs(total)


PAIR = [p for p in FIXTURES if "means" in p]


def _twin(path, monkeypatch, script):
    """script(g) on the fused plan and on a twin that runs node by node from the start"""
    from pyvb_amd import generic, _recognise
    got_g = _graph(path)[0]
    got = script(got_g)
    monkeypatch.setattr(_recognise, "bind", lambda node: generic.GenericPlan(node))
    ref_g = _graph(path)[0]
    ref = script(ref_g)
    assert isinstance(ref_g["W"]._plan, generic.GenericPlan)
    return got_g, got, ref


def _loop(g, n=1):
    net = g["net"]
    net.find_iterable()
    for _ in range(n):
        for node in net.iterable_nodes:
            node.update()


@pytest.mark.parametrize("path", PAIR, ids=_ids)
def test_a_lone_parent_update_moves_the_graph_to_the_generic_plan(path, monkeypatch):
    from pyvb_amd import generic, _recognise
    seen = []

    def script(g):
        _loop(g)
        seen.append(type(g["W"]._plan))
        g["parents"][1].update()
        _ = g["parents"][1].qb              # reading issues the request
        seen.append(type(g["W"]._plan))
        _loop(g)
        return _snapshot(g)
    g, got, ref = _twin(path, monkeypatch, script)
    assert seen[0] is _recognise.PCAPlan and seen[1] is generic.GenericPlan
    for a, b, what in zip(got, ref, ("W", "W_var", "Z", "X", "Mu", "Beta.qb", "qb")):
        assert _rel(a, b) <= RTOL, what


@pytest.mark.parametrize("path", PAIR, ids=_ids)
def test_assigning_qb_of_a_parent_while_bound_wins(path, monkeypatch):
    """The assignment releases the plan and the graph binds anew with it.  Before any update the graph comes back to the fused
    plan, whose handle starts from the assigned value (describe_pca reads the nodes' _h_qb).  After updates it comes back to
    whatever plan serves the state the nodes then hold -- partially observed rows that have been conditioned on their
    observations have no isotropic covariance any more, which the fused plan cannot start from, as before this test -- and
    the value still wins."""
    from pyvb_amd import nodes, _recognise
    seen = []

    def assign(p, factor):
        new = np.asarray(p.qb, dtype=float) * factor + 0.25
        p.qb = new if new.ndim else float(new)
        assert _rel(p.qb, new) == 0.0
        return new

    def script(g):
        seen.append(type(nodes._plan_of(g["W"])))       # bound, nothing updated yet
        new = assign(g["parents"][0], 3.0)
        assert _rel(_qb(g)[0], new) == 0.0              # (the fused plan was released: the nodes hold the state, with the assignment)
        _loop(g)
        seen.append(type(g["W"]._plan))
        first = _snapshot(g)
        new = assign(g["parents"][0], 0.5)              # and once more, with updates behind the graph
        assert _rel(_qb(g)[0], new) == 0.0
        _loop(g, 2)
        return first + _snapshot(g)
    g, got, ref = _twin(path, monkeypatch, script)
    assert seen[0] is _recognise.PCAPlan and seen[1] is _recognise.PCAPlan      # (seen[2:] are the twin's)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert _rel(a, b) <= RTOL, i


@pytest.mark.parametrize("path", PAIR, ids=_ids)
def test_demote_and_release_leave_qb_on_the_host_nodes(path):
    from pyvb_amd import generic, _recognise
    for leave in ("release", "demote"):
        g = _graph(path)[0]
        _loop(g)
        plan = g["W"]._plan
        assert isinstance(plan, _recognise.PCAPlan)
        want = _qb(g)
        for p in g["parents"]:
            p.__dict__["_h_qb"] = None
        if leave == "release":
            plan.release()
            assert all(p._plan is None for p in g["parents"])
        else:
            g["Ws"][0].update()
            plan.flush()
            assert isinstance(g["W"]._plan, generic.GenericPlan)
        host = np.stack([np.asarray(p.__dict__["_h_qb"], dtype=float) for p in g["parents"]])
        assert np.array_equal(host, want), leave
        if g["W"]._plan is not None:
            g["W"]._plan.release()
