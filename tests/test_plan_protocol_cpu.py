"""Host logic, no GPU: the lifecycle every plan behind the node API goes through (pyvb_amd/_plan.py; DESIGN.md "The plan
protocol") -- live, stale, dead, dead with a pending error -- at the corners where the three kinds of plan used to keep the
state under names of their own: a graph that changes after its row was evicted, an assignment to a node of a stale plan of
each kind, Network.learn called again after the plan of its graphs has died.  The LDS handle is tests/oracle_batch_masked.py's
stand-in, the node-by-node plan runs on the numpy interpreter, and the VB-PCA handle is the stand-in below, which only
holds a state (nothing here updates on it)."""
import numpy as np
import pytest

import group_scenarios as S
from oracle_batch import OracleBatch as OB

BAD = 5


class HeldPCABatch(object):
    """pyvb_amd.pca.PCABatch as far as a PCAPlan that never runs an update needs it: the state it was made from, read back."""
    instances = []

    @classmethod
    def from_problem(cls, init, pri, device=0):
        b = cls()
        N, d = init["X"].shape
        b.N, b.q, b.closed = N, init["Z"].shape[1], False
        b.st = {"X": init["X"].copy(), "X_rowvar": np.asarray(init["X_var0"], dtype=float).copy(), "W_mean": init["W_mean"].copy(),
                "W_var": init["W_var"].copy(), "Z": init["Z"].copy(), "Z_cov": init["Z_cov"].copy(), "Mu_mean": init["Mu_mean"].copy(),
                "Mu_var": init["Mu_var"].copy(), "beta_b": float(init["beta_b"])}
        cls.instances.append(b)
        return b

    def get_state(self):
        assert not self.closed
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.st.items()}

    def get_qld(self, rows=True):
        assert not self.closed
        return {"W": np.full(self.q, np.nan), "Z": np.nan, "Mu": np.nan, "X": np.full(self.N, np.nan)}

    def close(self):
        self.closed = True


@pytest.fixture
def host_only(monkeypatch):
    from oracle.tape_ref import NumpyExecutor
    from oracle_batch_masked import MaskedOracleBatch
    from pyvb_amd import generic, lds, pca, _recognise
    OB.instances = []
    HeldPCABatch.instances = []
    MaskedOracleBatch.fail_next = None
    monkeypatch.setattr(lds, "LDSBatch", MaskedOracleBatch)
    monkeypatch.setattr(pca, "PCABatch", HeldPCABatch)
    monkeypatch.setattr(generic, "DeviceExecutor", NumpyExecutor)
    _recognise._pool.clear()
    return MaskedOracleBatch


def _nothing_observed(node):
    """observe() with NaN everywhere: the graph counts as changed (its plan is stale), nothing else happens (gaussian.py:77-78)."""
    node.observe(np.full(node.shape, np.nan))


def _evicted(host_only, nodes):
    """Eight graphs on one handle, the row of graph BAD failed and found by a healthy neighbour's read: the graph is evicted, its
    nodes still point at the plan that keeps the error."""
    graphs = S.build(nodes, S.problems(12, 3, 4, 8))
    host_only.fail_next = (BAD, 3)
    for it in range(2):
        for g in graphs:
            S.loop_body(g)
    S.snapshot(graphs[0])
    g = graphs[BAD]
    plan = g["Xs"][0]._plan
    assert plan is not None and plan.failed is not None and plan.group is None
    assert all(n._plan is plan for n in S.all_nodes(g))
    return graphs, g, plan


# -- dead with a pending error, then the graph changes ---------------------------------------------------------------------
def test_an_observation_on_an_evicted_graph_raises_its_error_first(host_only):
    from pyvb_amd import nodes
    graphs, g, plan = _evicted(host_only, nodes)
    y, before = g["Ys"][2], g["Ys"][2].__dict__["_h_qmu"].copy()
    with pytest.raises(np.linalg.LinAlgError) as ei:        # the change flushes the old plan first: that raises the error
        y.observe(before + 1.0)
    assert ei.value.replicates == [BAD]
    assert plan.failed is None and not plan.stale           # raised once, before the plan was marked
    assert all(n._plan is None for n in S.all_nodes(g))
    assert np.array_equal(y.__dict__["_h_qmu"], before)     # and before the observation was stored
    y.observe(before + 1.0)                                 # once: now the graph is simply unbound
    assert np.array_equal(y.qmu, before + 1.0)
    S.loop_body(g)
    assert np.isfinite(S.snapshot(g)["X"]).all()
    assert g["Xs"][0]._plan is not plan and g["Xs"][0]._plan.failed is None
    assert len(graphs[0]["Xs"][0]._plan.group.live()) == 7  # the neighbours never noticed


def test_a_new_child_on_an_evicted_graph_raises_its_error_first(host_only):
    from pyvb_amd import nodes
    graphs, g, plan = _evicted(host_only, nodes)
    x = g["Xs"][4]
    with pytest.raises(np.linalg.LinAlgError):
        nodes.Gaussian(3, x, np.eye(3))                     # addChild
    assert plan.failed is None and all(n._plan is None for n in S.all_nodes(g))
    assert len(x.children) == 2                             # the child was not linked
    nodes.Gaussian(3, x, np.eye(3))
    assert len(x.children) == 3


# -- an assignment to a node of a stale plan -------------------------------------------------------------------------------
def test_assignment_on_a_stale_lds_plan(host_only):
    from pyvb_amd import nodes
    from pyvb_amd._recognise import LDSPlan
    g = S.build(nodes, S.problems(12, 3, 4, 1))[0]
    S.loop_body(g)
    snap = S.snapshot(g)
    old, handle = g["Xs"][0]._plan, OB.instances[0]
    grp = old.group
    assert isinstance(old, LDSPlan) and grp is not None and not handle.closed
    _nothing_observed(g["Xs"][3])
    assert old.stale and grp.epoch == 1 and g["Xs"][0]._plan is old
    value = np.array([[0.25], [-0.5], [1.5]])
    g["As"][1].qmu = value
    # the stale plan gave the graph up: device state in the nodes, the value on top, the last graph's handle closed
    assert all(n._plan is None for n in S.all_nodes(g)) and old.group is None and handle.closed
    assert g["As"][1].__dict__["_h_qmu"] is value
    assert np.array_equal(np.hstack([x.__dict__["_h_qmu"] for x in g["Xs"]]).T, snap["X"])
    assert np.array_equal(g["As"][0].__dict__["_h_qmu"], snap["A"][:, [0]])
    assert np.array_equal(g["As"][1].qmu, value) and g["As"][1]._plan is None      # unbound: the nodes are the state
    S.loop_body(g)                                          # the next request binds the graph anew, as it is now
    new = g["Xs"][0]._plan
    assert isinstance(new, LDSPlan) and new is not old and not new.stale and new.failed is None
    assert np.isfinite(S.snapshot(g)["X"]).all() and len(OB.instances) == 2


def test_assignment_on_a_stale_generic_plan(host_only):
    from pyvb_amd import nodes
    from pyvb_amd.generic import GenericPlan
    rng = np.random.default_rng(4)
    mu = nodes.Gaussian(2, np.zeros((2, 1)), np.eye(2) * 1e-2)
    ys = [nodes.Gaussian(2, mu, np.eye(2) * 4.0) for _ in range(3)]
    for n in [mu] + ys:
        n.qmu, n.qcov = rng.standard_normal((2, 1)), np.eye(2)
    ys[0].observe(np.array([[1.0], [2.0]]))
    mu.update()
    ys[1].update()
    on_device = ys[1].qmu.copy()
    old = mu._plan
    assert isinstance(old, GenericPlan) and old.ex is not None
    _nothing_observed(ys[2])
    assert old.stale and mu._plan is old
    value = np.array([[3.0], [-4.0]])
    mu.qmu = value
    assert all(n._plan is None for n in [mu] + ys) and old.ex is None
    assert mu.__dict__["_h_qmu"] is value and np.array_equal(ys[1].__dict__["_h_qmu"], on_device)
    with pytest.raises(RuntimeError, match="released"):     # the old plan serves nobody any more
        old.node_llb(mu)
    assert np.array_equal(mu.qmu, value) and mu._plan is None
    ys[1].update()                                          # the next request binds the graph anew
    new = mu._plan
    assert isinstance(new, GenericPlan) and new is not old and not new.stale
    assert np.abs(ys[1].qmu - value).max() <= 1e-12        # a latent child follows its parent: the new plan has the value


def test_assignment_on_a_stale_pca_plan(host_only):
    from pyvb_amd import nodes
    from pyvb_amd.network import Network
    from pyvb_amd._recognise import PCAPlan

    class mod(object):
        pass
    mod.nodes, mod.Network = nodes, Network
    G = S.golden_module()
    init, pri = G.pca_problem(6, 4, 2, seed=21)
    g = G.pca_build_graph(mod, init, pri)
    old = nodes._plan_of(g["W"])                            # what every request does first: the graph is bound
    w_before = g["Ws"][0].qmu.copy()
    assert isinstance(old, PCAPlan) and len(HeldPCABatch.instances) == 1
    handle = HeldPCABatch.instances[0]
    _nothing_observed(g["Zs"][1])
    assert old.stale and g["W"]._plan is old and not handle.closed
    value = np.arange(4.0).reshape(4, 1)
    g["Mu"].qmu = value
    every = g["Ws"] + g["Zs"] + g["Xs"] + [g["W"], g["Mu"], g["Beta"]]
    assert all(n._plan is None for n in every) and handle.closed
    assert g["Mu"].__dict__["_h_qmu"] is value and np.array_equal(g["Ws"][0].__dict__["_h_qmu"], w_before)
    assert np.array_equal(g["Mu"].qmu, value) and g["Mu"]._plan is None
    g["Beta"].update()                                      # the next request binds the graph anew (and waits in its queue)
    new = g["W"]._plan
    assert isinstance(new, PCAPlan) and new is not old and not new.stale and len(HeldPCABatch.instances) == 2
    assert np.array_equal(new.batch.st["Mu_mean"], value.reshape(-1)) and new.pending == [("beta", 0)]


# -- Network.learn again after the plan of its graphs has died --------------------------------------------------------------
def test_learn_again_after_the_plan_was_released(host_only):
    from pyvb_amd import nodes
    from pyvb_amd.network import Network
    probs = S.problems(12, 3, 4, 2)
    value = np.array([[0.25], [-0.5], [1.5]])

    def run(gs, die):
        net = Network([n for g in gs for n in S.all_nodes(g)])
        net.learn(2, tol=-np.inf, verbose=False)
        sched = net._kept[1]
        assert sched.valid()
        if die:
            _nothing_observed(gs[1]["Xs"][3])
            assert not sched.valid()                        # (a stale plan voids the handle's schedule)
        gs[1]["As"][1].qmu = value                          # on a stale plan: released; on a live one: patched in place
        net.learn(2, tol=-np.inf, verbose=False)
        assert net._kept[1].valid() and (net._kept[1] is sched) == (not die)
        return net.llb

    graphs, twins = S.build(nodes, probs), S.build(nodes, probs)
    old = graphs[1]["Xs"][0]._plan
    a = run(graphs, True)
    assert [b.N for b in OB.instances] == [2, 1] and not OB.instances[0].closed
    assert graphs[1]["Xs"][0]._plan is not old and graphs[1]["Xs"][0]._plan.group is not graphs[0]["Xs"][0]._plan.group
    assert len(graphs[0]["Xs"][0]._plan.group.live()) == 1
    b = run(twins, False)
    assert abs(a - b) <= 1e-11 * abs(b)
    for g, t in zip(graphs, twins):
        S.same(S.snapshot(g), S.snapshot(t), exact=False)


def test_learn_again_after_a_generic_plan_was_released(host_only):
    from pyvb_amd import nodes
    from pyvb_amd.network import Network

    def graph():
        rng = np.random.default_rng(8)
        mu = nodes.Gaussian(2, np.zeros((2, 1)), np.eye(2) * 1e-2)
        prec = nodes.Gamma(2, 1e-3, 1e-3)
        ys = [nodes.Gaussian(2, mu, prec) for _ in range(4)]
        mu.qmu, mu.qcov, prec.qb = rng.standard_normal((2, 1)), np.eye(2), 0.5
        for y in ys:
            y.observe(rng.standard_normal((2, 1)) + 2.0)
        return mu, prec, ys

    mu, prec, ys = graph()
    net = Network([mu, prec] + ys)
    net.learn(3, tol=-np.inf, verbose=False)
    old, sched = mu._plan, net._kept[1]
    old.release()                                           # (what profiles/soak.py does between its cycles)
    assert mu._plan is None and not sched.valid()
    net.learn(3, tol=-np.inf, verbose=False)
    assert mu._plan is not None and mu._plan is not old and net._kept[1] is not sched
    mu2, prec2, ys2 = graph()
    twin = Network([mu2, prec2] + ys2)
    twin.learn(6, tol=-np.inf, verbose=False)
    assert abs(net.llb - twin.llb) <= 1e-11 * abs(twin.llb) and np.abs(mu.qmu - mu2.qmu).max() <= 1e-12


def test_learn_again_after_a_graph_was_evicted(host_only):
    from pyvb_amd import nodes
    from pyvb_amd.network import Network
    probs = S.problems(12, 3, 4, 4)
    graphs = S.build(nodes, probs)
    host_only.fail_next = (2, 3)                            # graph 2, the forward sweep of the third iteration
    net = Network([n for g in graphs for n in S.all_nodes(g)])
    with pytest.raises(np.linalg.LinAlgError) as ei:
        net.learn(4, tol=-np.inf, verbose=False)
    assert ei.value.replicates == [2]
    assert all(n._plan is None for n in S.all_nodes(graphs[2]))
    grp = graphs[0]["Xs"][0]._plan.group
    assert len(grp.live()) == 3 and not OB.instances[0].closed
    net.learn(2, tol=-np.inf, verbose=False)                # once: the graph is bound anew from what its nodes kept
    assert np.isfinite(net.llb) and [b.N for b in OB.instances] == [4, 1]
    assert graphs[2]["Xs"][0]._plan.failed is None and graphs[2]["Xs"][0]._plan.group is not grp
    assert graphs[0]["Xs"][0]._plan.group is grp and len(grp.live()) == 3


# -- the protocol itself --------------------------------------------------------------------------------------------------
def test_the_three_plans_implement_the_protocol():
    from pyvb_amd import _plan
    from pyvb_amd._recognise import FusedPlan, LDSPlan, PCAPlan
    from pyvb_amd.generic import GenericPlan
    P = _plan.Plan
    assert (P.stale, P.dead, P.failed, P.group, P.generic) == (False, False, None, None, False)
    for cls in (LDSPlan, PCAPlan, GenericPlan):
        assert issubclass(cls, P)
        for name in ("enqueue", "flush", "read", "write", "release", "node_llb"):
            assert getattr(cls, name) is not getattr(P, name), (cls.__name__, name)
        for name in ("closed", "released"):                 # one name for the state: dead
            assert not hasattr(cls, name)
    assert issubclass(LDSPlan, FusedPlan) and issubclass(PCAPlan, FusedPlan) and GenericPlan.generic
    assert GenericPlan.update_nodes is not P.update_nodes and GenericPlan.llb_nodes is not P.llb_nodes
    assert "mirror" in vars(FusedPlan) and "mirror" not in vars(LDSPlan) and "mirror" not in vars(PCAPlan)
