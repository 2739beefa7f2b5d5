"""Host logic, no GPU: what pyvb_amd/_recognise.py: LDSGroup does with the per-replicate status and the activity mask of its
handle -- a graph whose row failed is evicted alone and raises from its own next use, once; a member that leaves has its row
switched off -- on tests/oracle_batch_masked.py's stand-in; and the same group on the plain stand-in, which has neither
method (the protocol is optional).  tests/test_group_status_gpu.py repeats the scenarios on the HIP library."""
import numpy as np
import pytest

import group_scenarios as S
from oracle_batch import OracleBatch as OB         # (its `instances` lists the handles of the subclass too)

BAD = 5


@pytest.fixture
def masked(monkeypatch):
    from oracle.tape_ref import NumpyExecutor
    from oracle_batch_masked import MaskedOracleBatch
    from pyvb_amd import generic, lds, _recognise
    OB.instances = []
    MaskedOracleBatch.fail_next = None
    monkeypatch.setattr(lds, "LDSBatch", MaskedOracleBatch)
    monkeypatch.setattr(generic, "DeviceExecutor", NumpyExecutor)
    _recognise._pool.clear()
    return MaskedOracleBatch


def _queue_two_iterations(graphs):
    for it in range(2):
        for g in graphs:
            S.loop_body(g)


def _host_x(g):
    return np.hstack([x.__dict__["_h_qmu"] for x in g["Xs"]]).T.copy()


def _seven_without_the_eighth(masked, nodes, probs):
    from pyvb_amd import _recognise
    _recognise._pool.clear()
    OB.instances = []
    twins = S.build(nodes, [p for k, p in enumerate(probs) if k != BAD])
    _queue_two_iterations(twins)
    snaps = [S.snapshot(g) for g in twins]
    assert [b.N for b in OB.instances] == [7]
    return snaps


def test_exactly_the_failing_graph_raises_exactly_once(masked):
    from pyvb_amd import nodes
    probs = S.problems(12, 3, 4, 8)
    graphs = S.build(nodes, probs)
    x0 = _host_x(graphs[BAD])
    masked.fail_next = (BAD, 3)                         # the forward sweep of the second iteration
    _queue_two_iterations(graphs)
    with pytest.raises(np.linalg.LinAlgError) as ei:    # the bad graph is the one being read: it raises at once
        S.snapshot(graphs[BAD])
    assert "X_t" in str(ei.value) and ei.value.replicates == [BAD]
    handle = OB.instances[0]
    assert handle.N == 8 and not handle.closed
    grp = graphs[0]["Xs"][0]._plan.group
    assert len(grp.live()) == 7 and grp.members[BAD] is None and grp.epoch == 1
    assert handle.log[-1] == ("set_active", tuple(k != BAD for k in range(8)))
    assert not handle.active()[BAD] and handle.active().sum() == 7
    # nothing of the garbage came back: the nodes keep the host attributes of their last synchronisation
    assert np.array_equal(_host_x(graphs[BAD]), x0)
    assert all(x._plan is None for x in graphs[BAD]["Xs"])
    snaps = [S.snapshot(g) for k, g in enumerate(graphs) if k != BAD]      # none of these raises
    assert len(OB.instances) == 1                   # the seven are still on the one handle
    again = S.snapshot(graphs[BAD])                     # once: from here on the graph is what its host attributes say
    assert np.array_equal(again["X"], x0)
    S.loop_body(graphs[BAD])                            # and is bound anew, on its own, at its next request
    assert graphs[BAD]["Xs"][0]._plan is not None and graphs[BAD]["Xs"][0]._plan.failed is None
    want = _seven_without_the_eighth(masked, nodes, probs)
    for a, b in zip(snaps, want):
        S.same(a, b, exact=False, tol=1e-12)


def test_a_healthy_read_discovers_the_failure_and_succeeds(masked):
    from pyvb_amd import nodes
    probs = S.problems(12, 3, 4, 8)
    graphs = S.build(nodes, probs)
    masked.fail_next = (BAD, 3)
    _queue_two_iterations(graphs)
    first = S.snapshot(graphs[0])                       # the call that synchronises: it must not raise for its neighbour
    assert np.isfinite(first["X"]).all()
    handle = OB.instances[0]
    grp = graphs[0]["Xs"][0]._plan.group
    assert grp.members[BAD] is None and len(grp.live()) == 7 and not handle.active()[BAD]
    graphs[1]["Q"].qb = np.asarray(graphs[1]["Q"].qb) * 1.0        # an assignment and a bound of healthy graphs do not raise either
    assert np.isfinite(graphs[2]["Xs"][0]._plan.elbo_parts()).all()
    plan = graphs[BAD]["Xs"][0]._plan
    assert plan is not None and plan.failed is not None
    with pytest.raises(np.linalg.LinAlgError):          # the bad graph raises at ITS next use: here an update() request
        graphs[BAD]["Xs"][0].update()
    assert plan.failed is None and graphs[BAD]["Xs"][0]._plan is None
    graphs[BAD]["Xs"][0].update()                       # once
    snaps = [S.snapshot(g) for k, g in enumerate(graphs) if k != BAD]
    want = _seven_without_the_eighth(masked, nodes, probs)
    for a, b in zip(snaps, want):
        S.same(a, b, exact=False, tol=1e-12)


def _departure(gs):
    """tests/test_groups_cpu.py::test_a_request_the_fused_kernels_do_not_serve_moves_one_graph_only"""
    for g in gs:
        S.loop_body(g)
    gs[3]["Xs"][5].update()                             # a lone X_t.update(): node by node
    got = gs[3]["Xs"][5].qmu
    for g in gs:
        S.loop_body(g)
    return got, [S.snapshot(g) for g in gs]


def test_a_member_that_leaves_has_its_row_switched_off(masked):
    from pyvb_amd import nodes
    graphs = S.build(nodes, S.problems(12, 3, 4, 8))
    _departure(graphs)
    handle = OB.instances[0]
    assert [b.N for b in OB.instances] == [8, 1] and not handle.closed
    off = ("set_active", tuple(k != 3 for k in range(8)))
    assert handle.log.count(off) == 1
    at = handle.log.index(off)
    assert handle.log[at + 1:] == ["forward", "backward", ("A", 0, 3), ("C", 0, 3), "Q", "R"]      # launches after it
    assert 3 in handle.frozen
    for k, v in handle.frozen[3].items():               # ... left the row as it was
        assert np.array_equal(handle.st[k][3], v), k
    for k, v in handle.frozen[3].items():               # (and did move the others)
        if k in ("X", "A_mean", "C_mean"):
            assert not np.array_equal(handle.st[k][2], handle.frozen[3][k])


def test_a_batch_without_the_new_methods_is_served_as_before(masked, monkeypatch):
    from oracle_batch import OracleBatch
    from pyvb_amd import nodes, lds, _recognise
    probs = S.problems(12, 3, 4, 8)
    a, snaps = _departure(S.build(nodes, probs))
    assert any(isinstance(e, tuple) and e[0] == "set_active" for e in OB.instances[0].log)     # (with the methods: used)
    assert not hasattr(OracleBatch, "set_active") and not hasattr(OracleBatch, "status")
    OracleBatch.instances = []
    monkeypatch.setattr(lds, "LDSBatch", OracleBatch)
    _recognise._pool.clear()
    graphs = S.build(nodes, probs)
    b, plain = _departure(graphs)
    handle = OracleBatch.instances[0]
    assert [h.N for h in OracleBatch.instances] == [8, 1] and not handle.closed
    assert not any(isinstance(e, tuple) and e[0] == "set_active" for e in handle.log)
    grp = graphs[0]["Xs"][0]._plan.group
    assert len(grp.live()) == 7 and grp.members[3] is None
    assert np.array_equal(a, b)
    for x, y in zip(snaps, plain):
        S.same(x, y, exact=True)
    # and an error of such a handle propagates as it always did: nobody can say whose it was
    monkeypatch.setattr(OracleBatch, "get_state", lambda self, what=None: (_ for _ in ()).throw(np.linalg.LinAlgError("whole handle")))
    grp.invalidate()
    with pytest.raises(np.linalg.LinAlgError, match="whole handle"):
        S.snapshot(graphs[0])
    assert len(grp.live()) == 7
