"""GPU: the scenarios of tests/test_group_status_cpu.py on libpyvb_hip.so -- one ill-posed graph among eight that share a
handle fails alone (pyvb_lds_get_status tells which row; LDSGroup evicts that graph and switches its row off), a member that
leaves has its row switched off (pyvb_lds_set_active), and Network.learn raises for the network that owns the bad graph only.

The bad graph is made through the node API: a negative qb assigned to its Q (tests/test_groups_cpu.py::
test_assignments_reach_the_right_replicate assigns qb the same way), which makes the expected precision negative, as
tests/test_gpu_parity.py::test_not_positive_definite_raises does on the batch.  "Bitwise": replicates share no arithmetic,
and both groups are handles of eight replicates of one shape (same time split and chunking, pyvb_lds_create)."""
import numpy as np
import pytest

import group_scenarios as S

pytestmark = pytest.mark.gpu
BAD = 5
SHAPE = (200, 2, 5)


@pytest.fixture(autouse=True)
def _fresh_pool():
    from pyvb_amd import _recognise
    _recognise._pool.clear()


def _spoil(g):
    g["Q"].qb = -np.abs(np.asarray(g["Q"].qb, dtype=float)) * 1e-9


def _queue_two_iterations(graphs):
    for it in range(2):
        for g in graphs:
            S.loop_body(g)


def _host_x(g):
    return np.hstack([x.__dict__["_h_qmu"] for x in g["Xs"]]).T.copy()


def _eight_healthy(nodes, probs):
    from pyvb_amd import _recognise
    _recognise._pool.clear()
    twins = S.build(nodes, probs)
    _queue_two_iterations(twins)
    snaps = [S.snapshot(g) for g in twins]
    assert twins[0]["Xs"][0]._plan.group.batch.N == 8 and len(twins[0]["Xs"][0]._plan.group.live()) == 8
    return snaps


def test_exactly_the_failing_graph_raises_exactly_once():
    from pyvb_amd import nodes
    probs = S.problems(*SHAPE, 8)
    graphs = S.build(nodes, probs)
    _spoil(graphs[BAD])
    x0 = _host_x(graphs[BAD])
    _queue_two_iterations(graphs)
    with pytest.raises(np.linalg.LinAlgError) as ei:    # the bad graph is the one being read: it raises at once
        S.snapshot(graphs[BAD])
    assert "X_t" in str(ei.value) and ei.value.replicates == [BAD], ei.value
    grp = graphs[0]["Xs"][0]._plan.group
    assert grp.batch.N == 8 and len(grp.live()) == 7 and grp.members[BAD] is None
    assert list(grp.batch.active()) == [k != BAD for k in range(8)]
    assert np.array_equal(_host_x(graphs[BAD]), x0)     # nothing of the garbage came back
    snaps = [S.snapshot(g) for k, g in enumerate(graphs) if k != BAD]      # none of these raises
    assert all(g["Xs"][0]._plan.group is grp for k, g in enumerate(graphs) if k != BAD)
    assert np.array_equal(S.snapshot(graphs[BAD])["X"], x0)     # once
    want = _eight_healthy(nodes, probs)
    for a, b in zip(snaps, [w for k, w in enumerate(want) if k != BAD]):
        S.same(a, b, exact=True)


def test_a_healthy_read_discovers_the_failure_and_succeeds():
    from pyvb_amd import nodes
    probs = S.problems(*SHAPE, 8)
    graphs = S.build(nodes, probs)
    _spoil(graphs[BAD])
    _queue_two_iterations(graphs)
    first = S.snapshot(graphs[0])                       # the call that synchronises: it must not raise for its neighbour
    assert np.isfinite(first["X"]).all()
    grp = graphs[0]["Xs"][0]._plan.group
    assert grp.members[BAD] is None and len(grp.live()) == 7 and not grp.batch.active()[BAD]
    graphs[1]["Q"].qb = np.asarray(graphs[1]["Q"].qb) * 1.0         # an assignment and a bound of healthy graphs do not raise either
    assert np.isfinite(graphs[2]["Xs"][0]._plan.elbo_parts()).all()
    assert np.isfinite(graphs[2]["Xs"][0]._plan.elbo_parts("exact")).all()
    plan = graphs[BAD]["Xs"][0]._plan
    assert plan is not None and plan.failed is not None
    with pytest.raises(np.linalg.LinAlgError):          # the bad graph raises at ITS next use: here an update() request
        graphs[BAD]["Xs"][0].update()
    graphs[BAD]["Xs"][1].update()                       # once
    snaps = [S.snapshot(g) for k, g in enumerate(graphs) if k != BAD]
    want = _eight_healthy(nodes, probs)
    for a, b in zip(snaps, [w for k, w in enumerate(want) if k != BAD]):
        S.same(a, b, exact=True)


def test_a_member_that_leaves_has_its_row_switched_off():
    from pyvb_amd import nodes
    gs = S.build(nodes, S.problems(12, 3, 4, 8))
    for g in gs:
        S.loop_body(g)
    gs[3]["Xs"][5].update()                             # a lone X_t.update(): node by node
    gs[3]["Xs"][5].qmu
    grp = gs[0]["Xs"][0]._plan.group
    assert grp.members[3] is None and len(grp.live()) == 7
    assert list(grp.batch.active()) == [k != 3 for k in range(8)]
    before = grp.batch.get_state()
    for k, g in enumerate(gs):
        if k != 3:
            S.loop_body(g)
    [S.snapshot(g) for k, g in enumerate(gs) if k != 3]
    assert gs[0]["Xs"][0]._plan.group is grp
    after = grp.batch.get_state()
    for k in before:
        assert np.array_equal(before[k][3], after[k][3]), k                 # later launches leave the row alone
    assert not np.array_equal(before["X"][2], after["X"][2])


def test_learn_raises_for_the_network_that_owns_the_bad_graph_only():
    from pyvb_amd import nodes
    from pyvb_amd.network import Network
    graphs = S.build(nodes, S.problems(*SHAPE, 8))
    for g in graphs:
        S.loop_body(g)
    [S.snapshot(g) for g in graphs]
    grp = graphs[0]["Xs"][0]._plan.group
    assert grp.batch.N == 8 and len(grp.live()) == 8    # two networks' graphs on one handle
    theirs = Network([n for g in graphs[:4] for n in S.all_nodes(g)])      # graphs 0..3, the bad one among them
    ours = Network([n for g in graphs[4:] for n in S.all_nodes(g)])
    _spoil(graphs[2])                                   # fails inside the learned schedule, not before
    with pytest.raises(np.linalg.LinAlgError) as ei:
        theirs.learn(4, tol=-np.inf, verbose=False)
    assert ei.value.replicates == [2] and "X_t" in str(ei.value)
    ours.learn(4, tol=-np.inf, verbose=False)
    assert np.isfinite(ours.llb)
    for g in graphs[4:]:
        assert np.isfinite(S.snapshot(g)["X"]).all()
    rest = Network([n for k in (0, 1, 3) for n in S.all_nodes(graphs[k])])  # the bad graph's neighbours carry on too
    rest.learn(2, tol=-np.inf, verbose=False)
    assert np.isfinite(rest.llb)
