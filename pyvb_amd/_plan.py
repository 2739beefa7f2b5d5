"""What pyvb_amd.nodes and pyvb_amd.network ask of the plan a bound graph runs on: the base class of LDSPlan, PCAPlan
(_recognise.py) and GenericPlan (generic.py).  DESIGN.md section 15 tabulates the states and what each entry does in them."""
import numpy as np


def component(start):
    """All nodes connected to `start` (parents and children), in discovery order."""
    seen, order, stack = set(), [], [start]
    while stack:
        n = stack.pop()
        if id(n) in seen:
            continue
        seen.add(id(n))
        order.append(n)
        nxt = list(getattr(n, "children", []))
        for attr in ("mean_parent", "precision_parent", "A", "B"):
            if hasattr(n, attr):
                nxt.append(getattr(n, attr))
        nxt.extend(getattr(n, "parents", []))
        stack.extend(nxt)
    return order


class Plan(object):
    """One connected graph on the device.  A plan is live from its constructor on; the flags only ever go up."""
    stale = False       # a node of the graph gained a child or an observation (nodes._graph_changed): released at the next use
    dead = False        # the plan serves its graph no longer: released, handed to another plan, or evicted from its handle
    failed = None       # dead with a pending error: the LinAlgError of an evicted graph, until it has been raised (LDSPlan only)
    group = None        # the shared device handle of an LDSPlan (_recognise.LDSGroup)
    generic = False     # runs node by node and serves single messages, terms and expectations itself (GenericPlan)
    n_random_nodes = 0  # how many nodes Network.learn must list for the graph to be listed whole

    def bound_to(self, node):
        """`node` is served by this plan (a plan covers one connected graph, so one node tells for all of them)."""
        return node._plan is self and not self.stale and not self.dead

    def _graph_nodes(self):             # operation nodes and Constants too: their messages go through the plan as well
        raise NotImplementedError

    def _adopt(self):
        for n in self._graph_nodes():
            n._plan = self

    def _unbind(self, every=False):
        """Let go of the nodes that still point at this plan -- every=True: of all nodes of the graph, for the plan that takes
        it over in the same breath.  Whoever calls this is done with the graph: the plan is dead."""
        for n in self._graph_nodes():
            if every or n._plan is self:
                n._plan = None
        self.dead = True

    # -- the protocol: every plan overrides these six ------------------------------------------------
    def enqueue(self, node):
        """node.update(): recorded, carried out by the next flush."""
        raise NotImplementedError

    def flush(self):
        """Carry out what is queued.  This can move the graph to another plan (callers look at node._plan again)."""
        raise NotImplementedError

    def read(self, node, name):
        """The posterior attribute `name` of `node`, after a flush."""
        raise NotImplementedError

    def write(self, node, name, value):
        """An assignment to a posterior attribute, after a flush.  False: not patched in place, the caller releases the plan."""
        raise NotImplementedError

    def release(self):
        """Flush, device state back into the nodes' host attributes, the nodes unbound; the plan is dead afterwards."""
        raise NotImplementedError

    def node_llb(self, node, bound="reference"):
        """node.log_lower_bound(bound), after a flush."""
        raise NotImplementedError

    # -- for Network.learn: GenericPlan overrides these two ------------------------------------------
    def update_nodes(self, nodes):
        """[n.update() for n in nodes] (network.py:46-48), carried out."""
        for n in nodes:
            n.update()
        self.flush()

    def llb_nodes(self, nodes, whole, bound="reference"):
        """sum of log_lower_bound() over `nodes` (network.py:49).  whole: every random node of the graph is listed, once --
        the class sums serve; a part of a fused graph gives its terms one by one."""
        if whole:
            return float(np.sum(self.elbo_parts(bound)))
        return float(sum(n.log_lower_bound(bound) for n in nodes))
