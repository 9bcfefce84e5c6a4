"""The chains with merged stages that test_chain_merge_gpu.py runs, built from
chainref's stage makers and trace builders, and what the reference
(chainref.chain_reference, which pushes every packet through all its cables
before the next) says about them. The links are written in depth-first order,
the order in which vigor_amd.Chain's tie rule equals the reference's.

The conditions the GPU comparison relies on are checked without a GPU by
test_chain_merge_ref.py."""
import numpy as np

import chainref as CR
import vigor_amd


class Recorded:
    """An oracle that notes the port of every packet it is handed."""

    def __init__(self, oracle):
        self.oracle, self.ports = oracle, []

    def process(self, port, buf, **kw):
        self.ports.append(port)
        return self.oracle.process(port, buf, **kw)

    def __getattr__(self, name):
        return getattr(self.oracle, name)


def cases():
    n = 3000
    return {
        # a 4-port bridge in front of a policer: ports 1 and 2 lead to the
        # policer's WAN port, port 3 to its LAN port. A flooded frame reaches
        # the policer up to three times, on two different ports.
        "bridge-fan-pol": CR.Case(
            [CR.bridge_stage(256, 300), CR.pol_stage(64, 10_000_000, 3000)],
            [(0, 1, 1, 0), (0, 2, 1, 0), (0, 3, 1, 1)],
            lambda: CR._bridge_ipv4_trace(21, n, 300, 90)),
        # both directions of a firewall pass one NAT: what the firewall sends
        # to its WAN port enters the NAT's LAN port, and the other way round
        "fw-both-nat": CR.Case(
            [CR.fw_stage(256, 1), CR.nat_stage(64, 1)], [(0, 1, 1, 0), (0, 0, 1, 1)],
            lambda: CR._fw_trace(22, n, 400)),
        # a diamond: the bridge's port 1 through the firewall, its port 2
        # through the policer, both into the NAT's LAN port
        "bridge-fw|pol-nat": CR.Case(
            [CR.bridge_stage(256, 300), CR.fw_stage(256, 1), CR.pol_stage(64, 10_000_000, 3000),
             CR.nat_stage(64, 150)],
            [(0, 1, 1, 0), (1, 1, 3, 0), (0, 2, 2, 0), (2, 1, 3, 0)],
            lambda: CR._bridge_ipv4_trace(23, n, 300, 90)),
    }


def merged_stages(links):
    """The stages with more than one inbound link."""
    t = [link[2] for link in links]
    return sorted({x for x in t if t.count(x) > 1})


def reference(case, snap=False):
    """The reference's run of a case: (trace, per-stage results, per-stage in
    ports, per-stage final state, per-stage snapshots or None)."""
    trace = case.trace()
    orcs = [Recorded(st.oracle()) for st in case.stages]
    for s, mk in (case.prime or {}).items():
        pf, pl, pd, pn = mk()
        orcs[s].oracle.run(pf.copy(), pl, pd, pn, CR.SLOT)
    shots = None
    if snap:
        res, shots = CR.chain_reference(orcs, case.links, *trace, CR.SLOT,
                                        snap=lambda s: case.stages[s].o_dump(orcs[s].oracle))
    else:
        res = CR.chain_reference(orcs, case.links, *trace, CR.SLOT)
    ins = [np.array(o.ports, np.uint16) for o in orcs]
    state = [st.o_dump(o.oracle) for st, o in zip(case.stages, orcs)]
    return trace, res, ins, state, shots


def link_origins(res, ins, link):
    """The origins of the packets that travel over `link`, in order: what its
    source stage sent to the link's out port, floods included."""
    s, p, _, _ = link
    origin, out = res[s][0], res[s][1]
    sent = (out != ins[s]) & ((out == p) | ((out == vigor_amd.FLOOD_FRAME) & (ins[s] != p)))
    return origin[sent]
