"""The chain cases with merged stages (chainmergeref.py), without a GPU:
vigor_amd.Chain accepts their links and still refuses backward links and more
than VP_TX_MERGE_MAX inbound links, and the reference's own run of every trace
meets the conditions the GPU comparison relies on: every merged stage receives
packets over each of its inbound links and at least a quarter of the input in
total, drops at least one packet and forwards at least one, expires at least
one entry; with a bridge at least 32 input packets reach the merged stage more
than once (ties), in the diamond at least one through both branches; and the
origins at every stage do not decrease."""
from types import SimpleNamespace

import numpy as np
import pytest

import chainmergeref as M
import chainref as CR
import vigor_amd

NAMES = ["bridge-fan-pol", "fw-both-nat", "bridge-fw|pol-nat"]


@pytest.mark.parametrize("name", NAMES)
def test_reference_meets_the_conditions(name):
    case = M.cases()[name]
    chain = vigor_amd.Chain(case.stages, case.links)  # (reads only cfg.n_devices)
    merged = M.merged_stages(case.links)
    assert merged == [len(case.stages) - 1]
    for t in range(1, len(case.stages)):
        want = [(s, p, q) for s, p, t2, q in case.links if t2 == t]
        assert chain.inbounds[t] == want and chain.inbound[t] == want[0]
    (fr, ln, dv, now), res, ins, state, shots = M.reference(case, snap=True)
    n = len(ln)
    assert n == 3000 and (np.diff(now) >= 0).all()
    for s, (origin, out, slots, ls) in enumerate(res):
        assert slots.size == origin.size * CR.SLOT == ins[s].size * CR.SLOT
        assert (np.diff(origin) >= 0).all(), "stage %d: origins decrease" % s
    for t in merged:
        origin, out = res[t][0], res[t][1]
        over = [M.link_origins(res, ins, l) for l in case.links if l[2] == t]
        assert all(o.size > 0 for o in over), "a link into stage %d carries nothing" % t
        assert sum(o.size for o in over) == origin.size
        assert origin.size >= n // 4, "stage %d receives %d of %d" % (t, origin.size, n)
        assert (out == ins[t]).any(), "stage %d drops nothing" % t
        assert (out != ins[t]).any(), "stage %d forwards nothing" % t
        assert CR.expired_between(shots[t]), "nothing expires at stage %d" % t
        if case.stages[0].kind == "bridge":
            _, times = np.unique(origin, return_counts=True)
            assert (times > 1).sum() >= 32, "few ties at stage %d" % t
    if name == "bridge-fan-pol":
        assert set(ins[1].tolist()) == {0, 1}  # the per-packet in port matters
    if name == "bridge-fw|pol-nat":
        a, b = (M.link_origins(res, ins, l) for l in case.links if l[2] == 3)
        assert np.intersect1d(a, b).size >= 1, "no packet arrives through both branches"


def _stage(nd=2):
    return SimpleNamespace(cfg=SimpleNamespace(n_devices=nd))


def test_chain_accepts_up_to_the_merge_limit():
    m = vigor_amd.TX_MERGE_MAX
    c = vigor_amd.Chain([_stage(m + 1), _stage()], [(0, p, 1, p % 2) for p in range(m)])
    assert len(c.inbounds[1]) == m and c.inbound[1] == (0, 0, 0)
    assert c.inbounds[0] == [] and c.inbound[0] is None
    with pytest.raises(ValueError):
        vigor_amd.Chain([_stage(m + 1), _stage()], [(0, p, 1, 0) for p in range(m + 1)])


@pytest.mark.parametrize("links", [
    [(0, 0, 1, 0), (0, 1, 1, 1), (1, 0, 0, 0)],   # a merge, and a backward link
    [(0, 0, 2, 0), (1, 1, 2, 0), (2, 0, 1, 0)],   # backward, into a stage that feeds the merge
    [(0, 0, 2, 0), (0, 1, 2, 0)],                 # stage 1 has no inbound link
    [(0, 0, 1, 0), (0, 1, 1, 0x10000)],           # an in port beyond 16 bits
])
def test_chain_still_rejects(links):
    with pytest.raises(ValueError):
        vigor_amd.Chain([_stage(), _stage(), _stage()], links)
