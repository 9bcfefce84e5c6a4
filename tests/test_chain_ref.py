"""The chain cases of test_chain_gpu.py, without a GPU: their links are ones
vigor_amd.Chain accepts, and the reference's own run of every trace
(chainref.chain_reference) meets the conditions the GPU comparison relies on
-- every stage receives at least a quarter of the input, drops at least one
packet and forwards at least one, and at least one entry expires at each
stage."""
import numpy as np
import pytest

import chainref as CR
import vigor_amd


@pytest.mark.parametrize("name", ["fw-nat", "bridge-pol", "fw-nat-lb"])
def test_reference_meets_the_conditions(name):
    case = CR.cases()[name]
    chain = vigor_amd.Chain(case.stages, case.links)  # (reads only cfg.n_devices)
    fr, ln, dv, now = case.trace()
    assert (np.diff(now) >= 0).all()
    orcs = [st.oracle() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        pf, pl, pd, pn = mk()
        assert int(pn.max()) <= int(now[0])
        orcs[s].run(pf.copy(), pl, pd, pn, CR.SLOT)
    res, shots = CR.chain_reference(orcs, case.links, fr, ln, dv, now, CR.SLOT,
                                    snap=lambda s: case.stages[s].o_dump(orcs[s]))
    n = len(ln)
    if name == "fw-nat":  # both directions in the input
        assert (dv == 0).any() and (dv == 1).any()
    for s, (origin, out, slots, ls) in enumerate(res):
        assert slots.size == origin.size * CR.SLOT and (np.diff(origin) > 0).all()
        ins = dv[origin] if s == 0 else np.full(origin.size, chain.inbound[s][2], np.uint16)
        assert origin.size >= n // 4, "stage %d receives %d of %d" % (s, origin.size, n)
        assert (out == ins).any(), "stage %d drops nothing" % s
        assert (out != ins).any(), "stage %d forwards nothing" % s
        assert CR.expired_between(shots[s]), "nothing expires at stage %d" % s
    if name == "bridge-pol":
        assert (res[0][1] == vigor_amd.FLOOD_FRAME).sum() > n // 4
        assert (res[1][3] > CR.SLOT).any()  # lengths beyond the slot come through
