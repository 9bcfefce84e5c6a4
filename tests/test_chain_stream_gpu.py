"""vigor_amd.Chain with cable="stream" on the GPU against
chainref.chain_reference: the fw -> nat and bridge -> pol chains of
test_chain_gpu.py, every link rehearsed as a packed byte stream (vp_tx_pack,
then vp_rx_unpack) instead of vp_tx_rebatch. Per stage the packets it received
(by their index in the input), its out ports, lengths and origins and, after
the run, every stage's whole table state must equal the reference's. A stream
drops what lies past a frame's length, so behind a link the frame bytes are
compared up to min(len, slot) and must be zero beyond. One more case runs the
same chains with the default cable, whole slots compared, as before."""
import numpy as np
import pytest
import torch

import chainref as CR
import vigor_amd
from gpuh import run_gpu

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name):
    """The reference's run of a case, computed once: (trace, per-stage
    results, per-stage final state)."""
    if name not in _ref:
        case = CR.cases()[name]
        trace = case.trace()
        orcs = [st.oracle() for st in case.stages]
        for s, mk in (case.prime or {}).items():
            pf, pl, pd, pn = mk()
            orcs[s].run(pf.copy(), pl, pd, pn, CR.SLOT)
        res = CR.chain_reference(orcs, case.links, *trace, CR.SLOT)
        state = [st.o_dump(o) for st, o in zip(case.stages, orcs)]
        _ref[name] = (trace, res, state)
    return _ref[name]


def to_dev(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


def run_case(name, feed, cable):
    case = CR.cases()[name]
    (fr, ln, dv, now), ref, ref_state = reference(name)
    n, slot = len(ln), CR.SLOT
    nfs = [st.gpu() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        run_gpu(nfs[s], *mk(), slot)
    if cable is None:
        chain = vigor_amd.Chain(nfs, case.links)
        assert chain.cable == "slots"
    else:
        chain = vigor_amd.Chain(nfs, case.links, cable=cable)
    cuts = [0, n] if feed == "one-batch" else [0, n // 3, n // 3 + 700, n]
    got = [([], [], [], []) for _ in nfs]
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = chain.run(to_dev(fr[a * slot:b * slot], np.uint8), to_dev(ln[a:b], np.uint16),
                        to_dev(dv[a:b], np.uint16), slot, now=to_dev(now[a:b], np.int64))
        assert len(res) == len(nfs)
        for s, r in enumerate(res):
            assert r["n"] == r["lens"].numel() == r["out"].numel() == r["origin"].numel()
            assert r["frames"].numel() == r["n"] * slot
            got[s][0].append(r["origin"].cpu().numpy() + a)
            got[s][1].append(r["out"].cpu().numpy().view(np.uint16))
            got[s][2].append(r["frames"].cpu().numpy())
            got[s][3].append(r["lens"].cpu().numpy().view(np.uint16))
    for s, (origin, out, slots, ls) in enumerate(ref):
        g_origin, g_out, g_slots, g_ls = (np.concatenate(x) for x in got[s])
        assert origin.size >= n // 4  # (the stage is exercised)
        assert g_origin.size == origin.size, "stage %d received %d packets, not %d" % (
            s, g_origin.size, origin.size)
        assert g_origin.tolist() == origin.tolist(), "stage %d: origin" % s
        assert g_ls.tolist() == ls.tolist(), "stage %d: len" % s
        bad = np.nonzero(g_out != out)[0]
        assert bad.size == 0, "stage %d: out ports differ at %s: %s vs %s" % (
            s, bad[:8], g_out[bad[:8]], out[bad[:8]])
        g2, r2 = g_slots.reshape(-1, slot), slots.reshape(-1, slot)
        if cable == "stream" and s > 0:
            past = np.arange(slot)[None, :] >= np.minimum(ls.astype(np.int64), slot)[:, None]
            dirty = np.nonzero((g2 * past).any(axis=1))[0]
            assert dirty.size == 0, "stage %d: bytes past len at its packets %s" % (s, dirty[:8])
            r2 = np.where(past, 0, r2)
        badf = np.nonzero((g2 != r2).any(axis=1))[0]
        assert badf.size == 0, "stage %d: frames differ at its packets %s" % (s, badf[:8])
    for s, (st, nf) in enumerate(zip(case.stages, nfs)):
        for g_tab, o_tab in zip(st.g_dump(nf), ref_state[s]):
            np.testing.assert_array_equal(g_tab[0], o_tab[0], "stage %d: alloc" % s)
            live = o_tab[0] == 1
            for g_col, o_col in zip(g_tab[1:], o_tab[1:]):
                np.testing.assert_array_equal(g_col[live], o_col[live], "stage %d: state" % s)
    for nf in nfs:
        nf.close()


@pytest.mark.parametrize("feed", ["one-batch", "three-batches"])
@pytest.mark.parametrize("name", ["fw-nat", "bridge-pol"])
def test_stream_cable_matches_the_per_packet_reference(name, feed):
    run_case(name, feed, "stream")


@pytest.mark.parametrize("name", ["fw-nat", "bridge-pol"])
def test_default_cable_returns_what_it_returned_before(name):
    run_case(name, "three-batches", None)
    run_case(name, "one-batch", "slots")
