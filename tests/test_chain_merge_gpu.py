"""vigor_amd.Chain with merged stages on the GPU against
chainref.chain_reference: per stage the packets it received (by their index
in the input), the port each arrived on, its out ports, every frame byte and
lens, and after the run every stage's whole table state against its oracle's.
Each trace is fed both as one batch and as two consecutive ones; state and the
chain's buffers carry over. The cases and the conditions their traces meet are
chainmergeref's (checked without a GPU by test_chain_merge_ref.py)."""
import numpy as np
import pytest
import torch

import chainmergeref as M
import chainref as CR
import vigor_amd

pytestmark = pytest.mark.gpu

_ref = {}


def reference(name):
    """The reference's run of a case, computed once."""
    if name not in _ref:
        _ref[name] = M.reference(M.cases()[name])
    return _ref[name]


def to_dev(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


@pytest.mark.parametrize("feed", ["one-batch", "two-batches"])
@pytest.mark.parametrize("name", ["bridge-fan-pol", "fw-both-nat", "bridge-fw|pol-nat"])
def test_chain_with_merged_stages_matches_the_per_packet_reference(name, feed):
    case = M.cases()[name]
    (fr, ln, dv, now), ref, ref_ins, ref_state, _ = reference(name)
    n, slot = len(ln), CR.SLOT
    nfs = [st.gpu() for st in case.stages]
    chain = vigor_amd.Chain(nfs, case.links)
    merged = M.merged_stages(case.links)
    cuts = [0, n] if feed == "one-batch" else [0, n // 2 + 311, n]
    got = [([], [], [], [], []) for _ in nfs]
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
            if s in merged:
                got[s][4].append(r["in_dev"].cpu().numpy().view(np.uint16))
            elif s:
                got[s][4].append(np.full(r["n"], chain.inbound[s][2], np.uint16))
            else:
                got[s][4].append(dv[a:b])
    for s, (origin, out, slots, ls) in enumerate(ref):
        g_origin, g_out, g_slots, g_ls, g_in = (np.concatenate(x) for x in got[s])
        assert g_origin.size == origin.size, "stage %d received %d packets, not %d" % (
            s, g_origin.size, origin.size)
        assert g_origin.tolist() == origin.tolist(), "stage %d: origin" % s
        assert g_in.tolist() == ref_ins[s].tolist(), "stage %d: in port" % s
        assert g_ls.tolist() == ls.tolist(), "stage %d: len" % s
        bad = np.nonzero(g_out != out)[0]
        assert bad.size == 0, "stage %d: out ports differ at %s: %s vs %s" % (
            s, bad[:8], g_out[bad[:8]], out[bad[:8]])
        badf = np.nonzero((g_slots.reshape(-1, slot) != slots.reshape(-1, slot)).any(axis=1))[0]
        assert badf.size == 0, "stage %d: frames differ at its packets %s" % (s, badf[:8])
    for s, (st, nf) in enumerate(zip(case.stages, nfs)):
        for g_tab, o_tab in zip(st.g_dump(nf), ref_state[s]):
            np.testing.assert_array_equal(g_tab[0], o_tab[0], "stage %d: alloc" % s)
            live = o_tab[0] == 1
            for g_col, o_col in zip(g_tab[1:], o_tab[1:]):
                np.testing.assert_array_equal(g_col[live], o_col[live], "stage %d: state" % s)
    for nf in nfs:
        nf.close()
