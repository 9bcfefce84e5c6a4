"""vigor_amd.Chain.process_device on the GPU against chainhomeref: the chains
fw -> nat, fw -> nat -> lb and bridge -> pol standing where one NF stands.
After every batch the caller's whole batch is compared with the composite
reference -- every out port (out is filled with a sentinel first: a packet
nobody writes must keep it), every frame byte up to the slot (cable "stream":
behind a link up to min(len, slot) and zero beyond, which the reference
models) -- then the summed return statistics and, after the run, every stage's
whole table state. Last, the batch is fed to vp_tx_build on a context with the
composite's port count and compared with txref: it is a valid batch for
whatever consumes one NF's."""
import numpy as np
import pytest
import torch

import chainhomeref as H
import chainref as CR
import vigor_amd
from gpuh import run_gpu
from txref import STATS_WORDS, tx_reference

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD
_ref = {}


def reference(name):
    """The reference's run of a case, computed once and left unchanged:
    (trace, per-stage results, per-stage final state)."""
    if name not in _ref:
        case = H.cases()[name][0]
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
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


CASES = [(name, "slots", feed) for name in H.NAMES for feed in ("one-batch", "three-batches")]
# (the stream cable where test_chain_stream_gpu.py covers the chain)
CASES += [(name, "stream", "three-batches") for name in ("fw-nat", "bridge-pol")]


@pytest.mark.parametrize("name,cable,feed", CASES, ids=["-".join(c) for c in CASES])
def test_the_chain_stands_where_one_nf_stands(name, cable, feed):
    case, exits, n_ports = H.cases()[name]
    (fr, ln, dv, now), ref, ref_state = reference(name)
    n, slot = len(ln), CR.SLOT
    want_fr, want_out, want_st, last = H.home_reference(
        case, exits, ref, dv, slot, np.full(n, SENTINEL, np.uint16), stream=cable == "stream")
    nfs = [st.gpu() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        run_gpu(nfs[s], *mk(), slot)
    chain = vigor_amd.Chain(nfs, case.links, cable=cable, exits=exits)
    cuts = [0, n] if feed == "one-batch" else [0, n // 3, n // 3 + 700, n]
    total = dict.fromkeys(H.STATS, 0)
    for a, b in zip(cuts[:-1], cuts[1:]):
        f_t, l_t = to_dev(fr[a * slot:b * slot], np.uint8), to_dev(ln[a:b], np.uint16)
        d_t, n_t = to_dev(dv[a:b], np.uint16), to_dev(now[a:b], np.int64)
        o_t = to_dev(np.full(b - a, SENTINEL, np.uint16), np.uint16)
        st = chain.process_device(f_t, l_t, d_t, o_t, slot, now=n_t)
        assert sorted(st) == sorted(H.STATS)
        for key, v in st.items():
            total[key] += v
        g_out = o_t.cpu().numpy().view(np.uint16)
        bad = np.nonzero(g_out != want_out[a:b])[0]
        assert bad.size == 0, "batch at %d: out differs at %s: %s vs %s (last word: stage %s)" % (
            a, bad[:8], g_out[bad[:8]], want_out[a + bad[:8]], last[a + bad[:8]])
        g2 = f_t.cpu().numpy().reshape(b - a, slot)
        badf = np.nonzero((g2 != want_fr[a * slot:b * slot].reshape(b - a, slot)).any(axis=1))[0]
        assert badf.size == 0, "batch at %d: frames differ at %s (last word: stage %s)" % (
            a, badf[:8], last[a + badf[:8]])
    assert total == want_st
    for s, (st, nf) in enumerate(zip(case.stages, nfs)):
        for g_tab, o_tab in zip(st.g_dump(nf), ref_state[s]):
            np.testing.assert_array_equal(g_tab[0], o_tab[0], "stage %d: alloc" % s)
            live = o_tab[0] == 1
            for g_col, o_col in zip(g_tab[1:], o_tab[1:]):
                np.testing.assert_array_equal(g_col[live], o_col[live], "stage %d: state" % s)
    # the last batch as any consumer of one NF's batch takes it
    box = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], n_ports), gpu=0)
    m = b - a
    idx = torch.zeros(m * max(1, n_ports - 1), dtype=torch.int32, device="cuda:0")
    offset = torch.zeros(n_ports + 1, dtype=torch.int32, device="cuda:0")
    stats = torch.zeros(STATS_WORDS, dtype=torch.int64, device="cuda:0")
    box.tx_build(o_t, d_t, l_t, idx, offset, stats)
    torch.cuda.synchronize()
    e_idx, e_off, e_stats = tx_reference(want_out[a:b], dv[a:b], ln[a:b], n_ports, idx.numel())
    assert offset.cpu().numpy().view(np.uint32).tolist() == e_off.tolist()
    assert stats.cpu().numpy().view(np.uint64).tolist() == e_stats.tolist()
    assert idx.cpu().numpy().view(np.uint32)[:e_idx.size].tolist() == e_idx.tolist()
    assert int(e_off[n_ports]) >= 32 * len(exits)  # (every exit's list holds packets)
    for nf in nfs + [box]:
        nf.close()
