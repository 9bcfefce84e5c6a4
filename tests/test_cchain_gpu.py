"""vigor_amd.CChain -- the C-ABI chain object (vp_chain_*) -- on the GPU,
against the references the Python chain is held to:

  * home: CChain.process_device against chainhomeref.home_reference, driven as
    test_chain_home_gpu.py drives Chain: every out port (out is filled with a
    sentinel first), every frame byte up to the slot, the summed statistics and
    every stage's whole table state;
  * stages: CChain.run against chainref.chain_reference per stage (packets by
    origin, in port, out port, lens, frame bytes), for the three-stage line and
    the chains with merged stages; the diamond also byte for byte against
    vigor_amd.Chain on twin contexts;
  * vp_chain_create's graph checks on real contexts, the empty batch, and the
    composing kernel one entry past a wave and past a block.

The references are computed once per case and left unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import chainhomeref as H
import chainmergeref as M
import chainref as CR
import vigor_amd
from gpuh import run_gpu
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD
_ref = {}


def line_reference(case):
    """chainmergeref.reference's tuple for a case with one cable into every
    stage: (trace, per-stage results, per-stage in ports, per-stage state)."""
    trace = case.trace()
    orcs = [st.oracle() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        pf, pl, pd, pn = mk()
        orcs[s].run(pf.copy(), pl, pd, pn, CR.SLOT)
    res = CR.chain_reference(orcs, case.links, *trace, CR.SLOT)
    ins = [np.asarray(trace[2], np.uint16)]
    for t in range(1, len(case.stages)):
        q = [link[3] for link in case.links if link[2] == t]
        ins.append(np.full(res[t][0].size, q[0], np.uint16))
    state = [st.o_dump(o) for st, o in zip(case.stages, orcs)]
    return trace, res, ins, state


def kernel_case():
    """fw -> nat -> lb fed LAN packets of 48 flows that all travel on: nothing
    expires, both tables hold every flow."""
    n = 65 + 2049
    return CR.Case([CR.fw_stage(256, 60_000_000), CR.nat_stage(128, 60_000_000),
                    CR.lb_stage(64, 16, 17, 60_000_000, 60_000_000)],
                   [(0, 1, 1, 0), (1, 1, 2, 2)], lambda: T.fw_trace(n, 48),
                   prime={2: lambda: CR._lb_heartbeats(8)})


def get_case(name):
    if name == "line-all-travel":
        return kernel_case()
    return (M.cases() if name in M.cases() else CR.cases())[name]


def reference(name):
    """(trace, per-stage results, per-stage in ports, per-stage final state) of
    a case, computed once."""
    if name not in _ref:
        case = get_case(name)
        _ref[name] = M.reference(case)[:4] if name in M.cases() else line_reference(case)
    return _ref[name]


def to_dev(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


def make(case):
    nfs = [st.gpu() for st in case.stages]
    for s, mk in (case.prime or {}).items():
        run_gpu(nfs[s], *mk(), CR.SLOT)
    return nfs


def check_state(case, nfs, ref_state):
    for s, (st, nf) in enumerate(zip(case.stages, nfs)):
        for g_tab, o_tab in zip(st.g_dump(nf), ref_state[s]):
            np.testing.assert_array_equal(g_tab[0], o_tab[0], "stage %d: alloc" % s)
            live = o_tab[0] == 1
            for g_col, o_col in zip(g_tab[1:], o_tab[1:]):
                np.testing.assert_array_equal(g_col[live], o_col[live], "stage %d: state" % s)


def received(chain):
    """Per stage, the packets it received in the chain's last run: n of
    vp_chain_view_get, read through the binding (process_device returns only
    the statistics)."""
    v, ns = vigor_amd.ChainViewC(), []
    for s in range(len(chain.stages)):
        assert chain.L.vp_chain_view_get(chain.h, s, C.byref(v)) == 0
        ns.append(int(v.n))
    return ns


def close(*things):
    for x in things:
        x.close()


# ------------------------------------------------------------------ home --

HOME = [(name, "slots", feed) for name in H.NAMES for feed in ("one-batch", "three-batches")]
HOME += [(name, "stream", "three-batches") for name in ("fw-nat", "bridge-pol")]


@pytest.mark.parametrize("name,cable,feed", HOME, ids=["-".join(c) for c in HOME])
def test_the_c_chain_stands_where_one_nf_stands(name, cable, feed):
    case, exits, n_ports = H.cases()[name]
    (fr, ln, dv, now), ref, _, ref_state = reference(name)
    n, slot = len(ln), CR.SLOT
    want_fr, want_out, want_st, last = H.home_reference(
        case, exits, ref, dv, slot, np.full(n, SENTINEL, np.uint16), stream=cable == "stream")
    nfs = make(case)
    chain = vigor_amd.CChain(nfs, case.links, cable=cable, exits=exits)
    cuts = [0, n] if feed == "one-batch" else [0, n // 3, n // 3 + 700, n]
    total = dict.fromkeys(H.STATS, 0)
    reached = np.zeros(len(nfs), np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        f_t, l_t = to_dev(fr[a * slot:b * slot], np.uint8), to_dev(ln[a:b], np.uint16)
        d_t, n_t = to_dev(dv[a:b], np.uint16), to_dev(now[a:b], np.int64)
        o_t = to_dev(np.full(b - a, SENTINEL, np.uint16), np.uint16)
        st = chain.process_device(f_t, l_t, d_t, o_t, slot, now=n_t)
        assert sorted(st) == sorted(H.STATS)
        for key, v in st.items():
            total[key] += v
        reached += np.array(received(chain))
        g_out = o_t.cpu().numpy().view(np.uint16)
        bad = np.nonzero(g_out != want_out[a:b])[0]
        assert bad.size == 0, "batch at %d: out differs at %s: %s vs %s (last word: stage %s)" % (
            a, bad[:8], g_out[bad[:8]], want_out[a + bad[:8]], last[a + bad[:8]])
        g2 = f_t.cpu().numpy().reshape(b - a, slot)
        badf = np.nonzero((g2 != want_fr[a * slot:b * slot].reshape(b - a, slot)).any(axis=1))[0]
        assert badf.size == 0, "batch at %d: frames differ at %s (last word: stage %s)" % (
            a, badf[:8], last[a + badf[:8]])
    assert total == want_st
    assert reached.tolist() == [r[0].size for r in ref]
    if name == "fw-nat-lb":  # stage 2's source is stage 1: its origins are composed
        assert reached[2] >= 32
    check_state(case, nfs, ref_state)
    close(chain, *nfs)


# ---------------------------------------------------------------- stages --

def feed_run(chain, trace, cuts, merged, in_ports):
    """The trace through chain.run, cut into batches; per stage the
    concatenated (origin, out, frames, lens, in port)."""
    fr, ln, dv, now = trace
    slot = CR.SLOT
    got = [([], [], [], [], []) for _ in chain.stages]
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = chain.run(to_dev(fr[a * slot:b * slot], np.uint8), to_dev(ln[a:b], np.uint16),
                        to_dev(dv[a:b], np.uint16), slot, now=to_dev(now[a:b], np.int64))
        assert len(res) == len(chain.stages)
        for s, r in enumerate(res):
            assert r["n"] == r["lens"].numel() == r["out"].numel() == r["origin"].numel()
            assert r["frames"].numel() == r["n"] * slot
            assert r["origin"].dtype == torch.int64
            got[s][0].append(r["origin"].cpu().numpy() + a)
            got[s][1].append(r["out"].cpu().numpy().view(np.uint16))
            got[s][2].append(r["frames"].cpu().numpy())
            got[s][3].append(r["lens"].cpu().numpy().view(np.uint16))
            if s in merged:
                got[s][4].append(r["in_dev"].cpu().numpy().view(np.uint16))
            elif s:
                assert "in_dev" not in r
                got[s][4].append(np.full(r["n"], in_ports[s], np.uint16))
            else:
                got[s][4].append(dv[a:b])
    return [tuple(np.concatenate(x) for x in g) for g in got]


def check_stages(got, ref, ref_ins):
    slot = CR.SLOT
    for s, (origin, out, slots, ls) in enumerate(ref):
        g_origin, g_out, g_slots, g_ls, g_in = got[s]
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


def first_in_ports(case):
    ports = [None] * len(case.stages)
    for s, p, t, q in case.links:
        if ports[t] is None:
            ports[t] = q
    return ports


@pytest.mark.parametrize("feed", ["one-batch", "several-batches"])
@pytest.mark.parametrize("name", ["fw-nat-lb", "bridge-fan-pol", "fw-both-nat",
                                  "bridge-fw|pol-nat"])
def test_c_chain_stages_match_the_per_packet_reference(name, feed):
    case = get_case(name)
    trace, ref, ref_ins, ref_state = reference(name)
    n = len(trace[1])
    nfs = make(case)
    chain = vigor_amd.CChain(nfs, case.links)
    merged = M.merged_stages(case.links)
    if feed == "one-batch":
        cuts = [0, n]
    else:
        cuts = [0, n // 2 + 311, n] if merged else [0, n // 3, n // 3 + 700, n]
    got = feed_run(chain, trace, cuts, merged, first_in_ports(case))
    check_stages(got, ref, ref_ins)
    check_state(case, nfs, ref_state)
    close(chain, *nfs)


def test_diamond_views_equal_the_python_chain_on_twin_contexts():
    """Both branches' origins are composed before the merge keys them: every
    view of the C object against vigor_amd.Chain.run, byte for byte, over two
    consecutive batches."""
    case = get_case("bridge-fw|pol-nat")
    fr, ln, dv, now = reference("bridge-fw|pol-nat")[0]
    n, slot = len(ln), CR.SLOT
    nfs_c, nfs_p = make(case), make(case)
    c_chain = vigor_amd.CChain(nfs_c, case.links)
    p_chain = vigor_amd.Chain(nfs_p, case.links)
    seen = 0
    for a, b in ((0, n // 2 + 311), (n // 2 + 311, n)):
        args = lambda: (to_dev(fr[a * slot:b * slot], np.uint8),  # noqa: E731
                        to_dev(ln[a:b], np.uint16), to_dev(dv[a:b], np.uint16), slot)
        res_c = c_chain.run(*args(), now=to_dev(now[a:b], np.int64))
        res_p = p_chain.run(*args(), now=to_dev(now[a:b], np.int64))
        for s, (rc, rp) in enumerate(zip(res_c, res_p)):
            assert rc["n"] == rp["n"], "stage %d" % s
            for key in ("frames", "lens", "out", "origin"):
                assert torch.equal(rc[key], rp[key]), "stage %d: %s" % (s, key)
            assert ("in_dev" in rc) == ("in_dev" in rp)
            if "in_dev" in rp:
                assert torch.equal(rc["in_dev"], rp["in_dev"]), "stage %d: in_dev" % s
        seen += res_c[3]["n"]
    assert seen >= 32  # (the merged stage received packets)
    close(c_chain, *nfs_c, *nfs_p)


# ---------------------------------------------------------------- create --

def test_create_checks_the_graph_and_a_valid_chain_still_works():
    case = get_case("fw-nat-lb")
    trace, ref, _, _ = reference("fw-nat-lb")
    nfs = make(case)  # fw: 2 ports, nat: 2 ports, lb: 3 ports
    two, line = nfs[:2], [(0, 1, 1, 0)]
    bad_links = [
        (two, [(0, 1, 5, 0)]),                     # a stage outside the chain
        (two, [(3, 1, 1, 0)]),
        (two, [(1, 1, 1, 0)]),                     # backward
        (two, line + [(1, 0, 0, 0)]),
        (two, [(0, 2, 1, 0)]),                     # a port stage 0 does not have
        (two, [(0, 1, 1, 0x10000)]),               # arrives beyond 16 bits
        (nfs, line),                               # stage 2 without an inbound link
        (two, [(0, 1, 1, 0)] * (vigor_amd.TX_MERGE_MAX + 1)),
        (two, [(0, 1, 1, 0), (0, 1, 1, 1)]),       # feeds a merging stage twice
        (nfs, line + [(0, 0, 2, 0), (1, 1, 2, 2), (0, 0, 1, 1)]),
    ]
    for stages, links in bad_links:
        with pytest.raises(ValueError) as e:
            vigor_amd.CChain(stages, links)
        assert "vp_chain_create" in str(e.value) and ("link" in str(e.value) or
                                                      "stage" in str(e.value)), links
    for bad in ({(0, 1): 3},        # a linked port
                {(0, 2): 3},        # a port stage 0 does not have
                {(2, 0): 3},        # a stage the chain does not have
                {(1, 1): 0x10000}):  # beyond 16 bits
        with pytest.raises(ValueError) as e:
            vigor_amd.CChain(two, line, exits=bad)
        assert "exit" in str(e.value), bad
    with pytest.raises(ValueError):
        vigor_amd.CChain(two, line, cable="wire")
    # the same contexts in a valid chain: the first 500 packets against the
    # reference's (it pushes packet by packet: a prefix of its results)
    (fr, ln, dv, now), m, slot = trace, 500, CR.SLOT
    chain = vigor_amd.CChain(nfs, case.links, exits=H.EXITS["fw-nat-lb"][0])
    res = chain.run(to_dev(fr[:m * slot], np.uint8), to_dev(ln[:m], np.uint16),
                    to_dev(dv[:m], np.uint16), slot, now=to_dev(now[:m], np.int64))
    for s, (origin, out, _, _) in enumerate(ref):
        keep = origin < m
        assert res[s]["origin"].cpu().numpy().tolist() == origin[keep].tolist(), "stage %d" % s
        assert res[s]["out"].cpu().numpy().view(np.uint16).tolist() == out[keep].tolist()
    close(chain, *nfs)


def test_empty_batch():
    case = get_case("fw-nat-lb")
    nfs = make(case)
    chain = vigor_amd.CChain(nfs, case.links, exits=H.EXITS["fw-nat-lb"][0])
    z8, z16 = to_dev(np.zeros(0, np.uint8), np.uint8), to_dev(np.zeros(0, np.uint16), np.uint16)
    st = chain.process_device(z8, z16, z16.clone(), z16.clone(), CR.SLOT,
                              now=to_dev(np.zeros(0, np.int64), np.int64))
    assert st == dict.fromkeys(H.STATS, 0)
    assert received(chain) == [0, 0, 0]
    res = chain.run(z8, z16, 0, CR.SLOT)
    assert [r["n"] for r in res] == [0, 0, 0]
    assert all(r["out"].numel() == 0 and r["origin"].numel() == 0 for r in res)
    for nf in nfs[:2]:
        assert nf.live_count() == 0  # (nothing ran)
    close(chain, *nfs)


# ---------------------------------------------------------------- kernel --

def test_composed_origins_one_past_a_wave_and_one_past_a_block():
    """fw -> nat -> lb fed 65 and then 2,049 packets that all travel on: stage
    2's origins come from chn_compose, one entry past a wave's turn and one
    past a block's share."""
    case = get_case("line-all-travel")
    trace, ref, ref_ins, ref_state = reference("line-all-travel")
    n = len(trace[1])
    assert n == 65 + 2049
    for origin, _, _, _ in ref:
        assert origin.tolist() == list(range(n))  # every packet reaches every stage
    nfs = make(case)
    chain = vigor_amd.CChain(nfs, case.links)
    got = feed_run(chain, trace, [0, 65, n], [], first_in_ports(case))
    assert got[2][0].tolist() == list(range(n))
    check_stages(got, ref, ref_ins)
    check_state(case, nfs, ref_state)
    close(chain, *nfs)
