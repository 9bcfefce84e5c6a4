"""The directed vigpol traces of pol_cases.py against the oracle alone: each
trace reaches what it names (the run lengths, the branch of the bucket
arithmetic, the misses and the expiries), and the literals the traces carry
(out ports and buckets computed with Python integers) are the oracle's. No
GPU: test_pol_edges_gpu.py feeds the same traces to the batch pipeline.
"""
import numpy as np
import pytest

import pol_cases as P
from pol_cases import LAN, WAN, OTHER, NS, RATE, BURST

CAP = 64


def policed(b, j, st1):
    """The packet touched a bucket: WAN, the header parses, and its address
    is in the table behind it (stamped and timed at the packet's time)."""
    k = P.key_of(b.rows[j])
    if b.dv[j] != WAN or not P.parses(b.rows[j], b.ln[j]) or k not in st1:
        return False
    assert st1[k][1] == b.now[j] and st1[k][3] == b.now[j]
    return True


def run_histogram(b, w):
    h = {}
    for j in range(len(b.ln)):
        if policed(b, j, w["states"][j]):
            h[b.k[j]] = h.get(b.k[j], 0) + 1
    return h


def misses(b, w):
    """WAN packets that parse to an address the table did not hold when the
    batch began."""
    return [j for j in range(len(b.ln)) if b.dv[j] == WAN and P.parses(b.rows[j], b.ln[j])
            and P.key_of(b.rows[j]) not in w["start"]]


def can_group(b, w, cap=CAP):
    """pol_segment's conditions for the grouping path over the whole batch:
    long enough, no expiry inside it, no miss, no run above 64."""
    h = run_histogram(b, w)
    life = P.lifetime(b.case.rate, b.case.burst)
    due = any(P.parses(b.rows[j], b.ln[j]) and
              any(v[1] < b.now[j] - life for v in before(w, j).values())
              for j in range(len(b.ln)))
    # the batch driver cuts wherever an expiry may be due by its lower bound
    # of the live stamps, which is exact at best when the batch begins
    floor = min((v[1] for v in w["start"].values()), default=b.now[0])
    due = due or b.now[-1] - life > min(floor, b.now[0])
    return 8 * len(b.ln) >= cap and not due and not misses(b, w) and \
        max(h.values(), default=0) <= 64


def check_literals(case, walk):
    for b, w in zip(case.batches, walk):
        exp = np.array(b.exp)
        m = exp >= 0
        np.testing.assert_array_equal(w["out"][m], exp[m], "%s, %s" % (case, b.note))
        for k, live in b.live_after.items():
            assert (P.key(k) in w["states"][-1]) == live, (case, b.note, k)
        if b.unchanged:
            assert w["states"][-1] == w["start"] and w["start"]
    if case.final is not None:
        st = walk[-1]["states"][-1]
        for k, v in case.final.items():
            if v is None:
                assert P.key(k) not in st, (case, k)
            else:
                assert st[P.key(k)][1:] == (v[1], v[0], v[1]), (case, k, st[P.key(k)], v)


def check_wants(case, walk, cap=CAP):
    """A batch marked "group" can take the grouping path whole; one marked
    "sort" cannot (its last segment holds the miss or the long run, or the
    batch is too short)."""
    for b, w in zip(case.batches, walk):
        assert can_group(b, w, cap) == (b.want == "group"), (case, b.note)
        assert 8 * len(b.ln) < P.PATHS["sort"][0]  # (never groups at capacity 4096)


def tagged(b, tag):
    return [j for j in range(len(b.ln)) if tag in b.tags[j].split(",") or b.tags[j] == tag]


def before(w, j):
    return w["states"][j - 1] if j else w["start"]


# ---------------------------------------------------------------- a. --
@pytest.mark.parametrize("slot", [64, 128])
def test_run_lengths_trace(slot):
    c = P.run_lengths_case(slot)
    walk = P.oracle_walk(c)
    check_literals(c, walk)
    check_wants(c, walk)
    assert len(walk[0]["states"][-1]) == 9 and not walk[0]["start"]
    for b, w, runs in ((c.batches[1], walk[1], P.RUNS), (c.batches[2], walk[2], P.RUNS + [65])):
        h = run_histogram(b, w)
        assert sorted(h.values()) == runs == [1, 2, 7, 8, 9, 16, 63, 64, 65][:len(runs)]
        assert len(b.ln) == sum(runs) and not misses(b, w)
        now = np.array(b.now)
        assert (np.diff(now) == 0).sum() > len(now) // 8 and (np.diff(now) > 0).any()  # ties
        # interleaved: a packet's neighbour mostly belongs to another run, and
        # every run of two or more has forwards and drops
        assert (np.diff(np.array(b.k)) != 0).sum() > len(b.k) // 2
        for k, n in h.items():
            outs = {int(w["out"][j]) for j in range(len(b.ln)) if b.k[j] == k}
            assert outs == ({LAN, WAN} if n >= 2 else {LAN}), (k, n, outs)
        # the strict test is met: some packet finds its bucket at exactly len
        eq = [j for j in range(len(b.ln))
              if c_level(c, before(w, j), b, j) == b.ln[j]]
        assert eq and all(w["out"][j] == WAN for j in eq)


def c_level(case, st0, b, j):
    """The bucket of packet j's address after the refill, from the state
    before the packet (None for an unknown address)."""
    k = P.key_of(b.rows[j])
    if k not in st0:
        return None
    _, _, size, bt = st0[k]
    diff = b.now[j] - bt
    thr = P.lifetime(case.rate, case.burst)
    return min(case.burst, size + (diff * case.rate % P.U64) // NS) if diff < thr else case.burst


# ---------------------------------------------------------------- b. --
@pytest.mark.parametrize("slot", [64, 128])
def test_state_trace(slot):
    c = P.state_case(slot)
    walk = P.oracle_walk(c)
    check_literals(c, walk)
    check_wants(c, walk)
    assert [b.want for b in c.batches] == \
        ["sort", "group", "sort", "group", "sort", "group", "sort", "group"]
    hs = [run_histogram(b, w) for b, w in zip(c.batches, walk)]
    for step in (1, 2, 3, 5, 6, 7):
        assert hs[step] == P.STATE_RUNS[step], step
    assert max(hs[2].values()) == 65 and not misses(c.batches[2], walk[2])
    assert set(hs[3]) == set(hs[2]) and all(hs[3][k] < hs[2][k] for k in hs[2])
    assert 8 * len(c.batches[6].ln) < CAP and not misses(c.batches[6], walk[6])
    b, w = c.batches[4], walk[4]
    assert max(hs[4].values()) <= 64 and len(misses(b, w)) == 6
    (bb,), (bu,), (ba,) = tagged(b, "big-before-alloc"), tagged(b, "big-unknown"), \
        tagged(b, "big-after-alloc")
    alloc = tagged(b, "alloc")
    assert bb < alloc[0] < ba and b.k[bb] == b.k[alloc[0]] == b.k[ba]
    for j in (bb, bu):  # dropped, nothing written
        assert b.ln[j] > BURST and w["states"][j] == before(w, j) and w["out"][j] == WAN
        assert P.key_of(b.rows[j]) not in w["states"][j]
    assert P.key(b.k[bu]) not in w["states"][-1]
    for j in alloc:
        assert P.key_of(b.rows[j]) not in before(w, j) and policed(b, j, w["states"][j])
    assert b.ln[ba] > BURST and policed(b, ba, w["states"][ba]) and w["out"][ba] == WAN
    assert before(w, ba)[P.key(b.k[ba])][1] < b.now[ba]  # (rejuvenated: the stamp moved)
    for w_ in walk[1:]:
        assert {LAN, WAN} <= set(w_["out"].tolist())


# ---------------------------------------------------------------- c. --
ARITH = P.arith_cases()


@pytest.fixture(scope="module")
def arith_walks():
    return {c.name: P.oracle_walk(c) for c in ARITH}


@pytest.mark.parametrize("case", ARITH, ids=repr)
def test_arith_literals_and_paths(case, arith_walks):
    walk = arith_walks[case.name]
    check_literals(case, walk)
    check_wants(case, walk)
    assert case.final and case.batches[0].want == "sort"


def test_arith_cases_hit_their_branches(arith_walks):
    cases = {c.name: c for c in ARITH}
    assert len(cases) == 9
    seen, ties = set(), 0
    for name, c in cases.items():
        thr = P.lifetime(c.rate, c.burst)
        for b, w in zip(c.batches, arith_walks[name]):
            for j, tag in enumerate(b.tags):
                st0, st1 = before(w, j), w["states"][j]
                k, ln, t = P.key_of(b.rows[j]), b.ln[j], b.now[j]
                lv = c_level(c, st0, b, j)
                if tag == "exact":  # dropped at size == len, the bucket unchanged
                    assert lv == ln and w["out"][j] == WAN and st1[k][2] == ln
                    seen.add("exact")
                elif tag == "plus1":
                    assert lv == ln + 1 and w["out"][j] == LAN and st1[k][2] == 1
                    seen.add("plus1")
                elif tag == "first":
                    assert k not in st0 and ln == c.burst and w["out"][j] == LAN and st1[k][2] == 0
                    seen.add("first")
                elif tag == "big-unknown":
                    assert ln == c.burst + 1 and k not in st0 and st1 == st0 and w["out"][j] == WAN
                    seen.add("big-unknown")
                elif tag == "big-before-alloc":
                    assert ln == c.burst + 1 and k not in st0 and st1 == st0
                    seen.add("big-before-alloc")
                elif tag == "big-after-alloc":
                    assert ln == c.burst + 1 and k not in w["start"] and k in st0
                    assert w["out"][j] == WAN and st0[k][1] < t == st1[k][1] == st1[k][3]
                    seen.add("big-after-alloc")
                elif tag in ("thr-1", "thr") and name == "diff_around_thr":
                    assert t - st0[k][3] == thr + (-1 if tag == "thr-1" else 0)
                    assert lv == (c.burst - 1 if tag == "thr-1" else c.burst) and st0[k][2] == 0
                    assert w["out"][j] == (WAN if tag == "thr-1" else LAN)
                    seen.add(tag)
                elif tag == "thr+1":  # the old entry expired: a new flow
                    assert t - st0[k][3] == thr + 1 and t - st0[k][1] == thr + 1
                    assert ln == c.burst and w["out"][j] == LAN and st1[k][2] == 0
                    seen.add(tag)
                elif tag == "floor0":
                    d = t - st0[k][3]
                    assert 0 < d and d * c.rate // NS == 0 and (d + 1) * c.rate // NS == 1
                    assert st1[k][2] == st0[k][2] == 0 and st1[k][3] == t and w["out"][j] == WAN
                    seen.add(tag)
                elif tag.startswith("gap ") and name == "product_above_2_63":
                    d = t - st0[k][3]
                    assert d < thr and d * c.rate < 2**64
                    if d > NS:  # above 2^63: as a signed product the refill is negative
                        assert d * c.rate > 2**63
                        signed = d * c.rate - 2**64
                        assert (st0[k][2] + int(signed / NS)) % 2**64 != lv == c.burst
                        seen.add("product")
                    else:
                        assert lv == min(c.burst, st0[k][2] + d * c.rate // NS)
                    assert st1[k][2] == lv - ln
                elif tag == "tie" and t == st0[k][3]:  # (not the run's first packet)
                    assert lv == st0[k][2]
                    ties += 1
    assert seen == {"exact", "plus1", "first", "big-unknown", "big-before-alloc",
                    "big-after-alloc", "thr-1", "thr", "thr+1", "floor0", "product"}
    assert ties == 9 + 2
    # the run of 20 floors and the run of 10 ties take the insertion sort
    assert len(tagged(cases["refill_floors_to_zero"].batches[1], "floor0")) == 20
    assert run_histogram(cases["equal_times_in_a_run"].batches[1],
                         arith_walks["equal_times_in_a_run"][1]) == {1: 10, 2: 3}
    # burst * 1e9 wraps: the lifetime is the wrapped product's, entry 1 is
    # gone at batch 2's first packet and address 3 takes its index
    c, w = cases["burst_ns_wraps"], arith_walks["burst_ns_wraps"]
    assert c.burst * NS >= 2**64 and P.lifetime(c.rate, c.burst) == 1553255926290448 < \
        c.burst * NS // c.rate
    old = w[1]["states"][-1]
    new = w[2]["states"][0]
    assert P.key(1) in old and P.key(1) not in new and new[P.key(3)][0] == old[P.key(1)][0]
    assert c.batches[2].now[0] - old[P.key(1)][1] < c.burst * NS // c.rate
    assert len(w[2]["states"][-1]) == 3


# ---------------------------------------------------------------- d. --
@pytest.mark.parametrize("slot", [64, 128])
def test_header_mix_trace(slot):
    c = P.header_mix_case(slot)
    walk = P.oracle_walk(c, 256)
    check_literals(c, walk)
    check_wants(c, walk, 256)
    b, w = c.batches[1], walk[1]
    by_len = {ln: set() for ln in P.LENGTHS}
    devs = set()
    for j, tag in enumerate(b.tags):
        if not tag:
            continue
        ln, dev, ok = b.ln[j], b.dv[j], P.parses(b.rows[j], b.ln[j])
        assert tag.endswith("len%d" % ln)
        # the predicate in Python integers is the oracle's
        if dev == WAN:
            assert policed(b, j, w["states"][j]) == ok, tag
        elif dev == LAN:
            assert (w["out"][j] == WAN) == ok, tag
        else:
            assert w["out"][j] == OTHER
        if not ok:
            assert w["states"][j] == before(w, j) and w["out"][j] == dev
        by_len[ln].add(ok)
        devs.add(dev)
    assert devs == {WAN, LAN, OTHER}
    for ln, oks in by_len.items():
        # 14 and 33 leave fewer than 20 bytes: nothing parses; below 14 the
        # 16-bit difference wraps and a header in the slot parses
        assert oks == ({False} if ln in (14, 33) else {False, True}), (ln, oks)
    assert sum(1 for t in b.tags if t) == 9 * 8 * 3


@pytest.mark.parametrize("slot", [64, 128])
def test_expiry_edge_trace(slot):
    c = P.expiry_edge_case(slot)
    walk = P.oracle_walk(c)
    check_literals(c, walk)
    gone = kept = 0
    for i, (b, w) in enumerate(zip(c.batches[:72], walk)):
        k = P.key(100 + i)
        # in the table until the variant, whose time alone makes it due
        assert k in w["states"][-2] and b.tags[-1] == "variant" and b.tags[0] == "entry"
        life = P.lifetime(RATE, BURST)
        assert b.now[-1] - w["states"][-2][k][1] == life + 1 and b.now[-2] - b.now[0] == 0
        if k in w["states"][-1]:
            kept += 1
        else:
            gone += 1
    assert gone >= 20 and kept >= 20 and gone + kept == 72 == len(c.batches) - 3
    b, w = c.batches[73], walk[73]
    assert not any(P.parses(r, ln) for r, ln in zip(b.rows, b.ln))
    assert b.now[0] - w["start"][P.key(300)][1] > P.lifetime(RATE, BURST)  # (due)


# ---------------------------------------------------------------- e. --
def test_segment_cut_trace():
    c = P.segment_cut_case()
    walk = P.oracle_walk(c)
    check_literals(c, walk)
    check_wants(c, walk)
    b, w = c.batches[1], walk[1]
    cut = P.CUT
    assert len(b.ln) == 200 and c.slot == 64 and cut % 64 and b.tags[cut] == "cut"
    for j in range(cut):  # nothing falls due before the cut
        assert set(w["states"][j]) == set(w["start"])
    assert {P.key(10), P.key(11)} <= set(w["states"][cut - 1])
    assert not {P.key(10), P.key(11)} & set(w["states"][cut])
    assert len(w["states"][cut]) == len(w["start"]) - 2
    (j,) = tagged(b, "realloc")
    assert j > cut and P.key(11) in w["states"][j] and P.key(11) not in w["states"][j - 1]
    hits1 = [j for j in range(200) if b.k[j] == 1]
    assert min(hits1) < cut - 1 in hits1 and cut in hits1 and cut + 1 in hits1 and max(hits1) > cut + 64
    assert {LAN, WAN} <= set(w["out"][:cut].tolist()) and {LAN, WAN} <= set(w["out"][cut:].tolist())
    assert P.key(10) not in w["states"][-1]


# ---------------------------------------------------------------- f. --
def test_free_order_trace():
    c = P.free_order_case()
    walk = P.oracle_walk(c)
    check_literals(c, walk)
    check_wants(c, walk)
    b, w = c.batches[1], walk[1]
    assert len(set(b.now)) == 1 and not misses(b, w)
    last = {}
    for j, k in enumerate(b.k):
        last[k] = j
    order = sorted(last, key=lambda k: last[k])  # oldest stamp first
    assert len(order) == P.N_FREE and order != sorted(order) and order != sorted(order, reverse=True)
    old = w["states"][-1]
    assert {v[1] for v in old.values()} == {b.now[0]}  # (all stamps tie)
    b2, w2 = c.batches[2], walk[2]
    assert not set(old) & set(w2["states"][0]) and len(w2["states"][0]) == 1  # all expire at once
    new = w2["states"][-1]
    assert len(new) == P.N_FREE
    # freed oldest stamp first, each freed index the next to be handed out
    # last: new address j takes the index of the j-th youngest stamp
    for j in range(P.N_FREE):
        assert new[P.key(1001 + j)][0] == old[P.key(order[P.N_FREE - 1 - j])][0], j
