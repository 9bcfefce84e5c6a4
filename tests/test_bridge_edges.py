"""The directed vigbridge traces of bridge_cases.py against the oracle alone:
the out ports the traces carry (the Python model's, and the ones written by
hand on every named packet) are the oracle's, the model's final table is the
oracle's, and each trace reaches what it names. No GPU:
test_bridge_edges_gpu.py feeds the same traces to the batch pipeline.
"""
import numpy as np
import pytest

import bridge_cases as B
from bridge_cases import FLOOD


def check_literals(case, walk):
    """Every packet's model port and every named packet's hand-written port
    are the oracle's; a named packet without one fails; the model's final
    table is the oracle's."""
    named = 0
    for b, w in zip(case.batches, walk):
        np.testing.assert_array_equal(w["out"], np.array(b.exp, np.uint16),
                                      "%s, %s" % (case, b.note))
        for j, tag in enumerate(b.tags):
            if tag:
                assert b.want[j] is not None, (case, b.note, j, tag)
                assert w["out"][j] == b.want[j], (case, b.note, j, tag)
                named += 1
    assert named
    last = walk[-1]["states"][len(case.batches[-1].now) - 1]
    assert {m: (v[2], v[1]) for m, v in last.items()} == case.final()


def before(w, j):
    return w["states"][j - 1] if j else w["start"]


# ---------------------------------------------------------------- a, f --
@pytest.mark.parametrize("slot,runts", [(64, False), (64, True), (80, True), (128, True),
                                        (2048, True)])
def test_order_trace(slot, runts):
    c = B.order_case(slot, runts)
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    assert c.all_affine() and [len(b.now) for b in c.batches] == [12, 320, 4096, 200, 64]
    b, w = c.batches[1], walk[1]
    pos = {t: b.tagged(t) for t in set(b.tags) if t}
    # learn precedes lookup: the packet's own src was unknown before it
    (j,) = pos["own-src"]
    assert b.src[j] == b.dst[j] and b.src[j] not in before(w, j) and w["out"][j] == b.dv[j]
    # before / learn / after in one wave; the next pair across the wave's end
    (jb,), (jl,), (ja,), (jn,) = pos["before-learn"], pos["learn"], pos["after-learn"], \
        pos["after-learn-next-wave"]
    assert (jb, jl, ja, jn) == (61, 62, 63, 64) and jl // 64 == ja // 64 != jn // 64
    m = b.src[jl]
    assert b.dst[jb] == b.dst[ja] == m and m not in before(w, jl) and m in w["states"][jl]
    assert w["out"][jb] == FLOOD and w["out"][ja] == b.dv[jl]
    assert b.dst[jn] == b.src[ja] and b.src[ja] not in before(w, ja) and \
        w["out"][jn] == b.dv[ja]
    # two first sightings from different ports, in different waves
    (j1,), (j2,), (jt,), (j0,) = pos["first-sighting"], pos["second-sighting"], \
        pos["to-first-port"], pos["before-first"]
    m = b.src[j1]
    assert b.src[j2] == m and b.dv[j1] != b.dv[j2] and j1 // 64 != j2 // 64 and j0 < j1 < j2 < jt
    assert m not in w["start"] and w["out"][j0] == FLOOD and w["out"][jt] == b.dv[j1]
    assert w["states"][j2][m][2] == b.dv[j1] and w["states"][j2][m][1] == b.now[j2]
    # a known station on a new port keeps its port (and is rejuvenated)
    (jm,), (jt,) = pos["moved"], pos["to-moved"]
    m = b.src[jm]
    assert m in w["start"] and w["start"][m][2] != b.dv[jm]
    assert w["states"][jm][m][2] == w["start"][m][2] == w["out"][jt]
    assert w["states"][jm][m][1] == b.now[jm]
    # the broadcast address as a src is learned
    (j0,), (js,), (ja,) = pos["bcast-before"], pos["bcast-src"], pos["bcast-after"]
    assert b.src[js] == B.BCAST and B.BCAST not in before(w, js)
    assert w["out"][j0] == FLOOD and w["out"][ja] == b.dv[js]
    # each of two neighbours across a boundary is sent to the other's new src
    pairs = [(255, 256, c.batches[1], walk[1])] + \
        [(64 * k - 1, 64 * k, c.batches[2], walk[2]) for k in range(1, 64)]
    for p, q, b, w in pairs:
        assert b.tags[p] == "flood-rev" and b.tags[q] == "fwd-next" and p // 64 != q // 64
        assert b.dst[p] == b.src[q] and b.dst[q] == b.src[p]
        assert b.src[p] not in before(w, p) and b.src[q] not in w["states"][p]
        assert w["out"][p] == FLOOD and w["out"][q] == b.dv[p]
    b, w = c.batches[2], walk[2]
    assert b.tags[0] == "first-to-last" and b.tags[4095] == "last-to-first"
    assert b.dst[0] == b.src[4095] and b.dst[4095] == b.src[0]
    assert b.src[4095] not in w["states"][4094] and b.src[0] not in w["start"]
    # the steady batch learns nothing and every named dst is known
    b, w = c.batches[3], walk[3]
    assert set(w["states"][len(b.now) - 1]) == set(w["start"])
    assert len(b.tagged("steady")) == 10 and FLOOD not in w["out"]
    if runts:
        for bb in c.batches[1:]:
            assert set(range(15)) <= set(bb.ln)
        named_lens = {c.batches[2].ln[j] for j, t in enumerate(c.batches[2].tags) if t}
        assert named_lens & set(range(12)) and {13, 14} <= named_lens  # runts carry rules too
    else:
        assert {ln for bb in c.batches for ln in bb.ln} == {60}
    F = c.batches[1].arrays()[0]
    assert F.shape == (320, slot) and (F[:, 12:] != 0).all()  # dirty past every length


# ------------------------------------------------------------------- b --
def test_table_full_trace():
    c = B.table_full_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[0], walk[0]
    (jf,) = b.tagged("fills")
    assert jf == 63 and len(w["states"][jf]) == c.cap == 64 and len(w["states"][jf - 1]) == 63
    news, again = b.tagged("full-new"), b.tagged("full-again")
    assert len(news) == len(again) == 6 and [b.src[j] for j in news] == [b.src[j] for j in again]
    for j in news + again:  # live == capacity and the MAC absent behind the packet
        assert len(w["states"][j]) == 64 and b.src[j] not in w["states"][j]
        assert w["states"][j] == before(w, j)
    unl = b.tagged("to-unlearned")
    assert {b.dst[j] for j in unl} == {b.src[j] for j in news} and min(unl) > max(again)
    assert all(w["out"][j] == FLOOD for j in unl)
    b1, w1 = c.batches[1], walk[1]
    assert not set(w["states"][len(b.now) - 1]) & set(w1["states"][0]) and len(w1["states"][0]) == 1
    for j in b1.tagged("learned-now"):
        assert b1.src[j] not in before(w1, j) and b1.src[j] in w1["states"][j]
    assert {b1.src[j] for j in b1.tagged("learned-now")} == {b.src[j] for j in news}
    assert all(w1["out"][j] == 1 for j in b1.tagged("to-learned-now"))


# ------------------------------------------------------------------- c --
def test_statics_trace():
    c = B.statics_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    rules = {}
    for m, frm, to in c.statics:
        rules.setdefault((m, frm), to)
    assert len(rules) == len(c.statics) - 1 and rules[(B.S3, 0)] == 2  # the duplicate key
    b, w = c.batches[1], walk[1]
    for m in (B.S1, B.S2, B.S4):  # learned inside batch 1's only segment
        assert m not in w["start"] and m in w["states"][len(b.now) - 1]
    assert B.S3 not in w["states"][len(b.now) - 1]
    seen = set()
    for bi in (1, 2):
        b, w = c.batches[bi], walk[bi]
        for j, tag in enumerate(b.tags):
            rule = rules.get((b.dst[j], b.dv[j]))
            known = b.dst[j] in w["states"][j]
            if tag == "static-flood":
                assert rule == -1 and w["out"][j] == FLOOD
                seen.add((tag, known, bi))
            elif tag == "static-drop":
                assert rule == -2 and w["out"][j] == b.dv[j]
                seen.add((tag, known, bi))
            elif tag == "dup-first":
                assert rule == 2 and w["out"][j] == 2
            elif tag == "other-port":
                assert rule is None and known and any(r[0] == b.dst[j] for r in rules)
                assert w["out"][j] == w["states"][j][b.dst[j]][2]
                seen.add((tag, bi))
            elif tag == "other-port-unknown":
                assert rule is None and not known and w["out"][j] == FLOOD
            elif tag == "own-from-port":
                assert rule == -1 and b.src[j] == b.dst[j] and b.src[j] not in before(w, j)
                assert known and w["states"][j][b.dst[j]][2] == b.dv[j] and w["out"][j] == FLOOD
                seen.add(tag)
    # a -1 rule floods before and after its MAC is learned, in the segment
    # that learns it and in a later one; so does -2 return the in port
    assert {("static-flood", False, 1), ("static-flood", True, 1), ("static-flood", True, 2),
            ("static-drop", False, 1), ("static-drop", True, 1), ("static-drop", True, 2),
            ("other-port", 1), ("other-port", 2), "own-from-port"} <= seen
    assert max(c.batches[1].tagged("other-port")) >= 64  # (and behind the first wave)


# ------------------------------------------------------------------- d --
def test_expiry_trace():
    c = B.expiry_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    e = (c.expire_us * 1000) & 0xFFFFFFFF
    assert e == 704 and c.expire_us * 1000 >= 2**32
    b, w = c.batches[1], walk[1]
    assert len(b.now) == 200 and c.slot == 64 and B.CUT % 64 and B.CUT_D % 64
    sx, sd = w["start"][B.X][1], w["start"][B.D][1]
    assert sx == min(v[1] for v in w["start"].values())
    # the stamp one above, at and one below the cutoff; gone at the cut alone
    for m, s, cut, pre in ((B.X, sx, B.CUT, "x-"), (B.D, sd, B.CUT_D, "d-")):
        assert [b.now[cut - 2 + i] - e - s for i in range(3)] == [-1, 0, 1]
        assert [b.tags[cut - 2 + i] for i in range(3)] == [pre + "below", pre + "at", pre + "above"]
        assert all(b.dst[cut - 2 + i] == m for i in range(3))
        assert m in w["states"][cut - 2] and m in w["states"][cut - 1] and m not in w["states"][cut]
        assert w["states"][cut - 1][m][1] == s  # (a lookup does not stamp)
    for j in range(B.CUT):  # nothing falls due before the cut
        assert set(w["states"][j]) == set(w["start"])
    assert set(w["start"]) - set(w["states"][B.CUT]) == {B.X}
    (jr,) = b.tagged("x-relearn")
    assert jr == B.CUT + 1 and b.dv[jr] != w["start"][B.X][2]
    assert w["states"][jr][B.X][2] == b.dv[jr] and w["out"][jr + 1] == b.dv[jr]
    # D is never a src: only the learn stamps
    assert all(B.D not in bb.src for bb in c.batches[1:]) and B.D in c.batches[0].src
    assert sum(1 for bb in c.batches for d in bb.dst if d == B.D) >= 4
    assert B.D not in w["states"][199] and len(w["states"][199]) == len(w["start"]) - 1


# ------------------------------------------------------------------- e --
def test_free_order_trace():
    c = B.free_order_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[1], walk[1]
    assert len(set(b.now)) == 1 and set(w["states"][len(b.now) - 1]) == set(w["start"])
    last = {}
    for j, m in enumerate(b.src):
        last[m] = j
    order = sorted(last, key=lambda m: last[m])  # oldest stamp first
    assert len(order) == B.N_FREE
    idx = [w["start"][m][0] for m in order]
    assert idx != sorted(idx) and idx != sorted(idx, reverse=True)
    old = w["states"][len(b.now) - 1]
    assert {v[1] for v in old.values()} == {b.now[0]}  # (all stamps tie)
    b2, w2 = c.batches[2], walk[2]
    assert not set(old) & set(w2["states"][0]) and len(w2["states"][0]) == 1
    new = w2["states"][len(b2.now) - 1]
    assert len(new) == B.N_FREE
    # freed oldest stamp first, each freed index the next to be handed out
    # last: new MAC j takes the index of the j-th youngest stamp
    for j in range(B.N_FREE):
        assert new[b2.src[j]][0] == old[order[B.N_FREE - 1 - j]][0], j


# ------------------------------------------------------------------- g --
def test_probe_trace():
    c = B.probe_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    assert c.env == B.PROBE_ENV and c.cap == B.PROBE_CAP
    # by the module's own arithmetic: one home bucket, and more MACs than the
    # home bucket and the next hold together
    assert len(c.G) == B.N_PROBE >= 7 and len(set(c.G)) == B.N_PROBE
    assert {B.home_bucket(B.ether_hash(m), B.PROBE_BUCKETS) for m in c.G} == {c.home}
    assert B.ether_hash(bytes(6)) == 0 and B.home_bucket(0xFFFFFFFF, 64) < 64
    import orc
    for m in c.G:  # the hash in Python is the oracle's
        assert B.ether_hash(m) == orc.lib().orc_ether_hash(m)
    others = {m for b in c.batches for m in b.src} - set(c.G)
    for m in others:
        assert (B.home_bucket(B.ether_hash(m), B.PROBE_BUCKETS) - c.home) % 64 > 8
    G = c.G
    st3 = walk[4]["states"][len(c.batches[4].now) - 1]
    assert all(G[i] in st3 for i in range(8))
    b, w = c.batches[5], walk[5]
    assert b.tombs == 2
    assert set(st3) - set(w["states"][0]) == {G[1], G[4]}  # one per bucket, mid-path
    srcs = {b.src[j] for j in b.tagged("deep-src")}
    assert {G[5], G[6], G[7]} <= srcs  # behind both tombstones
    for j in b.tagged("deep-src"):  # rejuvenated, not learned again
        assert w["states"][j][b.src[j]][2] == st3[b.src[j]][2] != b.dv[j]
        assert w["states"][j][b.src[j]][0] == st3[b.src[j]][0]
    assert {b.dst[j] for j in b.tagged("deep-dst")} == {G[i] for i in (0, 2, 3, 5, 6, 7)}
    b, w = c.batches[6], walk[6]
    end = w["states"][len(b.now) - 1]
    assert G[8] in end and end[G[4]][2] != st3[G[4]][2] and G[1] not in end


# ------------------------------------------------------------------- h --
def test_hot_src_trace():
    c = B.hot_src_case()
    walk = B.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[1], walk[1]
    assert len(b.now) == 4096 and set(b.src) == {c.hot} and set(b.dst) == set(c.dsts)
    end = w["states"][4095]
    assert end[c.hot][1] == c.t_last == b.now[-1]
    assert all(end[d][1] == w["start"][d][1] < b.now[0] for d in c.dsts)
    assert set(end) == set(w["start"])
    # every 256-packet block's touches go to one index, more than a bin slice holds
    for blk in range(0, 4096, B.HOT_BLOCK):
        assert set(b.src[blk:blk + B.HOT_BLOCK]) == {c.hot}
    assert B.HOT_BLOCK > B.HOT_SLICE == 2 * 64 and 4096 // B.HOT_BLOCK == 16
