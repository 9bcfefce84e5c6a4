"""The directed vigfw traces of fw_cases.py against the oracle alone: the out
ports and frames the traces carry (the Python model's, and the ports written
by hand on every named packet) are the oracle's, the model's final table is
the oracle's, and each trace reaches what it names. No GPU:
test_fw_edges_gpu.py feeds the same traces to the batch pipeline.
"""
import numpy as np
import pytest

import fw_cases as F
from fw_cases import DROP, LAN, LAN2, WAN


def check_literals(case, walk, matrix=()):
    """Every packet's model port and frame and every named packet's
    hand-written port are the oracle's; a named packet without one fails.
    Exempt are the batches listed in `matrix` (the header matrix alone): their
    tagged packets are generated and carry the model's port, and
    test_matrix_trace works each one's expected port out from its variant,
    length and device, independently of the model. The model's final table is
    the oracle's."""
    named = 0
    for bi, (b, w) in enumerate(zip(case.batches, walk)):
        what = "%s, %s" % (case, b.note)
        np.testing.assert_array_equal(w["out"], b.out_ports(), what)
        np.testing.assert_array_equal(w["frames"], b.frames_after(), what)
        rows = np.stack(b.rows)
        for j, tag in enumerate(b.tags):
            touched = (w["frames"][j] != rows[j]).any()
            assert touched == (not b.exp[j] & DROP), (what, j)
            if tag and bi not in matrix:
                assert b.want[j] is not None, (what, j, tag)
                assert b.want[j] == (int(w["out"][j]) | (0 if touched else DROP)), (what, j, tag)
                named += 1
    assert named or matrix
    last = walk[-1]["states"][len(case.batches[-1].now) - 1]
    assert {k: (v[2], v[1]) for k, v in last.items()} == case.final()


def before(w, j):
    return w["states"][j - 1] if j else w["start"]


def key_of(b, j):
    """The FlowId packet j looks up."""
    k = F.parse(b.rows[j], b.ln[j])
    return (k[1], k[0], k[3], k[2], k[4]) if b.dv[j] == WAN else k


# ------------------------------------------------------------------- a --
@pytest.mark.parametrize("slot", [64, 128])
def test_order_trace(slot):
    c = F.order_case(slot)
    walk = F.oracle_walk(c)
    check_literals(c, walk)
    assert c.all_affine() and [len(b.now) for b in c.batches] == [12, 320, 4096, 320, 200, 64]
    b, w = c.batches[1], walk[1]
    assert (b.tags[61], b.tags[62], b.tags[63]) == ("reply-before", "open", "reply-after")
    assert (b.tags[255], b.tags[256]) == ("open", "reply-after")
    # one 5-tuple opened from two devices: the first wins
    (j1,), (j2,), (jr,) = b.tagged("first-open"), b.tagged("second-open"), b.tagged("reply-to-first")
    k = key_of(b, j1)
    assert key_of(b, j2) == key_of(b, jr) == k and b.dv[j1] == LAN2 and b.dv[j2] == LAN
    assert j1 // 64 != j2 // 64 and k not in before(w, j1)
    assert w["states"][j2][k][2] == LAN2 and w["states"][j2][k][1] == b.now[j2]
    assert w["out"][jr] == LAN2
    assert bytes(w["frames"][jr][0:6]) == F.END_MACS[LAN2] and \
        bytes(w["frames"][jr][6:12]) == F.DEV_MACS[LAN2]
    n_fwd = n_rev = 0
    for bi in (1, 2, 3):
        b, w = c.batches[bi], walk[bi]
        for j, tag in enumerate(b.tags):
            if tag == "open":  # the flow is new at this packet
                k = key_of(b, j)
                assert k not in before(w, j) and w["states"][j][k][2] == b.dv[j]
            elif tag in ("reply-after", "last-reply"):  # opened earlier in this batch
                k = key_of(b, j)
                assert k not in w["start"] and k in before(w, j)
                assert w["out"][j] == before(w, j)[k][2] and w["states"][j][k][1] == b.now[j]
            elif tag == "reply-before":  # opened later in this batch
                k = key_of(b, j)
                assert k not in w["states"][j] and k in w["states"][len(b.now) - 1]
                assert w["out"][j] == WAN and (w["frames"][j] == b.rows[j]).all()
        for p in range(63, len(b.now) - 1, 64):  # neighbours across a multiple of 64
            tp, tq = b.tags[p], b.tags[p + 1]
            if (tp, tq) == ("open", "reply-after"):
                assert key_of(b, p) == key_of(b, p + 1)
                n_fwd += 1
            elif (tp, tq) == ("reply-before", "open"):
                assert key_of(b, p) == key_of(b, p + 1)
                n_rev += 1
    assert n_fwd == 1 + 32 and n_rev == 31 + 2
    b = c.batches[2]
    assert (b.tags[63], b.tags[64]) == ("open", "reply-after")
    assert key_of(b, 0) == key_of(b, 4095) and key_of(b, 1) == key_of(b, 4094)
    assert (c.batches[3].tags[63], c.batches[3].tags[64]) == ("reply-before", "open")
    # the steady batch opens nothing
    b, w = c.batches[4], walk[4]
    assert set(w["states"][len(b.now) - 1]) == set(w["start"]) and len(b.tagged("steady")) == 6
    assert not any(e & DROP for e in b.exp)
    rows = np.stack(c.batches[1].rows)
    assert rows.shape == (320, slot) and (rows[:, 60:] != 0).all()  # dirty past the length


# ------------------------------------------------------------------- b --
@pytest.mark.parametrize("slot", [64, 128])
def test_word3_trace(slot):
    c = F.word3_case(slot)
    walk = F.oracle_walk(c)
    check_literals(c, walk)
    for bi, (b, w) in enumerate(zip(c.batches, walk)):
        end = w["states"][len(b.now) - 1]
        udp, tcp = F.lan_key(2, 17), F.lan_key(2, 6)
        assert udp[:4] == tcp[:4] and udp != tcp and end[udp][2] == LAN and end[tcp][2] == LAN2
        assert end[udp][0] != end[tcp][0] and end[F.lan_key(1)][2] == LAN2
        for tag in ("dev2-open", "udp-open", "tcp-open"):
            (j,) = b.tagged(tag) if bi == 0 else b.tagged(tag.replace("open", "again"))[:1]
            assert (key_of(b, j) in before(w, j)) == (bi == 1)
        for j in b.tagged("dev2-again"):  # a hit: nothing allocated
            assert set(w["states"][j]) == set(before(w, j))
        for j in b.tagged("unreversed"):  # its own 5-tuple is stored, the reversed is not
            own = F.parse(b.rows[j], b.ln[j])
            assert own in w["states"][j] and key_of(b, j) not in w["states"][j]
            assert b.dv[j] == WAN and w["out"][j] == WAN
        (j,) = b.tagged("other-proto")
        k = key_of(b, j)
        assert k not in w["states"][j] and (k[:4] + (17,)) in w["states"][j]
        assert max(b.tagged("dev2-reply")) >= 64 and max(b.tagged("tcp-reply")) >= 64


# ------------------------------------------------------------------- c --
def test_table_full_trace():
    c = F.table_full_case()
    walk = F.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[0], walk[0]
    opens, fulls = b.tagged("open"), b.tagged("full-open")
    assert len(opens) == 16 == c.max_flows and len(fulls) == 4
    assert len(w["states"][opens[-1]]) == 16 and len(w["states"][opens[-1] - 1]) == 15
    for bb, ww in ((b, w), (c.batches[1], walk[1])):
        for j in bb.tagged("full-open"):  # full, the flow absent behind it, yet rewritten
            assert len(ww["states"][j]) == 16 and key_of(bb, j) not in ww["states"][j]
            assert ww["out"][j] == WAN and bytes(ww["frames"][j][6:12]) == F.DEV_MACS[WAN]
        for j in bb.tagged("reply-unstored"):
            assert key_of(bb, j) not in ww["states"][j] and (ww["frames"][j] == bb.rows[j]).all()
        assert len(bb.tagged("reply-unstored")) in (4, 8) and len(bb.tagged("reply-stored")) in (16, 20)
    b2, w2 = c.batches[2], walk[2]
    assert len(w2["states"][0]) == 1 and not set(walk[1]["states"][len(c.batches[1].now) - 1]) & \
        set(w2["states"][0]) - {key_of(b2, 0)}
    assert {key_of(b2, j) for j in b2.tagged("open-now")} == {key_of(b, j) for j in fulls}
    assert len(w2["states"][len(b2.now) - 1]) == 4


# ------------------------------------------------------------------- d --
@pytest.mark.parametrize("slot", [64, 128])
def test_matrix_trace(slot):
    c = F.matrix_case(slot)
    walk = F.oracle_walk(c)
    check_literals(c, walk, matrix=(1,))
    b, w = c.batches[1], walk[1]
    assert len(b.now) <= 4096
    lens = F.LENGTHS + (F.LONG_LENGTHS if slot >= 128 else [])
    cls, lean, offs, devs, by_len = {}, {True: set(), False: set()}, set(), set(), {}
    n = 0
    for j, tag in enumerate(b.tags):
        if not tag:
            continue
        n += 1
        name, ln, dev = tag.split()
        assert int(ln[3:]) == b.ln[j] and int(dev[3:]) == b.dv[j]
        k = F.parse(b.rows[j], b.ln[j])
        ok = k is not None
        cls.setdefault(name, set()).add(ok)
        lean[F.lean(b.rows[j])].add(ok)
        devs.add(b.dv[j])
        by_len.setdefault(b.ln[j], set()).add(ok)
        opt = 4 * ((int(b.rows[j][14]) & 15) - 5)
        moved = opt != 0 and ((b.ln[j] - 14) & 0xFFFF) - 20 >= opt  # (the u16 wrap below 14)
        past = moved and 34 + opt + 4 > slot  # the ports lie past the slot and read as 0
        # the predicate in Python integers is the oracle's: a WAN variant that
        # parses is a hit (unless its ports lie past the slot), any other that
        # parses goes out on the WAN device
        assert (w["out"][j] != b.dv[j] or (w["frames"][j] != b.rows[j]).any()) == \
            (ok and not (past and b.dv[j] == WAN)), tag
        if not ok:
            continue
        offs.add((opt, moved, past))
        if b.dv[j] == WAN:  # flow A's ports at 34, flow B's behind the options
            assert past or w["out"][j] == (LAN2 if moved else LAN), tag
        else:
            assert w["out"][j] == WAN and (k[0], k[1]) == \
                ((0, 0) if past else (0xB80B, 0x5100) if moved else (0xD007, 0x5000)), tag
    assert n == len(lens) * 12 * 3 and devs == {WAN, LAN, LAN2}
    for name, oks in cls.items():
        assert oks == ({False} if name in F.NEVER else {False, True}), (name, oks)
    assert set(cls) == {v for v, _ in F.variants(60)} and len(cls) == 12
    assert lean[True] == {False, True} and lean[False] == {False, True}
    # options borrowed (ihl 6: whenever it parses, from length 38 on) and not
    # (ihl 15 up to length 73); ihl 15's lie inside a 128-byte slot alone, and
    # past the slot for the lengths below 14 that wrap
    assert {(4, True, False), (0, False, False), (40, False, False)} <= offs
    assert ((40, True, False) in offs) == (slot >= 128) and (4, False, False) not in offs
    assert ((40, True, True) in offs) == (slot == 64)
    for ln, oks in by_len.items():
        # below 14 the 16-bit difference wraps and a header in the slot parses;
        # 14 .. 33 leave fewer than 20 bytes, 34 .. 37 fewer than 4 behind them
        assert oks == ({False} if 14 <= ln <= 37 else {False, True}), (ln, oks)
    # every opener the matrix stored is replied to in the next batch
    b2, w2 = c.batches[2], walk[2]
    assert len(b2.now) >= 100 and not any(e & DROP for e in b2.exp)
    assert {int(o) for o in w2["out"]} == {LAN, LAN2}


# ------------------------------------------------------------------- e --
def test_expiry_trace():
    c = F.expiry_case()
    walk = F.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[1], walk[1]
    e = c.expire_us * 1000
    assert len(b.now) == 200 and F.CUT % 64 and c.slot == 64
    ka, kb, kc = F.lan_key(F.XA), F.lan_key(F.XB), F.lan_key(F.XC)
    sa, sb, sc = (w["start"][k][1] for k in (ka, kb, kc))
    assert sa == min(v[1] for v in w["start"].values())
    cut = b.now[F.CUT] - e
    assert b.now[F.CUT] == b.now[F.CUT + 1] == b.now[F.CUT + 2] and b.now[F.CUT - 1] - e == sa
    assert (sa, sb, sc) == (cut - 1, cut, cut + 1)
    assert [b.tags[F.CUT + i] for i in range(3)] == ["x-below", "x-at", "x-above"]
    for j in range(F.CUT):  # nothing falls due before the cut
        assert set(w["states"][j]) == set(w["start"])
    assert set(w["start"]) - set(w["states"][F.CUT]) == {ka}
    assert w["states"][F.CUT + 1][kb][1] == b.now[F.CUT + 1]  # (the reply rejuvenates)
    (jr,) = b.tagged("x-reopen")
    assert w["start"][ka][2] == LAN2 and w["states"][jr][ka][2] == LAN == w["out"][jr + 1]
    # KEEP lives on replies alone for 3 E; IDLE, opened with it, is gone
    kk, ki = F.lan_key(F.KEEP), F.lan_key(F.IDLE)
    t0 = c.batches[2].now[0]
    for bi in range(3, 9):
        bb = c.batches[bi]
        assert all(d == WAN for d in bb.dv) and bb.now[0] - c.batches[bi - 1].now[-1] < e
    end = walk[-1]["states"][len(c.batches[-1].now) - 1]
    assert c.batches[-1].now[0] - t0 == 3 * e and kk in end and ki not in end
    assert end[kk][1] == c.t_keep and end[kk][2] == LAN2
    assert ki in walk[3]["states"][0] and ki not in walk[5]["states"][0]


def test_free_order_trace():
    c = F.free_order_case()
    walk = F.oracle_walk(c)
    check_literals(c, walk)
    b, w = c.batches[1], walk[1]
    assert len(set(b.now)) == 1 and all(d == WAN for d in b.dv)
    last = {}
    for j in range(len(b.now)):
        last[key_of(b, j)] = j
    order = sorted(last, key=lambda k: last[k])  # oldest stamp first
    assert len(order) == F.N_FREE
    idx = [w["start"][k][0] for k in order]
    assert idx != sorted(idx) and idx != sorted(idx, reverse=True)
    old = w["states"][len(b.now) - 1]
    assert {v[1] for v in old.values()} == {b.now[0]}  # (all stamps tie)
    b2, w2 = c.batches[2], walk[2]
    assert not w2["states"][0]  # all expire at the one packet, a reply to none
    new = w2["states"][len(b2.now) - 1]
    assert len(new) == F.N_FREE
    # freed oldest stamp first, each freed index the next to be handed out
    # last: new flow j takes the index of the j-th youngest stamp
    for j in range(F.N_FREE):
        assert new[key_of(b2, 1 + j)][0] == old[order[F.N_FREE - 1 - j]][0], j
