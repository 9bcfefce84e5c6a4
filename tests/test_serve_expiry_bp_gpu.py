"""Expiry inside vigbridge's and vigpol's resident kernels (the touch journal,
DESIGN.md 5.3), as test_serve_expiry_gpu.py has it for vignat and vigfw: once
a context has met a due expiry on the served path its kernel expires the
entries itself, in the reference's LRU order, and stays.

Every test compares out ports and the full dump (alloc, ts, keys, the bridge's
learned ports, vigpol's bucket_size / bucket_time) with the CPU oracle and
reads vp_serve_expiry_stats_get / vp_serve_stats_get to see which path ran.
Every trace and its precondition come from a builder that uses the oracle
alone; test_trace_preconditions runs them all without a GPU.

Reference behaviour: bridge_main.c:311-329 (the expiry before the learn; only
the learn stamps), policer_main.c:111-145 and 21-103 (the expiry behind the
IPv4 parse, for packets of any device; only a policed hit or an allocation
stamps). Every vigbridge packet learns its src, so there is no packet that
runs the expiry and touches nothing: the primer leaves two entries behind,
which the oracle's counts include.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import test_bridge_serve_gpu as B
import test_pol_serve_gpu as P
from tracegen import mixed_bridge_trace, mixed_pol_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 1_000_000_000
FLOOD = 0xFFFF
KINDS = ["bridge", "pol"]
ROUTE = {"bridge": 384, "pol": 512}  # kBridgeBurstRoute, kPolBurstRoute
POL_BURST = 1500


class Kit:
    """One NF's helpers under one set of names. A context is configured by its
    lifetime E in ns: vigbridge's expiration_time is E / 1000 us (or a value
    whose product with 1000 wraps to E in 32 bits), vigpol's is burst 1500 and
    the rate for which burst * 1e9 / rate is E exactly."""

    def __init__(self, kind):
        self.kind = kind
        self.m = B if kind == "bridge" else P
        self.slot = self.m.SLOT

    def cfg(self, e_ns, wrap=False):
        if self.kind == "bridge":
            e_us = e_ns // 1000 if not wrap else ((1 << 32) + e_ns) // 1000
            assert (e_us * 1000) & 0xFFFFFFFF == e_ns, (e_us, e_ns)
            return (e_us,)
        rate = POL_BURST * NS // e_ns
        assert POL_BURST * NS // rate == e_ns, (rate, e_ns)
        return (rate, POL_BURST)

    def pair(self, cap, e_ns, wrap=False):
        return self.m.make_pair(cap, *self.cfg(e_ns, wrap))

    def oracle(self, cap, e_ns, wrap=False):
        return self.m.make_oracle(cap, *self.cfg(e_ns, wrap))

    def touch(self, k, ln=None, dev=None, dst=1):
        """A packet that touches entry k, allocating it when new: a frame from
        station k (to station dst), or a WAN packet to policed address k."""
        if self.kind == "bridge":
            return B.fr(k, dst, k % B.N_DEV if dev is None else dev, 60 if ln is None else ln)
        return P.fr(k, 100 if ln is None else ln, P.WAN if dev is None else dev)[:3]

    def dump(self, o, cap):
        return o.bridge_dump(cap) if self.kind == "bridge" else o.pol_dump(cap)

    def key(self, row):
        """The dump's key of the entry the packet touches."""
        return bytes(row[6:12]) if self.kind == "bridge" else P.key_of(row)

    def live(self, o, cap):
        """{key: index} of the oracle's live entries."""
        d = self.dump(o, cap)
        return {(d[2][i].tobytes() if self.kind == "bridge" else int(d[2][i])): i
                for i in range(cap) if d[0][i]}

    def runs_expiry(self, row, ln):
        """bridge_main.c:311-315: every packet. policer_main.c:113-123: behind
        nf_then_get_rte_ipv4_header (nf-util.h:122-151)."""
        if self.kind == "bridge":
            return True
        unread = (int(ln) - 14) & 0xFFFF
        tl = (int(row[16]) << 8) | int(row[17])
        return bool(row[12] == 0x08 and row[13] == 0x00 and unread >= 20 and
                    (row[14] & 0x0F) >= 5 and unread >= tl)

    def orun(self, o, F, ln, dv, now, a, b):
        exp = F[a:b].reshape(-1).copy()
        out = o.run(exp, ln[a:b], dv[a:b], now[a:b], F.shape[1])
        assert (exp == F[a:b].reshape(-1)).all()  # (neither NF rewrites a frame)
        return out

    def check_state(self, nf, o, cap):
        self.m.check_state(nf, o, cap)

    def burst(self, nf, o, F, ln, dv, now, a, b):
        """Packets [a, b) as one call against the oracle's run of them in
        order. Returns the out ports."""
        eo = self.orun(o, F, ln, dv, now, a, b)
        self.m.send_burst(nf, F, ln, dv, now, a, b, eo)
        return eo

    def one(self, nf, o, F, ln, dv, now, i):
        eo = self.orun(o, F, ln, dv, now, i, i + 1)
        buf = bytearray(F[i, :ln[i]].tobytes())
        assert nf.process(int(dv[i]), buf, int(now[i])) == eo[0], i
        assert bytes(buf) == F[i, :ln[i]].tobytes(), i
        return int(eo[0])

    def mixed(self, seed, n):
        """The NF's mixed trace, as its own served-path tests build it."""
        rng = np.random.default_rng(seed)
        if self.kind == "bridge":
            fr, ln, dv, now = mixed_bridge_trace(rng, n, 50)
            F = fr.reshape(n, B.SLOT)
            B.static_dsts(rng, F)
            return B.rows_of(F, ln), ln, dv, now
        fr, ln, dv, now = mixed_pol_trace(rng, n, 40, gap_ns=2000, big=2000)
        return P.rows_of(fr, ln), ln, dv, now


def pack(kit, pk, now):
    """A list of (frame, len, dev) and their times as trace arrays."""
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    for i in range(F.shape[0]):
        F[i, ln[i]:] = 0
    now = np.asarray(now, np.int64)
    assert F.shape[1] == kit.slot and (np.diff(now) >= 0).all()
    return F, ln, dv, now


def oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now):
    """Entries the reference expires at each packet, from the oracle's dump
    before the packet: the allocated indices stamped below now - E, at a
    packet that runs the expiry; checked against the dump after it (such an
    index is free, or was handed out again and stamped at this packet; a
    packet that does not run the expiry changes nothing). Consumes o."""
    n = F.shape[0]
    cnt = np.zeros(n, np.int64)
    for i in range(n):
        a0, ts0 = kit.dump(o, cap)[:2]
        kit.orun(o, F, ln, dv, now, i, i + 1)
        a1, ts1 = kit.dump(o, cap)[:2]
        if not kit.runs_expiry(F[i], ln[i]):
            assert (a0 == a1).all() and (ts0 == ts1).all(), i
            continue
        gone = (a0 == 1) & (ts0 < int(now[i]) - e_ns)
        assert ((a1[gone] == 0) | (ts1[gone] == now[i])).all(), i
        cnt[i] = int(gone.sum())
    return cnt


def first_due(per):
    nz = np.nonzero(per)[0]
    return int(nz[0]) if nz.size else None


# ------------------------------------------------------------ the primer --
def primer(kit, t0, e_ns):
    """Three packets that turn the journal on: entry 900, entry 901 past 900's
    expiry (the first bounce: the pipeline's), and entry 902, whose launch
    seeds the journal. 901 and 902 stay behind."""
    return pack(kit, [kit.touch(900), kit.touch(901), kit.touch(902)],
                [t0, t0 + e_ns + 1, t0 + e_ns + 2])


def prime(kit, nf, o, t0, e_ns):
    """The primer on the GPU and the oracle. Returns the last packet's time."""
    F, ln, dv, now = primer(kit, t0, e_ns)
    x0 = nf.serve_expiry_stats()
    for i in range(3):
        kit.one(nf, o, F, ln, dv, now, i)
    x = nf.serve_expiry_stats()
    assert x["handed"] == x0["handed"] + 1 and x["seeds"] == x0["seeds"] + 1, (x0, x)
    assert x["expired"] == x0["expired"], (x0, x)
    return int(now[-1])


def primed_oracle(kit, cap, e_ns, t0=T.NOW0, wrap=False):
    """An oracle that has seen the primer, and the primer's last time."""
    o = kit.oracle(cap, e_ns, wrap)
    F, ln, dv, now = primer(kit, t0, e_ns)
    kit.orun(o, F, ln, dv, now, 0, 3)
    return o, int(now[-1])


def churn(kit, k0, n, t0, step):
    """n never-seen entries k0 .. k0 + n - 1, `step` ns apart."""
    return pack(kit, [kit.touch(k0 + i) for i in range(n)],
                t0 + step * np.arange(n, dtype=np.int64))


# =============================================================== builders ==
# Each returns the trace and what the oracle alone says about it; the asserts
# inside are the trace's preconditions.

# vigbridge: 1 us entries and gaps of up to 2 ns stretched by 20 (mean 20 ns:
# an entry lives about 50 packets, 50 stations). vigpol: 1 ms entries (rate
# 1.5e6, burst 1500) and gaps of up to 2 us stretched by 40 (mean 40 us: an
# entry lives about 25 packets, 40 addresses).
CHURN = {"bridge": (1_000, 20), "pol": (1_000_000, 40)}


def build_churn(kind, cap, n=400, seed=11):
    kit = Kit(kind)
    e_ns, stretch = CHURN[kind]
    F, ln, dv, now = kit.mixed(seed, n)
    now = T.NOW0 + (now - T.NOW0) * stretch
    per = oracle_expiries(kit, kit.oracle(cap, e_ns), cap, e_ns, F, ln, dv, now)
    h = first_due(per)
    assert h is not None and h < n // 2, h
    assert int(per[h + 1:].sum()) >= 20, per[h + 1:].sum()
    return dict(kit=kit, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per, handed_at=h)


def build_order(kind):
    """Entry 900, then 16 entries in one burst at one time in a scrambled
    order (their sequence numbers decide the LRU order), 900 again past its
    own expiry (the bounce) and once more (the seed), then 24 new entries
    whose first packet expires all 16: they take the freed indices youngest
    first, then the never-used ones."""
    kit = Kit(kind)
    cap, e_ns = 64, 5000
    t0 = T.NOW0
    perm = [int(k) for k in np.random.default_rng(2).permutation(16)]
    pk = [kit.touch(900)] + [kit.touch(k) for k in perm] + [kit.touch(900), kit.touch(900)]
    now = [t0] + [t0 + 4000] * 16 + [t0 + e_ns + 1, t0 + e_ns + 2]
    pk += [kit.touch(100 + k) for k in range(24)]
    t1 = t0 + 4000 + e_ns + 1
    now += [t1 + k for k in range(24)]
    F, ln, dv, now = pack(kit, pk, now)
    o = kit.oracle(cap, e_ns)
    per = oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now)
    assert per[17] == 1 and per[19] == 16 and per.sum() == 17, per
    # 900 holds index 0 (freed and taken again), the 16 hold 1..16 in the
    # order they came: the youngest is 16, and the first new entry takes it
    lv = kit.live(o, cap)
    got = [lv[kit.key(F[19 + k])] for k in range(24)]
    assert got == list(range(16, 0, -1)) + list(range(17, 25)), got
    assert lv[kit.key(F[0])] == 0
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now)


def build_inside(kind):
    """Behind the primer: ten entries, then 64 new ones 1 us apart in one call
    (5 us expiry). Entries fall due at lanes in its middle."""
    kit = Kit(kind)
    cap, e_ns = 16, 5000
    o, tp = primed_oracle(kit, cap, e_ns)
    t = tp + 10
    F, ln, dv, _ = churn(kit, 0, 74, 0, 0)
    now = np.concatenate([t + np.arange(10), t + 2000 + 1000 * np.arange(64)]).astype(np.int64)
    per = oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now)
    assert per[:10].sum() == 0 and per[10] == 0, per
    mid = np.nonzero(per[10:])[0]
    assert mid.size >= 10 and per[10:].sum() >= 20 and mid[0] > 0, per
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per)


def build_sizes(kind):
    """The mixed trace under churn, long enough for one call at the routing
    limit and a rest; it starts behind the primer."""
    kit = Kit(kind)
    cap = 16
    e_ns, stretch = CHURN[kind]
    n = ROUTE[kind] + 90
    F, ln, dv, now = kit.mixed(5, n)
    o, tp = primed_oracle(kit, cap, e_ns, T.NOW0 - 10 * e_ns - 10)
    now = T.NOW0 + (now - T.NOW0) * stretch
    assert tp < now[0]
    per = oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now)
    assert per.sum() >= 20 and (per[64:] > 0).sum() >= 5, per
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per)


# vigbridge: 5 us, and 4294968 us whose product with 1000 wraps to 704 ns.
# vigpol: 5 s (rate 300, burst 1500), above 2^32 ns, from a start at which the
# request times' low words have bit 31 set.
BOUNDARY = [("bridge", 5000, False), ("bridge", 704, True), ("pol", 5 * NS, False)]


def build_boundary(kind, e_ns, wrap):
    kit = Kit(kind)
    cap = 16
    o, tp = primed_oracle(kit, cap, e_ns, T.NOW0, wrap)
    t = tp + e_ns + 10  # (the primer's two entries expire at the first packet)
    pk = [kit.touch(1), kit.touch(2), kit.touch(3), kit.touch(1)]
    now = [t, t + e_ns, t + e_ns + 1, t + e_ns + 1]
    F, ln, dv, now = pack(kit, pk, now)
    if kind == "pol":
        assert e_ns > 1 << 32 and all((int(x) >> 31) & 1 for x in now), now
    elif wrap:
        assert kit.cfg(e_ns, wrap)[0] * 1000 >= 1 << 32
    per = oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now)
    # entry 1's stamp equals packet 1's cutoff and survives; packet 2's cutoff
    # is one above it
    assert list(per) == [2, 0, 1, 0], per
    return dict(kit=kit, cap=cap, F=F, ln=ln, dv=dv, now=now, per=per, wrap=wrap)


def build_rejuvenation(kind):
    """Entries 1 and 2, then entry 1 touched twelve times 1 us apart (5 us
    expiry): 2 goes along the way, 1 stays until one lifetime past its last
    touch."""
    kit = Kit(kind)
    cap, e_ns = 16, 5000
    o, tp = primed_oracle(kit, cap, e_ns)
    t = tp + 10
    pk, now = [kit.touch(1), kit.touch(2)], [t, t + 1]
    for r in range(12):
        pk.append(kit.touch(1))
        now.append(t + 1000 * (r + 1))
    last = now[-1]
    pk += [kit.touch(3), kit.touch(4)]
    now += [last + e_ns, last + e_ns + 1]
    F, ln, dv, now = pack(kit, pk, now)
    k1, k2 = kit.key(F[0]), kit.key(F[1])
    per = np.zeros(len(pk), np.int64)
    for i in range(len(pk)):
        per[i] = oracle_expiries(kit, o, cap, e_ns, F[i:i + 1], ln[i:i + 1], dv[i:i + 1],
                                 now[i:i + 1])[0]
        lv = kit.live(o, cap)
        if i == 13:
            assert k1 in lv and k2 not in lv  # (the untouched neighbour is gone)
        if i == 14:
            assert k1 in lv and per[i] == 0   # (stamp == cutoff)
        if i == 15:
            assert k1 not in lv and per[i] == 1
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per)


def build_ring(kind, path):
    """16 indices and a ring of 32 records (VIGPATH_SERVE_JOURNAL=2): entry 1
    stays idle while entries 2..11 are touched over and over, so the ring
    fills and is seeded again from the table; then entry 1's expiry."""
    kit = Kit(kind)
    cap, e_ns = 16, 60_000
    o, tp = primed_oracle(kit, cap, e_ns)
    t = tp + 10
    m = 150 if path == "one" else 480
    pk, now = [kit.touch(1)], [t]
    for r in range(m):
        pk.append(kit.touch(2 + r % 10))
        now.append(t + 1 + r)
    pk += [kit.touch(12), kit.touch(1)]
    now += [t + e_ns + 1, t + e_ns + 2]
    F, ln, dv, now = pack(kit, pk, now)
    per = oracle_expiries(kit, o, cap, e_ns, F, ln, dv, now)
    assert per[:1 + m].sum() == 0 and per[1 + m] == 3 and per.sum() == 3, per
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per, m=m)


def build_bridge_cases():
    """11 (a): a frame to a MAC that expires at that very packet floods. (b):
    a MAC that expired is learnt again from another port, and later frames to
    it go there."""
    kit = Kit("bridge")
    cap, e_ns = 16, 5000
    o, tp = primed_oracle(kit, cap, e_ns)
    t = tp + 10
    pk = [B.fr(20, 1, 0), B.fr(21, 20, 1),               # 20 on port 0; to it: port 0
          B.fr(22, 20, 1),                               # (a) 20 expires here: flooded
          B.fr(20, 1, 2), B.fr(23, 20, 1),               # (b) learnt again on port 2
          B.fr(30, 1, 0), B.fr(31, 30, 1),               # the same inside one burst:
          B.fr(30, 1, 2), B.fr(32, 30, 1)]               # relearn and lookup together
    now = [t, t + 1, t + e_ns + 1, t + e_ns + 2, t + e_ns + 3,
           t + 2 * e_ns, t + 2 * e_ns + 1, t + 3 * e_ns + 1, t + 3 * e_ns + 2]
    F, ln, dv, now = pack(kit, pk, now)
    out = [int(kit.orun(o, F, ln, dv, now, i, i + 1)[0]) for i in range(len(pk))]
    assert out[1] == 0 and out[2] == FLOOD and out[4] == 2, out
    assert out[6] == 0 and out[8] == 2, out
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, out=out)


def pol_fr(k, ln=100, dev=P.WAN, **kw):
    return P.fr(k, ln, dev, **kw)[:3]


V6 = dict(eth=(0x86, 0xDD))


def build_pol_cases():
    """12 (a)-(f), one context, 5 us entries (rate 3e8: 0.3 bytes a ns)."""
    kit = Kit("pol")
    cap, e_ns = 16, 5000
    o, tp = primed_oracle(kit, cap, e_ns)
    t = tp + 10
    seg, pk, now = {}, [], []

    def add(name, packets, times):
        seg[name] = (len(pk), len(pk) + len(packets))
        pk.extend(packets)
        now.extend(times)

    # (a) three entries, a frame that does not parse far past every lifetime,
    # then an IPv4 LAN packet
    add("a0", [pol_fr(1), pol_fr(2), pol_fr(3)], [t, t + 1, t + 2])
    add("a1", [pol_fr(1, **V6)], [t + 10 * e_ns])
    add("a2", [pol_fr(1, dev=P.LAN)], [t + 10 * e_ns + 1])
    t += 11 * e_ns
    # (b) two entries; a burst whose lanes 0-1 do not parse, past the lifetime
    add("b0", [pol_fr(4), pol_fr(5)], [t, t + 1])
    add("b1", [pol_fr(4, **V6), pol_fr(4, ln=20), pol_fr(4), pol_fr(6)],
        [t + e_ns + 2, t + e_ns + 3, t + e_ns + 4, t + e_ns + 5])
    t += 3 * e_ns
    # (c) entry 7 falls due at a lane that does not parse: the split is at the
    # next parsing lane
    add("c0", [pol_fr(7)], [t])
    add("c1", [pol_fr(8), pol_fr(9), pol_fr(7, **V6), pol_fr(7, ln=20), pol_fr(10), pol_fr(11)],
        [t + e_ns - 2, t + e_ns - 1, t + e_ns + 1, t + e_ns + 2, t + e_ns + 3, t + e_ns + 4])
    t += 3 * e_ns
    # (d) address 12 policed on both sides of a split (entry 13 falls due at
    # lane 3): 1500 - 700 at first, 300 tokens per 1000 ns
    add("d0", [pol_fr(13)], [t])
    t1 = t + e_ns - 2000
    add("d1", [pol_fr(12, 700), pol_fr(12, 600), pol_fr(12, 700), pol_fr(12, 700), pol_fr(12, 200),
               pol_fr(12, 700)],
        [t1, t1 + 1000, t1 + 2000, t1 + 2001, t1 + 2500, t1 + 3000])
    t += 4 * e_ns
    # (e) address 14, bucket emptied, policed again by the very packet at which
    # it expires, with a packet of exactly `burst` bytes: afresh it is forwarded
    # (bucket 0); the old entry refilled to `burst` would have dropped it
    # (size > len is the test). (f) address 15 the same with burst + 100 bytes:
    # dropped, nothing allocated. Inside one burst, behind a parsing lane 0.
    add("e0", [pol_fr(14, 1400), pol_fr(15)], [t, t])
    add("e1", [pol_fr(16), pol_fr(14, POL_BURST), pol_fr(15, POL_BURST + 100)],
        [t + e_ns, t + e_ns + 1, t + e_ns + 1])
    F, ln, dv, now = pack(kit, pk, now)
    per, lives = [], []  # per packet: entries expired, the state behind it
    for i in range(len(pk)):
        per.append(int(oracle_expiries(kit, o, cap, e_ns, F[i:i + 1], ln[i:i + 1], dv[i:i + 1],
                                       now[i:i + 1])[0]))
        lives.append(P.live_state(kit.dump(o, cap)))
    o2, _ = primed_oracle(kit, cap, e_ns)
    out = [int(kit.orun(o2, F, ln, dv, now, i, i + 1)[0]) for i in range(len(pk))]
    key = lambda i: P.key_of(F[i])  # noqa: E731
    s = seg
    # (a)
    a1, a2 = s["a1"][0], s["a2"][0]
    assert per[a1] == 0 and {key(a1 - 3), key(a1 - 2), key(a1 - 1)} <= set(lives[a1])
    assert lives[a1] == lives[a1 - 1] and now[a1] - e_ns > max(v[1] for v in lives[a1].values())
    # (LAN -> WAN, everything gone -- the primer's two entries as well --, nothing touched)
    assert per[a2] == len(lives[a1]) == 5 and not lives[a2] and out[a2] == P.WAN
    # (b) nothing at lanes 0-1, both entries at lane 2, whose address is
    # allocated afresh at lane 2's time
    b1 = s["b1"][0]
    assert per[b1:b1 + 4] == [0, 0, 2, 0], per[b1:b1 + 4]
    assert lives[b1 + 2][key(b1 + 2)][1] == now[b1 + 2] and out[b1 + 2] == P.LAN
    # (c) entry 7 is due from lane 2 on and goes at lane 4
    c1 = s["c1"][0]
    assert per[c1:c1 + 6] == [0, 0, 0, 0, 1, 0], per[c1:c1 + 6]
    assert now[c1 + 2] - e_ns > now[s["c0"][0]]
    # (d) entry 13 goes at lane 3; the recurrence on 12 across it
    d1 = s["d1"][0]
    assert per[d1:d1 + 6] == [0, 0, 0, 1, 0, 0], per[d1:d1 + 6]
    sizes = [lives[d1 + i][key(d1)][2] for i in range(6)]
    want, size = [], POL_BURST - 700
    for i in range(1, 6):  # (policer_main.c:39-72 from the bucket the packet before left)
        fwd, size = P.bucket_step(size, int(now[d1 + i - 1]), int(ln[d1 + i]), int(now[d1 + i]),
                                  3 * 10 ** 8, POL_BURST)
        want.append((P.LAN if fwd else P.WAN, size))
    assert [(out[d1 + i], sizes[i]) for i in range(1, 6)] == want, (sizes, want)
    assert sizes == [800, 500, 100, 100, 49, 199], sizes
    assert [out[d1 + i] for i in range(6)] == [P.LAN, P.LAN, P.LAN, P.WAN, P.LAN, P.WAN]
    # (e), (f)
    e1 = s["e1"][0]
    assert per[e1:e1 + 3] == [0, 2, 0], per[e1:e1 + 3]
    assert lives[e1][key(e1 + 1)][2] == POL_BURST - 1400
    assert out[e1 + 1] == P.LAN and lives[e1 + 1][key(e1 + 1)][2] == 0
    assert not P.bucket_step(100, 0, POL_BURST, e_ns + 1, 3 * 10 ** 8, POL_BURST)[0]
    assert out[e1 + 2] == P.WAN and key(e1 + 2) not in lives[e1 + 2]
    return dict(kit=kit, cap=cap, e_ns=e_ns, F=F, ln=ln, dv=dv, now=now, per=per, seg=seg)


def test_trace_preconditions():
    """Every builder's asserts, from the oracle alone (no GPU)."""
    for kind in KINDS:
        build_churn(kind, 64)
        build_churn(kind, 16)
        build_order(kind)
        build_inside(kind)
        build_sizes(kind)
        build_rejuvenation(kind)
        build_ring(kind, "one")
        build_ring(kind, "burst")
    for kind, e_ns, wrap in BOUNDARY:
        build_boundary(kind, e_ns, wrap)
    build_bridge_cases()
    build_pol_cases()


# ---------------------------------------------------- 1. per-packet churn --
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap,idle", [(64, True), (16, False)])
def test_per_packet_churn(kind, cap, idle):
    """The mixed traces with time stretched so that entries expire along the
    way: one packet is handed to the pipeline, every later expiry is the
    kernel's, and an idle exit in the middle seeds nothing again."""
    r = build_churn(kind, cap)
    kit, F, ln, dv, now, per = r["kit"], r["F"], r["ln"], r["dv"], r["now"], r["per"]
    n = F.shape[0]
    nf, o = kit.pair(cap, r["e_ns"])
    handed_at, mid = None, None
    for i in range(n):
        if i == n // 2:
            mid = nf.serve_expiry_stats()
            if idle:
                time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
        kit.one(nf, o, F, ln, dv, now, i)
        if handed_at is None and nf.serve_expiry_stats()["handed"]:
            handed_at = i
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    kit.check_state(nf, o, cap)
    print(kind, cap, "handed at", handed_at, x, s)
    assert handed_at is not None and handed_at <= r["handed_at"], (handed_at, r["handed_at"])
    want = int(per[handed_at + 1:].sum())
    assert want >= 20, want
    assert x["handed"] == 1, x
    assert s["packets_one"] >= n - 1, s
    assert x["expired"] == want, (x, want)
    assert x["walks"] == int((per[handed_at + 1:] > 0).sum()), x
    assert x["seeds"] == mid["seeds"] and x["seeds"] >= 1, (mid, x)
    if idle:
        assert s["launches"] >= 3, s  # (first, after the bounce, after the idle exit)


# ----------------------------------------------------- 2. order and reuse --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_order_and_reuse(kind):
    """Sixteen entries fall due at one packet of a served burst: the oldest
    stamp frees first and the youngest freed index is taken first (the
    builder reads the indices off the oracle; the dump shows the GPU's)."""
    r = build_order(kind)
    kit, cap, F, ln, dv, now = r["kit"], r["cap"], r["F"], r["ln"], r["dv"], r["now"]
    nf, o = kit.pair(cap, r["e_ns"])
    kit.burst(nf, o, F, ln, dv, now, 0, 1)
    kit.burst(nf, o, F, ln, dv, now, 1, 17)
    kit.burst(nf, o, F, ln, dv, now, 17, 18)  # entry 900 expires: the pipeline's
    x0 = nf.serve_expiry_stats()
    assert x0["handed"] == 1 and x0["expired"] == 0, x0
    kit.burst(nf, o, F, ln, dv, now, 18, 19)  # (launched again: the journal is seeded)
    s0 = nf.serve_stats()
    kit.burst(nf, o, F, ln, dv, now, 19, 43)
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    kit.check_state(nf, o, cap)
    assert x["seeds"] == 1 and x["handed"] == 1 and x["expired"] == 16 and x["walks"] == 1, x
    assert s["burst_packets"] == s0["burst_packets"] + 24 and s["declined"] == 0, (s0, s)


# ------------------------------------------------ 3. expiry inside a burst --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_expiry_inside_a_burst(kind):
    """A call of 64 with entries falling due at lanes in its middle is served
    in parts, each up to the packet at which the next entry falls due; the
    results are those of the packets processed one after another."""
    r = build_inside(kind)
    kit, cap, F, ln, dv, now, per = (r[k] for k in ("kit", "cap", "F", "ln", "dv", "now", "per"))
    nf, o = kit.pair(cap, r["e_ns"])
    prime(kit, nf, o, T.NOW0, r["e_ns"])
    kit.burst(nf, o, F, ln, dv, now, 0, 10)
    s0, x0 = nf.serve_stats(), nf.serve_expiry_stats()
    kit.burst(nf, o, F, ln, dv, now, 10, 74)
    s1, x1 = nf.serve_stats(), nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    print(kind, s0, s1, x0, x1)
    assert x1["splits"] >= x0["splits"] + 1, (x0, x1)
    assert s1["burst_packets"] == s0["burst_packets"] + 64 and s1["declined"] == 0, (s0, s1)
    assert x1["handed"] == x0["handed"] and x1["seeds"] == x0["seeds"], (x0, x1)
    assert x1["expired"] == x0["expired"] + int(per[10:].sum()), (x0, x1, per)


# ---------------------------------------------- 4. call sizes across churn --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_call_sizes_across_churn(kind):
    """One churn trace in calls of 1, 7, 32, 64 and the routing limit, a fresh
    context each: the same ports and the same state (each also checked
    against the oracle), nothing handed over, the same entries expired."""
    r = build_sizes(kind)
    kit, cap, F, ln, dv, now, per = (r[k] for k in ("kit", "cap", "F", "ln", "dv", "now", "per"))
    n = F.shape[0]
    ref = None
    for size in [1, 7, 32, 64, ROUTE[kind]]:
        nf, o = kit.pair(cap, r["e_ns"])
        prime(kit, nf, o, T.NOW0 - 10 * r["e_ns"] - 10, r["e_ns"])
        x0, s0 = nf.serve_expiry_stats(), nf.serve_stats()
        outs = [kit.burst(nf, o, F, ln, dv, now, a, min(a + size, n)) for a in range(0, n, size)]
        x, s = nf.serve_expiry_stats(), nf.serve_stats()
        kit.check_state(nf, o, cap)
        got = (np.concatenate(outs), nf.dump())
        print(kind, size, x, s)
        assert x["handed"] == x0["handed"] and x["seeds"] == x0["seeds"], (size, x0, x)
        assert s["burst_packets"] == s0["burst_packets"] + n and s["declined"] == 0, (size, s0, s)
        assert x["expired"] == x0["expired"] + int(per.sum()), (size, x0, x)
        if size >= 64:
            assert x["splits"] >= 1, (size, x)
        if ref is None:
            ref = got
        live = ref[1][0] == 1
        assert (got[0] == ref[0]).all() and (got[1][0] == ref[1][0]).all(), size
        for ga, ra in zip(got[1][1:], ref[1][1:]):
            assert (ga[live] == ra[live]).all(), size


# ----------------------------------------------------------- 5. boundary --
@gpu
@pytest.mark.parametrize("kind,e_ns,wrap", BOUNDARY)
def test_boundary(kind, e_ns, wrap):
    """A stamp equal to the cutoff survives (ts < cutoff is the test); one
    nanosecond later the kernel expires it, not the pipeline."""
    r = build_boundary(kind, e_ns, wrap)
    kit, cap, F, ln, dv, now = r["kit"], r["cap"], r["F"], r["ln"], r["dv"], r["now"]
    nf, o = kit.pair(cap, e_ns, wrap)
    prime(kit, nf, o, T.NOW0, e_ns)
    kit.one(nf, o, F, ln, dv, now, 0)
    x0 = nf.serve_expiry_stats()
    kit.one(nf, o, F, ln, dv, now, 1)
    x1 = nf.serve_expiry_stats()
    assert x1["expired"] == x0["expired"], (x0, x1)  # entry 1 is still there
    kit.one(nf, o, F, ln, dv, now, 2)
    kit.one(nf, o, F, ln, dv, now, 3)
    x2 = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert x2["expired"] == x1["expired"] + 1 and x2["handed"] == 1, (x1, x2)
    assert nf.serve_stats()["packets_one"] == 3 + 4 - 1


# -------------------------------------------------------- 6. rejuvenation --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rejuvenation(kind):
    """An entry touched many times survives when its stale records reach the
    journal's tail; its neighbour, never touched again, goes."""
    r = build_rejuvenation(kind)
    kit, cap, F, ln, dv, now, per = (r[k] for k in ("kit", "cap", "F", "ln", "dv", "now", "per"))
    nf, o = kit.pair(cap, r["e_ns"])
    prime(kit, nf, o, T.NOW0, r["e_ns"])
    x0 = nf.serve_expiry_stats()
    for i in range(F.shape[0]):
        kit.one(nf, o, F, ln, dv, now, i)
    x = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert x["expired"] == x0["expired"] + int(per.sum()), (x0, x, per)
    assert x["handed"] == x0["handed"] and x["seeds"] == x0["seeds"], (x0, x)


# ------------------------------------------------------ children (7, 10) --
def body_ring(kind, path):
    r = build_ring(kind, path)
    kit, cap, F, ln, dv, now, m = (r[k] for k in ("kit", "cap", "F", "ln", "dv", "now", "m"))
    nf, o = kit.pair(cap, r["e_ns"])
    prime(kit, nf, o, T.NOW0, r["e_ns"])
    n = F.shape[0]
    if path == "one":
        for i in range(n):
            kit.one(nf, o, F, ln, dv, now, i)
    else:
        kit.burst(nf, o, F, ln, dv, now, 0, 1)
        for a in range(1, 1 + m, 60):
            kit.burst(nf, o, F, ln, dv, now, a, min(a + 60, 1 + m))
        kit.burst(nf, o, F, ln, dv, now, 1 + m, n)
    kit.check_state(nf, o, cap)
    return dict(nf.serve_expiry_stats(), **nf.serve_stats())


def body_off(kind, _):
    kit = Kit(kind)
    nf, o = kit.pair(16, 5000)
    F, ln, dv, now = churn(kit, 0, 120, T.NOW0, 700)
    for i in range(40):
        kit.one(nf, o, F, ln, dv, now, i)
    kit.burst(nf, o, F, ln, dv, now, 40, 80)
    kit.burst(nf, o, F, ln, dv, now, 80, 120)
    kit.check_state(nf, o, 16)
    return dict(nf.serve_expiry_stats(), **nf.serve_stats())


CHILD = r"""
import json, sys
import test_serve_expiry_bp_gpu as X
print("STATS " + json.dumps(getattr(X, "body_" + sys.argv[1])(sys.argv[2], sys.argv[3])))
"""


def run_child(body, kind, arg, **env_add):
    """A body in a fresh process (the switches are read once per process)."""
    env = dict(os.environ, **env_add)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", CHILD, body, kind, arg], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("STATS ")][-1][6:])


# ----------------------------------------------------------- 7. ring full --
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["one", "burst"])
def test_ring_full(kind, path):
    """VIGPATH_SERVE_JOURNAL=2: the ring fills, nothing of the refused request
    is done, the journal is seeded again and the same request served; then the
    idle entry's expiry, still the kernel's. The child checks every port and
    the state."""
    st = run_child("ring", kind, path, VIGPATH_SERVE_JOURNAL="2")
    print(kind, path, st)
    assert st["seeds"] >= 3 and st["handed"] == 1 and st["expired"] == 3, st
    assert st["declined"] == 0, st


# ---------------------------------------------------------- 8. tombstones --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tombstones_purged_while_served(kind):
    """64 indices under churn until erased and live entries pass the purge
    bound: the kernel reports it, the host rebuilds (vp_table_stats_get) and
    launches it again; the journal survives and nothing takes the pipeline.
    vigpol's buckets are indexed by flow index, which a rebuild does not move:
    the state behind it equals the oracle's.

    The bound is 85 % of 64 buckets of 3 entries, 163. An insert takes a
    tombstone of its home bucket when there is one, so under steady churn the
    tombstones level off at about one per bucket (128 buckets): 16 indices
    stay below the bound for good (15 live + 113 erased after 3,840 entries),
    about 57 live ones (20 us entries, a new one every 350 ns) pass it."""
    kit = Kit(kind)
    cap, e_ns = 64, 20_000
    nf, o = kit.pair(cap, e_ns)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    x0, r0 = nf.serve_expiry_stats(), nf.table_stats()["rebuilds"]
    k0, rose = 1000, False
    for _ in range(60):
        F, ln, dv, now = churn(kit, k0, 64, t, 350)
        kit.burst(nf, o, F, ln, dv, now, 0, 64)
        k0, t = k0 + 64, int(now[-1]) + 350
        rose = nf.table_stats()["rebuilds"] > r0
        if rose:
            break
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    print(kind, "entries sent", k0 - 1000, x, s, nf.table_stats())
    assert rose, "the purge bound was never passed"
    # served again after the rebuild, hits on the entries it moved among them
    F, ln, dv, now = churn(kit, k0 - 8, 64, t, 350)
    kit.burst(nf, o, F, ln, dv, now, 0, 64)
    kit.check_state(nf, o, cap)
    x1, s1 = nf.serve_expiry_stats(), nf.serve_stats()
    assert x1["handed"] == x0["handed"] and x1["seeds"] == x0["seeds"], (x0, x1)
    assert x1["expired"] > x["expired"], (x, x1)
    assert s1["burst_packets"] == s["burst_packets"] + 64 and s1["declined"] == 0, (s, s1)


# --------------------------------------------------- 9. pipeline in between --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_pipeline_in_between(kind):
    """A dump keeps the journal; a batch of 1,024 through the pipeline drops
    it: the next due expiry is handed over once more and the journal seeded
    again."""
    kit = Kit(kind)
    cap, e_ns = 64, 5000
    nf, o = kit.pair(cap, e_ns)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    x0 = nf.serve_expiry_stats()

    def served_churn(k0, t):
        F, ln, dv, now = churn(kit, k0, 40, t, 500)
        kit.burst(nf, o, F, ln, dv, now, 0, 40)
        return int(now[-1]) + 500

    t = served_churn(0, t)
    x1 = nf.serve_expiry_stats()
    assert x1["expired"] > x0["expired"] and x1["handed"] == x0["handed"], (x0, x1)
    kit.check_state(nf, o, cap)  # a dump: the kernel stops, the journal stays
    t = served_churn(100, t)
    x2 = nf.serve_expiry_stats()
    assert x2["expired"] > x1["expired"], (x1, x2)
    assert x2["handed"] == x0["handed"] and x2["seeds"] == x0["seeds"], (x0, x2)
    s2 = nf.serve_stats()
    F, ln, dv, now = churn(kit, 2000, 1024, t, 500)  # above the routing limit: the pipeline's
    kit.burst(nf, o, F, ln, dv, now, 0, 1024)
    t = int(now[-1]) + 500
    s3, x3 = nf.serve_stats(), nf.serve_expiry_stats()
    assert s3["burst_packets"] == s2["burst_packets"], (s2, s3)
    assert x3["expired"] == x2["expired"] and x3["handed"] == x2["handed"], (x2, x3)
    t = served_churn(600, t)
    t = served_churn(700, t)
    x4 = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert x4["handed"] == x2["handed"] + 1 and x4["seeds"] == x2["seeds"] + 1, (x2, x4)
    assert x4["expired"] > x3["expired"], (x3, x4)


# ---------------------------------------------------------- 10. switch off --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_in_child(kind):
    """VIGPATH_SERVE_EXPIRE=0: the same ports and state (checked in the
    child), every due expiry through the pipeline."""
    st = run_child("off", kind, "-", VIGPATH_SERVE_EXPIRE="0")
    assert st["expired"] == 0 and st["seeds"] == 0 and st["walks"] == 0 and st["splits"] == 0, st
    assert st["handed"] > 1, st


# ------------------------------------------------------ 11. vigbridge only --
@gpu
@pytest.mark.parametrize("burst", [False, True])
def test_bridge_expired_dst_floods_and_src_moves(burst):
    """(a) a frame to a MAC that expires at that very packet floods; (b) a MAC
    that expired is learnt again from another port and frames to it go there
    -- packet by packet, and with the relearn and the lookup in one burst."""
    r = build_bridge_cases()
    kit, cap, F, ln, dv, now = r["kit"], r["cap"], r["F"], r["ln"], r["dv"], r["now"]
    nf, o = kit.pair(cap, r["e_ns"])
    prime(kit, nf, o, T.NOW0, r["e_ns"])
    x0 = nf.serve_expiry_stats()
    if burst:
        outs = [int(v) for a, b in [(0, 2), (2, 3), (3, 5), (5, 7), (7, 9)]
                for v in kit.burst(nf, o, F, ln, dv, now, a, b)]
    else:
        outs = [kit.one(nf, o, F, ln, dv, now, i) for i in range(F.shape[0])]
    x = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert outs == r["out"]
    assert x["handed"] == x0["handed"] and x["expired"] > x0["expired"], (x0, x)


# --------------------------------------------------------- 12. vigpol only --
@gpu
def test_pol_expiry_runs_behind_the_parse():
    """(a)-(f) of build_pol_cases, each part through the path it is about and
    against the oracle; the counters show where a walk or a split happened."""
    r = build_pol_cases()
    kit, cap, F, ln, dv, now, per, seg = (r[k] for k in
                                          ("kit", "cap", "F", "ln", "dv", "now", "per", "seg"))
    nf, o = kit.pair(cap, r["e_ns"])
    prime(kit, nf, o, T.NOW0, r["e_ns"])

    def ones(name):
        for i in range(*seg[name]):
            kit.one(nf, o, F, ln, dv, now, i)

    def call(name):
        x0, s0 = nf.serve_expiry_stats(), nf.serve_stats()
        kit.burst(nf, o, F, ln, dv, now, *seg[name])
        x1, s1 = nf.serve_expiry_stats(), nf.serve_stats()
        d = {k: x1[k] - x0[k] for k in x0}
        d["bursts"] = s1["bursts"] - s0["bursts"]
        d["packets"] = s1["burst_packets"] - s0["burst_packets"]
        assert d["handed"] == 0 and d["seeds"] == 0 and d["packets"] == seg[name][1] - seg[name][0]
        assert d["expired"] == sum(per[seg[name][0]:seg[name][1]]), (name, d)
        return d

    # (a) packet by packet
    ones("a0")
    x0 = nf.serve_expiry_stats()
    ones("a1")
    x1 = nf.serve_expiry_stats()
    assert x1 == x0, (x0, x1)  # (nothing expired, nothing handed over)
    assert int(nf.dump()[0].sum()) == 5  # (the three and the primer's two: still there)
    ones("a2")
    x2 = nf.serve_expiry_stats()
    assert x2["expired"] == x1["expired"] + 5 and x2["handed"] == x1["handed"], (x1, x2)
    assert int(nf.dump()[0].sum()) == 0
    # (b) the walk runs at the first parsing lane; no split
    ones("b0")
    d = call("b1")
    assert d["walks"] == 1 and d["splits"] == 0 and d["bursts"] == 1, d
    # (c) no split at the lanes that do not parse: one, at lane 4
    ones("c0")
    d = call("c1")
    assert d["splits"] == 1 and d["bursts"] == 2 and d["walks"] == 1, d
    # (d) one address on both sides of a split
    ones("d0")
    d = call("d1")
    assert d["splits"] == 1 and d["bursts"] == 2, d
    # (e), (f) inside one burst, behind a parsing lane
    ones("e0")
    d = call("e1")
    assert d["splits"] == 1 and d["bursts"] == 2 and d["walks"] == 1, d
    kit.check_state(nf, o, cap)
