"""Directed traces for vigbridge's batch pipeline (vp_bridge.hip), shared by
test_bridge_edges.py (CPU: each trace reaches what it names, against the
oracle alone) and test_bridge_edges_gpu.py (the pipeline against the oracle,
bit for bit).

A Case is a configuration and a sequence of batches. Every packet carries the
out port the Model below computes for it (Python integers, written from the
reference's text, not from the project's code); a packet a docstring names
also carries a tag and the out port written out by hand (`want`), which the
builder checks against the model. Untagged packets are filler.
Reference behaviour: vigbridge/bridge_main.c (bridge_expire_entries,
bridge_get_device, bridge_put_update_entry, nf_process).
"""
import os
import sys

import numpy as np

from vigor_amd import traces as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from spec_model import crc32c_u32  # noqa: E402

N_DEV = 3
FLOOD = 0xFFFF
BCAST = b"\xff" * 6
LONG_US = 300_000_000  # nothing expires in the trace


def mac(k):
    return bytes([2, 0, (k >> 24) & 255, (k >> 16) & 255, (k >> 8) & 255, k & 255])


class Model:
    """nf_process of vigbridge in Python integers: expire (u32-wrapped
    expiration_time * 1000, strictly older than now - E), learn or rejuvenate
    the src (a full table learns nothing; a known MAC keeps its port), look
    the dst up ({dst, in} static rule first, the first of a repeated key),
    resolve -1 to a flood and -2 to the in port."""

    def __init__(self, cap, expire_us, statics=()):
        self.cap = cap
        self.e = (expire_us * 1000) & 0xFFFFFFFF
        self.st = {}
        for m, frm, to in statics:
            self.st.setdefault((bytes(m), frm), to)
        self.t = {}  # mac -> [port, stamp]

    def step(self, src, dst, dev, now):
        last = now - self.e
        for m in [m for m, v in self.t.items() if v[1] < last]:
            del self.t[m]
        if src in self.t:
            self.t[src][1] = now
        elif len(self.t) < self.cap:
            self.t[src] = [dev, now]
        fwd = self.st.get((dst, dev))
        if fwd is None:
            fwd = self.t[dst][0] if dst in self.t else -1
        if fwd == -1:
            return FLOOD
        if fwd == -2:
            return dev
        return fwd & 0xFFFF

    def live(self):
        return {m: (v[0], v[1]) for m, v in self.t.items()}


RUNT_LENS = list(range(15)) + [60, 64]  # (17: every length meets every position mod 64)


class Batch:
    def __init__(self, case, note):
        self.case, self.note = case, note
        self.src, self.dst, self.dv, self.now, self.ln, self.tags, self.exp, self.want = \
            [], [], [], [], [], [], [], []
        self.tombs = None  # table_stats()["tombstones"] at least this behind the batch

    def add(self, src, dst, dev, t, ln=None, tag="", want=None):
        """want: the out port written by hand; a tagged packet must have one."""
        c = self.case
        assert not self.now or t >= self.now[-1]
        assert bool(tag) == (want is not None), (c, self.note, tag)
        out = c.model.step(src, dst, dev, t)
        assert want is None or out == want, (c, self.note, len(self.now), tag, out, want)
        if ln is None:
            ln = RUNT_LENS[len(self.now) % len(RUNT_LENS)] if c.runts else 60
        self.src.append(src)
        self.dst.append(dst)
        self.dv.append(dev)
        self.now.append(t)
        self.ln.append(ln)
        self.tags.append(tag)
        self.exp.append(out)
        self.want.append(want)
        return self

    def tagged(self, tag):
        return [j for j, t in enumerate(self.tags) if t == tag]

    def affine(self):
        """(now0, now_step) when the times are an affine function of the
        position, else None."""
        now = self.now
        step = now[1] - now[0] if len(now) > 1 else 1
        ok = all(now[i] == now[0] + i * step for i in range(len(now)))
        return (now[0], step) if ok else None

    def arrays(self):
        """Rows, lens, in ports, times. Bytes 12 on are dirty (never zero),
        whatever the frame's length."""
        n, slot = len(self.now), self.case.slot
        F = ((np.arange(slot, dtype=np.uint32)[None, :] * 7 +
              np.arange(n, dtype=np.uint32)[:, None] * 13) & 0xFF).astype(np.uint8) | 1
        F[:, 0:6] = np.frombuffer(b"".join(self.dst), np.uint8).reshape(n, 6)
        F[:, 6:12] = np.frombuffer(b"".join(self.src), np.uint8).reshape(n, 6)
        return (F, np.array(self.ln, np.uint16), np.array(self.dv, np.uint16),
                np.array(self.now, np.int64))


class Case:
    def __init__(self, name, cap=64, expire_us=LONG_US, statics=(), slot=64, runts=False,
                 env=None):
        self.name, self.cap, self.expire_us, self.slot = name, cap, expire_us, slot
        self.statics, self.runts, self.env = list(statics), runts, env or {}
        self.model = Model(cap, expire_us, statics)
        self.batches = []

    def batch(self, note=""):
        b = Batch(self, note)
        self.batches.append(b)
        return b

    def final(self):
        """{mac: (port, stamp)} behind the last batch, by the model."""
        return self.model.live()

    def all_affine(self):
        return all(b.affine() is not None for b in self.batches)

    def __repr__(self):
        return self.name


def live_state(dump):
    """{mac: (index, stamp, port)} of a dump."""
    alloc, ts, macs, port = dump
    return {bytes(macs[i]): (int(i), int(ts[i]), int(port[i]))
            for i in np.nonzero(alloc)[0]}


def make_oracle(case):
    import orc
    cfg = orc.BridgeCfg(expiration_time=case.expire_us, dyn_capacity=case.cap,
                        n_devices=N_DEV)
    return orc.Oracle("bridge", cfg, statics=case.statics)


def oracle_walk(case, every=512):
    """The case through the oracle alone, packet by packet. Per batch: the out
    ports, the state before the batch and {position: state behind that
    packet} -- every position of a batch of at most `every` packets; of a
    longer one, the tagged packets, the packets before them and the last."""
    o = make_oracle(case)
    res, st = [], {}
    for b in case.batches:
        F, ln, dv, now = b.arrays()
        n = len(ln)
        at = set(range(n)) if n <= every else \
            {n - 1} | {j for i, t in enumerate(b.tags) if t for j in (i - 1, i) if j >= 0}
        out, states = np.zeros(n, np.uint16), {}
        for j in range(n):
            fr = F[j].copy()
            out[j] = o.run(fr, ln[j:j + 1], dv[j:j + 1], now[j:j + 1], case.slot)[0]
            assert (fr == F[j]).all()  # (the bridge rewrites nothing)
            if j in at:
                states[j] = live_state(o.bridge_dump(case.cap))
        res.append(dict(out=out, start=st, states=states))
        st = states[n - 1]
    return res


# ------------------------------------------- a. order in one segment (f. slots) --
N_KNOWN = 12
KNOWN = [mac(100 + i) for i in range(N_KNOWN)]  # station i sits on port i % 3
A = [mac(1000 + i) for i in range(8)]
P = [mac(2000 + k) for k in range(64)]
Q = [mac(3000 + k) for k in range(64)]
FIRST, LAST = mac(4000), mac(4001)


def fill(b, n, t0, named):
    """n packets at t0, t0 + 1, ...: the named positions {pos: (src, dst, dev,
    tag, want)}, known stations talking to each other everywhere else."""
    for i in range(n):
        if i in named:
            src, dst, dev, tag, want = named[i]
            b.add(src, dst, dev, t0 + i, tag=tag, want=want)
        else:
            s = i % N_KNOWN
            b.add(KNOWN[s], KNOWN[(i * 5 + 1) % N_KNOWN], s % 3, t0 + i)
    return t0 + n


def order_case(slot=64, runts=False):
    """One context, every batch with affine times (step 1 ns), nothing expires.
    0  warm-up: the known stations.
    1  320 packets. own-src (10): a frame to its own new src forwards to its in
       port. before-learn (61) floods, learn (62), after-learn (63, the same
       wave) forwards; 63 also learns the MAC that 64 (the next wave) is sent
       to. first-sighting (100, port 0) and second-sighting (130, port 2) of
       one MAC: to-first-port (131) goes to port 0, before-first (99) floods.
       moved (140): a known station on a new port; to-moved (141) still goes to
       its old port. bcast-before (149) floods, bcast-src (150) learns the
       broadcast address, bcast-after (151) forwards to it. 255 and 256 (two
       blocks' waves): each is sent to the other's new src, flood-rev floods,
       fwd-next forwards.
    2  4096 packets. At every multiple of 64, packets 64k - 1 and 64k are sent
       to each other's new src (flood-rev / fwd-next); packet 0 is sent to the
       last packet's src (first-to-last: flood) and the last to packet 0's
       (last-to-first: forward).
    3  200 packets between known stations to MACs learned above (steady):
       nothing is learned, so with affine times only the fold stays pending.
    4  64 packets behind it."""
    c = Case("order_slot%d%s" % (slot, "_runts" if runts else ""), cap=4096, slot=slot,
             runts=runts)
    t = T.NOW0
    b = c.batch("0 warm-up")
    for i in range(N_KNOWN):
        b.add(KNOWN[i], KNOWN[0], i % 3, t + i)
    t += 1000
    k0, k1, k2 = KNOWN[0], KNOWN[1], KNOWN[2]
    named = {
        10: (A[0], A[0], 1, "own-src", 1),
        61: (k0, A[1], 0, "before-learn", FLOOD),
        62: (A[1], k0, 2, "learn", 0),
        63: (A[2], A[1], 1, "after-learn", 2),
        64: (k1, A[2], 1, "after-learn-next-wave", 1),
        99: (k0, A[3], 0, "before-first", FLOOD),
        100: (A[3], k1, 0, "first-sighting", 1),
        130: (A[3], k1, 2, "second-sighting", 1),
        131: (k2, A[3], 2, "to-first-port", 0),
        140: (k1, k0, 2, "moved", 0),
        141: (k0, k1, 0, "to-moved", 1),
        149: (k0, BCAST, 0, "bcast-before", FLOOD),
        150: (BCAST, k0, 2, "bcast-src", 0),
        151: (k1, BCAST, 1, "bcast-after", 2),
        255: (A[4], A[5], 1, "flood-rev", FLOOD),
        256: (A[5], A[4], 2, "fwd-next", 1),
    }
    t = fill(c.batch("1 pairs"), 320, t, named) + 1000
    named = {0: (FIRST, LAST, 1, "first-to-last", FLOOD),
             4095: (LAST, FIRST, 2, "last-to-first", 1)}
    for k in range(1, 64):
        named[64 * k - 1] = (P[k], Q[k], k % 3, "flood-rev", FLOOD)
        named[64 * k] = (Q[k], P[k], (k + 1) % 3, "fwd-next", k % 3)
    t = fill(c.batch("2 every 64"), 4096, t, named) + 1000
    learned = [(A[1], 2), (A[3], 0), (BCAST, 2), (LAST, 2), (FIRST, 1), (P[5], 2), (Q[5], 0),
               (P[63], 0), (Q[63], 1), (A[0], 1)]
    named = {7 * j + 3: (KNOWN[j], m, j % 3, "steady", port)
             for j, (m, port) in enumerate(learned)}
    t = fill(c.batch("3 steady"), 200, t, named) + 1000
    fill(c.batch("4 behind the pending fold"), 64, t, {5: (k0, Q[17], 0, "steady", 0)})
    return c


# --------------------------------------------------------------- b. table full --
FULL_E_US = 1000


def table_full_case():
    """Capacity 64. Batch 0: 70 new MACs, one per packet; fills (63) takes the
    last index, every full-new (64 .. 69) finds the table full and is not
    learned, yet its frame goes where its dst says (to-unlearned: the MAC the
    packet before failed to learn: flood). full-again (70 .. 75): the same six
    once more, still not learned. Then frames to each of them (to-unlearned:
    flood) and to-last-learned (MAC 63: forward). Batch 1, after every entry
    has expired: the six are learned (learned-now) and frames to them forward
    (to-learned-now); to-expired (MAC 0) floods."""
    c = Case("table_full", cap=64, expire_us=FULL_E_US)
    M = [mac(5000 + i) for i in range(70)]
    t = T.NOW0
    b = c.batch("0 fills and overflows")
    for i in range(70):
        if i < 64:
            tag = "fills" if i == 63 else ""
            b.add(M[i], M[0], i % 3, t, tag=tag, want=0 if tag else None)
        elif i == 64:
            b.add(M[i], M[63], i % 3, t, tag="full-new", want=0)
        else:
            b.add(M[i], M[i - 1], i % 3, t, tag="full-new", want=FLOOD)
        t += 1
    for i in range(64, 70):
        b.add(M[i], M[1], (i + 1) % 3, t, tag="full-again", want=1)
        t += 1
    for i in range(64, 70):
        b.add(M[2], M[i], 2, t, tag="to-unlearned", want=FLOOD)
        t += 1
    b.add(M[2], M[63], 2, t, tag="to-last-learned", want=0)
    t += FULL_E_US * 1000 + 200
    b = c.batch("1 after the expiry")
    for i in range(64, 70):
        b.add(M[i], M[64], 1, t, tag="learned-now", want=1)
        t += 1
    for i in range(64, 70):
        b.add(M[64], M[i], 1, t, tag="to-learned-now", want=1)
        t += 1
    b.add(M[64], M[0], 1, t, tag="to-expired", want=FLOOD)
    return c


# ------------------------------------------------------ c. statics and phase C --
S1, S2, S3, S4 = mac(6001), mac(6002), mac(6003), mac(6004)
STATICS = [
    (S1, 0, -1),   # explicit flood
    (S2, 1, -2),   # filter: back to the in port
    (S3, 0, 2),    # forward
    (S3, 0, 1),    # duplicate key: the first rule wins
    (S4, 1, -1),   # explicit flood from the port S4 itself is learned on
]


def statics_case():
    """Batch 1 is one segment in which S1, S2 and S4 are learned dynamically;
    batch 2 repeats its lookups with every MAC known when the segment starts.
    static-flood: a -1 rule floods whether or not the MAC is (being) learned;
    other-port: the same dst from a port without a rule takes the dynamic
    entry, or floods before the MAC is learned (other-port-unknown);
    static-drop: a -2 rule returns the in port; dup-first: the first of two
    rules with one key; own-from-port: S4 sent to itself from the rule's own
    port floods, although its src has just been learned."""
    c = Case("statics", cap=64, statics=STATICS)
    t = T.NOW0
    b = c.batch("0 warm-up")
    for i in range(6):
        b.add(KNOWN[i], KNOWN[0], i % 3, t + i)
    k0, k1, k2 = KNOWN[0], KNOWN[1], KNOWN[2]
    lookups = [(k0, S1, 0, "static-flood", FLOOD), (k2, S1, 2, "other-port", 1),
               (k1, S2, 1, "static-drop", 1), (k2, S2, 2, "other-port", 0),
               (k0, S3, 0, "dup-first", 2), (k1, S3, 1, "other-port-unknown", FLOOD),
               (k0, S4, 0, "other-port", 1), (k1, S4, 1, "static-flood", FLOOD)]
    named = {
        0: (k0, S1, 0, "static-flood", FLOOD),
        1: (k2, S1, 2, "other-port-unknown", FLOOD),
        2: (S1, k0, 1, "learn", 0),
        3: (k0, S1, 0, "static-flood", FLOOD),
        4: (k2, S1, 2, "other-port", 1),
        5: (k1, S2, 1, "static-drop", 1),
        6: (k2, S2, 2, "other-port-unknown", FLOOD),
        7: (S2, k1, 0, "learn", 1),
        8: (k1, S2, 1, "static-drop", 1),
        9: (k2, S2, 2, "other-port", 0),
        10: (k0, S3, 0, "dup-first", 2),
        11: (k1, S3, 1, "other-port-unknown", FLOOD),
        12: (S4, S4, 1, "own-from-port", FLOOD),
        13: (k0, S4, 0, "other-port", 1),
        14: (k1, S4, 1, "static-flood", FLOOD),
    }
    for j, x in enumerate(lookups):  # again behind the first wave
        named[66 + j] = x
    t = fill(c.batch("1 learned in this segment"), 80, t + 1000, named) + 1000
    fill(c.batch("2 known at the segment's start"), 80, t,
         {3 + 9 * j: x for j, x in enumerate(lookups)})
    return c


# ------------------------------------------------------------------- d. expiry --
WRAP_US = 4_294_968          # x 1000 wraps in 32 bits:
WRAP_NS = 704                # 4 294 968 000 - 2^32
CUT, CUT_D = 70, 79
X, D = mac(7000), mac(7001)
KE = [mac(7100 + j) for j in range(8)]


def expiry_case():
    """expiration_time 4 294 968 us, 704 ns after the 32-bit wrap. Warm-up: X
    stamped s, stations KE s + 1 .. s + 8, D stamped s + 9. Then 200 packets
    at s + 635 + i: X's stamp is one above the cutoff at packet 68 (x-below:
    forward), at the cutoff at 69 (x-at: forward), below it at 70 (x-above:
    X has expired, flood) -- the second segment starts inside a tile. 71
    (x-relearn) learns X again from port 2, 72 (x-new-port) goes there. D is
    only ever a destination: d-below (77), d-at (78) forward, d-above (79)
    floods, and D is gone for good (d-gone, 150)."""
    assert (WRAP_US * 1000) & 0xFFFFFFFF == WRAP_NS
    c = Case("expiry", cap=64, expire_us=WRAP_US)
    s = T.NOW0
    b = c.batch("0 warm-up")
    b.add(X, X, 1, s, tag="x", want=1)
    for j in range(8):
        b.add(KE[j], X, j % 3, s + 1 + j)
    b.add(D, X, 0, s + 9, tag="d", want=1)
    b = c.batch("1 the cuts at packets 70 and 79")
    named = {68: (X, 1, "x-below"), 69: (X, 1, "x-at"), CUT: (X, FLOOD, "x-above"),
             72: (X, 2, "x-new-port"), 77: (D, 0, "d-below"), 78: (D, 0, "d-at"),
             CUT_D: (D, FLOOD, "d-above"), 150: (D, FLOOD, "d-gone"), 151: (X, 2, "x-new-port")}
    for i in range(200):
        t = s + WRAP_NS - (CUT - 1) + i
        j = i % 8
        if i == 71:
            b.add(X, KE[0], 2, t, tag="x-relearn", want=0)
        elif i in named:
            dst, want, tag = named[i]
            b.add(KE[j], dst, j % 3, t, tag=tag, want=want)
        else:
            b.add(KE[j], KE[(i + 3) % 8], j % 3, t)
    return c


# --------------------------------------------------------------- e. free order --
N_FREE = 40


def free_order_case():
    """40 MACs learned, then all seen again at one single time in a scrambled
    order (their stamps tie: the order of expiry is the order of the last
    sightings), then one packet expires them all and 40 new MACs take the
    freed indices: the dump by index is the check."""
    rng = np.random.default_rng(0xE55)
    c = Case("free_order", cap=64, expire_us=FULL_E_US)
    M = [mac(8000 + i) for i in range(N_FREE)]
    N = [mac(8500 + i) for i in range(N_FREE)]
    t = T.NOW0
    b = c.batch("0 learn")
    for i in range(N_FREE):
        b.add(M[i], M[0], i % 3, t + i)
    t1 = t + 1000
    b = c.batch("1 every MAC at one timestamp")
    ks = np.arange(N_FREE)
    for k in rng.permutation(np.repeat(ks, 1 + ks % 3)):
        b.add(M[int(k)], M[(int(k) + 1) % N_FREE], int(k) % 3, t1)
    b = c.batch("2 all expire, 40 new MACs")
    t2 = t1 + FULL_E_US * 1000 + 1
    b.add(N[0], M[5], 1, t2, tag="expires-all", want=FLOOD)
    for j in range(1, N_FREE):
        b.add(N[j], N[j - 1], 1, t2 + j)
    return c


# ---------------------------------------------- g. probe past the home bucket --
PROBE_ENV = {"VIGPATH_MIX": "1", "VIGPATH_SPARSE": "-1", "VIGPATH_LIN": "0"}
PROBE_CAP, PROBE_BUCKETS, PROBE_LAYOUT = 64, 64, 32  # (64 >> 1 < the 64-bucket floor)
N_PROBE = 9


def ether_hash(m):
    """rte_ether_addr_hash: one CRC step per byte."""
    h = 0
    for x in m:
        h = crc32c_u32(h, x)
    return h


def home_bucket(h, buckets):
    """vp_table.h home_bucket, the multiplicative layout."""
    return (((h * 0x9E3779B1) & 0xFFFFFFFF) * buckets) >> 32


def probe_macs():
    """N_PROBE MACs that share one home bucket of PROBE_BUCKETS (three entries
    a bucket: the probe path runs three buckets on), and stations whose home
    buckets lie away from that path."""
    by = {}
    k = 9000
    while True:
        m = mac(k)
        k += 1
        g = by.setdefault(home_bucket(ether_hash(m), PROBE_BUCKETS), [])
        g.append(m)
        if len(g) == N_PROBE:
            break
    hb = home_bucket(ether_hash(g[0]), PROBE_BUCKETS)
    away, k = [], 200_000
    while len(away) < 3:
        m = mac(k)
        k += 1
        if (home_bucket(ether_hash(m), PROBE_BUCKETS) - hb) % PROBE_BUCKETS > 8:
            away.append(m)
    return hb, g, away


def probe_case():
    """G0 .. G7 share their home bucket (multiplicative layout, 64 buckets):
    learned three per batch (1 .. 3), they fill the home bucket and the two
    behind it. Batch 4 refreshes all but G1 and G4 and looks every one up as a
    dst (deep-dst, from the third bucket). Batch 5, after G1 and G4 alone have
    expired (one tombstone in the home bucket, one in the next): the MACs
    behind the tombstones as src (deep-src: rejuvenated, not learned again)
    and dst (deep-dst), the expired ones (gone: flood). Batch 6: G8, new, and
    G4 again from another port take the freed entries; every MAC once more."""
    hb, G, away = probe_macs()
    c = Case("probe", cap=PROBE_CAP, expire_us=FULL_E_US, env=PROBE_ENV)
    c.home, c.G = hb, G
    port = {m: i % 3 for i, m in enumerate(G)}
    t = T.NOW0
    b = c.batch("0 stations away from the path")
    for i, m in enumerate(away):
        b.add(m, away[0], i % 3, t + i)
    t += 100
    for r in range(3):
        b = c.batch("%d learn %d .. %d" % (r + 1, 3 * r, min(3 * r + 2, 7)))
        for i in range(3 * r, min(3 * r + 3, 8)):
            b.add(G[i], G[0], port[G[i]], t, tag="learn", want=0)
            t += 1
        t += 100
    t = T.NOW0 + FULL_E_US * 500
    b = c.batch("4 refresh all but G1 and G4")
    for i in (0, 2, 3, 5, 6, 7):
        b.add(G[i], G[(i + 4) % 8], port[G[i]], t, tag="deep-dst", want=port[G[(i + 4) % 8]])
        t += 1
    for i, m in enumerate(away):
        b.add(m, G[7 - i], i % 3, t, tag="deep-dst", want=port[G[7 - i]])
        t += 1
    t = T.NOW0 + FULL_E_US * 1000 + 500
    b = c.batch("5 behind the tombstones")
    b.tombs = 2
    b.add(away[0], G[1], 0, t, tag="gone", want=FLOOD)
    b.add(away[1], G[4], 1, t + 1, tag="gone", want=FLOOD)
    t += 2
    for i in (7, 6, 5, 3, 2):
        b.add(G[i], G[i], (port[G[i]] + 1) % 3, t, tag="deep-src", want=port[G[i]])
        t += 1
    for i in (0, 2, 3, 5, 6, 7):
        b.add(away[2], G[i], 2, t, tag="deep-dst", want=port[G[i]])
        t += 1
    b = c.batch("6 the freed entries taken again")
    b.add(G[8], G[7], 1, t, tag="learn", want=port[G[7]])
    b.add(G[4], G[8], 0, t + 1, tag="learn", want=1)
    t += 2
    now_port = dict(port)
    now_port[G[8]], now_port[G[4]] = 1, 0
    for i in (0, 2, 3, 4, 5, 6, 7, 8):
        b.add(away[0], G[i], 0, t, tag="deep-dst", want=now_port[G[i]])
        t += 1
    b.add(away[0], G[1], 0, t, tag="gone", want=FLOOD)
    return c


# ------------------------------------------------------------------ h. hot src --
HOT_BLOCK, HOT_SLICE = 256, 128  # packets a classify block takes; entries of a bin slice


def hot_src_case():
    """4096 packets from one src to three dsts in one batch: one index takes
    every touch, and its stamp is the last packet's time; the three dsts keep
    the stamps of the warm-up. The touches are meant to overflow a touch-bin
    slice (touch_ovf, tbl_late_touches). By tbl_bins_plan's arithmetic for
    this batch: 64 tiles over a grid of at most 16 blocks of four waves, so a
    block classifies at least HOT_BLOCK = 256 packets, all of which touch one
    index and so one bin, whose slice holds max(2 * 256 / 256 + 32 rounded up
    to 16, 2 * kBinRun) = HOT_SLICE = 128 entries. No counter reports the
    overflow; the CPU test asserts the arithmetic, and a change of the grid
    or of the slice size has to revisit it."""
    c = Case("hot_src", cap=4096)
    H, Ds = mac(9500), [mac(9501 + i) for i in range(3)]
    t = T.NOW0
    b = c.batch("0 warm-up")
    b.add(H, H, 1, t, tag="hot", want=1)
    for i in range(3):
        b.add(Ds[i], H, (2 * i) % 3, t + 1 + i)
    t += 1000
    b = c.batch("1 4096 from one src")
    for i in range(4096):
        last = i == 4095
        b.add(H, Ds[i % 3], 1, t + i, tag="last" if last else "",
              want=(2 * (i % 3)) % 3 if last else None)
    c.hot, c.dsts, c.t_last = H, Ds, t + 4095
    return c
