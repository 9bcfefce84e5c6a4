"""Directed traces for vigfw's batch pipeline (vp_fw.hip), shared by
test_fw_edges.py (CPU: each trace reaches what it names, against the oracle
alone) and test_fw_edges_gpu.py (the pipeline against the oracle, bit for
bit).

A Case is a configuration and a sequence of batches. Every packet carries the
out port and the frame the Model below computes for it (Python integers,
written from the reference's text, not from the project's code); a packet a
docstring names also carries a tag and the out port written out by hand
(`want`), which the builder checks against the model. The header matrix's
packets are tagged by their variant and carry the model's port alone.
Untagged packets are filler.
Reference behaviour: vigfw/fw_main.c:21-80, fw_flowmanager.c:38-86,
nf-util.h:116-162.
"""
import numpy as np

from vigor_amd import traces as T

N_DEV, WAN, LAN, LAN2 = 3, 1, 0, 2
DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17"),
            T.mac("22:23:24:25:26:27")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01"),
            T.mac("01:23:45:67:89:02")]
LONG_US = 60_000_000
E_US = 1000
E_NS = E_US * 1000
SERVER = T.ip4(9, 9, 9, 9)


def parse(row, ln):
    """nf_then_get_rte_ipv4_header and nf_then_get_tcpudp_header in Python
    integers over the slot's bytes (bytes past the slot read as 0): None, or
    the FlowId fields as the reference loads them (raw little-endian words)
    (src_port, dst_port, src_ip, dst_ip, protocol). The unread length is a
    uint16_t, so a length below 14 wraps."""
    def r8(o):
        return int(row[o]) if o < len(row) else 0

    def r16(o):
        return r8(o) | (r8(o + 1) << 8)
    unread = (ln - 14) & 0xFFFF
    if (r8(12), r8(13)) != (8, 0) or unread < 20:
        return None
    ihl = r8(14) & 15
    if ihl < 5 or unread < ((r8(16) << 8) | r8(17)):
        return None
    read = 34
    opt = (ihl - 5) * 4
    if opt != 0 and unread - 20 >= opt:
        read += opt
    proto = r8(23)
    if proto not in (6, 17) or ((ln - read) & 0xFFFFFFFF) < 4:
        return None
    return (r16(read), r16(read + 2), r16(26) | (r16(28) << 16), r16(30) | (r16(32) << 16), proto)


def lean(row):
    """The condition of the pipeline's register parse: IPv4 with ihl 5."""
    return (int(row[12]), int(row[13])) == (8, 0) and (int(row[14]) & 15) == 5


class Model:
    """nf_process of vigfw in Python integers: expire (64-bit
    expiration_time * 1000, strictly older than now - E), parse, then a WAN
    packet looks the reversed FlowId up (a hit rejuvenates and goes to the
    flow's internal device) and any other opens or rejuvenates its own (a
    full table stores nothing) and goes out on the WAN device."""

    def __init__(self, max_flows, expire_us):
        self.cap, self.e = max_flows, expire_us * 1000
        self.t = {}  # FlowId -> [int_device, stamp]

    def step(self, row, ln, dev, now):
        """The out port, or None for a frame that comes back untouched on
        its own device."""
        last = now - self.e
        for k in [k for k, v in self.t.items() if v[1] < last]:
            del self.t[k]
        k = parse(row, ln)
        if k is None:
            return None
        if dev == WAN:
            k = (k[1], k[0], k[3], k[2], k[4])
            if k not in self.t:
                return None
            self.t[k][1] = now
            return self.t[k][0]
        if k in self.t:
            self.t[k][1] = now
        elif len(self.t) < self.cap:
            self.t[k] = [dev, now]
        return WAN

    def live(self):
        return {k: (v[0], v[1]) for k, v in self.t.items()}


def be16(v):
    return ((v >> 8) & 255, v & 255)


def be32(v):
    return ((v >> 24) & 255, (v >> 16) & 255, (v >> 8) & 255, v & 255)


def frame(slot, seed, sip, dip, sp, dp, proto=17, ln=60, eth=(8, 0), ihl=5, tl=None,
          sp2=None, dp2=None):
    """A slot, dirty everywhere the header does not say otherwise (never
    zero past the frame's length). tl: the IPv4 total length, the frame's
    unread length unless said. sp2 / dp2: the ports behind the IP options
    (at 34 + 4 (ihl - 5)), where they fit in the slot."""
    f = (((np.arange(slot, dtype=np.uint32) * 7 + seed * 13) & 0xFF) | 1).astype(np.uint8)
    f[0:6] = (0x0A, 1, 2, 3, 4, seed & 0xFF)
    f[6:12] = (0x0A, 9, 8, 7, 6, (seed >> 8) & 0xFF)
    f[12:14] = eth
    f[14] = 0x40 | ihl
    f[16:18] = be16((ln - 14) & 0xFFFF if tl is None else tl)
    f[22:24] = (64, proto)
    f[26:30] = be32(sip)
    f[30:34] = be32(dip)
    f[34:36] = be16(sp)
    f[36:38] = be16(dp)
    o = 34 + 4 * (ihl - 5)
    if sp2 is not None and ihl > 5 and o + 4 <= slot:
        f[o:o + 2] = be16(sp2)
        f[o + 2:o + 4] = be16(dp2)
    return f


def flow(k):
    """Flow k as seen on the LAN side: (src ip, dst ip, src port, dst port)."""
    return (T.ip4(10, 0, (k >> 8) & 255, k & 255), SERVER, 1000 + (k & 0x7FFF), 80)


class Batch:
    def __init__(self, case, note):
        self.case, self.note = case, note
        self.rows, self.ln, self.dv, self.now, self.tags, self.exp, self.want = \
            [], [], [], [], [], [], []

    def put(self, row, ln, dev, t, tag="", want=None, matrix=False):
        """want: the out port written by hand; a tagged packet must have one.
        The one exemption is the header matrix (matrix=True): its 2000 and
        more packets are generated, tagged "<variant> len<n> dev<d>", and
        carry the model's port alone; test_fw_edges.test_matrix_trace derives
        each one's expected port from its variant, length and device
        (whether it parses, which L4 offset is read, whether the ports lie
        past the slot) without the model."""
        c = self.case
        assert not self.now or t >= self.now[-1]
        assert matrix or bool(tag) == (want is not None), (c, self.note, tag)
        out = c.model.step(row, ln, dev, t)
        out = dev | 0x100 if out is None else out  # 0x100: untouched
        assert want is None or out == want, (c, self.note, len(self.now), tag, out, want)
        self.rows.append(row)
        self.ln.append(ln)
        self.dv.append(dev)
        self.now.append(t)
        self.tags.append(tag)
        self.exp.append(out)
        self.want.append(want)
        return self

    def lan(self, k, t, dev=LAN, proto=17, tag="", want=None):
        sip, dip, sp, dp = flow(k)
        row = frame(self.case.slot, len(self.now), sip, dip, sp, dp, proto)
        return self.put(row, 60, dev, t, tag, want)

    def reply(self, k, t, proto=17, tag="", want=None, dev=WAN):
        sip, dip, sp, dp = flow(k)
        row = frame(self.case.slot, len(self.now), dip, sip, dp, sp, proto)
        return self.put(row, 60, dev, t, tag, want)

    def tagged(self, tag):
        return [j for j, t in enumerate(self.tags) if t == tag]

    def affine(self):
        now = self.now
        step = now[1] - now[0] if len(now) > 1 else 1
        ok = all(now[i] == now[0] + i * step for i in range(len(now)))
        return (now[0], step) if ok else None

    def arrays(self):
        return (np.stack(self.rows), np.array(self.ln, np.uint16),
                np.array(self.dv, np.uint16), np.array(self.now, np.int64))

    def out_ports(self):
        return np.array([e & 0xFF for e in self.exp], np.uint16)

    def frames_after(self):
        """The model's frames: bytes 0-11 are the out device's endpoint and
        device MACs on a forwarded frame; nothing else changes."""
        F = np.stack(self.rows).copy()
        for j, e in enumerate(self.exp):
            if not e & 0x100:
                F[j, 0:6] = np.frombuffer(END_MACS[e], np.uint8)
                F[j, 6:12] = np.frombuffer(DEV_MACS[e], np.uint8)
        return F


DROP = 0x100  # want: DROP | device for a frame that comes back untouched


class Case:
    def __init__(self, name, max_flows=64, expire_us=LONG_US, slot=64):
        self.name, self.max_flows, self.expire_us, self.slot = name, max_flows, expire_us, slot
        self.model = Model(max_flows, expire_us)
        self.batches = []

    def batch(self, note=""):
        b = Batch(self, note)
        self.batches.append(b)
        return b

    def final(self):
        """{FlowId: (int_device, stamp)} behind the last batch, by the model."""
        return self.model.live()

    def all_affine(self):
        return all(b.affine() is not None for b in self.batches)

    def __repr__(self):
        return self.name


def lan_key(k, proto=17):
    """Flow k's FlowId as the reference loads it."""
    sip, dip, sp, dp = flow(k)
    return parse(frame(64, 0, sip, dip, sp, dp, proto), 60)


def live_state(dump):
    """{FlowId: (index, stamp, int_device)} of a dump."""
    alloc, ts, keys, dev = dump
    le = lambda b: int.from_bytes(bytes(b), "little")  # noqa: E731
    return {(le(keys[i, 0:2]), le(keys[i, 2:4]), le(keys[i, 4:8]), le(keys[i, 8:12]),
             int(keys[i, 12])): (int(i), int(ts[i]), int(dev[i])) for i in np.nonzero(alloc)[0]}


def make_oracle(case):
    import orc
    cfg = orc.fw_cfg(wan=WAN, expire_us=case.expire_us, max_flows=case.max_flows,
                     device_macs=DEV_MACS, endpoint_macs=END_MACS, n_devices=N_DEV)
    return orc.Oracle("fw", cfg)


def oracle_walk(case, every=512):
    """The case through the oracle alone, packet by packet. Per batch: the out
    ports, the frames, the state before the batch and {position: state behind
    that packet} -- every position of a batch of at most `every` packets; of
    a longer one, the hand-checked packets, the packets before them and the
    last."""
    o = make_oracle(case)
    res, st = [], {}
    for b in case.batches:
        F, ln, dv, now = b.arrays()
        F = F.copy()
        n = len(ln)
        at = set(range(n)) if n <= every else \
            {n - 1} | {j for i, w in enumerate(b.want) if w is not None
                       for j in (i - 1, i) if j >= 0}
        out, states = np.zeros(n, np.uint16), {}
        for j in range(n):
            out[j] = o.run(F[j], ln[j:j + 1], dv[j:j + 1], now[j:j + 1], case.slot)[0]
            if j in at:
                states[j] = live_state(o.fw_dump(case.max_flows))
        res.append(dict(out=out, frames=F, start=st, states=states))
        st = states[n - 1]
    return res


# ---------------------------------------------------- a. order in one segment --
N_KNOWN = 12  # flows 100 .. 111, opened from device 0 (even) or 2 (odd)
FIRST, LAST = 4000, 4001


def kdev(i):
    return LAN2 if i & 1 else LAN


def fill(b, n, t0, named):
    """n packets at t0, t0 + 1, ...: the named positions {pos: (kind, flow,
    dev, tag, want)}, known flows' LAN packets and replies everywhere else."""
    for i in range(n):
        if i in named:
            kind, k, dev, tag, want = named[i]
            if kind == "lan":
                b.lan(k, t0 + i, dev=dev, tag=tag, want=want)
            else:
                b.reply(k, t0 + i, tag=tag, want=want)
        elif i % 3 == 2:
            b.reply(100 + (i * 5) % N_KNOWN, t0 + i)
        else:
            b.lan(100 + i % N_KNOWN, t0 + i, dev=kdev(i % N_KNOWN))
    return t0 + n


def order_case(slot=64):
    """One context, every batch with affine times (step 1 ns), nothing expires.
    0  warm-up: the known flows.
    1  320 packets. reply-before (61) is dropped untouched, open (62), reply-after
       (63, the same wave) goes to the opener's device. first-open (100, device 2)
       and second-open (130, device 0) of one 5-tuple: reply-to-first (131) goes
       to device 2 with device 2's MACs. open (255) and reply-after (256) in two
       blocks' waves.
    2  4096 packets. At every odd multiple of 64, packet 64k - 1 opens the flow
       packet 64k replies to (open / reply-after); at every even one the reply
       comes first (reply-before: dropped) and 64k opens. Packet 0 opens the
       flow the last packet replies to (last-reply); packet 1 replies to the
       flow packet 4094 opens (reply-before).
    3  320 packets: reply-before at 63 and 255, their openers at 64 and 256,
       reply-after at 65 and 257.
    4  200 packets of known flows (steady): nothing is opened, so with affine
       times only the fold stays pending.
    5  64 packets behind it."""
    c = Case("order_slot%d" % slot, max_flows=4096, slot=slot)
    t = T.NOW0
    b = c.batch("0 warm-up")
    for i in range(N_KNOWN):
        b.lan(100 + i, t + i, dev=kdev(i))
    t += 1000
    D = DROP | WAN
    named = {
        61: ("rep", 1001, WAN, "reply-before", D),
        62: ("lan", 1001, LAN2, "open", WAN),
        63: ("rep", 1001, WAN, "reply-after", LAN2),
        99: ("rep", 1003, WAN, "reply-before", D),
        100: ("lan", 1003, LAN2, "first-open", WAN),
        130: ("lan", 1003, LAN, "second-open", WAN),
        131: ("rep", 1003, WAN, "reply-to-first", LAN2),
        255: ("lan", 1004, LAN, "open", WAN),
        256: ("rep", 1004, WAN, "reply-after", LAN),
    }
    t = fill(c.batch("1 pairs"), 320, t, named) + 1000
    named = {0: ("lan", FIRST, LAN2, "open", WAN), 1: ("rep", LAST, WAN, "reply-before", D),
             4094: ("lan", LAST, LAN, "open", WAN), 4095: ("rep", FIRST, WAN, "last-reply", LAN2)}
    for k in range(1, 64):
        f, dev = 2000 + k, kdev(k)
        if k & 1:
            named[64 * k - 1] = ("lan", f, dev, "open", WAN)
            named[64 * k] = ("rep", f, WAN, "reply-after", dev)
        else:
            named[64 * k - 1] = ("rep", f, WAN, "reply-before", D)
            named[64 * k] = ("lan", f, dev, "open", WAN)
    t = fill(c.batch("2 every 64"), 4096, t, named) + 1000
    named = {63: ("rep", 1010, WAN, "reply-before", D), 64: ("lan", 1010, LAN2, "open", WAN),
             65: ("rep", 1010, WAN, "reply-after", LAN2),
             255: ("rep", 1011, WAN, "reply-before", D), 256: ("lan", 1011, LAN, "open", WAN),
             257: ("rep", 1011, WAN, "reply-after", LAN)}
    t = fill(c.batch("3 reversed pairs"), 320, t, named) + 1000
    named = {4: ("rep", 1003, WAN, "steady", LAN2), 11: ("rep", FIRST, WAN, "steady", LAN2),
             17: ("rep", LAST, WAN, "steady", LAN), 70: ("rep", 2002, WAN, "steady", LAN),
             71: ("lan", 2063, LAN, "steady", WAN), 130: ("rep", 2063, WAN, "steady", LAN2)}
    t = fill(c.batch("4 steady"), 200, t, named) + 1000
    fill(c.batch("5 behind the pending fold"), 64, t, {5: ("rep", 1011, WAN, "steady", LAN)})
    return c


# ------------------------------------------------------------- b. key word 3 --
def word3_case(slot=64):
    """The table's key word 3 holds the protocol and, above it, the internal
    device. dev2-open: a flow opened from device 2 is found again (dev2-again,
    a LAN hit that allocates nothing) and its reply goes to device 2
    (dev2-reply). One 4-tuple as UDP from device 0 (udp-open) and as TCP from
    device 2 (tcp-open) are two flows: udp-reply goes to 0, tcp-reply to 2.
    unreversed: a WAN packet whose own 5-tuple is a stored flow misses. Batch 0
    meets all of it inside the segment that opens the flows, batch 1 in a
    later one."""
    c = Case("word3_slot%d" % slot, max_flows=64, slot=slot)
    t = T.NOW0
    D = DROP | WAN
    for note in ("0 in the opening segment", "1 in a later segment"):
        b = c.batch(note)
        first = note[0] == "0"
        b.lan(1, t, dev=LAN2, tag="dev2-open" if first else "dev2-again", want=WAN)
        b.lan(2, t + 1, dev=LAN, proto=17, tag="udp-open" if first else "udp-again", want=WAN)
        b.lan(2, t + 2, dev=LAN2, proto=6, tag="tcp-open" if first else "tcp-again", want=WAN)
        b.lan(1, t + 3, dev=LAN2, tag="dev2-again", want=WAN)
        b.reply(1, t + 4, tag="dev2-reply", want=LAN2)
        b.reply(2, t + 5, proto=17, tag="udp-reply", want=LAN)
        b.reply(2, t + 6, proto=6, tag="tcp-reply", want=LAN2)
        b.lan(1, t + 7, dev=WAN, tag="unreversed", want=D)
        b.reply(1, t + 8, proto=6, tag="other-proto", want=D)
        for i in range(9, 80):  # (and behind the first wave)
            if i == 70:
                b.reply(1, t + i, tag="dev2-reply", want=LAN2)
            elif i == 71:
                b.reply(2, t + i, proto=6, tag="tcp-reply", want=LAN2)
            elif i == 72:
                b.lan(2, t + i, dev=WAN, proto=6, tag="unreversed", want=D)
            else:
                b.lan(3 + i % 5, t + i, dev=kdev(i % 5))
        t += 1000
    return c


# --------------------------------------------------------------- c. table full --
def table_full_case():
    """max_flows 16. Batch 0: 20 new flows, each followed by its reply: open
    (flows 0 .. 15) and their replies (reply-stored), then full-open (16 ..
    19: out on the WAN device, rewritten, nothing stored) and reply-unstored
    (dropped untouched). Batch 1: the 20 replies again, and the four openers
    once more. Batch 2, after every flow has expired: the four are stored
    (open-now) and their replies forward (reply-now); reply-expired (flow 0)
    is dropped."""
    c = Case("table_full", max_flows=16, expire_us=E_US)
    t = T.NOW0
    D = DROP | WAN
    b = c.batch("0 fills and overflows")
    for i in range(20):
        dev = kdev(i)
        b.lan(i, t, dev=dev, tag="open" if i < 16 else "full-open", want=WAN)
        b.reply(i, t + 1, tag="reply-stored" if i < 16 else "reply-unstored",
                want=dev if i < 16 else D)
        t += 2
    b = c.batch("1 the next batch")
    for i in range(20):
        b.reply(i, t, tag="reply-stored" if i < 16 else "reply-unstored",
                want=kdev(i) if i < 16 else D)
        t += 1
    for i in range(16, 20):
        b.lan(i, t, dev=kdev(i), tag="full-open", want=WAN)
        b.reply(i, t + 1, tag="reply-unstored", want=D)
        t += 2
    t += E_NS + 200
    b = c.batch("2 after the expiry")
    for i in range(16, 20):
        b.lan(i, t, dev=kdev(i), tag="open-now", want=WAN)
        b.reply(i, t + 1, tag="reply-now", want=kdev(i))
        t += 2
    b.reply(0, t, tag="reply-expired", want=D)
    return c


# ------------------------------------------------------------ d. header matrix --
LENGTHS = list(range(65))
LONG_LENGTHS = [73, 74, 77, 78, 100]  # (128-byte slots: ihl 15's options fit from 74 on)
PORT_A, PORT_B = 1111, 2222  # flows A (from device 0) and B (from device 2)
HOST = T.ip4(10, 1, 0, 1)


def variants(ln):
    u = (ln - 14) & 0xFFFF
    return [("noneth", dict(eth=(0x86, 0xDD))), ("ihl4", dict(ihl=4)), ("ihl5", {}),
            ("ihl6", dict(ihl=6)), ("ihl15", dict(ihl=15)), ("tl0", dict(tl=0)),
            ("tl-1", dict(tl=(u - 1) & 0xFFFF)), ("tl+1", dict(tl=(u + 1) & 0xFFFF)),
            ("tlFFFF", dict(tl=0xFFFF)), ("proto1", dict(proto=1)), ("proto6", dict(proto=6)),
            ("ihl6tcp+1", dict(ihl=6, proto=6, tl=(u + 1) & 0xFFFF))]


NEVER = ("noneth", "ihl4", "proto1")  # variants that cannot parse at any length


def matrix_case(slot):
    """Every length x variant x arrival device in one batch, valid traffic
    around them. A WAN variant is a reply: the ports at offset 34 are flow A's
    (opened from device 0), the ports behind the IP options flow B's (device
    2), as UDP and as TCP, so a variant that parses is a hit and its out port
    says which offset was read. A variant on device 0 or 2 is an opener of a
    flow of its own (ports 2000 -> 80 at offset 34, 3000 -> 81 behind the
    options): the dump says what was stored."""
    c = Case("matrix_slot%d" % slot, max_flows=4096, slot=slot)
    t = T.NOW0
    b = c.batch("0 warm-up")
    for proto in (17, 6):
        b.put(frame(slot, 0, HOST, SERVER, PORT_A, 80, proto), 60, LAN, t)
        b.put(frame(slot, 1, HOST, SERVER, PORT_B, 80, proto), 60, LAN2, t + 1)
        t += 2
    for i in range(N_KNOWN):
        b.lan(100 + i, t + i, dev=kdev(i))
    t += 1000
    b = c.batch("1 the matrix")
    i = 0
    for ln in LENGTHS + (LONG_LENGTHS if slot >= 128 else []):
        for name, hdr in variants(ln):
            for dev in (WAN, LAN, LAN2):
                tag = "%s len%d dev%d" % (name, ln, dev)
                if dev == WAN:
                    row = frame(slot, i, SERVER, HOST, 80, PORT_A, ln=ln, sp2=80, dp2=PORT_B,
                                **dict(dict(proto=17), **hdr))
                else:
                    row = frame(slot, i, T.ip4(10, 2, i >> 8, i & 255), SERVER, 2000, 80, ln=ln,
                                sp2=3000, dp2=81, **dict(dict(proto=17), **hdr))
                b.put(row, ln, dev, t, tag=tag, matrix=True)
                if i % 4 == 0:
                    b.lan(100 + (i // 4) % N_KNOWN, t, dev=kdev((i // 4) % N_KNOWN))
                elif i % 4 == 2:
                    b.reply(100 + (i // 4) % N_KNOWN, t)
                i += 1
                t += i % 2
    b = c.batch("2 replies to what the matrix opened")
    opened = [k for k in c.model.t if (k[2] >> 8) & 0xFF == 2 and k[2] & 0xFF == 10][:200]
    for j, k in enumerate(opened):
        sp, dp, sip, dip, proto = k
        row = frame(slot, j, 0, 0, 0, 0, proto)
        row[26:30] = np.frombuffer(dip.to_bytes(4, "little"), np.uint8)
        row[30:34] = np.frombuffer(sip.to_bytes(4, "little"), np.uint8)
        row[34:36] = np.frombuffer(dp.to_bytes(2, "little"), np.uint8)
        row[36:38] = np.frombuffer(sp.to_bytes(2, "little"), np.uint8)
        b.put(row, 60, WAN, t + j)
    return c


# ------------------------------------------------------------------- e. expiry --
CUT = 70
XA, XB, XC, KEEP, IDLE = 5000, 5001, 5002, 5003, 5004


def expiry_case():
    """expiration_time 1000 us. Warm-up: flows XA, XB, XC stamped s, s + 1,
    s + 2 (from device 2), the known flows behind them. Batch 1: 200 packets,
    packet i at s + E - 69 + i up to packet 69; packets 70, 71 and 72 share
    s + E + 1, whose cutoff is s + 1: the expiry falls due at packet 70, inside
    a tile. x-below (70): XA's stamp is one below the cutoff, its reply is
    dropped; x-at (71): XB's is the cutoff itself, its reply goes to device 2;
    x-above (72): XC's is one above. x-reopen (75) opens XA again from device
    0 and x-new-dev (76) goes there. Batches 2 .. 7: KEEP, opened once, gets
    nothing but replies (keep-reply) every E / 2 for 3 E and lives; IDLE,
    opened with it, is gone (idle-reply)."""
    c = Case("expiry", max_flows=64, expire_us=E_US)
    s = T.NOW0
    D = DROP | WAN
    b = c.batch("0 warm-up")
    b.lan(XA, s, dev=LAN2, tag="x", want=WAN)
    b.lan(XB, s + 1, dev=LAN2, tag="x", want=WAN)
    b.lan(XC, s + 2, dev=LAN2, tag="x", want=WAN)
    for i in range(8):
        b.lan(100 + i, s + 3 + i, dev=kdev(i))
    b = c.batch("1 the cut at packet 70")
    t = s
    for i in range(200):
        t = s + E_NS - (CUT - 1) + i if i < CUT else s + E_NS + 1 + max(0, i - 72)
        if i == CUT:
            b.reply(XA, t, tag="x-below", want=D)
        elif i == CUT + 1:
            b.reply(XB, t, tag="x-at", want=LAN2)
        elif i == CUT + 2:
            b.reply(XC, t, tag="x-above", want=LAN2)
        elif i == 75:
            b.lan(XA, t, dev=LAN, tag="x-reopen", want=WAN)
        elif i == 76:
            b.reply(XA, t, tag="x-new-dev", want=LAN)
        elif i % 3 == 2:
            b.reply(100 + i % 8, t)
        else:
            b.lan(100 + i % 8, t, dev=kdev(i % 8))
    t += 1000
    b = c.batch("2 the two flows")
    b.lan(KEEP, t, dev=LAN2, tag="keep-open", want=WAN)
    b.lan(IDLE, t, dev=LAN, tag="idle-open", want=WAN)
    t0 = t
    for r in range(1, 7):
        b = c.batch("%d replies alone" % (2 + r))
        t = t0 + r * (E_NS // 2)
        b.reply(KEEP, t, tag="keep-reply", want=LAN2)
        b.reply(KEEP, t + 1)
        if r == 6:
            b.reply(IDLE, t + 2, tag="idle-reply", want=D)
    c.t_keep = t + 1
    return c


N_FREE = 40


def free_order_case():
    """40 flows opened, then all replied to at one single time in a scrambled
    order (their stamps tie: the order of expiry is the order of the last
    replies), then one packet expires them all and 40 new flows take the freed
    indices: the dump by index is the check."""
    rng = np.random.default_rng(0xE56)
    c = Case("free_order", max_flows=64, expire_us=E_US)
    t = T.NOW0
    b = c.batch("0 open")
    for i in range(N_FREE):
        b.lan(6000 + i, t + i, dev=kdev(i))
    t1 = t + 1000
    b = c.batch("1 every flow at one timestamp")
    ks = np.arange(N_FREE)
    for k in rng.permutation(np.repeat(ks, 1 + ks % 3)):
        b.reply(6000 + int(k), t1)
    b = c.batch("2 all expire, 40 new flows")
    t2 = t1 + E_NS + 1
    b.reply(6005, t2, tag="expires-all", want=DROP | WAN)
    for j in range(N_FREE):
        b.lan(6500 + j, t2 + 1 + j, dev=kdev(j))
    return c
