"""Directed traces for vigpol's batch pipeline (vp_pol.hip), shared by
test_pol_edges.py (CPU: each trace reaches what it names, against the oracle
alone) and test_pol_edges_gpu.py (the pipeline against the oracle, bit for
bit, with the phase-T path asserted through vp_last_kernel).

A Case is a configuration and a sequence of batches; a Batch names the
phase-T path its last segment must take ("group": the grouping path of the
context, "sort": pol_buckets) and carries, where the expected value is simple,
the out port of each packet as a literal computed here with Python integers
(Model: policer_main.c:34-103 for addresses that never expire in the trace).
Reference behaviour: vigpol/policer_main.c:21-145, nf-util.h:122-151.
"""
import numpy as np

from vigor_amd import traces as T

N_DEV, LAN, WAN, OTHER = 3, 1, 0, 2
NS, MS = 10**9, 10**6
RATE, BURST = 500, 1500  # entries live 3 s, one token per 2 ms
U64 = 1 << 64

# path -> (capacity, VIGPATH_POL_RUNS): a segment groups when 8 n >= capacity
PATHS = {"runs": (64, None), "scatter": (64, "0"), "sort": (4096, None)}
FILL = 250  # the destination of LAN filler packets (never policed)
PAD = 12    # packets per small batch: 8 n >= 64 and 8 n < 4096


def lifetime(rate, burst):
    """policer_expire_entries' exp_time and policer_check_tb's threshold:
    burst * 1e9 / rate in unsigned 64-bit arithmetic (the product may wrap)."""
    return (burst * NS % U64) // rate


def kernel_name(path, slot, want):
    """What vp_last_kernel must say after a batch whose last segment takes
    `want` on a context of `path`."""
    k = "pol_classify64" if slot == 64 else "pol_classify"
    if want == "sort" or path == "sort":
        return k + "+pol_buckets"
    return k + ("+pol_runs" if path == "runs" else "+pol_scatter+pol_runs")


def frame(k, slot=64, eth=(0x08, 0x00), ihl=5, tl=20):
    """A slot holding a frame to address 10.(k >> 16).(k >> 8 & 255).(k & 255).
    The IPv4 total length is 20 unless said otherwise, so the header parses
    for every length of 34 bytes or more. The bytes past the frame's length
    are not zeroed: the slot is whatever the NIC left there."""
    f = np.zeros(slot, np.uint8)
    f[0:6] = (2, 0, 0, 0, 0, 1)
    f[6:12] = (2, 0, 0, 0, 0, 2)
    f[12:14] = eth
    f[14] = 0x40 | ihl
    f[16:18] = ((tl >> 8) & 0xFF, tl & 0xFF)
    f[22:24] = (64, 17)
    f[26:30] = (9, 9, 9, 9)
    f[30:34] = (10, (k >> 16) & 0xFF, (k >> 8) & 0xFF, k & 0xFF)
    f[34:] = (np.arange(slot - 34) * 7 + k) & 0xFF
    return f


def key_of(row):
    """dyn_keys' word for the frame's destination address (bytes 30-33)."""
    return int.from_bytes(bytes(row[30:34]), "little")


def key(k):
    return key_of(frame(k))


def parses(row, ln):
    """nf_then_get_rte_ipv4_header (nf-util.h:122-151) in Python integers;
    a length below 14 wraps in 16 bits, as (uint16_t)(len - 14) does."""
    unread = (ln - 14) & 0xFFFF
    return (int(row[12]), int(row[13])) == (8, 0) and unread >= 20 and \
        (int(row[14]) & 15) >= 5 and unread >= ((int(row[16]) << 8) | int(row[17]))


class Model:
    """policer_check_tb (policer_main.c:34-103) in Python integers for
    addresses that do not expire and a table that never fills."""

    def __init__(self, rate, burst):
        self.rate, self.burst, self.thr = rate, burst, lifetime(rate, burst)
        self.b = {}  # k -> [bucket_size, bucket_time]

    def level(self, k, t):
        """The bucket of a known address after the refill at time t."""
        size, bt = self.b[k]
        diff = t - bt
        if diff < self.thr:
            return min(self.burst, size + (diff * self.rate % U64) // NS)
        return self.burst

    def step(self, k, ln, t):
        """One policed packet: forwarded?"""
        if k not in self.b:
            if ln > self.burst:
                return False
            self.b[k] = [self.burst - ln, t]
            return True
        size = self.level(k, t)
        fwd = size > ln
        self.b[k] = [size - ln if fwd else size, t]
        return fwd

    def forget(self, k):
        self.b.pop(k, None)


class Batch:
    def __init__(self, case, want, note):
        self.case, self.want, self.note = case, want, note
        self.rows, self.ln, self.dv, self.now, self.tags, self.exp, self.k = \
            [], [], [], [], [], [], []
        self.live_after = {}   # address -> in the table after the batch?
        self.unchanged = False  # the dump after equals the dump before

    def add(self, k, ln, t, dev=WAN, tag="", exp=None, **hdr):
        """exp: the out port as a literal, None to take it from the case's
        model (a frame that parses), -1 to leave it to the oracle."""
        c = self.case
        row = frame(k, c.slot, **hdr)
        if exp is None:
            if not parses(row, ln):
                exp = dev
            elif dev == LAN:
                exp = WAN
            elif dev != WAN:
                exp = dev
            else:
                exp = LAN if c.model.step(k, ln, t) else WAN
        assert not self.now or t >= self.now[-1]
        self.rows.append(row)
        self.ln.append(ln)
        self.dv.append(dev)
        self.now.append(t)
        self.tags.append(tag)
        self.exp.append(exp)
        self.k.append(k)
        return self

    def pad(self, n=PAD):
        """LAN filler packets at the batch's last time (forwarded to the WAN
        device, never policed) up to n packets, so that a handful of policed
        packets still makes a segment that groups at capacity 64."""
        t = self.now[-1]
        while len(self.ln) < n:
            self.add(FILL, 60, t, dev=LAN, tag="fill")
        return self

    def arrays(self):
        return (np.stack(self.rows).astype(np.uint8), np.array(self.ln, np.uint16),
                np.array(self.dv, np.uint16), np.array(self.now, np.int64))


class Case:
    def __init__(self, name, rate=RATE, burst=BURST, slot=64, cap=None):
        self.name, self.rate, self.burst, self.slot, self.cap = name, rate, burst, slot, cap
        self.model = Model(rate, burst)
        self.batches = []
        self.final = None  # {address: (bucket_size, bucket_time) or None (absent)}

    def batch(self, want, note=""):
        b = Batch(self, want, note)
        self.batches.append(b)
        return b

    def final_from_model(self, absent=()):
        self.final = {k: tuple(v) for k, v in self.model.b.items()}
        self.final.update({k: None for k in absent})
        return self

    def __repr__(self):
        return self.name


def live_state(dump):
    """{address word: (index, ts, bucket_size, bucket_time)} of a dump."""
    alloc, ts, keys, bs, bt = dump
    return {int(keys[i]): (i, int(ts[i]), int(bs[i]), int(bt[i]))
            for i in range(alloc.shape[0]) if alloc[i]}


def make_oracle(case, cap):
    import orc
    return orc.Oracle("pol", orc.pol_cfg(lan=LAN, wan=WAN, rate=case.rate, burst=case.burst,
                                         capacity=cap, n_devices=N_DEV))


def oracle_walk(case, cap=64):
    """The case through the oracle alone, packet by packet: per batch the out
    ports, the state before the batch and the state after every packet."""
    o = make_oracle(case, cap)
    res, st = [], {}
    for b in case.batches:
        F, ln, dv, now = b.arrays()
        out, states = np.zeros(len(ln), np.uint16), []
        for j in range(len(ln)):
            fr = F[j].copy()
            out[j] = o.run(fr, ln[j:j + 1], dv[j:j + 1], now[j:j + 1], case.slot)[0]
            assert (fr == F[j]).all()  # (the policer rewrites nothing)
            states.append(live_state(o.pol_dump(cap)))
        res.append(dict(out=out, start=st, states=states))
        st = states[-1]
    return res


def straddle(case, k, t, j, rng):
    """A length around the bucket's level at time t: the run's even packets
    just below it (forwarded, leaving 1 to 3), its odd ones at it or just
    above (dropped; at it exactly: the test is >). Lengths 14 to 33 leave
    fewer than 20 bytes behind the Ethernet header and do not parse: 13
    (forwarded) or 34 (dropped) stand in for them."""
    lv = case.model.level(k, t)
    if j % 2 == 0 and lv >= 2:
        ln = max(1, lv - int(rng.integers(1, 4)))
        return 13 if 14 <= ln <= 33 else ln
    ln = max(1, lv + int(rng.integers(0, 3)))
    return 34 if 14 <= ln <= 33 else ln


def scrambled_hits(case, b, runs, t, rng, gaps=(0, 3)):
    """A miss-free steady batch: address k gets runs[k] packets, all the runs
    interleaved in a scrambled order, random times with ties, sizes that
    straddle the refill. Returns the last time."""
    ks = np.array(sorted(runs))
    order = rng.permutation(np.repeat(ks, [runs[int(k)] for k in ks]))
    seen = {}
    for k in order:
        k = int(k)
        t += int(rng.integers(*gaps)) * MS
        j = seen.get(k, 0)
        seen[k] = j + 1
        b.add(k, straddle(case, k, t, j, rng), t)
    return t


# ---------------------------------------------------------- a. run lengths --
RUNS = [1, 2, 7, 8, 9, 16, 63, 64]


def run_lengths_case(slot):
    """Warm-up (allocates addresses 1 .. 9), a steady batch whose runs are
    exactly RUNS packets long, a second one with a 65-packet run added."""
    rng = np.random.default_rng(0xA11 + slot)
    c = Case("run_lengths_slot%d" % slot, slot=slot)
    t = T.NOW0
    b = c.batch("sort", "warm-up")
    for k in range(1, 10):
        t += MS
        b.add(k, 100, t)
    b = c.batch("group", "runs 1 2 7 8 9 16 63 64")
    t = scrambled_hits(c, b, dict(zip(range(1, 9), RUNS)), t + MS, rng)
    b = c.batch("sort", "the same and a run of 65")
    scrambled_hits(c, b, dict(zip(range(1, 10), RUNS + [65])), t + MS, rng)
    return c.final_from_model()


# -------------------------------------------------- b. state across segments --
STATE_RUNS = [
    None,                                                    # 0 warm-up
    {k: 1 + (k * 5) % 9 for k in range(1, 13)},              # 1 grouping (clean)
    {**{k: 5 for k in range(4, 13)}, 1: 30, 2: 12, 3: 65},   # 2 a run of 65
    {**{k: 2 for k in range(4, 13)}, 1: 10, 2: 5, 3: 20},    # 3 strictly shorter
    {k: 3 for k in range(1, 13)},                            # 4 (and the misses)
    {k: 1 + k % 4 for k in range(1, 13)},                    # 5 grouping
    {1: 2, 2: 2, 3: 1},                                      # 6 8 n < capacity
    {k: 1 + (k * 3) % 11 for k in range(1, 13)},             # 7 grouping
]
STATE_WANT = ["sort", "group", "sort", "group", "sort", "group", "sort", "group"]


def state_case(slot=64):
    """clean grouping -> fallback (a run of 65) -> grouping with strictly
    shorter runs -> fallback (misses, some larger than the burst, before and
    after the packet that allocates their address) -> grouping -> a batch too
    short to group -> grouping."""
    rng = np.random.default_rng(0xB22)
    c = Case("state_across_segments_slot%d" % slot, slot=slot)
    t = T.NOW0
    b = c.batch("sort", "0 warm-up")
    for k in range(1, 13):
        t += MS
        b.add(k, 100, t)
    for step in range(1, 8):
        b = c.batch(STATE_WANT[step], "step %d" % step)
        t += MS
        if step == 4:  # the misses, spread through the batch's first packets
            big = BURST + 100
            b.add(1, 10, t)
            b.add(20, big, t, tag="big-before-alloc")
            b.add(21, big, t, tag="big-unknown")
            b.add(20, 100, t + MS, tag="alloc")
            b.add(2, 10, t + MS)
            b.add(20, big, t + 2 * MS, tag="big-after-alloc")
            b.add(22, 100, t + 2 * MS, tag="alloc")
            b.add(22, 50, t + 2 * MS)
            t += 2 * MS
        t = scrambled_hits(c, b, STATE_RUNS[step], t, rng)
    return c.final_from_model(absent=[21])


# -------------------------------------------------------- c. bucket arithmetic --
def arith_cases(slot=64):
    cases = []
    t0 = T.NOW0
    life = lifetime(RATE, BURST)

    def new(name, **kw):
        c = Case(name, slot=slot, **kw)
        cases.append(c)
        return c

    # bucket == len: dropped, unchanged; len + 1: forwarded, leaves 1
    c = new("bucket_eq_len_and_len_plus_1")
    c.batch("sort", "warm-up").add(1, 100, t0, exp=LAN).pad()
    t1 = t0 + 4 * MS  # two tokens: 1402
    c.batch("group").add(1, 1402, t1, exp=WAN, tag="exact").add(1, 1401, t1, exp=LAN, tag="plus1") \
        .add(1, 1, t1, exp=WAN, tag="exact").pad()
    c.final = {1: (1, t1)}

    # the first packet as long as the burst: forwarded, leaves 0
    c = new("first_len_eq_burst")
    c.batch("sort").add(1, BURST, t0, exp=LAN, tag="first").add(1, 1, t0, exp=WAN).pad()
    c.batch("group").add(1, 1, t0, exp=WAN).add(1, 1, t0 + 2 * MS, exp=WAN, tag="exact") \
        .add(1, 1, t0 + 4 * MS, exp=LAN).pad()
    c.final = {1: (1, t0 + 4 * MS)}

    # len == burst + 1 to an unknown address: dropped, nothing allocated (with
    # other misses in the segment, and as the segment's only miss)
    c = new("big_unknown")
    c.batch("sort").add(1, 100, t0, exp=LAN).add(7, BURST + 1, t0, exp=WAN, tag="big-unknown").pad()
    c.batch("sort").add(7, BURST + 1, t0 + MS, exp=WAN, tag="big-unknown") \
        .add(1, 10, t0 + MS, exp=LAN).pad()
    c.final = {1: (1390, t0 + MS), 7: None}

    # len == burst + 1 behind the packet that allocates its address: policed,
    # dropped, the entry rejuvenated (ts and bucket_time move, one token in)
    c = new("big_after_alloc")
    c.batch("sort").add(3, BURST + 1, t0, exp=WAN, tag="big-before-alloc") \
        .add(3, 200, t0 + MS, exp=LAN, tag="alloc") \
        .add(3, BURST + 1, t0 + 3 * MS, exp=WAN, tag="big-after-alloc").pad()
    c.final = {3: (1301, t0 + 3 * MS)}

    # diff == thr - 1, thr, thr + 1 from an empty bucket: 1499 tokens (a
    # 1499-byte packet is dropped), the full burst (forwarded, leaves 1), and
    # one past the lifetime the entry is gone: a new flow (a 1500-byte packet
    # is forwarded and leaves 0; as a hit it would have been dropped)
    c = new("diff_around_thr")
    c.batch("sort").add(1, BURST, t0, exp=LAN).add(2, BURST, t0, exp=LAN) \
        .add(3, BURST, t0, exp=LAN).pad()
    c.batch("group").add(1, 1499, t0 + life - 1, exp=WAN, tag="thr-1") \
        .add(2, 1499, t0 + life, exp=LAN, tag="thr").pad()
    c.batch("sort").add(3, BURST, t0 + life + 1, exp=LAN, tag="thr+1").pad()
    c.model.b = {}
    c.final = {1: (1499, t0 + life - 1), 2: (1, t0 + life), 3: (0, t0 + life + 1)}

    # 20 gaps just under 1e9 / rate ns: nothing added, bucket_time advances
    c = new("refill_floors_to_zero")
    gap = NS // RATE - 1
    c.batch("sort").add(1, BURST, t0, exp=LAN).pad()
    b = c.batch("group")
    for i in range(1, 21):
        b.add(1, 1, t0 + i * gap, exp=WAN, tag="floor0")
    b.pad(24)
    c.final = {1: (0, t0 + 20 * gap)}

    # diff * rate above 2^63 (and below 2^64): unsigned. Each long gap opens
    # a batch of its own: a batch that ends more than a lifetime behind the
    # oldest stamp it began with is cut by the batch driver (run_batch), and
    # the last segment would be too short to group
    c = new("product_above_2_63", rate=10**10, burst=15 * 10**9)
    c.batch("sort").add(1, 60000, t0).pad()
    t = t0
    for gaps in (((1000, 60000),), ((1_400_000_000, 65535), (1000, 60000)),
                 ((1_450_000_000, 1), (3, 65535)),
                 ((lifetime(10**10, 15 * 10**9) - 1, 65535),)):
        b = c.batch("group")
        for gap, ln in gaps:
            t += gap
            b.add(1, ln, t, tag="gap %d" % gap)
        b.pad()
    c.final_from_model()

    # burst * 1e9 wraps in 64 bits: the lifetime is the wrapped product's
    c = new("burst_ns_wraps", rate=1000, burst=2 * 10**10)
    wl = lifetime(1000, 2 * 10**10)
    c.batch("sort").add(1, 100, t0).add(2, 100, t0).pad()
    c.batch("group").add(1, 100, t0 + MS, tag="one token").add(2, 100, t0 + wl - 1, tag="thr-1").pad()
    c.model.forget(1)  # expired at the next packet: its stamp is t0 + 1 ms
    c.batch("sort").add(3, 100, t0 + wl + MS + 1, tag="expires 1").add(1, 100, t0 + wl + MS + 1).pad()
    c.final_from_model()

    # equal times inside a run of 10 (and one of 3)
    c = new("equal_times_in_a_run")
    c.batch("sort").add(1, 100, t0).add(2, 100, t0).pad()
    t1 = t0 + 10 * MS  # 1405
    b = c.batch("group")
    for i, ln in enumerate((500, 500, 500, 400, 5, 4, 1, 1, 2, 1)):
        b.add(1, ln, t1, tag="tie")
        if i % 4 == 0:
            b.add(2, 700, t1, tag="tie")
    b.pad()
    c.final_from_model()
    assert c.final[1] == (1, t1)
    return cases


# -------------------------------------------------- d. header and length edges --
LENGTHS = [0, 1, 13, 14, 33, 34, 35, 60, 64]


def variants(ln):
    return [("noneth", dict(eth=(0x86, 0xDD))), ("ihl4", dict(ihl=4)), ("ihl5", dict(ihl=5)),
            ("ihl6", dict(ihl=6)), ("ihl15", dict(ihl=15)),
            ("tl_fits", dict(tl=(ln - 14) & 0xFFFF)), ("tl_over", dict(tl=(ln - 13) & 0xFFFF)),
            ("plain", dict(tl=46))]


def header_mix_case(slot):
    """Every length x variant x input device in one batch, valid traffic
    around them (capacity 256: the batch is long enough to try to group)."""
    rng = np.random.default_rng(0xD44 + slot)
    c = Case("header_mix_slot%d" % slot, slot=slot, cap=256)
    t = T.NOW0
    b = c.batch("sort", "warm-up")
    for k in range(1, 9):
        t += MS
        b.add(k, 100, t)
    b = c.batch("sort", "the variants")
    i = 0
    for ln in LENGTHS:
        for name, hdr in variants(ln):
            for dev in (WAN, LAN, OTHER):
                t += int(rng.integers(0, 3)) * MS
                b.add(1 + (i // 3) % 12, ln, t, dev=dev, tag="%s len%d" % (name, ln), **hdr)
                if i % 3 == 0:
                    b.add(1 + int(rng.integers(0, 8)), int(rng.integers(60, 300)), t)
                i += 1
    b = c.batch("group", "steady behind them")
    scrambled_hits(c, b, {k: 4 for k in sorted(c.model.b)}, t + MS, rng)
    return c.final_from_model()


def expiry_edge_case(slot):
    """Each variant as the last packet of a batch in which entry 100 + i's
    expiry falls due at that packet alone: the entry is gone exactly when the
    variant's header parses. Then a batch without any IPv4 frame while an
    expiry is due (the table stays as it was), and one valid packet."""
    c = Case("expiry_edge_slot%d" % slot, slot=slot)
    life = lifetime(RATE, BURST)
    t = T.NOW0
    i = 0
    for ln in LENGTHS:
        for name, hdr in variants(ln):
            dev = (WAN, LAN, OTHER)[i % 3]
            b = c.batch("sort", "%s len%d dev%d" % (name, ln, dev))
            b.add(100 + i, 100, t, exp=LAN, tag="entry").pad(3)
            t += life + 1
            b.add(200, ln, t, dev=dev, exp=-1, tag="variant", **hdr)
            b.live_after = {100 + i: not parses(b.rows[-1], ln)}
            t += MS
            i += 1
    b = c.batch("sort", "the entry for the batch without IPv4")
    b.add(300, 100, t, exp=-1).pad(3)
    b = c.batch("sort", "no IPv4 frame at all, an expiry due")
    t += life + 1
    for name, hdr, ln in (("noneth", dict(eth=(0x86, 0xDD)), 60), ("ihl4", dict(ihl=4), 64),
                          ("len33", {}, 33), ("tl_over", dict(tl=47), 60), ("len14", {}, 14)):
        b.add(300, ln, t, dev=(WAN, LAN, OTHER)[len(b.ln) % 3], tag=name, **hdr)
    b.live_after = {300: True}
    b.unchanged = True
    b = c.batch("sort", "one valid packet")
    b.add(301, 100, t + 1, exp=-1)
    b.live_after = {300: False, 301: True}
    return c


# ------------------------------------------------------------ e. segment edges --
CUT = 70


def segment_cut_case():
    """200 packets in 64-byte slots: entries 10 and 11 fall due at packet 70
    (inside the second tile), address 1 is hit on both sides of the cut and
    address 11 is allocated again behind it."""
    rng = np.random.default_rng(0xE55)
    c = Case("segment_cut", slot=64)
    life = lifetime(RATE, BURST)
    t0 = T.NOW0
    b = c.batch("sort", "warm-up")
    for k in (1, 2, 3, 4, 5, 6, 10, 11):
        b.add(k, 100, t0)
    b = c.batch("sort", "the cut at packet 70")
    for i in range(200):
        t = t0 + life - CUT + i if i < CUT else t0 + life + 1 + (i - CUT)
        if i == CUT:
            c.model.forget(10)
            c.model.forget(11)
        k = 11 if i in (75, 80, 90, 150) else 1 if i in (CUT - 1, CUT, CUT + 1) else 1 + i % 6
        b.add(k, 100 if i == 75 else int(rng.integers(100, 200)), t,
              tag="cut" if i == CUT else "realloc" if i == 75 else "")
    return c.final_from_model(absent=[10])


# --------------------------------------------------------------- f. free order --
N_FREE = 40


def free_order_case(slot=64):
    """40 addresses, all touched in one steady batch at a single timestamp in
    a scrambled order; one later packet expires them all (oldest stamp first:
    equal times, so by sequence) and 40 new addresses take the freed
    indices."""
    rng = np.random.default_rng(0xF66)
    c = Case("free_order", slot=slot)
    life = lifetime(RATE, BURST)
    t = T.NOW0
    b = c.batch("sort", "warm-up")
    for k in range(1, N_FREE + 1):
        t += MS
        b.add(k, 100, t)
    t1 = t + 10 * MS
    b = c.batch("group", "every address at one timestamp")
    ks = np.arange(1, N_FREE + 1)
    for k in rng.permutation(np.repeat(ks, 1 + ks % 3)):
        b.add(int(k), 10, t1)
    b = c.batch("sort", "all expire, 40 new addresses")
    for k in range(1, N_FREE + 1):
        c.model.forget(k)
    for j in range(N_FREE):
        b.add(1001 + j, 100, t1 + life + 1 + j)
    return c.final_from_model(absent=range(1, N_FREE + 1))
