"""vigpol's per-packet and small-burst calls (vp_process_one, small
vp_process_batch / vp_process_mbufs calls: nf.c's two loops) served by the
resident kernel pol_serve: out ports, every frame byte (the policer changes
none) and the state (Pol.dump: alloc, ts, addresses, bucket_size, bucket_time)
against the CPU oracle, and vp_serve_stats_get showing which path ran.

The token bucket is a serial recurrence per destination address
(policer_main.c:39-72), so the lanes of one burst that police the same
address must run in packet order: the hand-built trace below is about that.
Each frame is its own buffer of len bytes (as an mbuf's data), so the oracle's
frames are zeroed past len. Reference behaviour: vigpol/policer_main.c:21-145.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import orc
import vigor_amd
from tracegen import mixed_pol_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 2064  # (frames of up to 2049 bytes)
N_DEV, LAN, WAN = 3, 1, 0
SIZES = [1, 2, 31, 32, 33, 64, 65, 130]
CAP, RATE, BURST = 16, 500, 1500  # entries live 3 s, one token per 2 ms
NS = 1_000_000_000
MS = 1_000_000


def lifetime(rate, burst):
    """policer_expire_entries' exp_time and policer_check_tb's threshold."""
    return burst * NS // rate


def make_oracle(cap=CAP, rate=RATE, burst=BURST):
    return orc.Oracle("pol", orc.pol_cfg(lan=LAN, wan=WAN, rate=rate, burst=burst,
                                         capacity=cap, n_devices=N_DEV))


def make_pair(cap=CAP, rate=RATE, burst=BURST):
    args = ["--lan", str(LAN), "--wan", str(WAN), "--rate", str(rate),
            "--burst", str(burst), "--capacity", str(cap)]
    pol = vigor_amd.Pol(vigor_amd.pol_config_from_args(args, N_DEV), gpu=0)
    return pol, make_oracle(cap, rate, burst)


def state_equals(pol, dump):
    """Pol.dump() against an oracle dump, as test_pol_gpu.check_state."""
    ga, gts, gk, gs, gt = pol.dump()
    oa, ots, ok, os_, ot = dump
    np.testing.assert_array_equal(ga, oa)
    live = oa == 1
    for g, o in ((gts, ots), (gk, ok), (gs, os_), (gt, ot)):
        np.testing.assert_array_equal(g[live], o[live])


def check_state(pol, oracle, cap):
    state_equals(pol, oracle.pol_dump(cap))


def dump_digest(dump):
    """alloc and, on live indices, ts, addresses and both bucket words."""
    alloc = np.asarray(dump[0])
    live = alloc == 1
    h = hashlib.sha256(alloc.astype(np.uint8).tobytes())
    for a in dump[1:]:
        h.update(np.ascontiguousarray(np.asarray(a)[live]).tobytes())
    return h.hexdigest()


def send_burst(pol, F, ln, dv, now, a, b, exp_out):
    """Packets [a, b) of the trace (F: n x slot, zero past len) as one
    vp_process_batch call, each frame its own buffer of len bytes; out ports
    against the oracle's and every byte against the input (never changed)."""
    bufs = [bytearray(F[j, :ln[j]].tobytes()) for j in range(a, b)]
    out = pol.process_mbufs(bufs, dv[a:b], now[a:b])
    np.testing.assert_array_equal(out, exp_out, "out ports, burst [%d, %d)" % (a, b))
    for j in range(b - a):
        assert bytes(bufs[j]) == F[a + j, :ln[a + j]].tobytes(), "frame %d" % (a + j)
    return out


def oracle_run(oracle, F, ln, dv, now, a, b):
    exp = F[a:b].reshape(-1).copy()
    out = oracle.run(exp, ln[a:b], dv[a:b], now[a:b], F.shape[1])
    assert (exp == F[a:b].reshape(-1)).all()  # (the policer rewrites nothing)
    return out


def burst_vs_oracle(pol, oracle, F, ln, dv, now, a, b):
    return send_burst(pol, F, ln, dv, now, a, b, oracle_run(oracle, F, ln, dv, now, a, b))


def one_vs_oracle(pol, oracle, F, ln, dv, now, i):
    eo = oracle_run(oracle, F, ln, dv, now, i, i + 1)
    b = bytearray(F[i, :ln[i]].tobytes())
    assert pol.process(int(dv[i]), b, int(now[i])) == eo[0], i
    assert bytes(b) == F[i, :ln[i]].tobytes(), i
    return eo[0]


# ------------------------------------------------ the hand-built trace --
def fr(k, ln=100, dev=WAN, dt=2 * MS, tag="", eth=(0x08, 0x00), ihl=5, tl=20):
    """A frame to address 10.0.(k >> 8).(k & 255) arriving on port dev, ln
    bytes long (zero past ln), dt ns after the packet before it. The IPv4 total
    length is 20 unless said otherwise, so every frame of 34 bytes or more
    parses (nf-util.h:122-151)."""
    f = np.zeros(SLOT, np.uint8)
    f[0:6] = (2, 0, 0, 0, 0, 1)
    f[6:12] = (2, 0, 0, 0, 0, 2)
    f[12:14] = eth
    f[14] = 0x40 | ihl
    f[16:18] = (tl >> 8, tl & 0xFF)
    f[22:24] = (64, 17)
    f[26:30] = (9, 9, 9, 9)
    f[30:34] = (10, 0, k >> 8, k & 0xFF)
    f[34:] = (np.arange(SLOT - 34) * 7 + k) & 0xFF
    f[ln:] = 0
    return f, ln, dev, dt, tag


def key_of(row):
    """dyn_keys' word for the frame's destination address (bytes 30-33)."""
    return int.from_bytes(bytes(row[30:34]), "little")


def build_order_trace():
    """The eight bursts (SIZES). No expiry is due anywhere in them."""
    rng = np.random.default_rng(0x7B0C)

    def hits(known, m):
        """Small packets: WAN to addresses of `known`, LAN, the third device."""
        out = []
        for _ in range(m):
            k, r = int(rng.choice(known)), rng.random()
            dev = LAN if r < 0.14 else 2 if r < 0.28 else WAN
            out.append(fr(k, int(rng.integers(60, 260)), dev, int(rng.integers(1, 4)) * 2 * MS))
        return out

    def tail():
        """Every address of the full table once, in a scrambled order."""
        return [fr(int(k), int(rng.integers(60, 200))) for k in rng.permutation(np.arange(1, 17))]

    bursts = [
        [fr(1, 100)],
        # the same new address on two lanes: the first allocates (bucket 800),
        # the second is a hit of exactly its size -- not forwarded (the test is >)
        [fr(2, 700), fr(2, 800, dt=1, tag="new2 equal")],
        [fr(2, 800, tag="refill-through"),   # one token later the same size passes
         fr(1, 600), fr(1, 600), fr(1, 600),  # 1400 -> 800 -> 200 -> dropped
         fr(99, 1600, tag="big-unknown"),
         fr(3, 1600, tag="big-before-alloc"), fr(3, 200), fr(3, 1600, tag="big-after-alloc"),
         fr(1, 1700, tag="big-known"),
         fr(4, 100), fr(5, 100), fr(6, 60),
         fr(1, 100, dev=LAN, tag="lan"), fr(1, 100, dev=2, tag="other"),
         fr(4, 100, eth=(0x86, 0xDD), tag="noneth"), fr(4, 100, ihl=4, tag="ihl4"),
         fr(4, 100, tl=200, tag="tlbig"), fr(4, 100, ihl=6, tag="opts"),
         fr(5, 0, tag="runt0"), fr(5, 13, tag="runt13"), fr(5, 33, tag="runt33"),
         fr(5, 34, tag="runt34")] + hits([3, 4, 5], 9),
        # 400 ms on: 200 tokens into address 6's bucket of 1440 -- clamped
        [fr(6, 100, dt=400 * MS, tag="clamp")] +
        [fr(4, 500)] * 4 + [fr(5, 450)] * 4 + [fr(3, 400)] * 4 +
        [fr(8, 100), fr(7, 100), fr(7, 1400, dt=1, tag="equal")] + hits([1, 2, 3, 4, 5, 7, 8], 16),
        [fr(9, 100), fr(10, 100)] + [fr(7, 500)] * 4 + [fr(8, 500)] * 4 + [fr(9, 700)] * 3 +
        [fr(7, 1501, tag="big-known")] + hits(list(range(1, 11)), 19),
        # ten entries so far: 11 .. 16 fill the table inside the burst; 17, 18
        # and 19 find no index, nothing is written, and later lanes to them are
        # dropped too
        [fr(11, 100), fr(12, 100), fr(11, 1600, tag="big-after-alloc"), fr(13, 100), fr(14, 100),
         fr(15, 100), fr(16, 100), fr(17, 100, tag="full"), fr(18, 100, tag="full"),
         fr(17, 100, tag="full"), fr(19, 1600, tag="big-unknown"), fr(18, 1600, tag="big-unknown")] +
        [fr(11, 500)] * 4 + [fr(6, 500)] * 4 + [fr(10, 500)] * 4 + hits(list(range(1, 17)), 40),
    ]
    # the last two bursts: one time each, and at their end every address in a
    # scrambled order (the stamps' sequence numbers decide the expiry order)
    bursts.append([fr(17, 100, tag="full"), fr(2, 1600, tag="big-known")] + [fr(12, 300)] * 3 +
                  hits(list(range(1, 17)), 65 - 5 - 16) + tail())
    bursts.append([fr(18, 100, tag="full")] + [fr(13, 400)] * 4 +
                  hits(list(range(1, 17)), 130 - 5 - 16) + tail())
    assert [len(b) for b in bursts] == SIZES
    pk = [p for b in bursts for p in b]
    n = len(pk)
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    tags = [p[4] for p in pk]
    now = np.zeros(n, np.int64)
    t, at = T.NOW0, 0
    for bi, b in enumerate(bursts):
        for j in range(len(b)):
            if bi < 6 or j == 0:
                t += b[j][3]  # strictly increasing / one time for the whole burst
            now[at + j] = t
        at += len(b)
    return F, ln, dv, now, tags


def live_state(dump):
    """{address word: (index, ts, bucket_size, bucket_time)} of an oracle dump."""
    alloc, ts, keys, bs, bt = dump
    return {int(keys[i]): (i, int(ts[i]), int(bs[i]), int(bt[i]))
            for i in range(alloc.shape[0]) if alloc[i]}


def late_batch(now_last):
    """24 new addresses past every entry's lifetime: all 16 entries expire at
    its first packet, oldest stamp first (equal times: by sequence), and the
    new addresses take the freed indices."""
    m = 24
    pk = [fr(100 + k, 100) for k in range(m)]
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.full(m, 100, np.uint16)
    dv = np.full(m, WAN, np.uint16)
    now = now_last + lifetime(RATE, BURST) + 1 + np.arange(m, dtype=np.int64)
    return F, ln, dv, now


@pytest.fixture(scope="module")
def order_ref():
    """The trace through the oracle alone, packet by packet, run once: every
    packet's port and the state after it, and the batch past the lifetime that
    follows."""
    F, ln, dv, now, tags = build_order_trace()
    o = make_oracle()
    n = F.shape[0]
    out = np.zeros(n, np.uint16)
    states, dumps = [], []
    bounds, a = [], 0
    for m in SIZES:
        for j in range(a, a + m):
            out[j] = oracle_run(o, F, ln, dv, now, j, j + 1)[0]
            states.append(live_state(o.pol_dump(CAP)))
        dumps.append(o.pol_dump(CAP))
        bounds.append((a, a + m))
        a += m
    F2, ln2, dv2, now2 = late_batch(int(now[-1]))
    out2 = oracle_run(o, F2, ln2, dv2, now2, 0, F2.shape[0])
    late = dict(F=F2, ln=ln2, dv=dv2, now=now2, out=out2, dump=o.pol_dump(CAP))
    return dict(F=F, ln=ln, dv=dv, now=now, tags=tags, out=out, states=states, dumps=dumps,
                bounds=bounds, late=late)


def bucket_step(size, btime, ln, now, rate=RATE, burst=BURST):
    """policer_main.c:39-72 for a known address: (forwarded, bucket_size)."""
    diff = now - btime
    size = min(burst, size + diff * rate // NS) if diff < lifetime(rate, burst) else burst
    return (True, size - ln) if size > ln else (False, size)


def test_trace_preconditions(order_ref):
    """The situations the trace is built for all occur, read off the oracle's
    ports and the state before and after each packet; and nothing in it may
    fall back to the pipeline."""
    r = order_ref
    F, ln, dv, now, tags, out = r["F"], r["ln"], r["dv"], r["now"], r["tags"], r["out"]
    seen = set()
    naive_differs = 0      # packets whose port a per-lane evaluation gets wrong
    serial_groups = 0      # >= 3 lanes to one known address, a later one decided by an earlier
    kinds = dict(forwarded=0, policed_drop=0, lan_to_wan=0, other_device=0)
    start = {}
    for bi, (a, b) in enumerate(r["bounds"]):
        end = r["states"][b - 1]
        assert set(start) <= set(end)  # (nothing expires)
        if len(start) < CAP and len(end) == CAP:
            seen.add("the table fills inside a burst")
        lanes_of, wrong_in = {}, {}
        first_len = {}     # address -> the length of the lane that allocated it in this burst
        touched = []       # (index) of every policed packet, in lane order
        for j in range(a, b):
            st0 = r["states"][j - 1] if j else {}
            st1 = r["states"][j]
            key, L, t, dev, tg = key_of(F[j]), int(ln[j]), int(now[j]), int(dv[j]), tags[j].split()
            same = st0 == st1
            policed = key in st1 and st1[key][3] == t and st1[key][1] == t and dev == WAN and \
                (not same or (key in st0 and st0[key][3] == t))
            if dev == WAN and not policed:
                assert same and out[j] == WAN, j   # dropped, nothing written
            if dev == WAN:
                kinds["forwarded" if out[j] == LAN else "policed_drop"] += 1
            elif dev == LAN and out[j] == WAN:
                kinds["lan_to_wan"] += 1
            elif dev == 2 and out[j] == 2:
                kinds["other_device"] += 1
            if policed:
                touched.append(st1[key][0])
                if key not in st0:       # allocated here
                    assert out[j] == LAN and st1[key][2] == BURST - L and L <= BURST, j
                    first_len[key] = L
                else:
                    fwd, size = bucket_step(st0[key][2], st0[key][3], L, t)
                    assert (out[j] == LAN) == fwd and st1[key][2] == size, j
                    if key in start:     # the per-lane evaluation from the pre-burst bucket
                        nf_, _ = bucket_step(start[key][2], start[key][3], L, t)
                        lanes_of[key] = lanes_of.get(key, 0) + 1
                        if nf_ != fwd:
                            naive_differs += 1
                            wrong_in[key] = True
                    if L > BURST:
                        assert out[j] == WAN, j
            # the tagged situations
            if "new2" in tg:
                assert key not in start and policed and key in first_len
                assert st0[key][2] == BURST - first_len[key] and st0[key][0] == st1[key][0]
                seen.add("same new address on two lanes: the second is a hit")
            if "equal" in tg:
                assert policed and key in st0
                d = t - st0[key][3]
                assert st0[key][2] + d * RATE // NS == L and out[j] == WAN and st1[key][2] == L
                seen.add("size == len: not forwarded")
            if "refill-through" in tg:
                assert policed and st0[key][2] <= L < st0[key][2] + (t - st0[key][3]) * RATE // NS
                assert out[j] == LAN
                seen.add("a refill lets a previously dropped size through")
            if "clamp" in tg:
                d = t - st0[key][3]
                assert policed and d < lifetime(RATE, BURST)
                assert st0[key][2] + d * RATE // NS > BURST and st1[key][2] == BURST - L
                seen.add("the refill clamp")
            if "big-unknown" in tg:
                assert L > BURST and key not in end and same and out[j] == WAN
                seen.add("len > burst to an unknown address")
            if "big-before-alloc" in tg:
                assert L > BURST and key not in st1 and key in end and same and out[j] == WAN
                seen.add("len > burst to an address a later lane allocates")
            if "big-after-alloc" in tg:
                assert L > BURST and key not in start and key in st0 and policed
                assert out[j] == WAN and st0[key][3] < t
                seen.add("len > burst to an address an earlier lane allocated")
            if "big-known" in tg:
                assert L > BURST and key in start and policed and out[j] == WAN
                assert st0[key][3] < t or bi >= 6
                seen.add("len > burst to a known address: time and stamp moved")
            if "full" in tg:
                assert len(st0) == CAP and key not in end and same and out[j] == WAN
                seen.add("no free index" if key not in
                         [key_of(F[i]) for i in range(a, j)] else "no free index, a later lane too")
            if "lan" in tg:
                assert same and out[j] == WAN
                seen.add("lan")
            if "other" in tg:
                assert same and out[j] == 2
                seen.add("other")
            for nm in ("noneth", "ihl4", "tlbig", "runt0", "runt13", "runt33"):
                if nm in tg:
                    assert same and out[j] == dev and not policed
                    assert L == {"runt0": 0, "runt13": 13, "runt33": 33}.get(nm, L)
                    seen.add(nm)
            for nm in ("opts", "runt34"):
                if nm in tg:
                    assert policed and (F[j, 14] & 0x0F) == (6 if nm == "opts" else 5)
                    assert L == (34 if nm == "runt34" else L)
                    seen.add(nm)
        serial_groups += sum(1 for k in wrong_in if lanes_of[k] >= 3)
        if bi >= 6:  # one time for the whole burst: the last toucher of every live index
            last = {}
            for pos, i in enumerate(touched):
                last[i] = pos
            order = sorted(last, key=lambda i: last[i])
            assert set(order) == {v[0] for v in end.values()} and len(order) == CAP
            assert order != sorted(order) and order != sorted(order, reverse=True)
            seen.add("every index touched in a scrambled order, burst %d" % bi)
        start = end
    want = {"the table fills inside a burst",
            "same new address on two lanes: the second is a hit", "size == len: not forwarded",
            "a refill lets a previously dropped size through", "the refill clamp",
            "len > burst to an unknown address", "len > burst to an address a later lane allocates",
            "len > burst to an address an earlier lane allocated",
            "len > burst to a known address: time and stamp moved", "no free index",
            "no free index, a later lane too", "lan", "other", "noneth", "ihl4", "tlbig", "opts",
            "runt0", "runt13", "runt33", "runt34",
            "every index touched in a scrambled order, burst 6",
            "every index touched in a scrambled order, burst 7"}
    assert want <= seen, want - seen
    print("ports a per-lane evaluation gets wrong: %d, in %d groups of >= 3 lanes; kinds %s"
          % (naive_differs, serial_groups, kinds))
    assert naive_differs >= 8 and serial_groups >= 1
    assert all(v >= 16 for v in kinds.values()), kinds
    # routing: times that never go back, frames the mailbox holds, and the
    # whole trace inside one lifetime, so no expiry is due anywhere in it
    bounds = r["bounds"]
    assert all((np.diff(now[a:b]) > 0).all() for a, b in bounds[:6])
    assert all((np.diff(now[a:b]) == 0).all() for a, b in bounds[6:])
    assert (np.diff(now) >= 0).all() and (ln <= 2048).all() and (ln > BURST).any()
    assert now[-1] - now[0] < lifetime(RATE, BURST) == 3 * NS
    assert [b - a for a, b in bounds] == SIZES and sum(SIZES) == 358
    # the batch past the lifetime: every old entry gone, 16 of 24 new addresses
    # in. The entries expire oldest stamp first -- all of burst 7's stamps
    # carry one time, so by sequence -- and each freed index goes on top of the
    # free stack, so new address k takes the index whose stamp is the k-th youngest
    late = r["late"]
    ls = live_state(late["dump"])
    assert not (set(ls) & set(start)) and len(ls) == CAP
    assert (late["out"][:CAP] == LAN).all() and (late["out"][CAP:] == WAN).all()
    for k in range(CAP):
        assert ls[key_of(late["F"][k])][0] == order[CAP - 1 - k], k


@pytest.fixture(scope="module")
def order_run(order_ref):
    """The eight bursts on the GPU, run once: every burst against the oracle's
    ports as it goes, the counters before and after, then the state
    (Pol.dump() stops the resident kernel, so the state is read once, behind
    the last burst: a read after every burst would cost a launch each)."""
    r = order_ref
    pol, _ = make_pair()
    st0 = pol.serve_stats()
    outs, per_burst = [], []
    for a, b in r["bounds"]:
        outs.append(send_burst(pol, r["F"], r["ln"], r["dv"], r["now"], a, b, r["out"][a:b]))
        per_burst.append(pol.serve_stats())
    st1 = pol.serve_stats()
    dump = pol.dump()
    state_equals(pol, r["dumps"][-1])
    return dict(pol=pol, st0=st0, st1=st1, per_burst=per_burst,
                ports=hashlib.sha256(np.concatenate(outs).tobytes()).hexdigest(),
                state=dump_digest(dump))


@gpu
def test_order_inside_a_burst(order_ref, order_run):
    """(the bursts themselves are checked as order_run makes them) Then the
    batch past the lifetime, which is not served: the new addresses take the
    freed indices in stamp order, so the addresses by index show ts / tseq were
    stamped in packet order."""
    pol, late = order_run["pol"], order_ref["late"]
    st = pol.serve_stats()
    m = late["F"].shape[0]
    send_burst(pol, late["F"], late["ln"], late["dv"], late["now"], 0, m, late["out"])
    after = pol.serve_stats()
    assert after["bursts"] == st["bursts"] and after["declined"] == st["declined"]
    state_equals(pol, late["dump"])


@gpu
def test_path_is_taken(order_ref, order_run):
    """Every one of the eight bursts is served whole: burst_packets is the sum
    of the eight sizes, 358 (none is declined or left to the pipeline, so no
    smaller count can be right), in 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 = 11 requests
    of at most 64 frames (65 -> 2, 130 -> 3). The counters stay 0 without the
    resident kernel."""
    r = order_run
    n = sum(SIZES)
    assert order_ref["F"].shape[0] == n == 358
    d = {k: r["st1"][k] - r["st0"][k] for k in r["st0"]}
    print("serve stats over the eight bursts:", d)
    assert d["burst_packets"] == 358, d
    assert d["bursts"] == sum((m + 63) // 64 for m in SIZES) == 11, d
    assert d["declined"] == 0 and d["packets_one"] == 0, d
    # one launch, and one more only where the test stalled past the idle exit
    assert d["launches"] in (1, 2), d


# ------------------------------------------------------ one at a time --
def rows_of(frames, ln, slot=64, width=SLOT):
    """The trace's slots as rows of `width` bytes, zero past len (a frame
    longer than its slot carries zeros behind it)."""
    F = np.zeros((ln.shape[0], width), np.uint8)
    F[:, :slot] = frames.reshape(-1, slot)
    for i in range(F.shape[0]):
        F[i, ln[i]:] = 0
    return F


@gpu
@pytest.mark.parametrize("cap,rate,burst,gap_ns", [
    (64, 500, 1500, 2000), (16, 500, 1500, 2000), (64, 1_000_000, 1000, 2000),
    (64, 1_000_000, 1000, 20000)])
def test_process_one_server(cap, rate, burst, gap_ns):
    """vp_process_one, packet by packet: LAN and third-device packets, frames
    that do not parse, sizes above the burst, a full table (cap 16). With 1 ms
    entries the gate is live: at gap_ns = 2000 the 600 packets span about
    0.6 ms, at 20000 about 6 ms, where expiries fall due throughout and those
    packets take the batch path; the results equal the oracle's whatever mix
    of paths ran."""
    rng = np.random.default_rng(23)
    n = 600
    frames, ln, dv, now = mixed_pol_trace(rng, n, 40, gap_ns=gap_ns, big=2000)
    F = rows_of(frames, ln)
    assert (ln > burst).any() and (dv == LAN).any() and (dv == 2).any()
    pol, o = make_pair(cap, rate, burst)
    outs = [one_vs_oracle(pol, o, F, ln, dv, now, i) for i in range(n)]
    st = pol.serve_stats()
    check_state(pol, o, cap)
    print("serve stats:", st)
    assert LAN in outs and WAN in outs and 2 in outs
    if rate == 500:  # (the trace lies inside one lifetime: nothing falls back)
        assert now[-1] - now[0] < lifetime(rate, burst)
        assert st["packets_one"] == n > 0, st
    elif gap_ns == 20000:  # (several lifetimes long: some do)
        assert now[-1] - now[0] > 3 * lifetime(rate, burst)
        assert st["packets_one"] < n, st


@gpu
@pytest.mark.parametrize("len2", [100, 1500, 1501])
def test_cutoff_boundary(len2):
    """An entry whose last stamp equals the cutoff exactly is not expired
    (the oracle confirms it: a 1501-byte packet to an expired address would
    allocate nothing, and the entry is still there behind it), so the packet
    exactly burst * 1e9 / rate ns after the first is served and takes the
    diff >= thr branch: the bucket is burst - len, or burst when len >= burst.
    One nanosecond past that stamp's lifetime the next packet goes to the
    batch path, which expires the entry and allocates it again."""
    life = lifetime(RATE, BURST)
    pk = [fr(1, 1000), fr(1, len2), fr(1, 100)]
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.full(3, WAN, np.uint16)
    now = np.array([T.NOW0, T.NOW0 + life, T.NOW0 + 2 * life + 1], np.int64)
    pol, o = make_pair()
    one_vs_oracle(pol, o, F, ln, dv, now, 0)
    s0 = pol.serve_stats()
    assert s0["packets_one"] == 1, s0
    out = one_vs_oracle(pol, o, F, ln, dv, now, 1)
    s1 = pol.serve_stats()
    st = live_state(o.pol_dump(CAP))
    key = key_of(F[0])
    # the oracle: the entry survived at equality, refilled to the full burst
    assert key in st and st[key][1] == now[1] and st[key][3] == now[1]
    assert st[key][2] == (BURST - len2 if len2 < BURST else BURST)
    assert out == (LAN if len2 < BURST else WAN)
    assert s1["packets_one"] == 2, s1  # (served)
    check_state(pol, o, CAP)           # (stops the server: one more launch below)
    out = one_vs_oracle(pol, o, F, ln, dv, now, 2)
    s2 = pol.serve_stats()
    assert s2["packets_one"] == 2 and out == LAN, s2  # (the batch path)
    st = live_state(o.pol_dump(CAP))
    assert st[key][1] == now[2] and st[key][2] == BURST - 100
    check_state(pol, o, CAP)


LENGTHS = [0, 1, 13, 14, 33, 34, 35, 60, 64, 1499, 1500, 1501, 2048]


@gpu
def test_lengths():
    """Frames of 0 to 2048 bytes in one burst and in one-packet calls, all
    served (only the first bytes cross to the kernel and none come back); a
    2049-byte frame is not: the call falls back with the same results."""
    m = len(LENGTHS)
    pk = [fr(1 + i % 3, L) for i, L in enumerate(LENGTHS)] * 2 + \
        [fr(1, 100), fr(2, 2049), fr(3, 100), fr(1, 2049)]
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.full(len(pk), WAN, np.uint16)
    now = (T.NOW0 + 3 * MS * np.arange(len(pk))).astype(np.int64)
    pol, o = make_pair()
    out = burst_vs_oracle(pol, o, F, ln, dv, now, 0, m)
    assert (out == LAN).any() and (out == WAN).any()
    for i in range(m, 2 * m):
        one_vs_oracle(pol, o, F, ln, dv, now, i)
    s0 = pol.serve_stats()
    assert s0["burst_packets"] == m and s0["bursts"] == 1 and s0["packets_one"] == m, s0
    assert s0["declined"] == 0, s0
    burst_vs_oracle(pol, o, F, ln, dv, now, 2 * m, 2 * m + 3)  # (one frame too long)
    one_vs_oracle(pol, o, F, ln, dv, now, 2 * m + 3)
    s1 = pol.serve_stats()
    assert s1["burst_packets"] == m and s1["packets_one"] == m and s1["declined"] == 0, s1
    check_state(pol, o, CAP)


CHILD = r"""
import hashlib, json
import numpy as np
import test_pol_serve_gpu as P
F, ln, dv, now, tags = P.build_order_trace()
pol, o = P.make_pair()
outs, a = [], 0
for m in P.SIZES:
    outs.append(P.burst_vs_oracle(pol, o, F, ln, dv, now, a, a + m))
    a += m
st = pol.serve_stats()
P.check_state(pol, o, P.CAP)
print("RESULT " + json.dumps(dict(stats=st, state=P.dump_digest(pol.dump()),
      ports=hashlib.sha256(np.concatenate(outs).tobytes()).hexdigest())))
"""


def run_child(**env_add):
    """The order trace in a fresh process (the switches are read once per
    process) with the environment given."""
    env = dict(os.environ, **env_add)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@gpu
def test_fallback_same_results(order_run):
    """VIGPATH_SERVE=0: the batch pipeline runs every burst; ports and state
    are the served run's, and every counter stays 0."""
    res = run_child(VIGPATH_SERVE="0")
    assert res["ports"] == order_run["ports"] and res["state"] == order_run["state"]
    assert all(v == 0 for v in res["stats"].values()), res["stats"]


@gpu
def test_routing_off_in_child(order_run):
    """VIGPATH_SERVE_BURST=0: no burst is routed, the results are the same."""
    res = run_child(VIGPATH_SERVE_BURST="0")
    assert res["ports"] == order_run["ports"] and res["state"] == order_run["state"]
    st = res["stats"]
    assert st["burst_packets"] == 0 and st["bursts"] == 0 and st["declined"] == 0, st


@gpu
def test_interleaving():
    """Served bursts, a vp_process_batch of 2000 packets (the pipeline: above
    the routing limit), single packets, a burst again: one table and one set
    of buckets throughout, each path seeing what the other left, and one more
    launch for the return to the server."""
    n, cap = 2300, 256
    rng = np.random.default_rng(9)
    frames, ln, dv, now = mixed_pol_trace(rng, n, 150, gap_ns=2000, big=1800)
    F = rows_of(frames, ln)
    assert now[-1] - now[0] < lifetime(RATE, BURST)
    pol, o = make_pair(cap)
    burst_vs_oracle(pol, o, F, ln, dv, now, 0, 50)
    burst_vs_oracle(pol, o, F, ln, dv, now, 50, 150)
    s0 = pol.serve_stats()
    assert s0["burst_packets"] == 150 and s0["bursts"] == 1 + 2, s0
    burst_vs_oracle(pol, o, F, ln, dv, now, 150, 2150)
    s1 = pol.serve_stats()
    assert {k: s1[k] for k in s1 if k != "launches"} == \
        {k: s0[k] for k in s0 if k != "launches"}, (s0, s1)
    for i in range(2150, 2200):
        one_vs_oracle(pol, o, F, ln, dv, now, i)
    burst_vs_oracle(pol, o, F, ln, dv, now, 2200, n)
    s2 = pol.serve_stats()
    assert s2["packets_one"] == 50 and s2["burst_packets"] == 250 and s2["declined"] == 0, s2
    # (one return to the server; one more only past an idle exit)
    assert s2["launches"] - s0["launches"] in (1, 2), (s0, s2)
    check_state(pol, o, cap)


@gpu
def test_pol_and_bridge_share_a_gpu():
    """A vigpol and a vigbridge context on one GPU, each with a resident
    kernel, taking turns: the launch of one yields the other's (serve_yield),
    so both make progress; each against its own oracle and counters."""
    import test_bridge_serve_gpu as B
    pol, po = make_pair(64)
    br, bo = B.make_pair(64)
    m = 40
    rng = np.random.default_rng(3)
    frames, ln, dv, now = mixed_pol_trace(rng, 4 * m, 30, gap_ns=2000)
    PF = rows_of(frames, ln)
    BF = np.stack([B.fr(k % 7, (k * 3 + 1) % 9, k % B.N_DEV)[0] for k in range(4 * m)]) \
        .astype(np.uint8)
    bdv = (np.arange(4 * m) % B.N_DEV).astype(np.uint16)
    bln = np.full(4 * m, 60, np.uint16)
    for a in range(0, 4 * m, m):
        burst_vs_oracle(pol, po, PF, ln, dv, now, a, a + m)
        B.burst_vs_oracle(br, bo, BF, bln, bdv, now, a, a + m)
    check_state(pol, po, 64)
    B.check_state(br, bo, 64)
    sp, sb = pol.serve_stats(), br.serve_stats()
    assert sp["burst_packets"] == 4 * m and sb["burst_packets"] == 4 * m, (sp, sb)
    assert sp["declined"] == 0 and sb["declined"] == 0, (sp, sb)
