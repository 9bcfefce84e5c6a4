"""viglb's per-packet and small-burst calls (vp_process_one, small
vp_process_batch / vp_process_mbufs calls: nf.c's two loops) served by the
resident kernel lb_serve: out ports, every frame byte and the state (Lb.dump:
flows and backends) against the CPU oracle, and vp_serve_stats_get showing
which path ran.

Inside a burst viglb's packets depend on each other as no other served NF's
do: a heartbeat from an unknown address allocates a backend and changes what
the CHT scan finds for every later packet, a miss's stored backend decides
where later packets of its flow go, and a flow whose backend died is
re-pointed by its first packet. The hand-built trace below is about that
order. Each frame is its own buffer of len bytes (as an mbuf's data), so the
oracle's frames are zeroed past len. Reference behaviour: viglb/lb_main.c:20-68,
lb_balancer.c:38-167.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import cksum_cases as CC
import orc
import vigor_amd
from gpuh import run_gpu
from tracegen import mixed_lb_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 2064  # (frames of up to 2049 bytes)
N_DEV, WAN = 3, 2
DEV_MACS = [bytes([0x10 * d + i for i in range(6)]) for d in range(N_DEV)]
# (the other servers' traces end in 65 and 130; here 67 and 128: the measured
# routing limit, kLbBurstRoute, is 128, and a larger call is not served; 358
# packets all the same)
SIZES = [1, 2, 31, 32, 33, 64, 67, 128]
# the smallest state that shows every case: 16 flows, 8 backends, and the CHT's
# height a prime above the backends
FCAP, BCAP, HEIGHT = 16, 8, 11
EXP_US = 1000  # both tables: 1 ms
US = 1000
MS = 1_000_000


def make_oracle(fcap=FCAP, bcap=BCAP, height=HEIGHT, fexp=EXP_US, bexp=EXP_US):
    cfg = orc.LbCfg(flow_capacity=fcap, flow_expiration_time=fexp, backend_capacity=bcap,
                    cht_height=height, backend_expiration_time=bexp, wan_device=WAN,
                    n_devices=N_DEV)
    for d in range(N_DEV):
        cfg.device_macs[d][:] = list(DEV_MACS[d])
    return orc.Oracle("lb", cfg)


def make_pair(fcap=FCAP, bcap=BCAP, height=HEIGHT, fexp=EXP_US, bexp=EXP_US):
    args = ["--flow-capacity", str(fcap), "--backend-capacity", str(bcap),
            "--cht-height", str(height), "--flow-expiration", str(fexp),
            "--backend-expiration", str(bexp), "--wan", str(WAN)]
    lb = vigor_amd.Lb(vigor_amd.lb_config_from_args(args, N_DEV, DEV_MACS), gpu=0)
    return lb, make_oracle(fcap, bcap, height, fexp, bexp)


def state_equals(lb, dump):
    """Lb.dump() against an oracle dump: flows, then backends."""
    for x, y in zip(lb.dump(), dump):
        np.testing.assert_array_equal(x[0], y[0])
        live = y[0] == 1
        for a, b in zip(x[1:], y[1:]):
            np.testing.assert_array_equal(a[live], b[live])


def check_state(lb, oracle):
    state_equals(lb, oracle.lb_dump(lb.cfg.flow_capacity, lb.cfg.backend_capacity))


def dump_digest(dump):
    """Both tables: alloc and, on live indices, every other column."""
    h = hashlib.sha256()
    for tab in dump:
        alloc = np.asarray(tab[0])
        live = alloc == 1
        h.update(alloc.astype(np.uint8).tobytes())
        for a in tab[1:]:
            h.update(np.ascontiguousarray(np.asarray(a)[live]).tobytes())
    return h.hexdigest()


def oracle_run(oracle, F, ln, dv, now, a, b):
    """Packets [a, b) through the oracle: (out ports, the frames after)."""
    exp = F[a:b].copy()
    out = oracle.run(exp.reshape(-1), ln[a:b], dv[a:b], now[a:b], F.shape[1])
    return out, exp


def send_burst(lb, F, ln, dv, now, a, b, exp_out, E):
    """Packets [a, b) of the trace (F: n x width, zero past len) as one
    vp_process_batch call, each frame its own buffer of len bytes; out ports
    and every byte against the oracle's (E: the frames after, from row 0 of
    the range)."""
    bufs = [bytearray(F[j, :ln[j]].tobytes()) for j in range(a, b)]
    out = lb.process_mbufs(bufs, dv[a:b], now[a:b])
    np.testing.assert_array_equal(out, exp_out, "out ports, burst [%d, %d)" % (a, b))
    for j in range(b - a):
        assert bytes(bufs[j]) == E[j, :ln[a + j]].tobytes(), "frame %d" % (a + j)
    return out


def burst_vs_oracle(lb, oracle, F, ln, dv, now, a, b):
    out, E = oracle_run(oracle, F, ln, dv, now, a, b)
    return send_burst(lb, F, ln, dv, now, a, b, out, E)


def one_vs_oracle(lb, oracle, F, ln, dv, now, i):
    out, E = oracle_run(oracle, F, ln, dv, now, i, i + 1)
    b = bytearray(F[i, :ln[i]].tobytes())
    assert lb.process(int(dv[i]), b, int(now[i])) == out[0], i
    assert bytes(b) == E[0, :ln[i]].tobytes(), i
    return out[0]


# ------------------------------------------------ the hand-built trace --
def frame(sip, dev, ln=60, proto=17, sport=2000, eth=(0x08, 0x00), ihl=5, tl=None, smac=2,
          width=SLOT):
    """A frame of ln bytes (zero past ln) from address sip to 10.9.8.7:80
    arriving on port dev; the IPv4 total length is ln - 14 unless said
    otherwise; ihl = 6 carries one option word, and the L4 header follows it."""
    f = np.zeros(width, np.uint8)
    f[0:6] = (2, 0, 0, 0, 0, 1)
    f[6:12] = (2, 0xBE, 0, 0, smac >> 8, smac & 0xFF)
    f[12:14] = eth
    f[14] = 0x40 | ihl
    tl = max(ln - 14, 0) if tl is None else tl
    f[16:18] = (tl >> 8, tl & 0xFF)
    f[22:24] = (64, proto)
    f[26:30] = tuple((sip >> s) & 0xFF for s in (24, 16, 8, 0))
    f[30:34] = (10, 9, 8, 7)
    l4 = 14 + 4 * max(ihl, 5)
    if ihl > 5:
        f[34:l4] = 1  # (no-operation options)
    f[l4:l4 + 4] = (sport >> 8, sport & 0xFF, 0, 80)
    f[l4 + 4:] = (np.arange(width - l4 - 4) * 7 + sip + sport) & 0xFF
    f[ln:] = 0
    return f


def W(k, ln=60, tag="", **kw):
    """A WAN packet of flow k (TCP when k is a multiple of 4)."""
    proto = kw.pop("proto", 6 if k % 4 == 0 else 17)
    return frame(T.ip4(11, 0, k >> 8, k & 0xFF), WAN, ln, proto, 2000 + k % 11, **kw), ln, WAN, tag


def H(b, ln=60, tag="", **kw):
    """A heartbeat of backend b: from 192.168.0.b on port b & 1, its own MAC."""
    return frame(T.ip4(192, 168, 0, b), b & 1, ln, smac=b, **kw), ln, b & 1, tag


def flow_key(row):
    """The LoadBalancedFlow of a frame with a 20-byte IPv4 header, as the
    dumps' 16-byte keys hold it (13 bytes)."""
    return bytes(row[26:38]) + bytes(row[23:24])


def src_ip(row):
    return int.from_bytes(bytes(row[26:30]), "little")


def build_order_trace():
    """The eight bursts (SIZES) and, between the fifth and the sixth, one
    packet that is not one of them: 1.3 ms on, where both tables' expiries are
    due, so it takes the pipeline (`calls`: (first, end, is a burst)). No
    expiry is due anywhere in a burst. Times rise by 500 ns per packet."""
    rng = np.random.default_rng(0x1B5E)

    def hits(flows, m, backends=()):
        """Packets of flows seen before (and heartbeats of known backends), a
        few of them long, odd or padded past total_length."""
        out = []
        for _ in range(m):
            r = rng.random()
            if backends and r < 0.2:
                out.append(H(int(rng.choice(backends))))
                continue
            k = int(rng.choice(flows))
            ln = 60 if r < 0.7 else int(rng.integers(61, 1519))
            out.append(W(k, ln, tl=(ln - 14 - int(rng.integers(1, 9))) if r > 0.93 else None))
        return out

    def others():
        """Frames that are not served as flows, on both kinds of device."""
        return [W(1, tag="nf", eth=(0x86, 0xDD)), H(1, tag="nf", eth=(0x08, 0x06)),
                W(2, tag="nf", proto=1), H(2, tag="nf", proto=1),
                W(1, 13, tag="nf"), H(1, 33, tag="nf"), W(2, 37, tag="nf"), H(2, 0, tag="nf"),
                W(1, 60, tag="nf", tl=200), W(1, 60, tag="nf", ihl=4)]

    bursts = [
        [H(1)],
        [W(1), W(1)],
        # backends 2 .. 6 arrive between the new flows 2 .. 10
        [H(2), W(2), W(3), W(4), W(5), W(6), W(7), W(8), H(3), W(8), W(9), H(4), W(9),
         W(10), H(5), W(10), H(6), H(6, tag="hb-again")] + others()[:7] + hits([1, 2, 3], 6),
        # flows 11 .. 16 fill the flow table; 20 .. 24 find no index, before
        # and behind the new backends 7 and 8, which fill the backend table;
        # 9 finds no index there
        [W(11), W(12), W(13), W(14), W(15), W(16), W(20), W(21), W(22), H(7), W(20), W(21),
         W(22), W(23), W(24), H(8), W(23), W(24), W(20), H(9, tag="be-full"), H(9, tag="be-full")]
        + hits(list(range(1, 17)), 11, list(range(1, 9))),
        # 0.6 ms on: backends 6 .. 8 and flows 1 .. 8 are seen again, the rest
        # will have expired at the packet between the bursts
        [H(6), H(7), H(8)] + [W(k) for k in range(1, 9)] + hits(list(range(1, 9)), 22, [6, 7, 8]),
        # behind the expiry: flows 1 .. 8 live on, those of backends 1 .. 5 are
        # stale. Each comes twice; backends 10 .. 12 take dead indices between
        # them; flows 9 .. 12 are new again
        [W(k) for k in (3, 7, 1, 5)] + [H(10), H(11)] + [W(k) for k in (2, 8, 6, 4)] + [H(12)] +
        [W(k) for k in (5, 2, 7, 4, 1, 8, 3, 6)] + [W(9), W(10), H(6), W(9), W(11), W(12), W(11)] +
        others() + hits(list(range(1, 13)), 28, [6, 7, 8, 10, 11, 12]),
        # 67: two requests; a new backend and new flows on both sides of lane 64
        [W(13), H(13), W(13), W(14)] + hits(list(range(1, 15)), 59, [6, 7, 8, 10, 11, 12, 13]) +
        [W(15), H(14), W(15), W(14)],
        # 128: two requests; the flow table fills, then the backend table
        [W(16), W(31), W(32), H(15, tag="be-full"), W(31), W(32)] +
        hits(list(range(1, 17)), 56, [6, 7, 8, 10, 11, 12, 13, 14]) + others() +
        [W(33), W(34), W(33)] + hits(list(range(1, 17)), 53, [6, 7, 8, 10, 11, 12, 13, 14]),
    ]
    assert [len(b) for b in bursts] == SIZES, [len(b) for b in bursts]
    starts = [0, 10 * US, 20 * US, 60 * US, 600 * US, 1310 * US, 1350 * US, 1390 * US]
    pk, now, calls = [], [], []
    for bi, b in enumerate(bursts):
        if bi == 5:  # the packet between: no flow, both expiries run at it
            calls.append((len(pk), len(pk) + 1, False))
            pk.append(W(1, tag="between", eth=(0x86, 0xDD)))
            now.append(T.NOW0 + 1300 * US)
        calls.append((len(pk), len(pk) + len(b), True))
        now += [T.NOW0 + starts[bi] + 500 * j for j in range(len(b))]
        pk += b
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    return F, ln, dv, np.array(now, np.int64), [p[3] for p in pk], calls


def tables(dump):
    """({flow key: (index, ts, backend index)}, {backend ip word: (index, ts,
    mac, nic)}) of an oracle dump."""
    (fa, fts, fk, fb), (ba, bts, bip, bm, bn) = dump
    flows = {bytes(fk[i, :13]): (i, int(fts[i]), int(fb[i])) for i in range(len(fa)) if fa[i]}
    backs = {int(bip[i]): (i, int(bts[i]), bytes(bm[i]), int(bn[i]))
             for i in range(len(ba)) if ba[i]}
    return flows, backs


@pytest.fixture(scope="module")
def order_ref():
    """The trace through the oracle alone, packet by packet, run once: every
    packet's port, frame and the state after it."""
    F, ln, dv, now, tags, calls = build_order_trace()
    o = make_oracle()
    n = F.shape[0]
    out = np.zeros(n, np.uint16)
    E = np.zeros_like(F)
    states, dumps = [], []
    for a, b, _ in calls:
        for j in range(a, b):
            oj, Ej = oracle_run(o, F, ln, dv, now, j, j + 1)
            out[j], E[j] = oj[0], Ej[0]
            states.append(tables(o.lb_dump(FCAP, BCAP)))
        dumps.append(o.lb_dump(FCAP, BCAP))
    return dict(F=F, ln=ln, dv=dv, now=now, tags=tags, calls=calls, out=out, E=E, states=states,
                dumps=dumps)


def replay(r, idx):
    """Packets idx, in that order, through a fresh oracle: the last one's port
    and frame."""
    idx = np.asarray(idx)
    o = make_oracle()
    exp = r["F"][idx].copy()
    out = o.run(exp.reshape(-1), r["ln"][idx], r["dv"][idx], r["now"][idx], SLOT)
    return int(out[-1]), exp[-1]


def test_trace_preconditions(order_ref):
    """The situations the trace is built for all occur inside one burst, read
    off the oracle's ports, frames and the state before and after each packet;
    and nothing in a burst may fall back to the pipeline. No GPU."""
    r = order_ref
    F, ln, dv, now, tags, out, E = (r[k] for k in ("F", "ln", "dv", "now", "tags", "out", "E"))
    st = r["states"]
    seen = set()
    naive_wrong = 0
    dst = lambda row: bytes(row[30:34])  # noqa: E731
    for a, b, is_burst in r["calls"]:
        if not is_burst:
            continue
        flows0, backs0 = st[a - 1] if a else ({}, {})
        live0 = {v[0] for v in backs0.values()}
        new_hb = {}  # backend ip -> the lane that allocated it in this burst
        first_of = {}  # flow key -> its first WAN lane in this burst
        for j in range(a, b):
            f0, b0 = st[j - 1] if j else ({}, {})
            f1, b1 = st[j]
            same = (f0, b0) == (f1, b1)
            fwd = out[j] != dv[j]
            # a per-lane evaluation against the state as the burst found it
            n_out, n_E = replay(r, list(range(a)) + [j])
            wrong = n_out != out[j] or (n_E != E[j]).any()
            naive_wrong += wrong
            if "nf" in tags[j]:
                assert same and out[j] == dv[j] and (E[j] == F[j]).all(), j
                seen.add("not a flow, on the WAN device" if dv[j] == WAN
                         else "not a flow, on a backend's device")
                continue
            if dv[j] != WAN:  # a heartbeat
                ip = src_ip(F[j])
                assert out[j] == dv[j] and (E[j] == F[j]).all() and f0 == f1, j
                if ip not in b0 and ip in b1:
                    assert len(b1) == len(b0) + 1 and b1[ip][1] == now[j], j
                    assert b1[ip][2] == bytes(F[j, 6:12]) and b1[ip][3] == dv[j], j
                    new_hb[ip] = j
                elif ip in b0:
                    assert b1[ip][0] == b0[ip][0] and b1[ip][1] == now[j], j
                    if ip in new_hb:
                        assert "hb-again" not in tags[j] or new_hb[ip] == j - 1
                        seen.add("6 one unknown address on two heartbeat lanes: one allocation, "
                                 "the later stamp")
                else:
                    assert same and len(b0) == BCAP and "be-full" in tags[j], j
                    seen.add("7 the backend table full")
                continue
            key = flow_key(F[j])
            hb_before = [i for i in new_hb.values() if i < j]
            if key not in f0:  # a miss
                assert len(b0) > 0 and fwd, j  # (some backend is alive in every burst)
                stored = key in f1
                assert stored == (len(f0) < FCAP), j
                if stored:
                    assert f1[key][1] == now[j], j
                    be_ip = [ip for ip, v in b1.items() if v[0] == f1[key][2]]
                    assert len(be_ip) == 1 and dst(E[j]) == be_ip[0].to_bytes(4, "little"), j
                else:
                    assert f0 == f1, j
                if hb_before and wrong and n_out != dv[j] and dst(n_E) != dst(E[j]) \
                        and key not in first_of:
                    seen.add("1 a miss behind a new backend goes where the old set would not")
                if key in first_of:
                    i = first_of[key]
                    between = [h for h in hb_before if h > i]
                    if between and key not in st[i][0]:  # the first lane stored nothing
                        assert len(st[i - 1][0]) == FCAP
                        if dst(E[j]) != dst(E[i]):
                            seen.add("3 table full: two lanes of one key go to different backends")
            else:
                fi, _, be = f0[key]
                alive = be in {v[0] for v in b0.values()}
                assert fwd and f1[key][0] == fi and f1[key][1] == now[j], j
                if alive:
                    assert f1[key][2] == be, j
                    be_ip = [ip for ip, v in b0.items() if v[0] == be][0]
                    assert dst(E[j]) == be_ip.to_bytes(4, "little"), j
                    i = first_of.get(key)
                    if i is not None and key not in flows0 and key in st[i][0] and \
                            [h for h in hb_before if h > i]:
                        # its own choice, had the first lane not stored the key
                        own = [x for x in range(a, j) if dv[x] != WAN or flow_key(F[x]) != key]
                        _, o_E = replay(r, list(range(a)) + own + [j])
                        assert dst(E[j]) == dst(E[i]), j
                        if dst(o_E) != dst(E[j]):
                            seen.add("2 a later lane follows the first lane's backend, "
                                     "not its own choice")
                    if key in flows0 and flows0[key][2] not in live0:
                        if i is not None and st[i][0][key][2] != flows0[key][2]:
                            assert st[i - 1][0][key][2] == flows0[key][2]
                            seen.add("4 a stale flow on two lanes: re-pointed, then hit")
                        elif be == flows0[key][2] and be_ip in new_hb:
                            seen.add("5 a stale flow whose dead index a heartbeat of the burst "
                                     "was handed")
                else:
                    assert f1[key][2] != be and f1[key][2] in {v[0] for v in b1.values()}, j
            first_of.setdefault(key, j)
        assert len(st[b - 1][1]) > 0
    want = {"1 a miss behind a new backend goes where the old set would not",
            "2 a later lane follows the first lane's backend, not its own choice",
            "3 table full: two lanes of one key go to different backends",
            "4 a stale flow on two lanes: re-pointed, then hit",
            "5 a stale flow whose dead index a heartbeat of the burst was handed",
            "6 one unknown address on two heartbeat lanes: one allocation, the later stamp",
            "7 the backend table full", "not a flow, on the WAN device",
            "not a flow, on a backend's device"}
    assert want <= seen, want - seen
    print("out ports or frames a per-lane evaluation gets wrong: %d of 358" % naive_wrong)
    assert naive_wrong >= 24
    # routing: 358 packets in the eight bursts, times that never go back,
    # frames the mailbox holds, no IPv4 options (which decline a burst), and
    # no expiry due in a burst: both floors are at least 0.6 ms behind the
    # packet between, and every burst ends inside 1 ms of its floor
    bl = [(a, b) for a, b, k in r["calls"] if k]
    assert [b - a for a, b in bl] == SIZES and sum(SIZES) == 358
    assert (np.diff(now) > 0).all() and (ln <= 2048).all() and (ln > 84).any()
    assert all((F[a:b, 14] & 0x0F <= 5).all() for a, b in bl)
    life = EXP_US * 1000
    assert now[bl[4][1] - 1] - now[0] < life
    between = [a for a, b, k in r["calls"] if not k][0]
    fl_b, be_b = st[between]
    assert set(fl_b) < set(st[between - 1][0]) and set(be_b) < set(st[between - 1][1])
    floor = min([v[1] for v in fl_b.values()] + [v[1] for v in be_b.values()])
    assert floor >= now[bl[4][0]] and now[-1] - floor < life


@pytest.fixture(scope="module")
def order_run(order_ref):
    """The trace on the GPU, run once: every burst against the oracle's ports
    and frames as it goes, the counters before and after, and the state behind
    the whole (Lb.dump() stops the resident kernel)."""
    r = order_ref
    lb, _ = make_pair()
    st0 = lb.serve_stats()
    outs = []
    for a, b, is_burst in r["calls"]:
        if is_burst:
            outs.append(send_burst(lb, r["F"], r["ln"], r["dv"], r["now"], a, b, r["out"][a:b],
                                   r["E"][a:b]))
        else:
            buf = bytearray(r["F"][a, :r["ln"][a]].tobytes())
            assert lb.process(int(r["dv"][a]), buf, int(r["now"][a])) == r["out"][a]
    st1 = lb.serve_stats()
    dump = lb.dump()
    state_equals(lb, r["dumps"][-1])
    return dict(lb=lb, st0=st0, st1=st1,
                ports=hashlib.sha256(np.concatenate(outs).tobytes()).hexdigest(),
                state=dump_digest(dump))


@gpu
def test_order_inside_a_burst(order_ref):
    """GPU against the oracle, burst by burst: ports and frames of every
    burst, and both tables behind every call."""
    r = order_ref
    lb, _ = make_pair()
    for c, (a, b, is_burst) in enumerate(r["calls"]):
        if is_burst:
            send_burst(lb, r["F"], r["ln"], r["dv"], r["now"], a, b, r["out"][a:b], r["E"][a:b])
        else:
            buf = bytearray(r["F"][a, :r["ln"][a]].tobytes())
            assert lb.process(int(r["dv"][a]), buf, int(r["now"][a])) == r["out"][a]
        state_equals(lb, r["dumps"][c])
    st = lb.serve_stats()
    assert st["burst_packets"] == 358 and st["declined"] == 0, st


@gpu
def test_path_is_taken(order_ref, order_run):
    """Every one of the eight bursts is served whole: 358 packets in 1 + 1 + 1
    + 1 + 1 + 1 + 2 + 2 = 10 requests of at most 64 frames, none declined (it
    would be 11 with bursts of 65 and 130, as the other servers' traces have:
    the sweep put viglb's routing limit at 128, so its two largest bursts are
    67 and 128). The
    packet between the bursts takes the pipeline (an expiry is due), so it is
    not counted and costs a launch. The counters stay 0 without lb_serve."""
    r = order_run
    assert sum(SIZES) == 358
    d = {k: r["st1"][k] - r["st0"][k] for k in r["st0"]}
    print("serve stats over the eight bursts:", d)
    assert d["burst_packets"] == 358, d
    assert d["bursts"] == sum((m + 63) // 64 for m in SIZES) == 10, d
    assert d["declined"] == 0 and d["packets_one"] == 0, d
    assert d["launches"] >= 1, d


# ------------------------------------------------------ one at a time --
RUNTS = [0, 13, 14, 33, 34, 37]


def mixed_rows(rng, n, n_flows, n_backends, gap_ns, t0):
    """mixed_lb_trace as rows of SLOT bytes, its gaps (0-2) stretched to
    gap_ns each and its times moved to t0; every eighth packet replaced by a
    frame of 60-1518 bytes (odd lengths, some padded past total_length, some
    with an IPv4 option word) or a runt, of the trace's own flows and
    backends."""
    frames, ln, dv, now = mixed_lb_trace(rng, n, n_flows, n_backends, hb_frac=0.08)
    now = t0 + (now - T.NOW0) * gap_ns
    F = np.zeros((n, SLOT), np.uint8)
    F[:, :64] = frames.reshape(n, 64)
    ln = ln.copy()
    for i in range(n):
        F[i, ln[i]:] = 0
    kinds = set()
    for i in range(0, n, 8):
        r = rng.random()
        L = int(rng.integers(60, 1519)) | 1 if r < 0.3 else int(rng.integers(60, 1519))
        kw = {}
        if 0.3 <= r < 0.5:
            kw["tl"] = L - 14 - int(rng.integers(1, 20))
            kinds.add("padded")
        elif 0.5 <= r < 0.7:
            kw["ihl"] = 6
            kinds.add("options")
        if (i // 8) % 6 == 5:  # every sixth of them a runt, each length in turn
            L, kw = RUNTS[(i // 48) % len(RUNTS)], {}
            kinds.add("runt")
        sip = int.from_bytes(bytes(F[i, 26:30]), "big")
        sport = int.from_bytes(bytes(F[i, 34:36]), "big")
        row = frame(sip, int(dv[i]), L, int(F[i, 23]) or 17, sport, smac=int(F[i, 9]), **kw)
        if dv[i] == WAN and L >= 60:
            row[30:34] = F[i, 30:34]
        F[i], ln[i] = row, L
    assert kinds == {"padded", "options", "runt"}
    return F, ln, dv, now.astype(np.int64)


@gpu
@pytest.mark.parametrize("fcap,t0", [(16, T.NOW0), (1024, T.NOW0),
                                     (16, (7 << 32) | 0x8000_0000), (1024, (7 << 32) | 0xF000_0000)])
def test_process_one_server(fcap, t0):
    """vp_process_one, packet by packet, over a mixed trace about 3 ms long
    with 1 ms flows and backends: expiries fall due on both tables, those
    packets take the pipeline, and the state stays the oracle's across the
    hand-overs. A full flow table at 16; times above 2^32 ns whose low word
    has bit 31 set (the request's time is read as unsigned words)."""
    rng = np.random.default_rng(29)
    n = 600
    F, ln, dv, now = mixed_rows(rng, n, 40, 6, 5000, t0)
    assert now[-1] - now[0] > 2 * EXP_US * 1000 and ((now >> 31) & 1).any() == (t0 > T.NOW0)
    assert set(RUNTS) <= set(ln.tolist()) and (ln > 1000).any() and (ln & 1).any()
    lb, o = make_pair(fcap=fcap)
    outs = []
    for i in range(n):
        outs.append(one_vs_oracle(lb, o, F, ln, dv, now, i))
        if i % 100 == 99:
            check_state(lb, o)
    st = lb.serve_stats()
    check_state(lb, o)
    print("serve stats:", st)
    assert 0 < st["packets_one"] < n, st  # (served, and handed over at the expiries)
    assert any(x != WAN for x, d in zip(outs, dv) if d == WAN)  # (some were balanced)


@gpu
@pytest.mark.parametrize("table", ["flows", "backends"])
def test_cutoff_boundary(table):
    """Once per table: a request whose cutoff equals the table's oldest stamp
    exactly is served (nothing expires at equality: the oracle still holds
    the entry); one nanosecond later it takes the pipeline, which expires it.
    The other table's entries live ten times as long."""
    life = EXP_US * 1000
    kw = dict(fexp=EXP_US, bexp=10 * EXP_US) if table == "flows" else \
        dict(fexp=10 * EXP_US, bexp=EXP_US)
    lb, o = make_pair(**kw)
    t0 = (3 << 32) | 0x9000_0000
    # backend 1 and flow 1 at t0; flow 2 (and backend 1 again) 10 ns later
    pk = [H(1), W(1), H(1), W(2), W(3, tag="at the cutoff"), W(3, tag="one past")]
    now = np.array([t0, t0, t0 + 10, t0 + 10, t0 + life, t0 + life + 1], np.int64)
    if table == "backends":  # backend 2 stays; backend 1's last stamp is t0
        pk[2] = H(2)
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    for i in range(4):
        one_vs_oracle(lb, o, F, ln, dv, now, i)
    s0 = lb.serve_stats()
    assert s0["packets_one"] == 4, s0
    one_vs_oracle(lb, o, F, ln, dv, now, 4)
    s1 = lb.serve_stats()
    fl, be = tables(o.lb_dump(FCAP, BCAP))
    old = flow_key(F[1]) in fl if table == "flows" else src_ip(F[0]) in be
    assert old, "the oracle expired the entry at equality"
    assert s1["packets_one"] == 5, s1  # (served)
    check_state(lb, o)
    one_vs_oracle(lb, o, F, ln, dv, now, 5)
    s2 = lb.serve_stats()
    fl, be = tables(o.lb_dump(FCAP, BCAP))
    gone = flow_key(F[1]) not in fl if table == "flows" else src_ip(F[0]) not in be
    assert gone and s2["packets_one"] == 5, s2  # (the pipeline)
    check_state(lb, o)


@gpu
def test_no_backend_alive():
    """All backends expire (flows live ten times as long), then bursts and
    single packets bring stale flows and misses. A stale flow's erasure is the
    pipeline's: the request is declined, once per flow -- afterwards the flow
    is gone and its packets are plain misses, served, as are the misses of
    flows never seen. The state equals the oracle's throughout."""
    lb, o = make_pair(fexp=10 * EXP_US, bexp=EXP_US)
    t1 = T.NOW0 + 2 * EXP_US * 1000
    pk = [H(1), H(2)] + [W(k) for k in range(1, 7)] + \
        [W(20, tag="between", eth=(0x86, 0xDD))] + \
        [W(1), W(1), W(7), W(1)] + [W(2), W(7), W(3), W(2), W(8), W(3)] + \
        [W(4), W(4), W(9), W(5), W(5), W(1)] + [W(k) for k in (6, 6, 9, 2, 4)]
    n = len(pk)
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    now = np.array([T.NOW0 + 500 * j for j in range(8)] + [t1 + 500 * j for j in range(n - 8)],
                   np.int64)
    burst_vs_oracle(lb, o, F, ln, dv, now, 0, 8)
    assert lb.serve_stats()["burst_packets"] == 8
    one_vs_oracle(lb, o, F, ln, dv, now, 8)  # (the backends expire here: the pipeline)
    fl, be = tables(o.lb_dump(FCAP, BCAP))
    assert len(be) == 0 and len(fl) == 6
    s = lb.serve_stats()
    assert s["declined"] == 0 and s["packets_one"] == 0, s
    # one at a time: stale flow 1 (declined, erased by the pipeline), flow 1
    # again (a miss now: served), a flow never seen, flow 1
    for i in range(9, 13):
        assert one_vs_oracle(lb, o, F, ln, dv, now, i) == WAN
    s = lb.serve_stats()
    assert s["declined"] == 1 and s["packets_one"] == 3, s
    check_state(lb, o)
    # a burst with stale flows 2 and 3: declined whole, once
    burst_vs_oracle(lb, o, F, ln, dv, now, 13, 19)
    s = lb.serve_stats()
    assert s["declined"] == 2 and s["burst_packets"] == 8, s
    check_state(lb, o)
    # one at a time again: flows 4 and 5 are declined once each
    for i in range(19, 25):
        assert one_vs_oracle(lb, o, F, ln, dv, now, i) == WAN
    s = lb.serve_stats()
    assert s["declined"] == 4 and s["packets_one"] == 3 + 4, s
    # flow 6 in a burst (declined), and then the same burst's flows as misses
    burst_vs_oracle(lb, o, F, ln, dv, now, 25, 30)
    s = lb.serve_stats()
    assert s["declined"] == 5 and s["burst_packets"] == 8, s
    fl, be = tables(o.lb_dump(FCAP, BCAP))
    assert len(fl) == 0 and len(be) == 0
    check_state(lb, o)
    # no flow is left: everything is a miss with no backend alive, and served
    later = now[25:30] + 10 * US
    out, E = oracle_run(o, F, ln, dv, np.concatenate([now[:25], later]), 25, 30)
    send_burst(lb, F, ln, dv, np.concatenate([now[:25], later]), 25, 30, out, E)
    s = lb.serve_stats()
    assert s["declined"] == 5 and s["burst_packets"] == 13, s
    check_state(lb, o)


@gpu
@pytest.mark.parametrize("case", ["tile64", "wide256"])
def test_checksum_edges(case):
    """cksum_cases' viglb frames (every position patched so that its rewrite
    there hits a value edge of the checksum arithmetic) through process_mbufs
    bursts of 64 and through process, one at a time: both equal the oracle's,
    and both ran served (all but the calls where the backends expire)."""
    c = CC.lb_case(case)
    slot, n = c["slot"], len(c["ln"])
    F, E = c["fr"].reshape(n, slot), c["exp"].reshape(n, slot)
    ln, dv, now = c["ln"], c["dv"], c["now"]
    args = dict(fcap=CC.LB_FLOW_CAP, bcap=c["bcap"], height=c["height"], fexp=60_000_000,
                bexp=CC.LB_BEXP_US)
    lb, _ = make_pair(**args)
    cuts = sorted(set([0, n] + [int(x) for x in c["cuts"]]))
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for a in range(lo, hi, 64):
            b = min(a + 64, hi)
            send_burst(lb, F, ln, dv, now, a, b, c["exp_out"][a:b], E[a:b])
    st = lb.serve_stats()
    assert st["burst_packets"] >= n - 2 * 64 and st["declined"] == 0, st
    o = CC.lb_oracle(c["bcap"], c["height"])
    o.run(c["fr"].copy(), ln, dv, now, slot)
    state_equals(lb, o.lb_dump(CC.LB_FLOW_CAP, c["bcap"]))
    lb2, _ = make_pair(**args)
    for i in range(n):
        buf = bytearray(F[i, :ln[i]].tobytes())
        assert lb2.process(int(dv[i]), buf, int(now[i])) == c["exp_out"][i], i
        assert bytes(buf) == E[i, :ln[i]].tobytes(), i
    st = lb2.serve_stats()
    assert st["packets_one"] >= n - 2 and st["declined"] == 0, st
    state_equals(lb2, o.lb_dump(CC.LB_FLOW_CAP, c["bcap"]))


CHILD = r"""
import hashlib, json
import numpy as np
import test_lb_serve_gpu as L
F, ln, dv, now, tags, calls = L.build_order_trace()
lb, o = L.make_pair()
outs = []
for a, b, is_burst in calls:
    if is_burst:
        outs.append(L.burst_vs_oracle(lb, o, F, ln, dv, now, a, b))
    else:
        L.one_vs_oracle(lb, o, F, ln, dv, now, a)
st = lb.serve_stats()
L.check_state(lb, o)
print("RESULT " + json.dumps(dict(stats=st, state=L.dump_digest(lb.dump()),
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
    """VIGPATH_SERVE=0: the batch pipeline runs every call; ports and state
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


def rows64(frames, ln):
    n = ln.shape[0]
    F = np.zeros((n, SLOT), np.uint8)
    F[:, :64] = frames.reshape(n, 64)
    for i in range(n):
        F[i, ln[i]:] = 0
    return F


@gpu
def test_interleaving():
    """Served bursts, a vp_process_device batch of 2000 packets (the
    pipeline), a dump, single packets, a burst again: one pair of tables
    throughout, each path seeing what the other left."""
    n = 2300
    rng = np.random.default_rng(9)
    frames, ln, dv, now = mixed_lb_trace(rng, n, 150, 6, hb_frac=0.05)
    F = rows64(frames, ln)
    lb, o = make_pair(fcap=256, fexp=60_000_000, bexp=60_000_000)
    burst_vs_oracle(lb, o, F, ln, dv, now, 0, 50)
    burst_vs_oracle(lb, o, F, ln, dv, now, 50, 150)
    s0 = lb.serve_stats()
    assert s0["burst_packets"] == 150 and s0["bursts"] == 1 + 2 and s0["declined"] == 0, s0
    # vp_process_device over 64-byte slots
    a, b = 150, 2150
    out, E = oracle_run(o, F, ln, dv, now, a, b)
    got, g_out = run_gpu(lb, np.ascontiguousarray(F[a:b, :64]).reshape(-1), ln[a:b], dv[a:b],
                         now[a:b], 64)
    np.testing.assert_array_equal(g_out, out)
    got = got.reshape(-1, 64)
    for j in range(b - a):
        assert (got[j, :ln[a + j]] == E[j, :ln[a + j]]).all(), a + j
    s1 = lb.serve_stats()
    assert {k: s1[k] for k in s1 if k != "launches"} == \
        {k: s0[k] for k in s0 if k != "launches"}, (s0, s1)
    check_state(lb, o)  # (a dump between the paths)
    for i in range(2150, 2200):
        one_vs_oracle(lb, o, F, ln, dv, now, i)
    burst_vs_oracle(lb, o, F, ln, dv, now, 2200, n)
    s2 = lb.serve_stats()
    assert s2["packets_one"] == 50 and s2["burst_packets"] == 250 and s2["declined"] == 0, s2
    assert s2["launches"] - s0["launches"] in (1, 2), (s0, s2)
    check_state(lb, o)


@gpu
def test_lb_and_nat_share_a_gpu():
    """A viglb and a vignat context on one GPU, each with a resident kernel,
    taking turns: the launch of one yields the other's (serve_yield), so both
    make progress; each against its own oracle and counters."""
    import test_nat_gpu as NG
    lb, lo = make_pair(fcap=64, fexp=60_000_000, bexp=60_000_000)
    nat, no = NG.make_pair(max_flows=4096)
    m = 40
    rng = np.random.default_rng(3)
    frames, ln, dv, now = mixed_lb_trace(rng, 4 * m, 30, 6, hb_frac=0.1)
    LF = rows64(frames, ln)
    nfr, nln, ndv, nnow = T.nat_lan_trace(4 * m, 50, order="uniform")
    NF = nfr.reshape(4 * m, 64)
    for a in range(0, 4 * m, m):
        burst_vs_oracle(lb, lo, LF, ln, dv, now, a, a + m)
        exp = NF[a:a + m].copy()
        eo = no.run(exp.reshape(-1), nln[a:a + m], ndv[a:a + m], nnow[a:a + m], 64)
        bufs = [bytearray(NF[j, :nln[j]].tobytes()) for j in range(a, a + m)]
        out = nat.process_mbufs(bufs, ndv[a:a + m], nnow[a:a + m])
        np.testing.assert_array_equal(out, eo)
        for j in range(m):
            assert bytes(bufs[j]) == exp[j, :nln[a + j]].tobytes(), a + j
    check_state(lb, lo)
    NG.check_state(nat, no, 4096)
    sl, sn = lb.serve_stats(), nat.serve_stats()
    assert sl["burst_packets"] == 4 * m and sn["burst_packets"] == 4 * m, (sl, sn)
    assert sl["declined"] == 0 and sn["declined"] == 0, (sl, sn)
