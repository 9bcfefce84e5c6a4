"""vigfw's per-packet and small-burst calls (vp_process_one, small
vp_process_batch / vp_process_mbufs calls: nf.c's two loops) served by the
resident kernel fw_serve: out ports, every frame byte and the flow state
(Fw.dump) against the CPU oracle, and vp_serve_stats_get showing which path
ran.

Each frame is its own buffer of len bytes (as an mbuf's data), so the oracle's
frames are zeroed past len. Reference behaviour: vigfw/fw_main.c:21-80,
fw_flowmanager.c:38-86.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import orc
import vigor_amd
from gpuh import run_gpu
from tracegen import mixed_fw_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17"),
            T.mac("22:23:24:25:26:27")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01"),
            T.mac("01:23:45:67:89:02")]
SERVER_IP = T.ip4(8, 8, 8, 8)
SLOT = 64
WAN = 1
SIZES = [1, 2, 31, 32, 33, 64, 65, 130]
MAX_FLOWS = 16
EXPIRE_US = 60_000_000
EXPIRE_NS = EXPIRE_US * 1000  # (64-bit in vigfw: no wrap, fw_flowmanager.c:66-68)


def make_oracle(max_flows, expire_us=EXPIRE_US):
    ocfg = orc.fw_cfg(wan=WAN, expire_us=expire_us, max_flows=max_flows,
                      device_macs=DEV_MACS, endpoint_macs=END_MACS, n_devices=3)
    return orc.Oracle("fw", ocfg)


def make_pair(max_flows, expire_us=EXPIRE_US):
    """As test_fw_gpu.make_pair: 3 devices, wan = 1."""
    args = ["--wan", str(WAN), "--expire", str(expire_us), "--max-flows", str(max_flows)]
    for d in range(3):
        args += ["--eth-dest", "%d,%s" % (d, END_MACS[d].hex(":"))]
    cfg = vigor_amd.fw_config_from_args(args, 3, DEV_MACS)
    return vigor_amd.Fw(cfg, gpu=0), make_oracle(max_flows, expire_us)


def state_equals(fw, dump):
    """Fw.dump() against an oracle dump (alloc, ts, keys, int_devices)."""
    ga, gts, gk, gd = fw.dump()
    oa, ots, ok, od = dump
    np.testing.assert_array_equal(ga, oa)
    live = oa == 1
    np.testing.assert_array_equal(gts[live], ots[live])
    np.testing.assert_array_equal(gk[live], ok[live])
    np.testing.assert_array_equal(gd[live], od[live])


def check_state(fw, oracle, max_flows):
    state_equals(fw, oracle.fw_dump(max_flows))


def send_burst(fw, F, ln, dv, now, a, b, E, exp_out):
    """Packets [a, b) of the trace (F: n x slot, zero past len) as one
    vp_process_batch call, each frame its own buffer of len bytes; out ports
    and every byte against the oracle's (E: its frames of [a, b))."""
    bufs = [bytearray(F[j, :ln[j]].tobytes()) for j in range(a, b)]
    out = fw.process_mbufs(bufs, dv[a:b], now[a:b])
    np.testing.assert_array_equal(out, exp_out, "out ports, burst [%d, %d)" % (a, b))
    for j in range(b - a):
        assert bytes(bufs[j]) == E[j, :ln[a + j]].tobytes(), "frame %d" % (a + j)


def burst_vs_oracle(fw, oracle, F, ln, dv, now, a, b):
    """send_burst against the oracle run over the same packets. Returns the
    oracle's (frames, out ports)."""
    slot = F.shape[1]
    exp = F[a:b].reshape(-1).copy()
    exp_out = oracle.run(exp, ln[a:b], dv[a:b], now[a:b], slot)
    E = exp.reshape(b - a, slot)
    send_burst(fw, F, ln, dv, now, a, b, E, exp_out)
    return E, exp_out


# ------------------------------------------------ the hand-built trace --
def proto_of(k):
    return 6 if k % 2 == 0 else 17


def lan_frame(k, dev=0):
    """LAN flow k: 10.0.0.k:1000+k -> 8.8.8.8:53, arriving on LAN device dev."""
    f, _ = T.udp_frames(np.array([T.ip4(10, 0, 0, 0) + k]), np.array([SERVER_IP]),
                        np.array([1000 + k]), np.array([53]), slot=SLOT, proto=proto_of(k))
    return f.copy(), 60, dev


def wan_frame(k):
    """The server's reply to flow k (the reversed 5-tuple, on the WAN device)."""
    f, _ = T.udp_frames(np.array([SERVER_IP]), np.array([T.ip4(10, 0, 0, 0) + k]),
                        np.array([53]), np.array([1000 + k]), slot=SLOT, proto=proto_of(k))
    return f.copy(), 60, WAN


def odd_frame(kind):
    f, ln, dv = lan_frame(0)
    if kind == "v6":
        f[12:14] = (0x86, 0xDD)
    elif kind == "icmp":
        f[23] = 1
    else:  # truncated: kind = its length
        ln = kind
        f[ln:] = 0
    return f, ln, dv


def build_order_trace():
    """The eight bursts (SIZES). No expiry is due anywhere (60 s)."""
    rng = np.random.default_rng(0xF1BE)
    L, W = lan_frame, wan_frame

    def hits(known, m):  # packets of flows that exist: LAN hits and replies
        out = []
        for k in rng.integers(0, known, m):
            out.append(L(int(k), dev=int(rng.choice([0, 2]))) if rng.random() < 0.6
                       else W(int(k)))
        return out

    bursts = [
        [L(0)],
        [L(1), L(1)],  # the same new 5-tuple on two lanes
        # the same new 5-tuple from two LAN devices (the reply goes to the first
        # one's), a reply before its flow is born (3: dropped) and after it,
        # odd frames
        [L(2, dev=2), L(2, dev=0), W(2), W(3), L(3), odd_frame("v6"), odd_frame(20),
         odd_frame(10), odd_frame(37), odd_frame("icmp"), W(3)] + hits(4, 20),
        [L(4), L(4, dev=2), W(5), L(5, dev=2), W(5), W(4), odd_frame("icmp")] + hits(6, 25),
        [L(6), odd_frame("v6"), W(6), odd_frame(37)] + hits(7, 29),
        # 7 flows so far, 9 indices free: 12 new flows, the last three find the
        # table full (still out on WAN), their replies are dropped; a reply to
        # the last flow that fits, before and after it is born
        [L(7), L(8), L(3), L(9), L(10), L(8), W(10), L(11), L(12), W(15), L(13), L(14),
         L(15, dev=2), W(15), L(16), L(17), L(16), L(2), L(18), W(16), W(17)] + hits(16, 43),
    ]
    # the last two bursts: one time each, every flow touched in a scrambled
    # order (the stamps' sequence numbers decide the expiry order afterwards)
    for m in (65, 130):
        b = [L(20), W(20), odd_frame("v6")] + hits(16, m - 3 - 16) + \
            [L(int(k)) for k in rng.permutation(16)]
        bursts.append(b)
    assert [len(b) for b in bursts] == SIZES
    pk = [p for b in bursts for p in b]
    n = len(pk)
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    now = np.zeros(n, np.int64)
    t, at = T.NOW0, 0
    for bi, b in enumerate(bursts):
        for j in range(len(b)):
            if bi < 6 or j == 0:
                t += 3  # strictly increasing / one time for the whole burst
            now[at + j] = t
        at += len(b)
    return F, ln, dv, now


def flow_id(row, reverse=False):
    """A frame's FlowId as Fw.dump() / the oracle's dump hold it (vigfw/flow.h:
    src_port, dst_port, src_ip, dst_ip, protocol, padding), raw wire bytes;
    reverse: the FlowId a WAN packet looks up."""
    sp, dp, sip, dip = row[34:36], row[36:38], row[26:30], row[30:34]
    if reverse:
        sp, dp, sip, dip = dp, sp, dip, sip
    return bytes(sp) + bytes(dp) + bytes(sip) + bytes(dip) + bytes(row[23:24]) + b"\0\0\0"


def live_keys(dump):
    alloc, _, keys, dev = dump
    return {keys[i].tobytes(): int(dev[i]) for i in range(alloc.shape[0]) if alloc[i]}


@pytest.fixture(scope="module")
def order_ref():
    """The trace of (b) through the oracle alone, run once: every burst's
    frames and ports, the state after it, and the batch past the expiry time
    that follows."""
    F, ln, dv, now = build_order_trace()
    o = make_oracle(MAX_FLOWS)
    bounds, a, per = [], 0, []
    for m in SIZES:
        exp = F[a:a + m].reshape(-1).copy()
        out = o.run(exp, ln[a:a + m], dv[a:a + m], now[a:a + m], SLOT)
        per.append(dict(E=exp.reshape(m, SLOT), out=out, dump=o.fw_dump(MAX_FLOWS)))
        bounds.append((a, a + m))
        a += m
    # 24 new flows past the expiry time: all 16 old flows expire at its first
    # packet, oldest stamp first (equal times: by sequence), and the new flows
    # take the freed indices in that order
    m = 24
    F2 = np.stack([lan_frame(100 + k)[0] for k in range(m)]).astype(np.uint8)
    ln2 = np.full(m, 60, np.uint16)
    dv2 = np.zeros(m, np.uint16)
    now2 = now[-1] + EXPIRE_NS + 1 + np.arange(m, dtype=np.int64)
    exp2 = F2.reshape(-1).copy()
    out2 = o.run(exp2, ln2, dv2, now2, SLOT)
    late = dict(F=F2, ln=ln2, dv=dv2, now=now2, E=exp2.reshape(m, SLOT), out=out2,
                dump=o.fw_dump(MAX_FLOWS))
    return dict(F=F, ln=ln, dv=dv, now=now, bounds=bounds, per=per, late=late)


def valid(F, ln, j):
    """nf_then_get_rte_ipv4_header / nf_then_get_tcpudp_header let frame j
    through (the trace's frames have 20-byte IPv4 headers)."""
    return ln[j] >= 38 and F[j, 12] == 8 and F[j, 13] == 0 and F[j, 23] in (6, 17)


def test_trace_preconditions(order_ref):
    """The situations the trace of (b) is built for all occur, read off the
    oracle's results; and nothing in it may fall back to the pipeline."""
    r = order_ref
    F, ln, dv, now = r["F"], r["ln"], r["dv"], r["now"]
    seen = set()
    before = {}
    for (a, b), p in zip(r["bounds"], r["per"]):
        after = live_keys(p["dump"])
        born = set(after) - set(before)
        full = len(after) == MAX_FLOWS
        E, out = p["E"], p["out"]
        lan_at, full_keys = {}, set()  # FlowId -> its LAN packets' (position, device)
        for j in range(a, b):
            i = j - a
            if not valid(F, ln, j):
                assert out[i] == dv[j] and (E[i] == F[j]).all()
                if ln[j] < 60:
                    seen.add("truncated %d" % ln[j])
                elif F[j, 12] != 8:
                    seen.add("not IPv4")
                elif F[j, 23] == 1:
                    seen.add("ICMP")
                continue
            if dv[j] != WAN:
                k = flow_id(F[j])
                assert out[i] == WAN  # (every LAN packet goes out, flow or not)
                lan_at.setdefault(k, []).append((j, int(dv[j])))
                if k not in after:
                    assert full
                    full_keys.add(k)
                    seen.add("LAN packet at table full")
                    if born:
                        seen.add("flows born and table full in one burst")
            else:
                k = flow_id(F[j], reverse=True)
                first = lan_at.get(k, [(b, -1)])[0]
                if out[i] == dv[j]:  # dropped
                    assert (E[i] == F[j]).all()
                    if k in born and first[0] > j:
                        seen.add("reply before its flow is born")
                    if k in full_keys:
                        seen.add("reply to a flow that found the table full")
                elif k in born:
                    assert first[0] < j
                    seen.add("reply after its flow is born")
                    devs = {d for _, d in lan_at[k]}
                    if len(devs) > 1 and out[i] == first[1] == after[k]:
                        seen.add("reply goes to the first of two LAN devices")
        for k in born:
            if len(lan_at.get(k, [])) > 1:
                seen.add("same new 5-tuple twice")
                if len({d for _, d in lan_at[k]}) > 1:
                    seen.add("same new 5-tuple from two LAN devices")
        before = after
    want = {"same new 5-tuple twice", "same new 5-tuple from two LAN devices",
            "reply goes to the first of two LAN devices", "reply after its flow is born",
            "reply before its flow is born", "LAN packet at table full",
            "reply to a flow that found the table full",
            "flows born and table full in one burst", "not IPv4", "truncated 10",
            "truncated 20", "truncated 37", "ICMP"}
    assert want <= seen, want - seen
    assert len(before) == MAX_FLOWS
    # routing: times that never go back, frames the mailbox holds, no IPv4
    # options, and 60 s to the first expiry -- every burst is eligible
    bounds = r["bounds"]
    assert all((np.diff(now[a:b]) > 0).all() for a, b in bounds[:6])
    assert all((np.diff(now[a:b]) == 0).all() for a, b in bounds[6:])
    assert (np.diff(now) >= 0).all() and (ln <= 2048).all()
    assert not ((F[:, 12] == 8) & ((F[:, 14] & 15) > 5)).any()
    assert now[-1] - now[0] < EXPIRE_NS
    assert [b - a for a, b in bounds] == SIZES
    # the batch past the expiry time: every old flow gone, 16 of 24 new ones in
    late = r["late"]
    assert (late["out"] == WAN).all()
    assert not (set(live_keys(late["dump"])) & set(before))
    assert len(live_keys(late["dump"])) == MAX_FLOWS


@pytest.fixture(scope="module")
def order_run(order_ref):
    """The eight bursts on the GPU, run once: every burst against the oracle's
    results as it goes, the counters before, between and after, then the state
    (Fw.dump() stops the resident kernel, so the state is read once, behind
    the last burst: a read after every burst would cost a launch each)."""
    r = order_ref
    fw, _ = make_pair(MAX_FLOWS)
    st0 = fw.serve_stats()
    per_burst = []
    for (a, b), p in zip(r["bounds"], r["per"]):
        send_burst(fw, r["F"], r["ln"], r["dv"], r["now"], a, b, p["E"], p["out"])
        per_burst.append(fw.serve_stats())
    st1 = fw.serve_stats()
    state_equals(fw, r["per"][-1]["dump"])
    return dict(fw=fw, st0=st0, st1=st1, per_burst=per_burst)


@gpu
def test_order_inside_a_burst(order_ref, order_run):
    """(the bursts themselves are checked as order_run makes them) Then the
    batch past the expiry time: the new flows take the freed indices in stamp
    order, so the keys by index show ts / tseq were stamped in packet order."""
    fw, late = order_run["fw"], order_ref["late"]
    st = fw.serve_stats()
    m = late["F"].shape[0]
    send_burst(fw, late["F"], late["ln"], late["dv"], late["now"], 0, m, late["E"], late["out"])
    after = fw.serve_stats()
    assert after["bursts"] == st["bursts"] and after["declined"] == st["declined"]
    state_equals(fw, late["dump"])


@gpu
def test_path_is_taken(order_ref, order_run):
    r = order_run
    n = sum(SIZES)
    assert order_ref["F"].shape[0] == n
    d = {k: r["st1"][k] - r["st0"][k] for k in r["st0"]}
    print("serve stats over the eight bursts:", d)
    assert d["burst_packets"] == n, d
    assert d["bursts"] == sum((m + 63) // 64 for m in SIZES), d
    assert d["declined"] == 0 and d["packets_one"] == 0, d
    # one launch, and one more only where the test stalled past the idle exit
    assert 1 <= d["launches"] <= 2, d
    grew = sum(1 for x, y in zip(r["per_burst"][:-1], r["per_burst"][1:])
               if y["launches"] > x["launches"])
    assert grew <= 1, [s["launches"] for s in r["per_burst"]]


# ------------------------------------------------------ one at a time --
def rows_of(fr, ln, slot=SLOT):
    F = fr.reshape(-1, slot).copy()
    for i in range(F.shape[0]):
        F[i, ln[i]:] = 0
    return F


def one_vs_oracle(fw, o, F, ln, dv, now, i):
    exp = F[i].copy()
    eo = o.run(exp, ln[i:i + 1], dv[i:i + 1], now[i:i + 1], F.shape[1])
    b = bytearray(F[i, :ln[i]].tobytes())
    assert fw.process(int(dv[i]), b, int(now[i])) == eo[0], i
    assert bytes(b) == exp[:ln[i]].tobytes(), i


@gpu
@pytest.mark.parametrize("max_flows,expire_us", [(64, EXPIRE_US), (16, EXPIRE_US), (64, 1)])
def test_process_one_server(max_flows, expire_us):
    """vp_process_one, packet by packet: IPv4 options and malformed frames
    (lane 0's byte-addressed path), a full table, an idle exit in the middle;
    with 1 us expiry packets fall back whenever an expiry is due."""
    rng = np.random.default_rng(11)
    n = 400
    fr, ln, dv, now = mixed_fw_trace(rng, n, 50)
    F = rows_of(fr, ln)
    assert ((F[:, 14] & 15) == 6).any() and (F[:, 12] != 8).any()
    if expire_us == 1:  # (gaps of up to 20 ns: flows do expire along the way)
        now = T.NOW0 + (now - T.NOW0) * 10
        assert now[-1] - now[0] > 2000
    fw, o = make_pair(max_flows, expire_us)
    for i in range(n // 2):
        one_vs_oracle(fw, o, F, ln, dv, now, i)
    s0 = fw.serve_stats()
    time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
    for i in range(n // 2, n):
        one_vs_oracle(fw, o, F, ln, dv, now, i)
    s1 = fw.serve_stats()
    check_state(fw, o, max_flows)
    if expire_us != 1:
        assert s1["packets_one"] == n and s0["packets_one"] == n // 2, (s0, s1)
        assert s1["launches"] >= s0["launches"] + 1, (s0, s1)


@gpu
def test_lengths():
    """Frames of 60 to 1518 bytes, odd lengths among them: only the first 64
    bytes cross to the kernel and only the MACs come back; bytes from offset
    12 on are the input's."""
    rng = np.random.default_rng(1518)
    n, slot, max_flows = 120, 1536, 64
    fl = rng.integers(0, 30, n)
    rep = rng.random(n) < 0.3
    a_ip, b_ip = T.ip4(10, 0, 0, 0) + fl, np.full(n, SERVER_IP)
    a_p, b_p = 1000 + fl, np.full(n, 53)
    fr, _ = T.udp_frames(np.where(rep, b_ip, a_ip), np.where(rep, a_ip, b_ip),
                         np.where(rep, b_p, a_p), np.where(rep, a_p, b_p), slot=slot)
    ln = rng.integers(60, 1519, n).astype(np.uint16)
    ln[:4] = (60, 61, 1517, 1518)
    dv = np.where(rep, WAN, rng.choice([0, 2], n)).astype(np.uint16)
    now = (T.NOW0 + np.cumsum(rng.integers(0, 3, n))).astype(np.int64)
    F = fr.reshape(n, slot).copy()
    F[:, 60:] = rng.integers(0, 256, (n, slot - 60), dtype=np.uint8)  # (payload / padding)
    for i in range(n):
        F[i, ln[i]:] = 0
    assert (ln % 2 == 1).any() and ln.min() == 60 and ln.max() == 1518
    fw, o = make_pair(max_flows)
    st0 = fw.serve_stats()
    a, fwd = 0, 0
    for m in [7, 64, 49]:
        E, out = burst_vs_oracle(fw, o, F, ln, dv, now, a, a + m)
        np.testing.assert_array_equal(E[:, 12:], F[a:a + m, 12:])
        fwd += int((out != dv[a:a + m]).sum())
        a += m
    assert a == n and fwd > n // 2
    d = fw.serve_stats()
    assert d["burst_packets"] - st0["burst_packets"] == n and d["declined"] == 0, d
    check_state(fw, o, max_flows)


def declines(F, ln, a, b):
    """fw_burst hands the request [a, b) back: a frame that parses as IPv4
    with options (the byte-addressed path's)."""
    tl = (F[a:b, 16].astype(int) << 8) | F[a:b, 17]
    unread = ln[a:b].astype(int) - 14
    return bool(((F[a:b, 12] == 8) & (F[a:b, 13] == 0) & (unread >= 20) & (unread >= tl) &
                 ((F[a:b, 14] & 15) > 5)).any())


def plain_fw_trace(seed, n, n_flows):
    """mixed_fw_trace with its IPv4-option frames given 20-byte headers."""
    fr, ln, dv, now = mixed_fw_trace(np.random.default_rng(seed), n, n_flows)
    F = rows_of(fr, ln)
    F[:, 14] = np.where(F[:, 14] == 0x46, 0x45, F[:, 14])
    assert not declines(F, ln, 0, n)
    return F, ln, dv, now


@gpu
def test_fallbacks_same_bytes():
    """A burst the kernel hands back (IPv4 options) and one the host does not
    route (an expiry due in its middle): the pipeline's results, the counters
    saying so."""
    n = 60
    F, ln, dv, now = plain_fw_trace(4, n, 12)
    F[30] = lan_frame(3)[0]
    F[30, 14] = 0x46  # one frame with an option word
    dv[30] = 0
    assert declines(F, ln, 20, 40) and not declines(F, ln, 0, 20) and not declines(F, ln, 40, 60)
    fw, o = make_pair(MAX_FLOWS)
    burst_vs_oracle(fw, o, F, ln, dv, now, 0, 20)
    s0 = fw.serve_stats()
    assert s0["bursts"] == 1 and s0["burst_packets"] == 20 and s0["declined"] == 0, s0
    burst_vs_oracle(fw, o, F, ln, dv, now, 20, 40)
    s1 = fw.serve_stats()
    assert s1["declined"] == 1 and s1["bursts"] == 1 and s1["burst_packets"] == 20, s1
    burst_vs_oracle(fw, o, F, ln, dv, now, 40, 60)
    s2 = fw.serve_stats()
    assert s2["bursts"] == 2 and s2["declined"] == 1, s2
    check_state(fw, o, MAX_FLOWS)
    # expiry of 5 us: ten flows, then twenty new ones 1 us apart -- the first
    # ten expire one after another inside the second burst
    fw, o = make_pair(MAX_FLOWS, expire_us=5)
    m = 30
    G = np.stack([lan_frame(k)[0] for k in range(m)]).astype(np.uint8)
    ln = np.full(m, 60, np.uint16)
    dv = np.zeros(m, np.uint16)
    now = np.concatenate([T.NOW0 + np.arange(10), T.NOW0 + 2000 + 1000 * np.arange(20)]) \
        .astype(np.int64)
    burst_vs_oracle(fw, o, G, ln, dv, now, 0, 10)
    s0 = fw.serve_stats()
    assert s0["bursts"] == 1 and s0["burst_packets"] == 10, s0
    first = live_keys(o.fw_dump(MAX_FLOWS))
    E, out = burst_vs_oracle(fw, o, G, ln, dv, now, 10, 30)
    s1 = fw.serve_stats()
    assert {k: s1[k] for k in ("bursts", "burst_packets", "declined")} == \
        {k: s0[k] for k in ("bursts", "burst_packets", "declined")}, (s0, s1)
    check_state(fw, o, MAX_FLOWS)
    alloc, _, keys, _ = o.fw_dump(MAX_FLOWS)
    assert (out == WAN).all()
    # (indices of expired flows, reused by the second burst's flows)
    assert any(alloc[i] and keys[i].tobytes() not in first for i in range(10))


CHILD = r"""
import json, sys
import numpy as np
import test_fw_serve_gpu as B
from vigor_amd import traces as T
fw, o = B.make_pair(64)
n = 40
F = np.stack([(B.lan_frame(k % 9) if k % 3 else B.wan_frame(k % 9))[0] for k in range(n)]) \
    .astype(np.uint8)
ln = np.full(n, 60, np.uint16)
dv = np.array([0 if k % 3 else 1 for k in range(n)], np.uint16)
now = (T.NOW0 + np.arange(n)).astype(np.int64)
B.burst_vs_oracle(fw, o, F, ln, dv, now, 0, 20)
B.burst_vs_oracle(fw, o, F, ln, dv, now, 20, 40)
B.check_state(fw, o, 64)
print("STATS " + json.dumps(fw.serve_stats()))
"""


@gpu
def test_routing_off_in_child():
    """VIGPATH_SERVE_BURST=0 (read once per process: a fresh child): no
    burst is routed, the results are the pipeline's."""
    env = dict(os.environ, VIGPATH_SERVE_BURST="0")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("STATS ")][-1]
    st = json.loads(line[6:])
    assert st["bursts"] == 0 and st["burst_packets"] == 0 and st["declined"] == 0, st


@gpu
def test_interleaving():
    """Single packets, bursts, a device batch, an idle exit, a burst again,
    single packets: one flow state throughout, and the counters add up."""
    n, max_flows = 260, 64
    F, ln, dv, now = plain_fw_trace(5, n, 50)
    fw, o = make_pair(max_flows)

    def device(a, b):
        exp = F[a:b].reshape(-1).copy()
        eo = o.run(exp, ln[a:b], dv[a:b], now[a:b], SLOT)
        got, out = run_gpu(fw, F[a:b].reshape(-1), ln[a:b], dv[a:b], now[a:b], SLOT)
        np.testing.assert_array_equal(out, eo)
        np.testing.assert_array_equal(got, exp)

    for i in range(0, 10):
        one_vs_oracle(fw, o, F, ln, dv, now, i)
    burst_vs_oracle(fw, o, F, ln, dv, now, 10, 40)
    one_vs_oracle(fw, o, F, ln, dv, now, 40)
    device(41, 141)
    burst_vs_oracle(fw, o, F, ln, dv, now, 141, 171)
    s0 = fw.serve_stats()
    time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
    burst_vs_oracle(fw, o, F, ln, dv, now, 171, 241)
    for i in range(241, n):
        one_vs_oracle(fw, o, F, ln, dv, now, i)
    s1 = fw.serve_stats()
    assert s1["launches"] >= s0["launches"] + 1, (s0, s1)  # (launched again after the idle exit)
    assert s1["burst_packets"] == 30 + 30 + 70 and s1["bursts"] == 1 + 1 + 2, s1
    assert s1["packets_one"] == 11 + n - 241 and s1["declined"] == 0, s1
    check_state(fw, o, max_flows)


@gpu
def test_nat_and_fw_share_a_gpu():
    """A vignat and a vigfw context on one GPU, each with a resident kernel,
    taking turns: the launch of one yields the other's (serve_yield), so both
    make progress; each against its own oracle."""
    import test_serve_burst_gpu as N
    nat, no = N.make_pair(64)
    fw, fo = make_pair(64)
    m = 40
    NF = np.stack([(N.lan_frame(k % 7) if k % 4 else N.wan_frame(k % 7, k % 7))[0]
                   for k in range(2 * m)]).astype(np.uint8)
    ndv = np.array([0 if k % 4 else 1 for k in range(2 * m)], np.uint16)
    FF = np.stack([(lan_frame(k % 7) if k % 4 else wan_frame(k % 7))[0]
                   for k in range(2 * m)]).astype(np.uint8)
    fdv = np.array([0 if k % 4 else WAN for k in range(2 * m)], np.uint16)
    ln = np.full(2 * m, 60, np.uint16)
    now = (T.NOW0 + 5 * np.arange(2 * m)).astype(np.int64)
    for i in range(m):
        one_vs_oracle(nat, no, NF, ln, ndv, now, i)
        one_vs_oracle(fw, fo, FF, ln, fdv, now, i)
    N.burst_vs_oracle(nat, no, NF, ln, ndv, now, m, 2 * m)
    burst_vs_oracle(fw, fo, FF, ln, fdv, now, m, 2 * m)
    N.check_state(nat, no, 64)
    check_state(fw, fo, 64)
    sn, sf = nat.serve_stats(), fw.serve_stats()
    assert sn["packets_one"] == m and sf["packets_one"] == m, (sn, sf)
    assert sn["burst_packets"] == m and sf["burst_packets"] == m, (sn, sf)
