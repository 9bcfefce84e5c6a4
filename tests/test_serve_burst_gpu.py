"""Small vignat host bursts (vp_process_batch / vp_process_mbufs, nf.c's
VIGOR_BATCH_SIZE loop) served by the resident kernel as burst requests, one
lane of a wave per packet: out ports, every frame byte and the flow state
against the CPU oracle, and vp_serve_stats_get showing which path ran.

Each frame is its own buffer of len bytes (as an mbuf's data), so the oracle's
frames are zeroed past len.
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
from tracegen import mixed_nat_trace, wide_nat_trace
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01")]
EXT_IP = T.ip4(192, 168, 4, 2)
SERVER_IP = T.ip4(8, 8, 8, 8)
SLOT = 64
SIZES = [1, 2, 31, 32, 33, 64, 65, 130]
MAX_FLOWS = 16
# (60 s; expiration_time * 1000 in 32 bits, nat_flowmanager.c:57-65: 4.17 s)
EXPIRE_NS = (60_000_000 * 1000) % (1 << 32)


def make_pair(max_flows, expire_us=60_000_000):
    args = ["--wan", "1", "--expire", str(expire_us), "--starting-port", "0",
            "--max-flows", str(max_flows), "--extip", "192.168.4.2"]
    for d in range(2):
        args += ["--eth-dest", "%d,%s" % (d, END_MACS[d].hex(":"))]
    cfg = vigor_amd.nat_config_from_args(args, 2, DEV_MACS)
    ocfg = orc.nat_cfg(wan=1, start_port=0, ext_ip=EXT_IP, expire_us=expire_us,
                       max_flows=max_flows, device_macs=DEV_MACS,
                       endpoint_macs=END_MACS, n_devices=2)
    return vigor_amd.Nat(cfg, gpu=0), orc.Oracle("nat", ocfg)


def check_state(nat, oracle, max_flows):
    ga, gts, gk = nat.dump()
    oa, ots, ok = oracle.nat_dump(max_flows)
    np.testing.assert_array_equal(ga, oa)
    np.testing.assert_array_equal(gts[oa == 1], ots[oa == 1])
    np.testing.assert_array_equal(gk[oa == 1], ok[oa == 1])


def burst_vs_oracle(nat, oracle, F, ln, dv, now, a, b):
    """Packets [a, b) of the trace (F: n x slot, zero past len) as one
    vp_process_batch call; out ports and every byte against the oracle run
    over the same packets. Returns the oracle's (frames, out ports)."""
    slot = F.shape[1]
    exp = F[a:b].reshape(-1).copy()
    exp_out = oracle.run(exp, ln[a:b], dv[a:b], now[a:b], slot)
    E = exp.reshape(b - a, slot)
    bufs = [bytearray(F[j, :ln[j]].tobytes()) for j in range(a, b)]
    out = nat.process_mbufs(bufs, dv[a:b], now[a:b])
    np.testing.assert_array_equal(out, exp_out, "out ports, burst [%d, %d)" % (a, b))
    for j in range(b - a):
        assert bytes(bufs[j]) == E[j, :ln[a + j]].tobytes(), "frame %d" % (a + j)
    return E, exp_out


# ------------------------------------------------ the hand-built trace --
def proto_of(k):
    return 6 if k % 2 == 0 else 17


def lan_frame(k):
    """LAN flow k: 10.0.0.k:1000+k -> 8.8.8.8:53."""
    f, _ = T.udp_frames(np.array([T.ip4(10, 0, 0, 0) + k]), np.array([SERVER_IP]),
                        np.array([1000 + k]), np.array([53]), slot=SLOT, proto=proto_of(k))
    return f.copy(), 60, 0


def wan_frame(idx, k, spoof=False):
    """The server's reply to flow k, which holds external port idx (start
    port 0: the port on the wire is the index, raw LE); spoof: from another
    address."""
    src = SERVER_IP + (1 if spoof else 0)
    f, _ = T.udp_frames(np.array([src]), np.array([EXT_IP]), np.array([53]), np.array([0]),
                        slot=SLOT, proto=proto_of(k))
    f = f.copy()
    f[36], f[37] = idx & 0xFF, idx >> 8
    return f, 60, 1


def odd_frame(kind):
    f, ln, dv = lan_frame(0)
    if kind == "v6":
        f[12:14] = (0x86, 0xDD)
    else:  # truncated: kind = its length
        ln = kind
        f[ln:] = 0
    return f, ln, dv


def build_order_trace():
    """The bursts of test 1 (SIZES). Flow k first appears k-th, so it takes
    index k while indices are free (no expiry is due: 60 s)."""
    rng = np.random.default_rng(0xB0057)
    L, W, S = lan_frame, wan_frame, lambda i: wan_frame(i, i, spoof=True)

    def hits(known, m):  # packets of flows that exist: LAN hits and replies
        out = []
        for k in rng.integers(0, known, m):
            out.append(L(int(k)) if rng.random() < 0.6 else W(int(k), int(k)))
        return out

    bursts = [
        [L(0)],
        [L(1), L(1)],  # the same new 5-tuple on two lanes
        # a reply to a flow born earlier in the burst (2), one to a port whose
        # flow is born later in it (3: dropped), a spoofed reply, odd frames
        [L(2), W(2, 2), W(3, 3), L(3), S(0), odd_frame("v6"), odd_frame(20), odd_frame(10),
         odd_frame(37), W(3, 3)] + hits(4, 21),
        [L(4), L(4), W(5, 5), L(5), W(5, 5), W(4, 4), S(4)] + hits(6, 25),
        [L(6), odd_frame("v6"), S(2), W(6, 6)] + hits(7, 29),
        # 7 flows so far, 9 indices free: 12 new flows, the last three dropped
        # (table full), their repeats too; a reply to the last flow that fits
        [L(7), L(8), L(3), L(9), L(10), L(8), W(10, 10), L(11), L(12), W(15, 15), L(13),
         L(14), L(15), W(15, 15), L(16), L(17), L(16), L(2), L(18), W(16, 16), S(15)]
        + hits(16, 43),
    ]
    # the last two bursts: one time each, every flow touched in a scrambled
    # order (the stamps' sequence numbers decide the expiry order afterwards)
    for m in (65, 130):
        b = [L(20), S(7), odd_frame("v6")] + hits(16, m - 3 - 16) + \
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


def lan_key(F, j):
    return F[j, 23:24].tobytes() + F[j, 26:38].tobytes()


def wire_port(row):
    return int(row[36]) | (int(row[37]) << 8)


def cases_seen(F, ln, dv, E, out, bounds):
    """Which of the listed situations the oracle's run went through, from its
    results alone. E / out: the oracle's frames and ports of the whole trace."""
    seen = set()
    flows, alloc = {}, set()  # LAN key -> index; the indices allocated
    for a, b in bounds:
        born = {}  # index -> position, flows born in this burst
        wan_drops = []
        for j in range(a, b):
            valid = ln[j] == 60 and F[j, 12] == 8
            if not valid:
                seen.add("not IPv4" if ln[j] == 60 else "truncated")
                assert out[j] == dv[j]
                continue
            if dv[j] == 0:
                k = lan_key(F, j)
                if out[j] == dv[j]:
                    assert len(alloc) == MAX_FLOWS and k not in flows
                    seen.add("table-full drop")
                    if born:
                        seen.add("flows born and dropped in one burst")
                    continue
                idx = int(E[j, 34]) | (int(E[j, 35]) << 8)
                if k not in flows:
                    flows[k] = idx
                    alloc.add(idx)
                    born[idx] = j
                elif born.get(idx, j) < j and flows[k] == idx:
                    seen.add("same new 5-tuple twice in a burst")
            else:
                p = wire_port(F[j])
                if out[j] != dv[j]:
                    if p in born:
                        seen.add("reply to a flow born earlier in the burst")
                elif p in alloc:
                    seen.add("spoofed reply")
                else:
                    wan_drops.append(p)
        if any(p in born for p in wan_drops):
            seen.add("reply before its flow is born in the burst")
    return seen, len(alloc)


@pytest.fixture(scope="module")
def order_run():
    """Test 1's bursts, run once: every burst against the oracle as it goes,
    the counters before and after, then the state and the expiry batch."""
    F, ln, dv, now = build_order_trace()
    n = F.shape[0]
    nat, o = make_pair(MAX_FLOWS)
    st0 = nat.serve_stats()
    bounds, a = [], 0
    E = np.zeros_like(F)
    out = np.zeros(n, np.uint16)
    per_burst = []
    for m in SIZES:
        E[a:a + m], out[a:a + m] = burst_vs_oracle(nat, o, F, ln, dv, now, a, a + m)
        per_burst.append(nat.serve_stats())
        bounds.append((a, a + m))
        a += m
    st1 = nat.serve_stats()
    return dict(nat=nat, o=o, F=F, ln=ln, dv=dv, now=now, E=E, out=out, bounds=bounds,
                st0=st0, st1=st1, per_burst=per_burst)


def test_order_inside_a_burst(order_run):
    r = order_run
    seen, live = cases_seen(r["F"], r["ln"], r["dv"], r["E"], r["out"], r["bounds"])
    want = {"same new 5-tuple twice in a burst", "reply to a flow born earlier in the burst",
            "reply before its flow is born in the burst", "spoofed reply", "table-full drop",
            "flows born and dropped in one burst", "not IPv4", "truncated"}
    assert want <= seen, want - seen
    assert live == MAX_FLOWS
    now, bounds = r["now"], r["bounds"]
    assert all((np.diff(now[a:b]) > 0).all() for a, b in bounds[:6])
    assert all((np.diff(now[a:b]) == 0).all() for a, b in bounds[6:])
    nat, o = r["nat"], r["o"]
    check_state(nat, o, MAX_FLOWS)
    # every flow expires at the next batch's first packet, oldest stamp first
    # (equal times: by sequence), and its new flows take the freed indices in
    # that order: the ports show whether ts / tseq were stamped in packet order
    m = 24
    fr = np.stack([lan_frame(100 + k)[0] for k in range(m)]).astype(np.uint8)
    ln2 = np.full(m, 60, np.uint16)
    dv2 = np.zeros(m, np.uint16)
    now2 = now[-1] + EXPIRE_NS + 1 + np.arange(m, dtype=np.int64)
    st = nat.serve_stats()
    E2, out2 = burst_vs_oracle(nat, o, fr, ln2, dv2, now2, 0, m)
    assert (out2[:MAX_FLOWS] == 1).all() and (out2[MAX_FLOWS:] == 0).all()  # all 16 were freed
    after = nat.serve_stats()
    assert after["bursts"] == st["bursts"] and after["declined"] == st["declined"]
    check_state(nat, o, MAX_FLOWS)


def test_path_is_taken(order_run):
    r = order_run
    n = r["F"].shape[0]
    # nothing in the trace may fall back: frames of at most 60 bytes, no IPv4
    # options, times that never go back, 60 s to the first expiry
    eligible = sum(b - a for a, b in r["bounds"]
                   if (np.diff(r["now"][a:b]) >= 0).all() and (r["ln"][a:b] <= 2048).all()
                   and not ((r["F"][a:b, 12] == 8) & ((r["F"][a:b, 14] & 15) > 5)).any())
    assert eligible == n == sum(SIZES)
    d = {k: r["st1"][k] - r["st0"][k] for k in r["st0"]}
    print("serve stats over test 1's bursts:", d)
    assert d["burst_packets"] >= 3 * n / 4, d
    assert d["burst_packets"] == eligible, d
    assert d["bursts"] == sum((m + 63) // 64 for m in SIZES), d
    assert d["declined"] == 0 and d["packets_one"] == 0, d
    # one launch, and one more only where the test stalled past the idle exit
    assert 1 <= d["launches"] <= 2, d
    grew = sum(1 for x, y in zip(r["per_burst"][:-1], r["per_burst"][1:])
               if y["launches"] > x["launches"])
    assert grew <= 1, [s["launches"] for s in r["per_burst"]]


def test_lengths():
    """Frames of 60 to 1518 bytes, odd lengths, some padded past
    total_length: the L4 sum's bytes past 64 come from the mailbox; bytes
    past 64 come back untouched."""
    rng = np.random.default_rng(1518)
    n, slot, max_flows = 300, 1536, 64
    fr, ln, dv, now = wide_nat_trace(rng, n, 40, slot, bad_frac=0.0)
    F = fr.reshape(n, slot).copy()
    for i in range(n):
        F[i, ln[i]:] = 0
    assert (ln % 2 == 1).any() and ln.min() < 100 and ln.max() > 1400
    tl = (F[:, 16].astype(int) << 8) | F[:, 17]
    assert (tl + 14 < ln).any()
    nat, o = make_pair(max_flows)
    st0 = nat.serve_stats()
    a = 0
    fwd = 0
    for m in [7, 64, 33, 100, 96]:
        E, out = burst_vs_oracle(nat, o, F, ln, dv, now, a, a + m)
        np.testing.assert_array_equal(E[:, 64:], F[a:a + m, 64:])
        fwd += int((out != dv[a:a + m]).sum())
        a += m
    assert a == n and fwd > n // 2
    d = nat.serve_stats()
    assert d["burst_packets"] - st0["burst_packets"] == n and d["declined"] == 0, d
    check_state(nat, o, max_flows)


def test_fallbacks_same_bytes():
    """A burst the kernel hands back (IPv4 options) and one the host does not
    route (an expiry due in its middle): the pipeline's results, the counters
    saying so."""
    rng = np.random.default_rng(4)
    n = 60
    fr, ln, dv, now = mixed_nat_trace(rng, n, 12, max_idx=16)
    F = fr.reshape(n, SLOT).copy()
    F[:, 14] = np.where(F[:, 14] == 0x44, 0x45, F[:, 14])
    F[30, 14] = 0x46  # one frame with an option word: the byte-addressed path
    F[30, 12:14] = (8, 0)
    F[30, 16:18] = (0, 46)
    nat, o = make_pair(MAX_FLOWS)
    burst_vs_oracle(nat, o, F, ln, dv, now, 0, 20)
    s0 = nat.serve_stats()
    assert s0["bursts"] == 1 and s0["burst_packets"] == 20 and s0["declined"] == 0, s0
    burst_vs_oracle(nat, o, F, ln, dv, now, 20, 40)
    s1 = nat.serve_stats()
    assert s1["declined"] == 1 and s1["bursts"] == 1 and s1["burst_packets"] == 20, s1
    burst_vs_oracle(nat, o, F, ln, dv, now, 40, 60)
    s2 = nat.serve_stats()
    assert s2["bursts"] == 2 and s2["declined"] == 1, s2
    check_state(nat, o, MAX_FLOWS)
    # expiry of 5 us: ten flows, then twenty new ones 1 us apart -- the first
    # ten expire one after another inside the second burst
    nat, o = make_pair(MAX_FLOWS, expire_us=5)
    m = 30
    G = np.stack([lan_frame(k)[0] for k in range(m)]).astype(np.uint8)
    ln = np.full(m, 60, np.uint16)
    dv = np.zeros(m, np.uint16)
    now = np.concatenate([T.NOW0 + np.arange(10), T.NOW0 + 2000 + 1000 * np.arange(20)]) \
        .astype(np.int64)
    burst_vs_oracle(nat, o, G, ln, dv, now, 0, 10)
    s0 = nat.serve_stats()
    assert s0["bursts"] == 1 and s0["burst_packets"] == 10, s0
    E, out = burst_vs_oracle(nat, o, G, ln, dv, now, 10, 30)
    ports = E[:, 34].astype(int) | (E[:, 35].astype(int) << 8)
    assert (out == 1).all() and (ports < 10).any()  # (indices of expired flows, reused)
    s1 = nat.serve_stats()
    assert {k: s1[k] for k in ("bursts", "burst_packets", "declined")} == \
        {k: s0[k] for k in ("bursts", "burst_packets", "declined")}, (s0, s1)
    check_state(nat, o, MAX_FLOWS)


CHILD = r"""
import json, sys
import numpy as np
import test_serve_burst_gpu as B
from vigor_amd import traces as T
nat, o = B.make_pair(64)
n = 40
F = np.stack([B.lan_frame(k % 9)[0] for k in range(n)]).astype(np.uint8)
ln = np.full(n, 60, np.uint16)
dv = np.zeros(n, np.uint16)
now = (T.NOW0 + np.arange(n)).astype(np.int64)
B.burst_vs_oracle(nat, o, F, ln, dv, now, 0, 20)
B.burst_vs_oracle(nat, o, F, ln, dv, now, 20, 40)
B.check_state(nat, o, 64)
print("STATS " + json.dumps(nat.serve_stats()))
"""


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


def test_interleaving():
    """One packet, a burst, a device batch, an idle exit, a burst again: one
    flow state throughout."""
    rng = np.random.default_rng(5)
    n, max_flows = 260, 64
    fr, ln, dv, now = mixed_nat_trace(rng, n, 50, max_idx=max_flows)
    F = fr.reshape(n, SLOT).copy()
    for i in range(n):
        F[i, ln[i]:] = 0
    nat, o = make_pair(max_flows)

    def one(i):
        exp = F[i].copy()
        eo = o.run(exp, ln[i:i + 1], dv[i:i + 1], now[i:i + 1], SLOT)
        b = bytearray(F[i, :ln[i]].tobytes())
        assert nat.process(int(dv[i]), b, int(now[i])) == eo[0], i
        assert bytes(b) == exp[:ln[i]].tobytes(), i

    def device(a, b):
        exp = F[a:b].reshape(-1).copy()
        eo = o.run(exp, ln[a:b], dv[a:b], now[a:b], SLOT)
        got, out = run_gpu(nat, F[a:b].reshape(-1), ln[a:b], dv[a:b], now[a:b], SLOT)
        np.testing.assert_array_equal(out, eo)
        np.testing.assert_array_equal(got, exp)

    for i in range(0, 10):
        one(i)
    burst_vs_oracle(nat, o, F, ln, dv, now, 10, 40)
    one(40)
    device(41, 141)
    burst_vs_oracle(nat, o, F, ln, dv, now, 141, 171)
    s0 = nat.serve_stats()
    time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
    burst_vs_oracle(nat, o, F, ln, dv, now, 171, 241)
    for i in range(241, n):
        one(i)
    s1 = nat.serve_stats()
    assert s1["launches"] >= s0["launches"] + 1, (s0, s1)  # (launched again after the idle exit)
    assert s1["burst_packets"] == 30 + 30 + 70 and s1["packets_one"] == 11 + n - 241, s1
    assert s1["declined"] == 0, s1
    check_state(nat, o, max_flows)
