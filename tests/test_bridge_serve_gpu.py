"""vigbridge's per-packet and small-burst calls (vp_process_one, small
vp_process_batch / vp_process_mbufs calls: nf.c's two loops) served by the
resident kernel bridge_serve: out ports, every frame byte (the bridge changes
none) and the dynamic table (Bridge.dump: alloc, ts, MACs, learned ports)
against the CPU oracle, and vp_serve_stats_get showing which path ran.

Each frame is its own buffer of len bytes (as an mbuf's data), so the oracle's
frames are zeroed past len: a runt's missing MAC bytes read as 0. Reference
behaviour: vigbridge/bridge_main.c:38-89, 311-329.
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
from test_bridge_gpu import STATICS
from tracegen import mixed_bridge_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 64
N_DEV = 3
FLOOD = 0xFFFF
SIZES = [1, 2, 31, 32, 33, 64, 65, 130]
CAP = 16
EXPIRE_US = 60_000_000
BCAST = "bcast"


def expire_ns(expire_us):
    """expiration_time * 1000 wraps in 32 bits (bridge_main.c:29-36), so 60 s
    is about 4.17 s."""
    return (expire_us * 1000) & 0xFFFFFFFF


EXPIRE_NS = expire_ns(EXPIRE_US)


def make_oracle(cap, expire_us=EXPIRE_US, statics=STATICS):
    ocfg = orc.BridgeCfg(expiration_time=expire_us, dyn_capacity=cap, n_devices=N_DEV)
    return orc.Oracle("bridge", ocfg, statics=list(statics))


def make_pair(cap, expire_us=EXPIRE_US, statics=STATICS):
    """Three devices and test_bridge_gpu's static rules."""
    args = ["--expire", str(expire_us), "--capacity", str(cap)]
    cfg = vigor_amd.bridge_config_from_args(args, N_DEV, list(statics))
    return vigor_amd.Bridge(cfg, gpu=0), make_oracle(cap, expire_us, statics)


def state_equals(br, dump):
    """Bridge.dump() against an oracle dump (alloc, ts, MACs, ports)."""
    ga, gts, gm, gp = br.dump()
    oa, ots, om, op = dump
    np.testing.assert_array_equal(ga, oa)
    live = oa == 1
    np.testing.assert_array_equal(gts[live], ots[live])
    np.testing.assert_array_equal(gm[live], om[live])
    np.testing.assert_array_equal(gp[live], op[live])


def check_state(br, oracle, cap):
    state_equals(br, oracle.bridge_dump(cap))


def send_burst(br, F, ln, dv, now, a, b, exp_out):
    """Packets [a, b) of the trace (F: n x slot, zero past len) as one
    vp_process_batch call, each frame its own buffer of len bytes; out ports
    against the oracle's and every byte against the input (never changed)."""
    bufs = [bytearray(F[j, :ln[j]].tobytes()) for j in range(a, b)]
    out = br.process_mbufs(bufs, dv[a:b], now[a:b])
    np.testing.assert_array_equal(out, exp_out, "out ports, burst [%d, %d)" % (a, b))
    for j in range(b - a):
        assert bytes(bufs[j]) == F[a + j, :ln[a + j]].tobytes(), "frame %d" % (a + j)


def burst_vs_oracle(br, oracle, F, ln, dv, now, a, b):
    """send_burst against the oracle run over the same packets. Returns the
    oracle's out ports."""
    slot = F.shape[1]
    exp = F[a:b].reshape(-1).copy()
    exp_out = oracle.run(exp, ln[a:b], dv[a:b], now[a:b], slot)
    np.testing.assert_array_equal(exp, F[a:b].reshape(-1))  # (the bridge rewrites nothing)
    send_burst(br, F, ln, dv, now, a, b, exp_out)
    return exp_out


# ------------------------------------------------ the hand-built trace --
def mac_of(k):
    """Station k: 02:00:00:00:hh:ll (7, 9 and 11 are the static rules' MACs)."""
    if k == BCAST:
        return bytes([0xFF] * 6)
    return bytes([2, 0, 0, 0, (k >> 8) & 0xFF, k & 0xFF])


ZERO = bytes(6)  # (what a runt's missing src reads as)


def fr(src, dst, dev, ln=60):
    """A frame from station src to station dst arriving on port dev, ln bytes
    long (zero past ln)."""
    f = np.zeros(SLOT, np.uint8)
    f[0:6] = list(mac_of(dst))
    f[6:12] = list(mac_of(src))
    f[12:14] = (0x08, 0x00)
    f[14:] = (np.arange(SLOT - 14) * 7 + src) & 0xFF
    f[ln:] = 0
    return f, ln, dev


def src_mac(row):
    return bytes(row[6:12])


def dst_mac(row):
    return bytes(row[0:6])


# the stations that end up in the table, in learning order; 19, 20 and 21 come
# when it is full
LEARNED = [1, 3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 15, 16, 17, 18]  # + the zero MAC
FULL = [19, 20, 21]


def build_order_trace():
    """The eight bursts (SIZES). No expiry is due anywhere."""
    rng = np.random.default_rng(0xB21D)

    def hits(known, m):  # frames between stations the table already holds
        out = []
        for _ in range(m):
            s, d = rng.choice(known, 2)
            out.append(fr(int(s), int(d), int(rng.integers(0, N_DEV))))
        return out

    bursts = [
        [fr(1, 2, 0)],  # 1 learned on port 0, 2 unknown: flooded
        # the same new src on two lanes from two ports: the first port is learned
        [fr(3, 1, 1), fr(3, 1, 2)],
        [fr(1, 3, 2),            # a known MAC on another port: stamped, port kept
         fr(3, 1, 0),            # (goes to port 0 still)
         fr(4, 1, 2), fr(1, 4, 0),   # to a MAC an earlier lane learned: forwarded
         fr(1, 5, 0), fr(5, 1, 1),   # to a MAC a later lane learns: flooded
         fr(6, 6, 1),            # to its own new src, an index free: forwarded
         fr(1, 7, 0),            # static forward
         fr(1, 9, 1),            # static filter, and the duplicate key's first rule
         fr(1, 11, 2),           # static explicit flood
         fr(7, 1, 1),            # 7 learned on port 1 ...
         fr(1, 7, 0),            # ... the static rule {7, from 0} still wins
         fr(1, 7, 2),            # ... no rule from port 2: the dynamic entry
         fr(1, BCAST, 0),        # broadcast with a static rule
         fr(1, BCAST, 2),        # broadcast without one: flooded
         fr(1, 3, 0, ln=13),     # runts: both MACs whole,
         fr(1, 3, 1, ln=6),      # the src reads as zero (and is learned),
         fr(1, 3, 2, ln=0),      # both do (to the zero MAC just learned)
         ] + hits([1, 3, 4, 5, 6, 7], 13),
        [fr(8, 8, 2), fr(3, 10, 0), fr(10, 8, 1), fr(1, 9, 1), fr(4, 11, 2), fr(5, 3, 1, ln=6),
         fr(5, 7, 0), fr(6, BCAST, 0)] + hits([1, 3, 4, 5, 6, 7, 8, 10], 24),
        [fr(4, 12, 0), fr(12, 4, 2), fr(12, 12, 0), fr(1, 3, 0, ln=13), fr(3, 7, 0)] +
        hits([1, 3, 4, 5, 6, 7, 8, 10, 12], 28),
        # ten entries so far, six indices free: 13 .. 18 fill the table inside
        # the burst; 19, 20 and 21 find no index, nothing is learned and frames
        # to them flood, a frame to its own src among them
        [fr(13, 1, 0), fr(1, 18, 1), fr(14, 13, 1), fr(15, 14, 2), fr(13, 15, 0), fr(16, 16, 1),
         fr(17, 3, 2), fr(1, 18, 0), fr(18, 17, 0), fr(1, 18, 2), fr(19, 1, 1), fr(1, 19, 0),
         fr(20, 19, 2), fr(21, 21, 0), fr(19, 20, 1), fr(3, 21, 2), fr(1, 7, 0), fr(1, 9, 1)] +
        hits(LEARNED, 46),
    ]
    # the last two bursts: one time each, every entry's src in a scrambled
    # order (the stamps' sequence numbers decide the expiry order afterwards)
    for m in (65, 130):
        b = [fr(19, 3, 1), fr(3, 19, 0), fr(1, 11, 2)] + hits(LEARNED, m - 3 - 16)
        tail = [fr(int(k), int(rng.choice(LEARNED)), int(rng.integers(0, N_DEV)))
                for k in LEARNED] + [fr(1, 3, 1, ln=6)]  # (the zero MAC's stamp)
        b += [tail[i] for i in rng.permutation(16)]
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


def live_macs(dump):
    """{MAC: (index, port)} of an oracle dump."""
    alloc, _, macs, port = dump
    return {macs[i].tobytes(): (i, int(port[i])) for i in range(alloc.shape[0]) if alloc[i]}


STATIC_FIRST = {}
for _m, _f, _t in STATICS:
    STATIC_FIRST.setdefault((_m, _f), _t)


@pytest.fixture(scope="module")
def order_ref():
    """The trace through the oracle alone, run once: every burst's ports, the
    state after it, and the batch past the expiry time that follows."""
    F, ln, dv, now = build_order_trace()
    o = make_oracle(CAP)
    bounds, a, per = [], 0, []
    for m in SIZES:
        exp = F[a:a + m].reshape(-1).copy()
        out = o.run(exp, ln[a:a + m], dv[a:a + m], now[a:a + m], SLOT)
        assert (exp == F[a:a + m].reshape(-1)).all()
        per.append(dict(out=out, dump=o.bridge_dump(CAP)))
        bounds.append((a, a + m))
        a += m
    # 24 new MACs past the expiry time: all 16 entries expire at its first
    # packet, oldest stamp first (equal times: by sequence), and the new MACs
    # take the freed indices
    m = 24
    F2 = np.stack([fr(100 + k, 1, k % N_DEV)[0] for k in range(m)]).astype(np.uint8)
    ln2 = np.full(m, 60, np.uint16)
    dv2 = (np.arange(m) % N_DEV).astype(np.uint16)
    now2 = now[-1] + EXPIRE_NS + 1 + np.arange(m, dtype=np.int64)
    exp2 = F2.reshape(-1).copy()
    out2 = o.run(exp2, ln2, dv2, now2, SLOT)
    late = dict(F=F2, ln=ln2, dv=dv2, now=now2, out=out2, dump=o.bridge_dump(CAP))
    return dict(F=F, ln=ln, dv=dv, now=now, bounds=bounds, per=per, late=late)


def test_trace_preconditions(order_ref):
    """The situations the trace is built for all occur, read off the oracle's
    results; and nothing in it may fall back to the pipeline."""
    r = order_ref
    F, ln, dv, now = r["F"], r["ln"], r["dv"], r["now"]
    seen = set()
    before = {}
    unlearned = set()  # srcs that found the table full
    last_src = {}      # MAC -> the last packet that stamped it
    for (a, b), p in zip(r["bounds"], r["per"]):
        after = live_macs(p["dump"])
        assert set(before) <= set(after)  # (nothing expires)
        born = set(after) - set(before)
        out = p["out"]
        first_at = {}  # MAC -> its first packet as a src in this burst (position, port)
        for j in range(a, b):
            i, s, d, dev = j - a, src_mac(F[j]), dst_mac(F[j]), int(dv[j])
            if ln[j] < 14:
                seen.add("runt %d" % ln[j])
                assert s == (ZERO if ln[j] < 12 else s) and (ln[j] or d == ZERO)
            first_at.setdefault(s, (j, dev))
            if s in after:
                last_src[s] = j
            # the learn
            if s in before and before[s][1] != dev:
                assert after[s] == before[s]
                seen.add("known MAC on another port: port kept")
            if s in born and first_at[s][0] < j and first_at[s][1] != dev:
                assert after[s][1] == first_at[s][1]
                seen.add("same new src from two ports: the first is learned")
            if s not in after:
                assert len(after) == CAP
                unlearned.add(s)
                seen.add("new src, no free index")
                if born:
                    seen.add("MACs learned and the table filling in one burst")
            # the lookup
            rule = STATIC_FIRST.get((d, dev))
            if rule is not None:
                want = {-1: FLOOD, -2: dev}.get(rule, rule)
                assert out[i] == want, (j, out[i], want)
                seen.add({-1: "static flood", -2: "static filter"}.get(rule, "static forward"))
                if rule == -2 and sum(1 for m_, f_, _ in STATICS if (m_, f_) == (d, dev)) > 1:
                    seen.add("duplicate static key: the first rule")
                if d in after and first_at.get(d, (b,))[0] <= j and after[d][1] != want:
                    seen.add("static rule wins over the dynamic entry")
                if d == mac_of(BCAST):
                    seen.add("broadcast, static")
                continue
            if d == mac_of(BCAST):
                assert out[i] == FLOOD
                seen.add("broadcast, flooded")
            known = d in before or (d in born and first_at.get(d, (b,))[0] <= j)
            assert out[i] == (after[d][1] if known else FLOOD), (j, out[i])
            if d in born and known and first_at[d][0] < j:
                seen.add("to a MAC an earlier lane learned: forwarded")
            if d in born and not known:
                seen.add("to a MAC a later lane learns: flooded")
            if d == s and d in born and first_at[d][0] == j:
                seen.add("to its own new src, index free: forwarded")
            if d == s and d not in after:
                seen.add("to its own new src, table full: flooded")
            if d in unlearned and d != s:
                seen.add("to a MAC that found the table full: flooded")
            if d in after and any(m_ == d for m_, _, _ in STATICS) and known:
                seen.add("static MAC, no rule for this port: the dynamic entry")
        before = after
    want = {"known MAC on another port: port kept",
            "same new src from two ports: the first is learned", "new src, no free index",
            "MACs learned and the table filling in one burst",
            "to a MAC an earlier lane learned: forwarded", "to a MAC a later lane learns: flooded",
            "to its own new src, index free: forwarded", "to its own new src, table full: flooded",
            "to a MAC that found the table full: flooded", "static forward", "static filter",
            "static flood", "duplicate static key: the first rule",
            "static rule wins over the dynamic entry",
            "static MAC, no rule for this port: the dynamic entry", "broadcast, static",
            "broadcast, flooded", "runt 0", "runt 6", "runt 13"}
    assert want <= seen, want - seen
    assert set(before) == {mac_of(k) for k in LEARNED} | {ZERO} and len(before) == CAP
    assert unlearned == {mac_of(k) for k in FULL}
    # routing: times that never go back, frames the mailbox holds, and the
    # whole trace well inside the expiry time -- every burst is eligible
    bounds = r["bounds"]
    assert all((np.diff(now[a:b]) > 0).all() for a, b in bounds[:6])
    assert all((np.diff(now[a:b]) == 0).all() for a, b in bounds[6:])
    assert (np.diff(now) >= 0).all() and (ln <= 2048).all()
    assert now[-1] - now[0] < EXPIRE_NS
    assert [b - a for a, b in bounds] == SIZES
    # bursts 7 and 8 stamp every entry, burst 8 last and at one time: the
    # order of its stamps is the order of the packets alone
    a8 = bounds[-1][0]
    assert all(j >= a8 for j in last_src.values()) and len(last_src) == CAP
    # the batch past the expiry time: every old entry gone, 16 of 24 new MACs
    # in. The entries expire oldest stamp first and each freed index goes on
    # top of the free stack (dchain_expire_one_index / dchain_free_index), so
    # new MAC k takes the index whose last stamp is the k-th youngest
    late = r["late"]
    lm = live_macs(late["dump"])
    assert not (set(lm) & set(before)) and len(lm) == CAP
    assert (late["out"] == FLOOD).all()  # (to station 1, expired by then)
    by_age = sorted(last_src, key=lambda m_: last_src[m_])
    for k in range(CAP):
        assert lm[mac_of(100 + k)][0] == before[by_age[CAP - 1 - k]][0], k


@pytest.fixture(scope="module")
def order_run(order_ref):
    """The eight bursts on the GPU, run once: every burst against the oracle's
    results as it goes, the counters before, between and after, then the state
    (Bridge.dump() stops the resident kernel, so the state is read once, behind
    the last burst: a read after every burst would cost a launch each)."""
    r = order_ref
    br, _ = make_pair(CAP)
    st0 = br.serve_stats()
    per_burst = []
    for (a, b), p in zip(r["bounds"], r["per"]):
        send_burst(br, r["F"], r["ln"], r["dv"], r["now"], a, b, p["out"])
        per_burst.append(br.serve_stats())
    st1 = br.serve_stats()
    state_equals(br, r["per"][-1]["dump"])
    return dict(br=br, st0=st0, st1=st1, per_burst=per_burst)


@gpu
def test_order_inside_a_burst(order_ref, order_run):
    """(the bursts themselves are checked as order_run makes them) Then the
    batch past the expiry time, which is not served: the new MACs take the
    freed indices in stamp order, so the MACs by index show ts / tseq were
    stamped in packet order."""
    br, late = order_run["br"], order_ref["late"]
    st = br.serve_stats()
    m = late["F"].shape[0]
    send_burst(br, late["F"], late["ln"], late["dv"], late["now"], 0, m, late["out"])
    after = br.serve_stats()
    assert after["bursts"] == st["bursts"] and after["declined"] == st["declined"]
    state_equals(br, late["dump"])


@gpu
def test_path_is_taken(order_ref, order_run):
    """Every one of the eight bursts is served whole: burst_packets is the sum
    of the eight sizes, 1 + 2 + 31 + 32 + 33 + 64 + 65 + 130 = 358 (none is
    declined or left to the pipeline, so no smaller count can be right), in
    1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 = 11 requests. The counters stay 0 without
    the resident kernel."""
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
def rows_of(frames, ln, slot=SLOT):
    F = frames.reshape(-1, slot).copy()
    for i in range(F.shape[0]):
        F[i, ln[i]:] = 0
    return F


def one_vs_oracle(br, o, F, ln, dv, now, i):
    exp = F[i].copy()
    eo = o.run(exp, ln[i:i + 1], dv[i:i + 1], now[i:i + 1], F.shape[1])
    b = bytearray(F[i, :ln[i]].tobytes())
    assert br.process(int(dv[i]), b, int(now[i])) == eo[0], i
    assert bytes(b) == F[i, :ln[i]].tobytes(), i


def static_dsts(rng, F, frac=0.2):
    """Some frames addressed to the static rules' MACs."""
    n = F.shape[0]
    pick = rng.integers(0, len(STATICS), n)
    for i in np.nonzero(rng.random(n) < frac)[0]:
        F[i, 0:6] = list(STATICS[pick[i]][0])


@gpu
@pytest.mark.parametrize("cap,expire_us", [(64, EXPIRE_US), (16, EXPIRE_US), (64, 1)])
def test_process_one_server(cap, expire_us):
    """vp_process_one, packet by packet: MAC moves, static rules, runts, a full
    table, an idle exit in the middle; with 1 us expiry packets fall back
    whenever an expiry is due."""
    rng = np.random.default_rng(11)
    n = 400
    frames, ln, dv, now = mixed_bridge_trace(rng, n, 50)
    F = frames.reshape(n, SLOT)
    static_dsts(rng, F)
    F = rows_of(F, ln)
    assert (ln < 14).any()
    if expire_us == 1:  # (gaps of up to 20 ns: entries do expire along the way)
        now = T.NOW0 + (now - T.NOW0) * 10
        assert now[-1] - now[0] > 2000
    br, o = make_pair(cap, expire_us)
    for i in range(n // 2):
        one_vs_oracle(br, o, F, ln, dv, now, i)
    s0 = br.serve_stats()
    time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
    for i in range(n // 2, n):
        one_vs_oracle(br, o, F, ln, dv, now, i)
    s1 = br.serve_stats()
    check_state(br, o, cap)
    if expire_us != 1:
        assert s1["packets_one"] == n and s0["packets_one"] == n // 2, (s0, s1)
        assert s1["launches"] >= s0["launches"] + 1, (s0, s1)


@gpu
def test_lengths():
    """Frames of 14 to 1518 bytes, odd lengths among them: only the first 16
    bytes cross to the kernel and none come back; every byte is the input's."""
    rng = np.random.default_rng(1518)
    n, slot, cap = 120, 1536, 64
    F = rng.integers(0, 256, (n, slot), dtype=np.uint8)  # (payload / padding)
    src, dst = rng.integers(0, 30, n), rng.integers(0, 40, n)
    for i in range(n):
        F[i, 0:6] = list(mac_of(int(dst[i])))
        F[i, 6:12] = list(mac_of(int(src[i])))
    ln = rng.integers(14, 1519, n).astype(np.uint16)
    ln[:4] = (14, 15, 1517, 1518)
    dv = rng.integers(0, N_DEV, n).astype(np.uint16)
    now = (T.NOW0 + np.cumsum(rng.integers(0, 3, n))).astype(np.int64)
    for i in range(n):
        F[i, ln[i]:] = 0
    assert (ln % 2 == 1).any() and ln.min() == 14 and ln.max() == 1518
    br, o = make_pair(cap)
    st0 = br.serve_stats()
    a, fwd = 0, 0
    for m in [7, 64, 49]:
        out = burst_vs_oracle(br, o, F, ln, dv, now, a, a + m)
        fwd += int((out != FLOOD).sum())
        a += m
    assert a == n and fwd > n // 4
    d = br.serve_stats()
    assert d["burst_packets"] - st0["burst_packets"] == n and d["declined"] == 0, d
    check_state(br, o, cap)


@gpu
def test_fallback_same_results():
    """A burst the host does not route (expiries due in its middle): the
    pipeline's results, the counters saying so. Expiry 5 us: ten MACs 500 ns
    apart in a served burst, then twenty new ones 1 us apart, during which the
    ten expire one after another and their indices are taken again."""
    br, o = make_pair(CAP, expire_us=5)
    m = 30
    G = np.stack([fr(k, (k - 10) % 10 if k >= 10 else k + 1, k % N_DEV)[0] for k in range(m)]) \
        .astype(np.uint8)
    ln = np.full(m, 60, np.uint16)
    dv = (np.arange(m) % N_DEV).astype(np.uint16)
    now = np.concatenate([T.NOW0 + 500 * np.arange(10), T.NOW0 + 5000 + 1000 * np.arange(20)]) \
        .astype(np.int64)
    burst_vs_oracle(br, o, G, ln, dv, now, 0, 10)
    s0 = br.serve_stats()
    assert s0["bursts"] == 1 and s0["burst_packets"] == 10 and s0["declined"] == 0, s0
    first = live_macs(o.bridge_dump(CAP))
    assert len(first) == 10
    out = burst_vs_oracle(br, o, G, ln, dv, now, 10, 30)
    s1 = br.serve_stats()
    assert {k: s1[k] for k in ("bursts", "burst_packets", "declined")} == \
        {k: s0[k] for k in ("bursts", "burst_packets", "declined")}, (s0, s1)
    check_state(br, o, CAP)
    # (the first ten were there for some of the burst's frames and gone for others)
    assert (out != FLOOD).any() and (out == FLOOD).any()
    last = live_macs(o.bridge_dump(CAP))
    assert not (set(last) & set(first))
    # (indices of expired entries, reused by the second burst's MACs)
    assert {i for i, _ in last.values()} & {i for i, _ in first.values()}


CHILD = r"""
import json, sys
import numpy as np
import test_bridge_serve_gpu as B
from vigor_amd import traces as T
br, o = B.make_pair(64)
n = 40
F = np.stack([B.fr(k % 9, (k * 5 + 1) % 11, k % 3)[0] for k in range(n)]).astype(np.uint8)
ln = np.full(n, 60, np.uint16)
dv = (np.arange(n) % 3).astype(np.uint16)
now = (T.NOW0 + np.arange(n)).astype(np.int64)
B.burst_vs_oracle(br, o, F, ln, dv, now, 0, 20)
B.burst_vs_oracle(br, o, F, ln, dv, now, 20, 40)
B.check_state(br, o, 64)
print("STATS " + json.dumps(br.serve_stats()))
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
    single packets: one table throughout, and the counters add up."""
    n, cap = 260, 64
    rng = np.random.default_rng(5)
    frames, ln, dv, now = mixed_bridge_trace(rng, n, 50)
    F = frames.reshape(n, SLOT)
    static_dsts(rng, F)
    F = rows_of(F, ln)
    br, o = make_pair(cap)

    def device(a, b):
        exp = F[a:b].reshape(-1).copy()
        eo = o.run(exp, ln[a:b], dv[a:b], now[a:b], SLOT)
        got, out = run_gpu(br, F[a:b].reshape(-1), ln[a:b], dv[a:b], now[a:b], SLOT)
        np.testing.assert_array_equal(out, eo)
        np.testing.assert_array_equal(got, exp)

    for i in range(0, 10):
        one_vs_oracle(br, o, F, ln, dv, now, i)
    burst_vs_oracle(br, o, F, ln, dv, now, 10, 40)
    one_vs_oracle(br, o, F, ln, dv, now, 40)
    device(41, 141)
    burst_vs_oracle(br, o, F, ln, dv, now, 141, 171)
    s0 = br.serve_stats()
    time.sleep(0.1)  # past the idle exit (VIGPATH_SERVE_IDLE_MS, 20)
    burst_vs_oracle(br, o, F, ln, dv, now, 171, 241)
    for i in range(241, n):
        one_vs_oracle(br, o, F, ln, dv, now, i)
    s1 = br.serve_stats()
    assert s1["launches"] >= s0["launches"] + 1, (s0, s1)  # (launched again after the idle exit)
    assert s1["burst_packets"] == 30 + 30 + 70 and s1["bursts"] == 1 + 1 + 2, s1
    assert s1["packets_one"] == 11 + n - 241 and s1["declined"] == 0, s1
    check_state(br, o, cap)


@gpu
def test_bridge_and_fw_share_a_gpu():
    """A vigbridge and a vigfw context on one GPU, each with a resident
    kernel, taking turns: the launch of one yields the other's (serve_yield),
    so both make progress; each against its own oracle and counters."""
    import test_fw_serve_gpu as W
    br, bo = make_pair(64)
    fw, fo = W.make_pair(64)
    m = 40
    BF = np.stack([fr(k % 7, (k * 3 + 1) % 9, k % N_DEV)[0] for k in range(2 * m)]) \
        .astype(np.uint8)
    bdv = (np.arange(2 * m) % N_DEV).astype(np.uint16)
    FF = np.stack([(W.lan_frame(k % 7) if k % 4 else W.wan_frame(k % 7))[0]
                   for k in range(2 * m)]).astype(np.uint8)
    fdv = np.array([0 if k % 4 else W.WAN for k in range(2 * m)], np.uint16)
    ln = np.full(2 * m, 60, np.uint16)
    now = (T.NOW0 + 5 * np.arange(2 * m)).astype(np.int64)
    for i in range(m):
        one_vs_oracle(br, bo, BF, ln, bdv, now, i)
        W.one_vs_oracle(fw, fo, FF, ln, fdv, now, i)
    burst_vs_oracle(br, bo, BF, ln, bdv, now, m, 2 * m)
    W.burst_vs_oracle(fw, fo, FF, ln, fdv, now, m, 2 * m)
    check_state(br, bo, 64)
    W.check_state(fw, fo, 64)
    sb, sf = br.serve_stats(), fw.serve_stats()
    assert sb["packets_one"] == m and sf["packets_one"] == m, (sb, sf)
    assert sb["burst_packets"] == m and sf["burst_packets"] == m, (sb, sf)
    assert sb["declined"] == 0 and sf["declined"] == 0, (sb, sf)
