"""Expiry inside vignat's and vigfw's resident kernels (the touch journal,
DESIGN.md 5.3): once a context has met a due expiry on the served path its
kernel expires the entries itself, in the reference's LRU order, and stays.

Every test compares out ports, every frame byte and the full dump (alloc, ts,
keys, vigfw's int_devices) with the CPU oracle, as test_fw_serve_gpu.py and
test_serve_burst_gpu.py do, and reads vp_serve_expiry_stats_get /
vp_serve_stats_get to see which path ran. vignat's external port is the flow
index, so the order freed indices are handed out again shows in the frames.
Reference behaviour: expire_items_single_map at the top of nf_process
(nat_main.c, fw_main.c; expirator.c:110-218).
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import orc
import pytest
import test_fw_serve_gpu as FWT
import test_serve_burst_gpu as NATT
from tracegen import mixed_fw_trace, mixed_nat_trace
from vigor_amd import traces as T

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 64


class Kit:
    """One NF's helpers under one set of names."""

    def __init__(self, kind):
        self.kind = kind
        self.m = NATT if kind == "nat" else FWT

    def pair(self, cap, expire_us):
        return self.m.make_pair(cap, expire_us)

    def oracle(self, cap, expire_us):
        """The oracle alone (no GPU context)."""
        if self.kind == "fw":
            return FWT.make_oracle(cap, expire_us)
        ocfg = orc.nat_cfg(wan=1, start_port=0, ext_ip=NATT.EXT_IP, expire_us=expire_us,
                           max_flows=cap, device_macs=NATT.DEV_MACS,
                           endpoint_macs=NATT.END_MACS, n_devices=2)
        return orc.Oracle("nat", ocfg)

    def expire_ns(self, expire_us):
        """E of cutoff = now - E: vignat multiplies in 32 bits
        (nat_flowmanager.c:57-65), vigfw in 64 (fw_flowmanager.c:66-68)."""
        return (expire_us * 1000) % (1 << 32) if self.kind == "nat" else expire_us * 1000

    def lan(self, k):
        return self.m.lan_frame(k)

    def odd(self):
        return self.m.odd_frame("v6")  # not IPv4: touches nothing, the expiry still runs

    def dump(self, o, cap):
        return o.nat_dump(cap) if self.kind == "nat" else o.fw_dump(cap)

    def check_state(self, nf, o, cap):
        self.m.check_state(nf, o, cap)

    def burst(self, nf, o, F, ln, dv, now, a, b):
        return self.m.burst_vs_oracle(nf, o, F, ln, dv, now, a, b)

    def one(self, nf, o, F, ln, dv, now, i):
        FWT.one_vs_oracle(nf, o, F, ln, dv, now, i)

    def mixed(self, seed, n, flows, cap, plain=True):
        """The NF's mixed trace (LAN, WAN, malformed frames); plain: IPv4
        options given 20-byte headers, so that no burst is declined."""
        rng = np.random.default_rng(seed)
        if self.kind == "nat":
            fr, ln, dv, now = mixed_nat_trace(rng, n, flows, max_idx=cap)
        else:
            fr, ln, dv, now = mixed_fw_trace(rng, n, flows)
        F = FWT.rows_of(fr, ln)
        if plain:
            F[:, 14] = np.where(F[:, 14] == 0x46, 0x45, F[:, 14])
        return F, ln, dv, now


KINDS = ["nat", "fw"]


def pack(pk, now):
    """A list of (frame, len, dev) and their times as trace arrays."""
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    for i in range(F.shape[0]):
        F[i, ln[i]:] = 0
    return F, ln, dv, np.asarray(now, np.int64)


def oracle_expiries(kit, make_oracle, cap, e_ns, F, ln, dv, now):
    """Entries the reference expires at each packet, from the oracle's dump
    before the packet: the allocated indices stamped below now - E; checked
    against the dump after it (such an index is free, or was handed out again
    and stamped at this packet)."""
    o = make_oracle()
    n = F.shape[0]
    cnt = np.zeros(n, np.int64)
    for i in range(n):
        a0, ts0 = kit.dump(o, cap)[:2]
        exp = F[i].copy()
        o.run(exp, ln[i:i + 1], dv[i:i + 1], now[i:i + 1], SLOT)
        a1, ts1 = kit.dump(o, cap)[:2]
        gone = (a0 == 1) & (ts0 < int(now[i]) - e_ns)
        assert ((a1[gone] == 0) | (ts1[gone] == now[i])).all(), i
        cnt[i] = int(gone.sum())
    return cnt


def prime(kit, nf, o, t0, e_ns, k0=900):
    """Turn the journal on: a throwaway flow, a packet past its expiry (the
    first bounce: the pipeline's), and one more packet, whose launch seeds the
    journal. Returns the time of the last packet."""
    pk = [kit.lan(k0), kit.odd(), kit.odd()]
    now = [t0, t0 + e_ns + 1, t0 + e_ns + 2]
    F, ln, dv, now = pack(pk, now)
    x0 = nf.serve_expiry_stats()
    for i in range(3):
        kit.one(nf, o, F, ln, dv, now, i)
    x = nf.serve_expiry_stats()
    assert x["handed"] == x0["handed"] + 1 and x["seeds"] == x0["seeds"] + 1, (x0, x)
    return int(now[-1])


def churn(kit, k0, n, t0, step):
    """n never-seen LAN flows k0 .. k0 + n - 1, `step` ns apart."""
    return pack([kit.lan(k0 + i) for i in range(n)], t0 + step * np.arange(n, dtype=np.int64))


# ---------------------------------------------------- 1. per-packet churn --
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cap,idle", [(64, True), (16, False)])
def test_per_packet_churn(kind, cap, idle):
    """The mixed traces with time stretched so that flows expire along the way
    (1 us expiry): one packet is handed to the pipeline, every later expiry is
    the kernel's, and an idle exit in the middle seeds nothing again."""
    kit = Kit(kind)
    n = 400
    F, ln, dv, now = kit.mixed(11, n, 50, cap, plain=False)
    # (gaps of up to 40 ns; at 20 the 16-index vignat table, mostly full, sees
    # 8 expiries after the first, below the precondition's 20)
    now = T.NOW0 + (now - T.NOW0) * 20
    e_ns = kit.expire_ns(1)
    per = oracle_expiries(kit, lambda: kit.oracle(cap, 1), cap, e_ns, F, ln, dv, now)
    nf, o = kit.pair(cap, 1)
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
    assert handed_at is not None and handed_at < n // 2
    want = int(per[handed_at + 1:].sum())
    assert want >= 20, want  # (the trace's precondition, from the oracle alone)
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
    """16 flows stamped at one time in a scrambled order (their sequence
    numbers decide the LRU order), a throwaway flow whose expiry is the first
    bounce, then a served burst whose first packet expires all 16: its 24 new
    flows take the freed indices youngest first, then fresh ones."""
    kit = Kit(kind)
    cap, e_us = 64, 5
    e_ns = kit.expire_ns(e_us)
    nf, o = kit.pair(cap, e_us)
    t0 = T.NOW0
    perm = np.random.default_rng(2).permutation(16)
    pk = [kit.lan(900)] + [kit.lan(int(k)) for k in perm] + [kit.odd(), kit.odd()]
    now = [t0] + [t0 + 4000] * 16 + [t0 + e_ns + 1, t0 + e_ns + 2]
    pk += [kit.lan(100 + k) for k in range(24)]
    t1 = t0 + 4000 + e_ns + 1
    now += [t1 + k for k in range(24)]
    F, ln, dv, now = pack(pk, now)
    kit.burst(nf, o, F, ln, dv, now, 0, 1)
    kit.burst(nf, o, F, ln, dv, now, 1, 17)
    kit.burst(nf, o, F, ln, dv, now, 17, 18)  # the throwaway flow expires: the pipeline's
    x0 = nf.serve_expiry_stats()
    assert x0["handed"] == 1 and x0["expired"] == 0, x0
    kit.burst(nf, o, F, ln, dv, now, 18, 19)  # (launched again: the journal is seeded)
    s0 = nf.serve_stats()
    E, out = kit.burst(nf, o, F, ln, dv, now, 19, 43)
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    kit.check_state(nf, o, cap)
    assert x["seeds"] == 1 and x["handed"] == 1 and x["expired"] == 16 and x["walks"] == 1, x
    assert s["burst_packets"] == s0["burst_packets"] + 24 and s["declined"] == 0, (s0, s)
    if kind == "nat":
        # vignat's external port is the index (start port 0, raw on the wire):
        # the throwaway flow held 0 and the 16 took 1..16 in the order they
        # were stamped, so the youngest is 16 and the first new flow takes it,
        # the next 15, ... then 0, then the never-used range
        ports = [int(E[j, 34]) | (int(E[j, 35]) << 8) for j in range(24)]
        assert ports == list(range(16, -1, -1)) + list(range(17, 24)), ports


# ------------------------------------------------ 3. expiry inside a burst --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_expiry_inside_a_burst(kind):
    """With the journal on: ten flows, then twenty new ones 1 us apart in one
    call (5 us expiry). The call is served in parts, each up to the packet at
    which the next flow falls due, and freed indices are reused inside it."""
    kit = Kit(kind)
    cap, e_us = 16, 5
    nf, o = kit.pair(cap, e_us)
    t = prime(kit, nf, o, T.NOW0, kit.expire_ns(e_us)) + 10
    F, ln, dv, _ = churn(kit, 0, 30, 0, 0)
    now = np.concatenate([t + np.arange(10), t + 2000 + 1000 * np.arange(20)]).astype(np.int64)
    per = oracle_expiries(kit, lambda: _primed_oracle(kit, cap, e_us, kit.expire_ns(e_us)), cap,
                          kit.expire_ns(e_us), F, ln, dv, now)
    assert per[:10].sum() == 0 and per[10:].sum() >= 10 and (per[10:] > 0).sum() >= 2, per
    kit.burst(nf, o, F, ln, dv, now, 0, 10)
    first = {k.tobytes() for a, k in zip(*kit.dump(o, cap)[0:3:2]) if a}
    s0, x0 = nf.serve_stats(), nf.serve_expiry_stats()
    kit.burst(nf, o, F, ln, dv, now, 10, 30)
    s1, x1 = nf.serve_stats(), nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    print(kind, s0, s1, x0, x1)
    assert x1["splits"] >= x0["splits"] + 1, (x0, x1)
    assert s1["burst_packets"] == s0["burst_packets"] + 20 and s1["declined"] == 0, (s0, s1)
    assert x1["handed"] == x0["handed"] and x1["seeds"] == x0["seeds"], (x0, x1)
    assert x1["expired"] == x0["expired"] + int(per.sum()), (x0, x1, per)
    alloc, _, keys = kit.dump(o, cap)[:3]
    assert any(alloc[i] and keys[i].tobytes() not in first for i in range(10))


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_call_sizes_across_churn(kind):
    """Calls of 1, 2, 63, 64, 65 and 130 packets across a churn trace."""
    kit = Kit(kind)
    cap, sizes = 16, [1, 2, 63, 64, 65, 130]
    n = sum(sizes)
    F, ln, dv, now = kit.mixed(5, n, 40, cap)
    now = T.NOW0 + (now - T.NOW0) * 20
    nf, o = kit.pair(cap, 1)
    t = prime(kit, nf, o, T.NOW0 - 10_000, kit.expire_ns(1))
    assert t < now[0]
    x0, s0 = nf.serve_expiry_stats(), nf.serve_stats()
    a = 0
    for m in sizes:
        kit.burst(nf, o, F, ln, dv, now, a, a + m)
        a += m
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    kit.check_state(nf, o, cap)
    print(kind, x, s)
    assert x["handed"] == x0["handed"] and x["seeds"] == x0["seeds"], (x0, x)
    assert s["burst_packets"] == s0["burst_packets"] + n and s["declined"] == 0, (s0, s)
    assert x["expired"] >= x0["expired"] + 20 and x["splits"] >= 1, (x0, x)


# ----------------------------------------------------------- 4. boundary --
@gpu
@pytest.mark.parametrize("kind,e_us", [("nat", 5), ("fw", 5), ("nat", 4_294_968)])
def test_boundary(kind, e_us):
    """A stamp equal to the cutoff survives (ts < cutoff is the test); one
    nanosecond later the kernel expires it. 4294968 us: vignat's
    expiration_time * 1000 wraps in 32 bits, to 704 ns."""
    kit = Kit(kind)
    cap = 16
    e_ns = kit.expire_ns(e_us)
    if e_us > 5:
        assert e_ns == 704
    nf, o = kit.pair(cap, e_us)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    pk = [kit.lan(1), kit.odd(), kit.lan(2), kit.odd(), kit.lan(1)]
    now = [t, t + e_ns, t + e_ns, t + e_ns + 1, t + e_ns + 1]
    F, ln, dv, now = pack(pk, now)
    x0 = nf.serve_expiry_stats()
    for i in range(3):
        kit.one(nf, o, F, ln, dv, now, i)
    x1 = nf.serve_expiry_stats()
    assert x1["expired"] == x0["expired"], (x0, x1)  # flow 1 is still there
    for i in range(3, 5):
        kit.one(nf, o, F, ln, dv, now, i)
    x2 = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert x2["expired"] == x1["expired"] + 1 and x2["handed"] == x0["handed"], (x1, x2)
    assert nf.serve_stats()["packets_one"] == 3 + 5 - 1


# -------------------------------------------------------- 5. rejuvenation --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rejuvenation(kind):
    """A flow touched many times (LAN hits and, for vignat, WAN hits) survives
    when its stale records reach the journal's tail; its neighbour, never
    touched again, goes."""
    kit = Kit(kind)
    cap, e_us = 16, 5
    e_ns = kit.expire_ns(e_us)
    nf, o = kit.pair(cap, e_us)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    # the primer's flow took index 0 and expired: flow 1 takes index 0 again
    pk, now = [kit.lan(1), kit.lan(2)], [t, t + 1]
    for r in range(12):
        hit = kit.lan(1)
        if kind == "nat" and r % 2:
            hit = NATT.wan_frame(0, 1)  # (flow 1 holds external port 0)
        pk.append(hit)
        now.append(t + 1000 * (r + 1))
    last = now[-1]
    pk += [kit.odd(), kit.lan(1), kit.odd()]
    now += [last + e_ns, last + e_ns, last + 2 * e_ns + 1]
    F, ln, dv, now = pack(pk, now)
    per = oracle_expiries(kit, lambda: _primed_oracle(kit, cap, e_us, e_ns), cap, e_ns,
                          F, ln, dv, now)
    assert per.sum() == 2 and per[-1] == 1, per  # flow 2 along the way, flow 1 at the end
    x0 = nf.serve_expiry_stats()
    for i in range(len(pk)):
        kit.one(nf, o, F, ln, dv, now, i)
    x = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    assert x["expired"] == x0["expired"] + 2 and x["handed"] == x0["handed"], (x0, x)
    assert x["seeds"] == x0["seeds"], (x0, x)


def _primed_oracle(kit, cap, e_us, e_ns):
    """An oracle that has seen prime()'s three packets."""
    o = kit.oracle(cap, e_us)
    F, ln, dv, now = pack([kit.lan(900), kit.odd(), kit.odd()],
                          [T.NOW0, T.NOW0 + e_ns + 1, T.NOW0 + e_ns + 2])
    exp = F.reshape(-1).copy()
    o.run(exp, ln, dv, now, SLOT)
    return o


# ----------------------------------------------------------- 6. ring full --
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", ["one", "burst"])
def test_ring_full(kind, path):
    """16 indices, 128 records: one idle flow pins the tail while more than
    128 touches are served, so the ring fills and is seeded again from the
    table; then the idle flow's expiry, still the kernel's."""
    kit = Kit(kind)
    cap, e_us = 16, 60
    e_ns = kit.expire_ns(e_us)
    nf, o = kit.pair(cap, e_us)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    x0 = nf.serve_expiry_stats()
    pk, now = [kit.lan(1)], [t]
    m = 150 if path == "one" else 600  # (a burst journals one record per index)
    for r in range(m):
        pk.append(kit.lan(2 + r % 15))
        now.append(t + 1 + r)
    pk += [kit.odd(), kit.lan(1)]
    now += [t + e_ns + 1, t + e_ns + 2]
    F, ln, dv, now = pack(pk, now)
    n = len(pk)
    if path == "one":
        for i in range(n):
            kit.one(nf, o, F, ln, dv, now, i)
    else:
        kit.burst(nf, o, F, ln, dv, now, 0, 1)
        for a in range(1, 1 + m, 60):
            kit.burst(nf, o, F, ln, dv, now, a, min(a + 60, 1 + m))
        kit.burst(nf, o, F, ln, dv, now, 1 + m, n)
    x = nf.serve_expiry_stats()
    kit.check_state(nf, o, cap)
    print(kind, path, x)
    assert x["seeds"] >= x0["seeds"] + 1 and x["seeds"] >= 2, (x0, x)
    assert x["handed"] == x0["handed"], (x0, x)
    assert x["expired"] == x0["expired"] + 1, (x0, x)


# ---------------------------------------------------------- 7. tombstones --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_tombstones_purged_while_served(kind):
    """16 indices under churn until erased and live entries pass the purge
    bound (tbl_check_tombs' 85 %): the kernel reports it, the host rebuilds and
    launches it again, and no request takes the pipeline for it."""
    kit = Kit(kind)
    cap, e_us = 16, 5
    e_ns = kit.expire_ns(e_us)
    nf, o = kit.pair(cap, e_us)
    t = prime(kit, nf, o, T.NOW0, e_ns) + 10
    x0, r0 = nf.serve_expiry_stats(), nf.table_stats()["rebuilds"]
    k0, rose = 1000, False
    for _ in range(60):  # (about 14 flows live at a time, a new one every 350 ns)
        F, ln, dv, now = churn(kit, k0, 64, t, 350)
        kit.burst(nf, o, F, ln, dv, now, 0, 64)
        k0, t = k0 + 64, int(now[-1]) + 350
        rose = nf.table_stats()["rebuilds"] > r0
        if rose:
            break
    x, s = nf.serve_expiry_stats(), nf.serve_stats()
    print(kind, "flows sent", k0 - 1000, x, s, nf.table_stats())
    assert rose, "the purge bound was never passed"
    # served again after the rebuild, and still nothing handed over
    F, ln, dv, now = churn(kit, k0, 64, t, 350)
    kit.burst(nf, o, F, ln, dv, now, 0, 64)
    kit.check_state(nf, o, cap)
    x1, s1 = nf.serve_expiry_stats(), nf.serve_stats()
    assert x1["handed"] == x0["handed"] and x1["seeds"] == x0["seeds"], (x0, x1)
    assert s1["burst_packets"] == s["burst_packets"] + 64 and s1["declined"] == 0, (s, s1)


# --------------------------------------------------- 8. pipeline in between --
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_pipeline_in_between(kind):
    """A dump keeps the journal; a batch through the pipeline drops it: the
    next due expiry is handed over once more and the journal seeded again."""
    kit = Kit(kind)
    cap, e_us = 64, 5
    e_ns = kit.expire_ns(e_us)
    nf, o = kit.pair(cap, e_us)
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
    # above the burst-route limit (256): the pipeline's
    s2 = nf.serve_stats()
    F, ln, dv, now = churn(kit, 200, 300, t, 500)
    kit.burst(nf, o, F, ln, dv, now, 0, 300)
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


# ----------------------------------------------------------- 9. switch off --
CHILD = r"""
import json, sys
import numpy as np
import test_serve_expiry_gpu as X
from vigor_amd import traces as T
kit = X.Kit(sys.argv[1])
nf, o = kit.pair(16, 5)
F, ln, dv, now = X.churn(kit, 0, 120, T.NOW0, 700)
for i in range(40):
    kit.one(nf, o, F, ln, dv, now, i)
kit.burst(nf, o, F, ln, dv, now, 40, 80)
kit.burst(nf, o, F, ln, dv, now, 80, 120)
kit.check_state(nf, o, 16)
print("STATS " + json.dumps(dict(nf.serve_expiry_stats(), **nf.serve_stats())))
"""


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_in_child(kind):
    """VIGPATH_SERVE_EXPIRE=0 (read once per process: a fresh child): the same
    bytes, every due expiry through the pipeline."""
    env = dict(os.environ, VIGPATH_SERVE_EXPIRE="0")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", CHILD, kind], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    st = json.loads([x for x in r.stdout.splitlines() if x.startswith("STATS ")][-1][6:])
    assert st["expired"] == 0 and st["seeds"] == 0 and st["handed"] > 1, st
