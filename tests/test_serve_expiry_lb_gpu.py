"""Expiry inside viglb's resident kernel (the touch journals),
as test_serve_expiry_bp_gpu.py has it for vigbridge and vigpol: once a context
has met a due expiry on the served path lb_serve expires flows and backends
itself, each table from its own journal and on its own lifetime, and stays.

Every GPU test compares out ports, every frame byte and both tables' full dump
with the CPU oracle and reads vp_serve_expiry_stats_get / vp_serve_stats_get
to see which path ran. Every trace and its precondition come from a builder
that uses the oracle alone; test_trace_preconditions runs them all without a
GPU. Flows live 1000 us and backends 700 us wherever nothing else is needed,
so that swapping the two lifetimes fails.

Reference behaviour: lb_main.c:20-68 (lb_expire_flows, then lb_expire_backends,
at the top of every nf_process: before the parse), lb_balancer.c:38-143 (a hit
on a live backend, a re-pointing and an allocation stamp the flow; a heartbeat
stamps its backend; a WAN packet never stamps a backend).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import test_lb_serve_gpu as L
from test_lb_serve_gpu import H, W
from vigor_amd import traces as T

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
US = 1000
WAN = L.WAN
FEXP, BEXP = 1000, 700  # us: flows, backends
ROUTE = 128             # kLbBurstRoute


class Cfg:
    """A context's shape: capacities, the CHT's height, both lifetimes (us)."""

    def __init__(self, fcap=L.FCAP, bcap=L.BCAP, height=L.HEIGHT, fexp=FEXP, bexp=BEXP):
        self.fcap, self.bcap, self.height, self.fexp, self.bexp = fcap, bcap, height, fexp, bexp
        self.ef, self.eb = fexp * US, bexp * US  # ns

    def args(self):
        return (self.fcap, self.bcap, self.height, self.fexp, self.bexp)

    def pair(self):
        return L.make_pair(*self.args())

    def oracle(self):
        return L.make_oracle(*self.args())

    def dump(self, o):
        return o.lb_dump(self.fcap, self.bcap)


STD = Cfg()


def NP(kind="arp", dev=WAN):
    """A frame lb_main.c's parse refuses: an ARP-sized frame that is not IPv4,
    or an IPv4 frame that is neither TCP nor UDP (ICMP)."""
    if kind == "arp":
        return L.frame(T.ip4(11, 0, 0, 1), dev, 42, eth=(0x08, 0x06)), 42, dev, "np"
    return L.frame(T.ip4(11, 0, 0, 1), dev, 60, proto=1), 60, dev, "np"


def pack(pk, now):
    """A list of (frame, len, dev, tag) and their times as trace arrays."""
    F = np.stack([p[0] for p in pk]).astype(np.uint8)
    ln = np.array([p[1] for p in pk], np.uint16)
    dv = np.array([p[2] for p in pk], np.uint16)
    now = np.asarray(now, np.int64)
    assert F.shape[0] == now.shape[0] and (np.diff(now) >= 0).all()
    return F, ln, dv, now


def oracle_steps(cfg, o, F, ln, dv, now):
    """The trace through o packet by packet: per packet the flows and the
    backends the reference expires (allocated before it and stamped below
    now - E of their own table; checked against the dump behind the packet: such
    an index is free, or was handed out again and stamped at this packet), the
    out port, the frame after, and the state behind it. Consumes o."""
    n = F.shape[0]
    pf, pb = np.zeros(n, np.int64), np.zeros(n, np.int64)
    out, E, st = np.zeros(n, np.uint16), np.zeros_like(F), []
    for i in range(n):
        (fa0, ft0, _, _), (ba0, bt0, _, _, _) = cfg.dump(o)
        oi, Ei = L.oracle_run(o, F, ln, dv, now, i, i + 1)
        out[i], E[i] = oi[0], Ei[0]
        d1 = cfg.dump(o)
        (fa1, ft1, _, _), (ba1, bt1, _, _, _) = d1
        gf = (fa0 == 1) & (ft0 < int(now[i]) - cfg.ef)
        gb = (ba0 == 1) & (bt0 < int(now[i]) - cfg.eb)
        assert ((fa1[gf] == 0) | (ft1[gf] == now[i])).all(), i
        assert ((ba1[gb] == 0) | (bt1[gb] == now[i])).all(), i
        pf[i], pb[i] = int(gf.sum()), int(gb.sum())
        st.append(L.tables(d1))
    return dict(pf=pf, pb=pb, per=pf + pb, out=out, E=E, st=st)


def splits_of(per, a, b):
    """The requests a served call [a, b) is cut into beyond its chunks of 64:
    one more at every lane above a request's first at which an entry expires
    (the rest is posted again, and its own first lane runs the walk)."""
    k, first = 0, a
    for j in range(a, b):
        if j - first == 64:
            first = j
        if j > first and per[j] > 0:
            k, first = k + 1, j
    return k


def dst_ip(row):
    return bytes(row[30:34])


def be_ip(b):
    return bytes((192, 168, 0, b))


# ------------------------------------------------------------ the primer --
def primer(cfg, t0):
    """Four packets that turn the journals on: backend 100 and a flow on it,
    backend 101 past both lifetimes (the first bounce: the pipeline's), and
    backend 102, whose launch seeds both journals. 101 and 102 stay behind."""
    e = max(cfg.ef, cfg.eb)
    return pack([H(100), W(900), H(101), H(102)], [t0, t0 + 1, t0 + e + 2, t0 + e + 3])


def primed_oracle(cfg, t0=T.NOW0):
    """An oracle that has seen the primer, and the primer's last time."""
    o = cfg.oracle()
    F, ln, dv, now = primer(cfg, t0)
    r = oracle_steps(cfg, o, F, ln, dv, now)
    assert list(r["pf"]) == [0, 0, 1, 0] and list(r["pb"]) == [0, 0, 1, 0], r
    return o, int(now[-1])


def one(lb, o, F, ln, dv, now, i):
    return int(L.one_vs_oracle(lb, o, F, ln, dv, now, i))


def burst(lb, o, F, ln, dv, now, a, b):
    return L.burst_vs_oracle(lb, o, F, ln, dv, now, a, b)


def prime(cfg, lb, o, t0=T.NOW0):
    """The primer on the GPU and the oracle: one request handed over, both
    tables seeded. Returns the last packet's time."""
    F, ln, dv, now = primer(cfg, t0)
    x0 = lb.serve_expiry_stats()
    for i in range(4):
        one(lb, o, F, ln, dv, now, i)
    x = lb.serve_expiry_stats()
    assert x["handed"] == x0["handed"] + 1 and x["seeds"] == x0["seeds"] + 2, (x0, x)
    assert x["expired"] == x0["expired"], (x0, x)
    return int(now[-1])


def delta(lb, x0, s0):
    x, s = lb.serve_expiry_stats(), lb.serve_stats()
    d = {k: x[k] - x0[k] for k in x0}
    d.update({k: s[k] - s0[k] for k in s0})
    return d


def stats(lb):
    return lb.serve_expiry_stats(), lb.serve_stats()


def behind_primer(cfg, pk, dt, t0=T.NOW0):
    """pk at times base + dt behind the primer, base far enough on that the
    primer's two backends expire at pk's first packet: the trace, the oracle's
    steps, the base."""
    o, tp = primed_oracle(cfg, t0)
    base = tp + max(cfg.ef, cfg.eb) + 10
    F, ln, dv, now = pack(pk, [base + d for d in dt])
    r = oracle_steps(cfg, o, F, ln, dv, now)
    assert r["pb"][0] == 2 and r["pf"][0] == 0, (r["pf"], r["pb"])
    r.update(cfg=cfg, F=F, ln=ln, dv=dv, now=now, base=base)
    return r


# =============================================================== builders ==
def churn_trace(n, seed, step=20 * US, t0=T.NOW0):
    """Every fourth packet a heartbeat, round robin over six backends of which
    two in turn stay silent for 64 packets (1.28 ms: they expire and come
    back); the others WAN packets, every eighth a never-seen flow and the rest
    hits on the eight newest (a flow ages out about 50 packets after it has
    left them, and the flows of a silent backend are re-pointed)."""
    rng = np.random.default_rng(seed)
    pk, nflow = [], 0
    for i in range(n):
        w = i // 64
        silent = {1 + w % 6, 1 + (w + 3) % 6} if i else set()  # (a backend first)
        b = 1 + (i // 4) % 6
        if i % 4 == 0 and b not in silent:
            pk.append(H(b))
        elif i % 8 == 1 or nflow == 0:
            nflow += 1
            pk.append(W(nflow))
        else:
            pk.append(W(int(rng.integers(max(1, nflow - 7), nflow + 1))))
    return pack(pk, t0 + step * np.arange(n, dtype=np.int64))


def no_erasure(r):
    """No packet of the trace is the erasure (a backend is alive throughout)."""
    assert all(len(s[1]) > 0 for s in r["st"]), "no backend alive"


def build_churn(n=900):
    cfg = STD
    F, ln, dv, now = churn_trace(n, 11)
    r = oracle_steps(cfg, cfg.oracle(), F, ln, dv, now)
    no_erasure(r)
    nz = np.nonzero(r["per"])[0]
    h = int(nz[0])
    assert h < n // 4, h
    assert r["pf"][h + 1:].sum() >= 20 and r["pb"][h + 1:].sum() >= 20, (r["pf"].sum(), r["pb"].sum())
    r.update(cfg=cfg, F=F, ln=ln, dv=dv, now=now, handed_at=h)
    return r


def build_order():
    """Backend 50; six backends and ten flows allocated in order and then
    touched again in a scrambled order at one time (their sequence numbers
    decide the LRU order); 50 past its own lifetime (the bounce) and once more
    (the seed); then one packet at which all of them expire, and new backends
    and flows, which take the freed indices youngest first."""
    cfg = Cfg(fexp=7, bexp=5)
    t0 = T.NOW0
    rng = np.random.default_rng(2)
    pb_, pf_ = [int(k) for k in 1 + rng.permutation(6)], [int(k) for k in 1 + rng.permutation(10)]
    assert pb_ != sorted(pb_) and pf_ != sorted(pf_)
    pk = [H(50)] + [H(k) for k in range(1, 7)] + [W(k) for k in range(1, 11)]
    now = [t0] + [t0 + 3000] * 16
    pk += [H(k) for k in pb_] + [W(k) for k in pf_]
    now += [t0 + 4000] * 16
    pk += [H(50), H(50)]
    now += [t0 + 5001, t0 + 5002]
    t1 = t0 + 4000 + cfg.ef + 1
    newb, newf = [21, 22, 23, 24, 25, 26, 27], list(range(21, 35))
    pk += [H(k) for k in newb] + [W(k) for k in newf]
    now += [t1 + k for k in range(len(newb) + len(newf))]
    F, ln, dv, now = pack(pk, now)
    o = cfg.oracle()
    r = oracle_steps(cfg, o, F, ln, dv, now)
    assert r["pb"][33] == 1 and r["per"][:33].sum() == 0 and r["per"][34] == 0, r["per"]
    assert r["pf"][35] == 10 and r["pb"][35] == 7 and r["per"][36:].sum() == 0, r["per"]
    # 50 holds backend index 0, the six 1..6 and the ten flows 0..9 in the order
    # they came; the oldest stamp frees first, so the youngest lies on top: 50,
    # stamped last (it goes as well: 5 us), then the scrambled order's last
    flows, backs = r["st"][-1]
    gotb = [backs[L.src_ip(F[35 + k])][0] for k in range(len(newb))]
    gotf = [flows[L.flow_key(F[35 + len(newb) + k])][0] for k in range(len(newf))]
    assert gotb == [0] + [k for k in reversed(pb_)], (gotb, pb_)
    assert gotf == [k - 1 for k in reversed(pf_)] + [10, 11, 12, 13], (gotf, pf_)
    r.update(cfg=cfg, F=F, ln=ln, dv=dv, now=now)
    return r


def build_backend_dies(new_address):
    """Backends 1-3 and flows 1-6; 2 and 3 stay alive by heartbeats, every
    flow is hit 400 us on, and the backend v of flow 1 falls due at the lane k
    = 4 of the last call. new_address: lane k is a heartbeat from address 9,
    which takes v's index, and flow 1 then goes to backend 9 (the reference's
    quirk); else flow 1 is re-pointed to the CHT's choice among the living."""
    cfg = STD
    e = cfg.eb
    setup = [H(1), H(2), H(3)] + [W(k) for k in range(1, 7)]
    sdt = [0, 0, 0] + [US] * 6
    r0 = behind_primer(cfg, setup, sdt)
    flows, backs = r0["st"][-1]
    vi = flows[L.flow_key(r0["F"][3])][2]
    v = [ip for ip, b in backs.items() if b[0] == vi][0] >> 24  # (192.168.0.v, little endian)
    assert v in (1, 2, 3)
    others = [b for b in (1, 2, 3) if b != v]
    pk = setup + [H(others[0]), H(others[1])] + [W(k) for k in range(1, 7)]
    dt = sdt + [400 * US] * 8
    a = len(pk)
    mid = [H(9)] if new_address else [W(3)]
    pk += [W(1), W(2), W(1), W(3)] + mid + [W(1), W(2), W(1)]
    dt += [e - 3, e - 2, e - 1, e] + [e + 1, e + 2, e + 3, e + 4]
    r = behind_primer(cfg, pk, dt)
    k = a + 4
    assert r["per"][a:k].sum() == 0 and r["pb"][k] == 1 and r["pf"][k] == 0, (r["pf"], r["pb"])
    assert r["per"][k + 1:].sum() == 0
    old = be_ip(v)
    assert dst_ip(r["E"][a]) == old and dst_ip(r["E"][a + 2]) == old, "lanes below k: the old one"
    if new_address:
        assert r["st"][k][1][L.src_ip(r["F"][k])][0] == vi, "the new address takes v's index"
        assert dst_ip(r["E"][k + 1]) == be_ip(9) and dst_ip(r["E"][k + 3]) == be_ip(9)
        assert r["st"][-1][0][L.flow_key(r["F"][a])][2] == vi  # (never re-pointed)
    else:
        new = dst_ip(r["E"][k + 1])
        assert new != old and new in [be_ip(b) for b in others], new
        assert dst_ip(r["E"][k + 3]) == new
        assert r["st"][-1][0][L.flow_key(r["F"][a])][2] != vi
    r.update(a=a, k=k)
    return r


CUTS = ["flow", "backend", "both", "apart"]


def build_cut(case):
    """Backend 1 and flow 1 on it, backend 2 later, backend 3 later still;
    backend 1 goes at a packet of its own. Then one call of eight lanes, new
    flows and frames that do not parse, in which flow 1 (stamped at 1 us)
    and / or backend 2 fall due. Every entry is stamped once, so each journal's
    floor is its oldest live stamp and a burst is cut exactly where the
    reference expires."""
    cfg = STD
    ef, eb = cfg.ef, cfg.eb
    tf = US                       # flow 1's stamp
    due_f = tf + ef + 1
    # backend 2's stamp: due with flow 1, 3 ns behind it, or not in the call
    tb2 = {"flow": due_f - eb + 5000, "backend": None, "both": due_f - eb - 1,
           "apart": due_f - eb + 2}[case]
    if case == "backend":  # flow 1 comes 100 us later and is not due in the call
        tb2, tf2 = 301 * US, 101 * US
        pk = [H(1), W(1), H(2), H(3), NP()]
        dt = [0, tf2, tb2, 600 * US, eb + 1]
        t = tb2 + eb - 1
    else:
        pk = [H(1), W(1), H(2), H(3), NP()]
        dt = [0, tf, tb2, 600 * US, eb + 1]
        t = due_f - 2
    a = len(pk)
    pk += [W(10), NP("icmp"), W(11), W(12), NP(), W(13), W(14), W(15)]
    dt += [t, t + 1, t + 2, t + 3, t + 4, t + 5, t + 6, t + 7]
    r = behind_primer(cfg, pk, dt)
    assert r["pb"][4] == 1 and r["per"][1:4].sum() == 0, (r["pf"], r["pb"])
    want = {"flow": ([0, 0, 1, 0, 0, 0, 0, 0], [0] * 8),
            "backend": ([0] * 8, [0, 0, 1, 0, 0, 0, 0, 0]),
            "both": ([0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0]),
            "apart": ([0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0, 0])}[case]
    assert (list(r["pf"][a:]), list(r["pb"][a:])) == want, (case, r["pf"][a:], r["pb"][a:])
    no_erasure(r)
    r.update(a=a, splits={"flow": 1, "backend": 1, "both": 1, "apart": 2}[case])
    assert splits_of(r["per"], a, a + 8) == r["splits"]
    return r


def build_unparsed(kind):
    """Backend 1 with flow 1 on it, backend 2 later; a frame that does not
    parse comes at the very time backend 1 falls due, between packets of
    flow 1: it expires the backend, and flow 1 is re-pointed behind it."""
    cfg = STD
    e = cfg.eb
    pk = [H(1), W(1), H(2), W(1), NP(kind), W(1)]
    dt = [0, US, 600 * US, e - 1, e + 1, e + 2]
    r = behind_primer(cfg, pk, dt)
    assert list(r["pb"][1:]) == [0, 0, 0, 1, 0] and r["pf"].sum() == 0, (r["pf"], r["pb"])
    assert r["out"][4] == WAN and (r["E"][4] == r["F"][4]).all()
    assert dst_ip(r["E"][3]) == be_ip(1) and dst_ip(r["E"][5]) == be_ip(2)
    return r


def build_boundary():
    """Backend 1 stamped at 0 and flow 1 at 1 us; frames that do not parse at
    stamp + E (alive) and stamp + E + 1 (gone) of each table."""
    cfg = STD
    pk = [H(1), W(1), H(2), NP(), NP("icmp"), NP(), NP("icmp")]
    dt = [0, US, 500 * US, cfg.eb, cfg.eb + 1, US + cfg.ef, US + cfg.ef + 1]
    r = behind_primer(cfg, pk, dt)
    assert list(r["pb"][1:]) == [0, 0, 0, 1, 0, 0], r["pb"]
    assert list(r["pf"]) == [0, 0, 0, 0, 0, 0, 1], r["pf"]
    return r


def build_rejuvenation():
    """(a) backend 1 is kept by its heartbeats. (b) flow 2 on backend 2 is hit
    at 300 and 600 us: the flow stays, backend 2 goes at 700 us + 1 all the
    same. (c) flow 2 re-pointed at 800 us is stamped there: alive at 1650 us
    (gone at 1600 us + 1 had the re-pointing not stamped) and at 1800 us, gone
    one nanosecond later."""
    cfg = STD
    pk = [H(2), W(2), H(1), W(2), H(1), W(2), NP(), W(2), H(1), H(1), NP(), NP(), NP("icmp")]
    dt = [0, US, 2 * US, 300 * US, 500 * US, 600 * US, 700 * US + 1, 800 * US, 1000 * US,
          1600 * US, 1650 * US, 1800 * US, 1800 * US + 1]
    r = behind_primer(cfg, pk, dt)
    assert list(r["pb"][1:]) == [0, 0, 0, 0, 0, 1] + [0] * 6, r["pb"]
    assert list(r["pf"]) == [0] * 12 + [1], r["pf"]
    assert dst_ip(r["E"][1]) == be_ip(2) and dst_ip(r["E"][5]) == be_ip(2)
    assert dst_ip(r["E"][7]) == be_ip(1)
    key = L.flow_key(r["F"][1])
    assert r["st"][7][0][key][1] == r["now"][7] and key in r["st"][11][0]
    assert L.src_ip(r["F"][2]) in r["st"][-1][1]  # (backend 1: four heartbeats, alive)
    return r


def build_last_backend():
    """Backend 1 alone, flow 1 on it. At 700 us + 1 a packet of the unknown
    flow 5 expires the backend (none is alive) and leaves on the WAN device
    with nothing written; flow 1's next packet is the erasure; then backend 2,
    flow 3, and a packet at which backend 2 is due."""
    cfg = STD
    e = cfg.eb
    pk = [H(1), W(1), NP(), W(5), W(1), H(2), W(3), NP(), H(3), W(3)]
    dt = [0, US, e - 1, e + 1, e + 2, 800 * US, 801 * US, 800 * US + e + 1, 800 * US + e + 2,
          800 * US + e + 3]
    r = behind_primer(cfg, pk, dt)
    assert list(r["pb"][1:]) == [0, 0, 1, 0, 0, 0, 1, 0, 0] and r["pf"].sum() == 0, (r["pf"], r["pb"])
    assert not r["st"][3][1] and r["out"][3] == WAN and (r["E"][3] == r["F"][3]).all()
    assert L.flow_key(r["F"][3]) not in r["st"][3][0]
    key = L.flow_key(r["F"][1])
    assert key in r["st"][3][0] and key not in r["st"][4][0], "the erasure"
    assert r["out"][4] == WAN and (r["E"][4] == r["F"][4]).all()
    return r


def build_options():
    """Backend 1 and flow 1, backend 2; a call of four whose first lane comes
    when backend 1 is due and whose second frame has IPv4 options."""
    cfg = STD
    e = cfg.eb
    pk = [H(1), W(1), H(2), W(1), W(1, 64, ihl=6), W(2), H(2)]
    dt = [0, US, 600 * US, e + 1, e + 2, e + 3, e + 4]
    r = behind_primer(cfg, pk, dt)
    assert list(r["pb"][1:]) == [0, 0, 1, 0, 0, 0] and r["pf"].sum() == 0, (r["pf"], r["pb"])
    assert dst_ip(r["E"][4]) == be_ip(2)  # (the options frame is a packet of flow 1)
    return r


RING = Cfg(fexp=60, bexp=40)


def build_ring(table, path):
    """Rings of 32 (flows) and 16 (backends) records (VIGPATH_SERVE_JOURNAL=2):
    flow 1 and backend 1 stay idle while flows 2..11, or backends 2..5, are
    touched over and over, so that table's ring fills and both are seeded
    again; then the idle entries' expiry."""
    cfg = RING
    m = 150 if path == "one" else 480
    pk, dt = [H(1), H(2), W(1)], [0, 0, 1]
    for q in range(m):
        pk.append(W(2 + q % 10) if table == "flows" else H(2 + q % 4))
        dt.append(2 + q)
    pk += [H(2), NP(), H(3), W(1)]
    dt += [3 + m, cfg.eb + 1, cfg.ef + 2, cfg.ef + 3]
    r = behind_primer(cfg, pk, dt)
    assert r["per"][1:4 + m].sum() == 0 and r["pb"][4 + m] == 1, (r["pf"], r["pb"])
    assert r["pf"][5 + m] >= 1 and r["per"][6 + m] == 0
    no_erasure(r)
    r.update(m=m)
    return r


TOMB = {"flows": Cfg(fcap=64, bcap=8, height=11, fexp=20, bexp=1000),
        "backends": Cfg(fcap=16, bcap=64, height=67, fexp=1000, bexp=20)}


def tomb_burst(table, k0, t):
    """64 packets 350 ns apart from t: never-seen flows behind a heartbeat of
    backend 1, or never-seen backends (addresses 192.168.x.y)."""
    if table == "flows":
        pk = [H(1)] + [W(k0 + i) for i in range(63)]
    else:
        pk = []
        for i in range(64):
            k = k0 + i
            fr = L.frame(T.ip4(192, 168, 1 + (k >> 8), k & 0xFF), k & 1, smac=k & 0xFFFF)
            pk.append((fr, 60, k & 1, ""))
    return pack(pk, t + 350 * np.arange(64, dtype=np.int64))


def build_tombs(table, rounds=60):
    """The precondition, from the oracle's counts: the table holds about 57
    live entries (20 us at one every 350 ns) behind every burst and has
    expired far more entries than the purge bound of 163 (85 % of 64 buckets
    of 3) -- what 64 indices need to pass it and 16 do not
    (test_serve_expiry_bp_gpu's note)."""
    cfg = TOMB[table]
    o, tp = primed_oracle(cfg)
    t, k0, sent = tp + 10, 1000, 0
    for q in range(rounds):
        F, ln, dv, now = tomb_burst(table, k0, t)
        L.oracle_run(o, F, ln, dv, now, 0, 64)
        k0, t, sent = k0 + 64, int(now[-1]) + 350, sent + (63 if table == "flows" else 64)
        d = cfg.dump(o)[0 if table == "flows" else 1]
        live = int(d[0].sum())
        if q:
            assert 50 <= live <= 64, (q, live)
    assert sent - live >= 10 * 163
    return cfg


def sizes_trace():
    n = sum(L.SIZES)
    return churn_trace(n, 5, t0=T.NOW0 + 10_000 * US)


def build_sizes():
    """The churn trace in calls of SIZES, behind the primer."""
    cfg = STD
    F, ln, dv, now = sizes_trace()
    o, tp = primed_oracle(cfg)
    assert tp < now[0]
    r = oracle_steps(cfg, o, F, ln, dv, now)
    no_erasure(r)
    assert r["pf"].sum() >= 10 and r["pb"].sum() >= 5 and (r["per"][64:] > 0).sum() >= 5, r["per"]
    calls, a = [], 0
    for s in L.SIZES:
        calls.append((a, a + s))
        a += s
    r.update(cfg=cfg, F=F, ln=ln, dv=dv, now=now, calls=calls)
    assert sum(splits_of(r["per"], a, b) for a, b in calls) >= 3
    return r


def build_between():
    """Served churn, 129 packets in one call (above kLbBurstRoute: the
    pipeline's), served churn again."""
    cfg = STD
    F, ln, dv, now = churn_trace(120 + 129 + 240, 7, t0=T.NOW0 + 10_000 * US)
    o, tp = primed_oracle(cfg)
    assert tp < now[0]
    r = oracle_steps(cfg, o, F, ln, dv, now)
    no_erasure(r)
    assert r["per"][:120].sum() >= 3 and r["per"][249:].sum() >= 3, r["per"]
    r.update(cfg=cfg, F=F, ln=ln, dv=dv, now=now)
    return r


def test_trace_preconditions():
    """Every builder's asserts, from the oracle alone (no GPU)."""
    build_churn()
    build_order()
    build_backend_dies(False)
    build_backend_dies(True)
    for case in CUTS:
        build_cut(case)
    for kind in ("arp", "icmp"):
        build_unparsed(kind)
    build_boundary()
    build_rejuvenation()
    build_last_backend()
    build_options()
    for table in ("flows", "backends"):
        for path in ("one", "burst"):
            build_ring(table, path)
        build_tombs(table)
    build_sizes()
    build_between()


def run(lb, o, r, a, b, as_burst):
    """Packets [a, b) of r: one call, or packet by packet."""
    if as_burst:
        burst(lb, o, r["F"], r["ln"], r["dv"], r["now"], a, b)
    else:
        for i in range(a, b):
            one(lb, o, r["F"], r["ln"], r["dv"], r["now"], i)


def primed_pair(cfg):
    lb, o = cfg.pair()
    prime(cfg, lb, o)
    return lb, o


# ---------------------------------------------------- 1. per-packet churn --
@gpu
def test_per_packet_churn_both_tables():
    """Flows age out and backends fall silent and come back, packet by packet:
    one packet is handed to the pipeline, both tables are seeded, and every
    later expiry on either table is the kernel's."""
    r = build_churn()
    cfg, F, ln, dv, now = r["cfg"], r["F"], r["ln"], r["dv"], r["now"]
    n = F.shape[0]
    lb, o = cfg.pair()
    handed_at = None
    for i in range(n):
        one(lb, o, F, ln, dv, now, i)
        if handed_at is None and lb.serve_expiry_stats()["handed"]:
            handed_at = i
    x, s = stats(lb)
    L.check_state(lb, o)
    print("handed at", handed_at, x, s)
    assert handed_at is not None and handed_at <= r["handed_at"], (handed_at, r["handed_at"])
    pf, pb = int(r["pf"][handed_at + 1:].sum()), int(r["pb"][handed_at + 1:].sum())
    assert pf >= 20 and pb >= 20, (pf, pb)
    assert x["handed"] == 1 and x["seeds"] == 2, x
    assert x["expired"] == pf + pb, (x, pf, pb)
    assert x["walks"] == int((r["per"][handed_at + 1:] > 0).sum()), x
    assert s["packets_one"] == n - 1 and s["declined"] == 0, s


# ----------------------------------------------------- 2. order and reuse --
@gpu
def test_order_and_reuse_per_table():
    """Ten flows and six backends, rejuvenated out of allocation order, fall
    due at one packet of a served burst: the oldest stamp frees first and the
    youngest freed index is taken first, on each table (the builder reads the
    indices off the oracle; the dump shows the GPU's)."""
    r = build_order()
    cfg = r["cfg"]
    lb, o = cfg.pair()
    run(lb, o, r, 0, 1, True)
    run(lb, o, r, 1, 33, True)
    run(lb, o, r, 33, 34, True)  # backend 50 expires: the pipeline's
    x0 = lb.serve_expiry_stats()
    assert x0["handed"] == 1 and x0["expired"] == 0, x0
    run(lb, o, r, 34, 35, True)  # (launched again: both journals are seeded)
    x0, s0 = stats(lb)
    assert x0["seeds"] == 2, x0
    run(lb, o, r, 35, r["F"].shape[0], True)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["expired"] == 17 and d["walks"] == 1 and d["handed"] == 0 and d["seeds"] == 0, d
    assert d["burst_packets"] == r["F"].shape[0] - 35 and d["declined"] == 0 and d["splits"] == 0, d


# --------------------------------- 3, 4. a backend expires under its flows --
@gpu
@pytest.mark.parametrize("as_burst", [False, True])
@pytest.mark.parametrize("new_address", [False, True])
def test_backend_expires_under_its_flows(new_address, as_burst):
    """The backend of flow 1 falls due at lane 4 of the last call: the lanes
    below go to it, the lanes behind to the CHT's choice among the living --
    or, when lane 4 is a heartbeat from a new address that takes the dead
    backend's index, to that new backend."""
    r = build_backend_dies(new_address)
    lb, o = primed_pair(r["cfg"])
    a, n = r["a"], r["F"].shape[0]
    run(lb, o, r, 0, 3, True)
    run(lb, o, r, 3, a, False)
    x0, s0 = stats(lb)
    run(lb, o, r, a, n, as_burst)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["expired"] == 1 and d["walks"] == 1 and d["handed"] == 0 and d["seeds"] == 0, d
    assert d["declined"] == 0 and d["packets_one"] + d["burst_packets"] == n - a, d
    assert d["splits"] == (1 if as_burst else 0) and d["bursts"] == (2 if as_burst else 0), d


# ------------------------------------------------------------------ 5. cuts --
@gpu
@pytest.mark.parametrize("case", CUTS)
def test_cuts(case):
    """A call of eight cut by a flow alone, by a backend alone, by both at one
    lane, and by each at a lane of its own: as many requests more as there are
    lanes above a request's first at which the reference expires."""
    r = build_cut(case)
    lb, o = primed_pair(r["cfg"])
    a = r["a"]
    run(lb, o, r, 0, a, False)
    x0, s0 = stats(lb)
    run(lb, o, r, a, a + 8, True)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["splits"] == r["splits"] and d["bursts"] == r["splits"] + 1, (case, d)
    assert d["expired"] == int(r["per"][a:].sum()) and d["walks"] == r["splits"], (case, d)
    assert d["burst_packets"] == 8 and d["declined"] == 0 and d["handed"] == 0, (case, d)


# ------------------------------------------ 6. a lane that does not parse --
@gpu
@pytest.mark.parametrize("as_burst", [False, True])
@pytest.mark.parametrize("kind", ["arp", "icmp"])
def test_unparsed_frame_expires_and_cuts(kind, as_burst):
    """lb_main.c:21-22 precede the parse: an ARP-sized frame and an ICMP packet
    expire the backend that falls due at them, alone and as lane 1 of a burst,
    which they cut."""
    r = build_unparsed(kind)
    lb, o = primed_pair(r["cfg"])
    run(lb, o, r, 0, 3, False)
    x0, s0 = stats(lb)
    if as_burst:
        run(lb, o, r, 3, 6, True)
    else:
        run(lb, o, r, 3, 4, False)
        x1 = lb.serve_expiry_stats()
        assert x1["expired"] == x0["expired"], (x0, x1)
        run(lb, o, r, 4, 5, False)
        x2 = lb.serve_expiry_stats()
        assert x2["expired"] == x1["expired"] + 1 and x2["walks"] == x1["walks"] + 1, (x1, x2)
        run(lb, o, r, 5, 6, False)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["expired"] == 1 and d["handed"] == 0 and d["declined"] == 0, d
    assert d["splits"] == (1 if as_burst else 0) and d["packets_one"] + d["burst_packets"] == 3, d


# ----------------------------------------------------------- 7. boundary --
@gpu
@pytest.mark.parametrize("as_burst", [False, True])
def test_boundary_per_table(as_burst):
    """A stamp equal to the cutoff survives (ts < cutoff is the test) and goes
    one nanosecond later, the backend on 700 us and the flow on 1000 us."""
    r = build_boundary()
    lb, o = primed_pair(r["cfg"])
    run(lb, o, r, 0, 3, False)
    x0, s0 = stats(lb)
    if as_burst:
        run(lb, o, r, 3, 7, True)
    else:
        for i in range(3, 7):
            xa = lb.serve_expiry_stats()
            run(lb, o, r, i, i + 1, False)
            xb = lb.serve_expiry_stats()
            assert xb["expired"] == xa["expired"] + int(r["per"][i]), (i, xa, xb)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["expired"] == 2 and d["handed"] == 0 and d["seeds"] == 0 and d["declined"] == 0, d
    assert d["splits"] == (2 if as_burst else 0), d


# -------------------------------------------------------- 8. rejuvenation --
@gpu
def test_rejuvenation():
    """A heartbeat keeps its backend; a WAN hit keeps its flow and not its
    backend; a re-pointed flow is stamped."""
    r = build_rejuvenation()
    lb, o = primed_pair(r["cfg"])
    x0, s0 = stats(lb)
    run(lb, o, r, 0, r["F"].shape[0], False)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["expired"] == int(r["per"].sum()) and d["handed"] == 0 and d["seeds"] == 0, d
    assert d["packets_one"] == r["F"].shape[0] and d["declined"] == 0, d


# ------------------------------------------------- 9. the last backend goes --
@gpu
@pytest.mark.parametrize("as_burst", [False, True])
def test_last_backend_expires_inside_the_kernel(as_burst):
    """The walk takes the last backend: a WAN miss behind it leaves on the WAN
    device with nothing written; a stale hit is declined behind the walk and
    erased by the pipeline, which drops both journals; the next due expiry is
    handed over once and both are seeded again."""
    r = build_last_backend()
    lb, o = primed_pair(r["cfg"])
    run(lb, o, r, 0, 2, False)
    x0, s0 = stats(lb)
    if as_burst:
        run(lb, o, r, 2, 5, True)  # [NP | W(5), W(1)]: cut, walk, declined behind it
        d = delta(lb, x0, s0)
        assert d["splits"] == 1 and d["burst_packets"] == 1 and d["bursts"] == 1, d
    else:
        run(lb, o, r, 2, 4, False)
        d = delta(lb, x0, s0)
        assert d["expired"] == 1 and d["packets_one"] == 2 and d["declined"] == 0, d
        run(lb, o, r, 4, 5, False)
        d = delta(lb, x0, s0)
        assert d["packets_one"] == 2, d
    assert d["expired"] == 1 and d["walks"] == 1 and d["declined"] == 1, d
    assert d["handed"] == 0 and d["seeds"] == 0, d
    L.check_state(lb, o)
    run(lb, o, r, 5, 7, False)   # served, the journals off
    d = delta(lb, x0, s0)
    assert d["handed"] == 0 and d["seeds"] == 0 and d["expired"] == 1, d
    run(lb, o, r, 7, 8, False)   # backend 2 is due: the pipeline's, once
    d = delta(lb, x0, s0)
    assert d["handed"] == 1 and d["seeds"] == 0, d
    run(lb, o, r, 8, 10, False)  # seeded again, both
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["handed"] == 1 and d["seeds"] == 2 and d["declined"] == 1 and d["expired"] == 1, d


# ------------------------------------------------------ 10. IPv4 options --
@gpu
def test_options_burst_with_expiries_due():
    """A burst with an IPv4-options frame is declined before the walk: the
    pipeline expires and serves it, the counters show no walk."""
    r = build_options()
    lb, o = primed_pair(r["cfg"])
    run(lb, o, r, 0, 3, False)
    x0, s0 = stats(lb)
    run(lb, o, r, 3, 7, True)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d["declined"] == 1 and d["expired"] == 0 and d["walks"] == 0 and d["splits"] == 0, d
    assert d["burst_packets"] == 0 and d["bursts"] == 0, d


# ------------------------------------------------------ children (11, 16) --
def body_ring(table, path):
    r = build_ring(table, path)
    cfg, m, n = r["cfg"], r["m"], r["F"].shape[0]
    lb, o = primed_pair(cfg)
    x0 = lb.serve_expiry_stats()
    if path == "one":
        run(lb, o, r, 0, n, False)
    else:
        run(lb, o, r, 0, 3, True)
        for a in range(3, 3 + m, 60):
            run(lb, o, r, a, min(a + 60, 3 + m), True)
        run(lb, o, r, 3 + m, n, True)
    L.check_state(lb, o)
    st = dict(lb.serve_expiry_stats(), **lb.serve_stats())
    st["want"] = x0["expired"] + int(r["per"].sum())
    return st


def body_off(_a, _b):
    cfg = STD
    lb, o = cfg.pair()
    F, ln, dv, now = churn_trace(360, 11)
    r = dict(F=F, ln=ln, dv=dv, now=now)
    run(lb, o, r, 0, 120, False)
    for a in range(120, 360, 40):
        run(lb, o, r, a, a + 40, True)
    L.check_state(lb, o)
    return dict(lb.serve_expiry_stats(), **lb.serve_stats())


CHILD = r"""
import json, sys
import test_serve_expiry_lb_gpu as X
print("STATS " + json.dumps(getattr(X, "body_" + sys.argv[1])(sys.argv[2], sys.argv[3])))
"""


def run_child(body, a, b, **env_add):
    """A body in a fresh process (the switches are read once per process)."""
    env = dict(os.environ, **env_add)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", CHILD, body, a, b], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("STATS ")][-1][6:])


# ---------------------------------------------------------- 11. ring full --
@gpu
@pytest.mark.parametrize("path", ["one", "burst"])
@pytest.mark.parametrize("table", ["flows", "backends"])
def test_ring_full(table, path):
    """VIGPATH_SERVE_JOURNAL=2: one table's ring fills, nothing of the refused
    request is done, both journals are seeded again and the same request
    served; then the idle entries' expiry, still the kernel's. The child checks
    every port, every frame and the state."""
    st = run_child("ring", table, path, VIGPATH_SERVE_JOURNAL="2")
    print(table, path, st)
    assert st["seeds"] >= 6 and st["seeds"] % 2 == 0 and st["handed"] == 1, st
    assert st["expired"] == st["want"] and st["declined"] == 0, st


# --------------------------------------------------------- 12. tombstones --
@gpu
@pytest.mark.parametrize("table", ["flows", "backends"])
def test_tombstones_purged_while_served(table):
    """64 indices of one table under churn until erased and live entries pass
    the purge bound: the kernel reports it, the host checks both tables and
    rebuilds that one (vp_table_stats_get), and launches the kernel again; the
    journals survive and nothing takes the pipeline."""
    cfg = TOMB[table]
    ti = 0 if table == "flows" else 1
    lb, o = cfg.pair()
    t = prime(cfg, lb, o) + 10
    x0, r0 = lb.serve_expiry_stats(), lb.table_stats(ti)["rebuilds"]
    k0, rose = 1000, False
    for _ in range(60):
        F, ln, dv, now = tomb_burst(table, k0, t)
        burst(lb, o, F, ln, dv, now, 0, 64)
        k0, t = k0 + 64, int(now[-1]) + 350
        rose = lb.table_stats(ti)["rebuilds"] > r0
        if rose:
            break
    x, s = stats(lb)
    print(table, "entries sent", k0 - 1000, x, s, lb.table_stats(ti))
    assert rose, "the purge bound was never passed"
    F, ln, dv, now = tomb_burst(table, k0 - 8, t)  # hits on the entries it moved among them
    burst(lb, o, F, ln, dv, now, 0, 64)
    L.check_state(lb, o)
    x1, s1 = stats(lb)
    assert x1["handed"] == x0["handed"] and x1["seeds"] == x0["seeds"], (x0, x1)
    assert x1["expired"] > x["expired"], (x, x1)
    assert s1["burst_packets"] == s["burst_packets"] + 64 and s1["declined"] == 0, (s, s1)


# -------------------------------------------------- 13. pipeline in between --
@gpu
def test_pipeline_in_between():
    """A dump keeps the journals; a call of 129 through the pipeline drops
    both: the next due expiry is handed over once more and both are seeded
    again."""
    r = build_between()
    per = r["per"]
    lb, o = primed_pair(r["cfg"])
    x0, s0 = stats(lb)
    run(lb, o, r, 0, 60, True)
    L.check_state(lb, o)  # a dump: the kernel stops, the journals stay
    run(lb, o, r, 60, 120, True)
    d = delta(lb, x0, s0)
    assert d["expired"] == int(per[:120].sum()) and d["handed"] == 0 and d["seeds"] == 0, d
    run(lb, o, r, 120, 249, True)  # above the routing limit: the pipeline's
    d1 = delta(lb, x0, s0)
    assert d1["burst_packets"] == d["burst_packets"] == 120 and d1["expired"] == d["expired"], d1
    assert d1["handed"] == 0, d1
    for a in range(249, 489, 60):
        run(lb, o, r, a, a + 60, True)
    d2 = delta(lb, x0, s0)
    L.check_state(lb, o)
    assert d2["handed"] == 1 and d2["seeds"] == 2 and d2["declined"] == 0, d2
    assert d2["expired"] > d1["expired"], (d1, d2)


# ---------------------------------------------- 14. call sizes across churn --
@gpu
def test_call_sizes_across_churn():
    """The churn trace in calls of 1, 2, 31, 32, 33, 64, 67 and 128: all
    served, cut where entries expire, nothing handed over."""
    r = build_sizes()
    lb, o = primed_pair(r["cfg"])
    x0, s0 = stats(lb)
    for a, b in r["calls"]:
        run(lb, o, r, a, b, True)
    d = delta(lb, x0, s0)
    L.check_state(lb, o)
    print(d)
    n = r["F"].shape[0]
    assert d["handed"] == 0 and d["seeds"] == 0 and d["declined"] == 0, d
    assert d["burst_packets"] == n and d["expired"] == int(r["per"].sum()), d
    assert d["splits"] >= sum(splits_of(r["per"], a, b) for a, b in r["calls"]), d


# ---------------------------------------------------------- 15. switch off --
@gpu
def test_switch_off_in_child():
    """VIGPATH_SERVE_EXPIRE=0: the same ports, frames and state (checked in
    the child against the oracle), no journal, no walk: every due expiry goes
    through the pipeline (`handed` counts those requests, as for the other
    NFs)."""
    st = run_child("off", "-", "-", VIGPATH_SERVE_EXPIRE="0")
    assert st["expired"] == 0 and st["seeds"] == 0 and st["walks"] == 0 and st["splits"] == 0, st
    assert st["handed"] > 1, st
