"""The checksum-edge cases shared by tests/test_cksum_edges.py (the oracle
alone, CPU) and tests/test_cksum_edges_gpu.py (the HIP paths against it): one
case per NF, slot size and code path, each a trace whose rewritten frames land
on the values at which the checksum arithmetic branches (tracegen.EDGES), and
a census of the oracle's output that says how many frames really did.
"""
import functools

import numpy as np

import oracle_cases as OC
import orc
from tracegen import EDGES, cksum_edge_frames, lb_cksum_batch, nat_cksum_trace
from vigor_amd import traces as T

MIN_FRAMES = 32  # of every edge, in every case's oracle output
WAN_LB = 2

# name -> (slot, max_flows, packets, flows, nat_cksum_trace's keywords)
NAT_CASES = {
    # slot 64, LAN only, no malformed frame: every tile lean
    "tile64_lean": (64, 1024, 4608, 600, {}),
    # WAN replies and one malformed frame in every tile: the per-lane path
    "tile64_lanes": (64, 1024, 4608, 600, dict(wan_frac=0.3, bad_tiles=1.0)),
    # wide tiles: the spare word below byte 64 or in the tail sum
    "wide256": (256, 1024, 3000, 300, dict(max_len=256, wan_frac=0.2)),
    "wide1536": (1536, 1024, 3000, 300, dict(max_len=1518, wan_frac=0.2)),
    # IHL 6: set_checksums over options (64-byte slots: from inside the tile
    # kernel; 128: nat_classify's byte path)
    "options64": (64, 1024, 3000, 300, dict(ihl6_frac=0.6, only_ihl6=True)),
    "options128": (128, 1024, 3000, 300, dict(max_len=124, ihl6_frac=0.6, only_ihl6=True)),
    # mbuf header slots: frames past 64 bytes, every spare word in the tail
    "mbuf": (2048, 1024, 3000, 300, dict(max_len=1518, min_len=90, wan_frac=0.2, past64=1.0)),
    # the resident kernel: a packet at a time, and bursts of 32
    "serve_one": (64, 64, 384, 40, dict(wan_frac=0.2)),
    "serve_burst": (64, 64, 384, 40, dict(wan_frac=0.2)),
}

# name -> (slot, backend capacity, CHT height, backends, flows, max_len)
LB_CASES = {
    "tile64": (64, 32, 97, 20, 1024, 60),          # backends staged in LDS
    "tile64_bcap512": (64, 512, 521, 400, 1024, 60),  # lb_rewrite_fast
    "wide256": (256, 32, 97, 20, 1024, 256),       # lb_classify
}
LB_FLOW_CAP = 2048
LB_BEXP_US = 1000


def nat_oracle(max_flows):
    cfg = orc.nat_cfg(wan=1, start_port=0, ext_ip=T.ip4(192, 168, 4, 2),
                      expire_us=60_000_000, max_flows=max_flows,
                      device_macs=OC.DEV_MACS, endpoint_macs=OC.END_MACS, n_devices=2)
    return orc.Oracle("nat", cfg)


def lb_oracle(bcap, height):
    return orc.Oracle("lb", OC.lb_cfg(flow_cap=LB_FLOW_CAP, bcap=bcap, height=height,
                                      bexp=LB_BEXP_US))


def zero_past_len(fr, ln, slot):
    f = fr.reshape(-1, slot)
    for i in np.nonzero(ln < slot)[0]:
        f[i, ln[i]:] = 0
    return fr


@functools.lru_cache(maxsize=None)
def nat_case(name):
    """The patched trace of a vignat case and the oracle's answer to it:
    dict(fr, ln, dv, now, slot, max_flows, labels, exp, exp_out). The arrays
    are shared between tests: copy before changing one."""
    slot, max_flows, n, n_flows, kw = NAT_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    (fr, ln, dv, now), labels, at = nat_cksum_trace(rng, n, n_flows, slot, **kw)
    if name.startswith(("mbuf", "serve")):  # a frame is its buffer of len bytes
        zero_past_len(fr, ln, slot)
    fr = cksum_edge_frames(lambda: nat_oracle(max_flows), fr, ln, dv, now, slot, labels, at)
    exp = fr.copy()
    exp_out = nat_oracle(max_flows).run(exp, ln, dv, now, slot)
    for a in (fr, ln, dv, now, labels, exp, exp_out):
        a.setflags(write=False)
    return dict(fr=fr, ln=ln, dv=dv, now=now, slot=slot, max_flows=max_flows, labels=labels,
                at=at, exp=exp, exp_out=exp_out, forwarded=exp_out != dv)


@functools.lru_cache(maxsize=None)
def lb_case(name):
    """A viglb case: heartbeats, the edge batch three times (first
    sightings; hits; after the backends expired and fewer came back, stale
    flows and hits), each position patched for the rewrite it gets there.
    `cuts`: the segments' bounds."""
    slot, bcap, height, nb, ne, max_len = LB_CASES[name]
    rng = np.random.default_rng(sum(name.encode()))
    (ef, el, ed), elab, eat = lb_cksum_batch(rng, ne, slot, max_len=max_len)
    hb = T.lb_heartbeats(nb, slot=slot)
    t3 = T.NOW0 + 5 * LB_BEXP_US * 1000
    hb2 = T.lb_heartbeats(nb // 3, slot=slot, t0=t3)
    step = np.arange(ne, dtype=np.int64)
    segs = [hb, (ef, el, ed, T.NOW0 + step), (ef, el, ed, T.NOW0 + 10_000 + step), hb2,
            (ef, el, ed, t3 + 1000 + step)]
    fr, ln, dv, now = (np.concatenate(x) for x in zip(*segs))
    none = lambda m: np.full(m, -1, np.int64)  # noqa: E731
    labels = np.concatenate([none(nb), elab, elab, none(nb // 3), elab])
    at = np.concatenate([none(nb), eat, eat, none(nb // 3), eat])
    cuts = list(np.cumsum([len(s[1]) for s in segs])[:-1])
    fr = cksum_edge_frames(lambda: lb_oracle(bcap, height), fr, ln, dv, now, slot, labels, at)
    exp = fr.copy()
    o = lb_oracle(bcap, height)
    exp_out = o.run(exp, ln, dv, now, slot)
    for a in (fr, ln, dv, now, labels, exp, exp_out):
        a.setflags(write=False)
    return dict(fr=fr, ln=ln, dv=dv, now=now, slot=slot, bcap=bcap, height=height,
                labels=labels, at=at, exp=exp, exp_out=exp_out, cuts=cuts,
                forwarded=(dv == WAN_LB) & (exp_out != WAN_LB))


def lb_reassigned(case):
    """How many flows of a viglb case go to another backend address in the
    third feeding of the edge batch than in the second (stale flows, and
    flows whose backend index another backend took)."""
    E = case["exp"].reshape(-1, case["slot"])
    b = [0] + [int(x) for x in case["cuts"]] + [E.shape[0]]
    return int((E[b[2]:b[3], 30:34] != E[b[4]:b[5], 30:34]).any(axis=1).sum())


def raw32(f, l4):
    """__rte_raw_cksum's 32-bit sum before any fold, restated: the L4 bytes
    [l4, l4 + total_length - 20) of a rewritten frame as little-endian words
    (an odd last byte as a low byte), the stored checksum counted as zero."""
    b = f[l4:l4 + ((int(f[16]) << 8) | int(f[17])) - 20].astype(np.int64)
    if b.size & 1:
        b = np.append(b, 0)
    c = 16 if f[23] == 6 else 6
    return int((b[0::2] | (b[1::2] << 8)).sum()) - int(b[c] | (b[c + 1] << 8))


TARGET = {"l4_zero": ("l4", 0xFFFF), "l4_0001": ("l4", 1), "l4_fffe": ("l4", 0xFFFE),
          "ip_zero": ("ip", 0), "ip_0001": ("ip", 1), "ip_fffe": ("ip", 0xFFFE)}


def census(case, lo=0, hi=None):
    """How many forwarded frames of packets [lo, hi) of the oracle's output
    sit on each edge, and the labelled frames that are not where their label
    says (dropped, or another value): ({edge: count}, [packet, ...])."""
    slot = case["slot"]
    E = case["exp"].reshape(-1, slot)
    hi = E.shape[0] if hi is None else hi
    cnt = dict.fromkeys(["l4_zero_udp", "l4_zero_tcp", "l4_0001", "l4_fffe", "ip_zero",
                         "ip_0001", "ip_fffe", "fold2", "ip_fold2"], 0)
    missed = []
    for i in range(lo, hi):
        lab = case["labels"][i]
        if not case["forwarded"][i]:
            if lab >= 0:
                missed.append(i)
            continue
        f = E[i]
        l4 = 14 + 4 * (int(f[14]) & 15)
        o = l4 + (16 if f[23] == 6 else 6)
        # (host-order words, as the code stores them)
        val = {"l4": int(f[o]) | (int(f[o + 1]) << 8), "ip": int(f[24]) | (int(f[25]) << 8)}
        s = raw32(f, l4)
        carry = (s >> 16) + (s & 0xFFFF) >= 0x10000
        if val["l4"] == 0xFFFF:
            cnt["l4_zero_tcp" if f[23] == 6 else "l4_zero_udp"] += 1
        for edge, (which, v) in TARGET.items():
            if edge != "l4_zero" and val[which] == v:
                cnt[edge] += 1
        cnt["fold2"] += carry
        h = f[14:34].astype(np.int64)  # the header's raw sum, its checksum as zero
        hs = int((h[0::2] | (h[1::2] << 8)).sum()) - val["ip"]
        cnt["ip_fold2"] += (hs >> 16) + (hs & 0xFFFF) >= 0x10000
        if lab >= 0:
            edge = EDGES[lab]
            ok = carry if edge == "fold2" else val[TARGET[edge][0]] == TARGET[edge][1]
            if not ok:
                missed.append(i)
    return cnt, missed


def require_edges(case, lo=0, hi=None):
    """The conditions on the reference alone: at least MIN_FRAMES frames on
    every edge among packets [lo, hi) of the oracle's output, and no labelled
    frame dropped or off its edge."""
    cnt, missed = census(case, lo, hi)
    assert not missed, "labelled frames off their edge: %s" % missed[:10]
    short = {k: v for k, v in cnt.items() if v < MIN_FRAMES}
    assert not short, "too few frames on %s (all: %s)" % (short, cnt)
    return cnt
