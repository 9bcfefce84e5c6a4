"""The seeded cases that pin the restated libVig and the oracle glue against
the reference's own libVig (tests/test_oracle.py, parts 2 and 3).

Each case builds its random input from its parameters, runs it through one
build of the oracle library (orc.lib(ref)) and returns its answers as a list
of arrays in a canonical form: fields the reference leaves undefined (time
stamps and values of unallocated indices) are zeroed, and processed frames are
returned as their XOR with the input frames (the bytes the NF rewrote).

tests/golden/make_ref_golden.py runs every case over the reference's libVig
(ref=True) and stores the answers in tests/golden/ref_libvig.npz; the tests
run the same cases over the restatement and compare with the stored answers.
"""
import os

import numpy as np

import orc
from tracegen import (edge_lb_trace, mixed_fw_trace, mixed_nat_trace, mixed_pol_trace,
                      wide_lb_trace)
from vigor_amd import traces as T

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "ref_libvig.npz")

DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01")]
DEV3_MACS = DEV_MACS + [T.mac("22:23:24:25:26:27")]
END3_MACS = END_MACS + [T.mac("01:23:45:67:89:02")]


def _live(alloc, *fields):
    """`fields` with the rows of unallocated indices zeroed."""
    live = alloc == 1
    return [np.where(live.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(a.dtype)
            for a in fields]


def crc(ref):
    rng = np.random.default_rng(1)
    L = orc.lib(ref)
    c = [L.orc_crc32c_u32(*(int(x) for x in rng.integers(0, 2**32, 2, dtype=np.uint64)))
         for _ in range(2000)]
    e = [L.orc_ether_hash(bytes(rng.integers(0, 256, 6, dtype=np.uint8)))
         for _ in range(200)]
    return [np.array(c, np.uint32), np.array(e, np.uint32)]


def _rand_dchain_ops(rng, range_, n):
    op = rng.integers(0, 5, n).astype(np.int32)
    arg = rng.integers(-1, range_ + 1, n).astype(np.int32)
    arg = np.clip(arg, 0, range_ - 1).astype(np.int32)
    t = np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    # expiry cut-offs a little behind "now"
    t = np.where(op == 2, t - rng.integers(0, 20, n), t).astype(np.int64)
    return op, arg, t


def dchain(ref, seed):
    rng = np.random.default_rng(seed)
    range_ = int(rng.choice([1, 2, 5, 64, 300]))
    op, arg, t = _rand_dchain_ops(rng, range_, 3000)
    L = orc.lib(ref)
    n = op.shape[0]
    res = np.zeros(n, np.int32)
    ao = np.zeros(range_, np.int32)
    fo = np.zeros(range_, np.int32)
    na = np.zeros(1, np.int32)
    nf = np.zeros(1, np.int32)
    ts = np.zeros(range_, np.int64)
    P = orc._ptr
    assert L.orc_test_dchain(range_, n, P(op), P(arg), P(t), P(res), P(ao),
                             P(na), P(fo), P(nf), P(ts))
    ao, fo = ao[:na[0]], fo[:nf[0]]
    # the reference mallocs timestamps uninitialised (double-chain.c:113-157):
    # only stamps of allocated indices are defined
    return [res, ao, fo, ts[ao]]


def map_(ref, seed):
    rng = np.random.default_rng(100 + seed)
    cap = int(rng.choice([8, 64, 1024]))
    hmod = int(rng.choice([1, 3, 7, 1000003]))
    live = {}
    free = list(range(cap))
    ops, keys, vals = [], [], []
    for _ in range(4000):
        r = rng.random()
        if r < 0.4 and free:
            k = int(rng.integers(0, 50 * cap))
            if k in live:
                continue
            s = free.pop(int(rng.integers(0, len(free))))
            live[k] = s
            ops.append(0), keys.append(k), vals.append(s)
        elif r < 0.7 and live:
            k = list(live)[int(rng.integers(0, len(live)))]
            s = live.pop(k)
            free.append(s)
            ops.append(2), keys.append(k), vals.append(s)
        else:
            k = int(rng.integers(0, 50 * cap)) if rng.random() < .5 or not live \
                else list(live)[int(rng.integers(0, len(live)))]
            ops.append(1), keys.append(k), vals.append(0)
    op = np.array(ops, np.int32)
    key = np.array(keys, np.uint32)
    val = np.array(vals, np.int32)
    res = np.zeros(op.shape[0], np.int32)
    P = orc._ptr
    assert orc.lib(ref).orc_test_map(cap, hmod, op.shape[0], P(op), P(key),
                                     P(val), P(res))
    return [res]


def cht(ref, height, cap):
    rng = np.random.default_rng(height)
    active = (rng.random(cap) < 0.6).astype(np.uint8)
    hashes = rng.integers(0, 2**63, 500, dtype=np.uint64)
    tab = np.zeros(height * cap, np.uint32)
    ch = np.zeros(500, np.int32)
    P = orc._ptr
    assert orc.lib(ref).orc_test_cht(height, cap, P(tab), P(active), 500,
                                     P(hashes), P(ch))
    return [tab, ch]


def nat_trace(ref, seed, max_flows, expire_us, n_flows):
    rng = np.random.default_rng(seed)
    fr, ln, dv, now = mixed_nat_trace(rng, 5000, n_flows, max_idx=max_flows)
    cfg = orc.nat_cfg(wan=1, ext_ip=T.ip4(192, 168, 4, 2),
                      expire_us=expire_us, max_flows=max_flows,
                      device_macs=DEV_MACS, endpoint_macs=END_MACS)
    o = orc.Oracle("nat", cfg, ref=ref)
    f = fr.copy()
    out = o.run(f, ln, dv, now, 64)
    alloc, ts, keys = o.nat_dump(max_flows)
    return [out, f ^ fr, alloc, *_live(alloc, ts), keys]


def bridge_trace(ref, seed, cap, expire_us):
    rng = np.random.default_rng(seed)
    n = 4000
    fr, ln, dv, now = T.bridge_trace(n, 100)
    f2 = fr.reshape(n, 64)
    f2[:, 11] = rng.integers(0, 40, n)  # fewer stations, random mixes
    f2[:, 5] = rng.integers(0, 40, n)
    dv = rng.integers(0, 3, n).astype(np.uint16)
    now = T.NOW0 + np.cumsum(rng.integers(0, 4, n)).astype(np.int64)
    statics = [(bytes([2, 0, 0, 0, 0, 7]), 0, 2), (bytes([2, 0, 0, 0, 0, 9]),
                                                   1, -2)]
    cfg = orc.BridgeCfg(expiration_time=expire_us, dyn_capacity=cap,
                        n_devices=3)
    o = orc.Oracle("bridge", cfg, ref=ref, statics=statics)
    f = fr.copy()
    out = o.run(f, ln, dv, now, 64)
    alloc, ts, macs, port = o.bridge_dump(cap)
    return [out, f ^ fr, alloc, *_live(alloc, ts), macs, port]


def lb_cfg(flow_cap=1024, bcap=32, height=97, fexp=60_000_000, bexp=3_600_000):
    c = orc.LbCfg(flow_capacity=flow_cap, flow_expiration_time=fexp,
                  backend_capacity=bcap, cht_height=height,
                  backend_expiration_time=bexp, wan_device=2, n_devices=3)
    for d in range(3):
        for i in range(6):
            c.device_macs[d][i] = 0x10 * d + i
    return c


def lb_trace(ref, seed, fexp, bexp):
    rng = np.random.default_rng(seed)
    hb = T.lb_heartbeats(20)
    tr = T.lb_traffic(3000, 500, order="uniform", seed=seed)
    fr = np.concatenate([hb[0], tr[0]])
    ln = np.concatenate([hb[1], tr[1]])
    dv = np.concatenate([hb[2], tr[2]])
    # interleave some more heartbeats inside the traffic
    dv = dv.copy()
    k = rng.random(dv.shape[0]) < 0.05
    dv[k] = rng.integers(0, 2, k.sum())
    now = T.NOW0 + np.cumsum(rng.integers(0, 3, dv.shape[0])).astype(np.int64)
    o = orc.Oracle("lb", lb_cfg(fexp=fexp, bexp=bexp), ref=ref)
    f = fr.copy()
    out = o.run(f, ln, dv, now, 64)
    res = [out, f ^ fr]
    for x in o.lb_dump(1024, 32):  # flows, then backends: live entries only
        res += [x[0], *_live(x[0], *x[1:])]
    return res


def lb_shape_trace(ref, shape, seed, fexp, bexp):
    """viglb over 256-byte slots: wide_lb_trace (payload bytes under the L4
    sum, odd and padded lengths) or edge_lb_trace (options, short frames,
    total_length edges; WAN packets and heartbeats alike)."""
    rng = np.random.default_rng(seed)
    slot = 256
    if shape == "wide":
        fr, ln, dv, now = wide_lb_trace(rng, 3000, 200, 12, slot, max_len=slot)
    else:
        fr, ln, dv, now = edge_lb_trace(rng, 3000, 100, 12, slot, long_frames=True)
    now = T.NOW0 + (now - T.NOW0) * 10  # (2 us: some 200 packets)
    o = orc.Oracle("lb", lb_cfg(fexp=fexp, bexp=bexp), ref=ref)
    f = fr.copy()
    out = o.run(f, ln, dv, now, slot)
    res = [out, f ^ fr]
    for x in o.lb_dump(1024, 32):
        res += [x[0], *_live(x[0], *x[1:])]
    return res


def fw_oracle(ref, max_flows=64, expire_us=60_000_000, n_dev=3, wan=1):
    cfg = orc.fw_cfg(wan=wan, expire_us=expire_us, max_flows=max_flows,
                     device_macs=DEV3_MACS[:n_dev], endpoint_macs=END3_MACS[:n_dev],
                     n_devices=n_dev)
    return orc.Oracle("fw", cfg, ref=ref)


def fw_trace(ref, seed, max_flows, expire_us, n_flows):
    rng = np.random.default_rng(seed)
    fr, ln, dv, now = mixed_fw_trace(rng, 5000, n_flows)
    o = fw_oracle(ref, max_flows=max_flows, expire_us=expire_us)
    f = fr.copy()
    out = o.run(f, ln, dv, now, 64)
    alloc, ts, keys, dev = o.fw_dump(max_flows)
    return [out, f ^ fr, alloc, *_live(alloc, ts), keys, dev]


def pol_oracle(ref, cap=64, rate=1_000_000, burst=1000, n_dev=3, lan=1, wan=0):
    return orc.Oracle("pol", orc.pol_cfg(lan=lan, wan=wan, rate=rate, burst=burst,
                                         capacity=cap, n_devices=n_dev), ref=ref)


def pol_trace(ref, seed, cap, n_dsts, burst, gap):
    rng = np.random.default_rng(seed)
    fr, ln, dv, now = mixed_pol_trace(rng, 6000, n_dsts, gap_ns=gap)
    o = pol_oracle(ref, cap=cap, burst=burst)
    f = fr.copy()
    out = o.run(f, ln, dv, now, 64)
    alloc, ts, *vals = o.pol_dump(cap)
    return [out, f ^ fr, alloc, *_live(alloc, ts), *vals]


# every case of tests/test_oracle.py parts 2 and 3: name -> (function, [parameters])
CASES = {
    "crc": (crc, [()]),
    "dchain": (dchain, [(s,) for s in range(6)]),
    "map": (map_, [(s,) for s in range(6)]),
    "cht": (cht, [(97, 32), (257, 256), (7, 4), (13, 1), (521, 512)]),
    "nat": (nat_trace, [(0, 64, 60_000_000, 40), (1, 64, 1, 100),
                        (2, 16, 60_000_000, 40), (3, 256, 5, 300)]),
    "bridge": (bridge_trace, [(0, 64, 300_000_000), (1, 16, 2), (2, 1024, 10)]),
    "lb": (lb_trace, [(0, 60_000_000, 3_600_000_000), (1, 3, 50), (2, 20, 2)]),
    "lb_shape": (lb_shape_trace, [("wide", 10, 2, 3_600_000), ("edge", 11, 60_000_000, 2)]),
    "fw": (fw_trace, [(0, 64, 60_000_000, 40), (1, 64, 1, 100),
                      (2, 16, 60_000_000, 40), (3, 256, 5, 300)]),
    "pol": (pol_trace, [(0, 64, 40, 3000, 500), (1, 16, 60, 1000, 2000),
                        (2, 256, 300, 2000, 50), (3, 64, 20, 1000, 10)]),
}


def key(name, params, i):
    return "%s/%s/%d" % (name, "-".join(str(p) for p in params), i)


_fixture = {}


def reference(name, params):
    """The reference libVig's answers to a case (tests/golden/ref_libvig.npz)."""
    if not _fixture:
        with np.load(FIXTURE, allow_pickle=False) as z:
            _fixture.update({k: z[k] for k in z.files})
    out = []
    while key(name, params, len(out)) in _fixture:
        out.append(_fixture[key(name, params, len(out))])
    assert out, "no stored answers for %s %r" % (name, params)
    return out


def check(name, *params):
    """Run a case over the restatement; its answers equal the reference's.
    Returns the restatement's answers."""
    got = CASES[name][0](False, *params)
    want = reference(name, params)
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert x.dtype == y.dtype, (name, params, i)
        np.testing.assert_array_equal(x, y, err_msg="%s %r answer %d" % (name, params, i))
    return got
