"""Two-act traces for the state save / load tests (tests/test_state_gpu.py)
and their census from the oracle alone (tests/test_state_cases.py).

Per NF a trace of a few thousand packets from tracegen's mixed builders over
a table of 256 indices. Time advances by STEP every GROUP packets, so several
packets share a stamp, and an entry expires WINDOW packets after its last
touch: with more flows than a window's packets reach, act 1 allocates,
expires and re-allocates all the time. The cut falls with freed indices on
the stack and never-used ones left ("part"), or with the table full ("full").
Act 2 opens with traffic over a larger population: the entries last touched
in act 1 expire, new flows take the freed indices and then the never-used.
"""
import functools
import json
import os

import numpy as np

import deltacases
import orc
import stateref as SR
from tracegen import (mixed_bridge_trace, mixed_fw_trace, mixed_lb_trace, mixed_nat_trace,
                      mixed_pol_trace)
from vigor_amd import traces as T

CAP = 256
GROUP = 4        # packets per time stamp
WINDOW = 400     # packets an idle entry outlives
STEP = 4000      # ns per stamp
# every NF's expiry by variant: WINDOW packets, and twice that, which with
# "full"'s many flows keeps the table full
EXPIRE_US = {"part": STEP * WINDOW // GROUP // 1000, "full": 2 * STEP * WINDOW // GROUP // 1000}
KINDS = ("nat", "bridge", "lb", "fw", "pol")
VARIANTS = ("part", "full")
N1, N2 = 2000, 1200
# flows of act 1, of its last QUIET packets, and of act 2, by variant. "part":
# few enough that never-used indices stay, and a quiet end of act 1 in which
# more entries expire than open, so that the cut finds indices on the stack;
# "full": enough that the table is full
QUIET = 600
FLOWS = {"part": (150, 40, 420), "full": (1500, 1500, 1800)}
# the seed per case for which the oracle meets test_state_cases's conditions
SEEDS = {(k, v): 1 for k in KINDS for v in VARIANTS}
LB_BCAP = 32

DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17"),
            T.mac("22:23:24:25:26:27")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01"),
            T.mac("01:23:45:67:89:02")]


def pair_args(kind, variant="part", expire_us=None, cap=CAP):
    """make_pair's arguments in tests/test_<kind>_gpu.py for these cases
    (expire_us: another expiry than the variant's)."""
    expire_us = expire_us or EXPIRE_US[variant]
    if kind == "nat":
        return dict(max_flows=cap, expire_us=expire_us)
    if kind == "fw":
        return dict(max_flows=cap, expire_us=expire_us)
    if kind == "bridge":
        return dict(cap=cap, expire_us=expire_us)
    if kind == "pol":  # the expiry is burst / rate, at 10 bytes per us
        return dict(cap=cap, rate=10_000_000, burst=10 * expire_us)
    if kind == "lb":
        return dict(flow_cap=cap, bcap=LB_BCAP, fexp=expire_us, bexp=40 * expire_us)
    raise ValueError(kind)


def oracle(kind, **kw):
    """The oracle make_pair(**pair_args(kind, **kw)) returns beside the NF."""
    a = pair_args(kind, **kw)
    if kind == "nat":
        return orc.Oracle("nat", orc.nat_cfg(
            wan=1, start_port=0, ext_ip=T.ip4(192, 168, 4, 2), expire_us=a["expire_us"],
            max_flows=a["max_flows"], device_macs=DEV_MACS[:2], endpoint_macs=END_MACS[:2],
            n_devices=2))
    if kind == "fw":
        return orc.Oracle("fw", orc.fw_cfg(
            wan=1, expire_us=a["expire_us"], max_flows=a["max_flows"], device_macs=DEV_MACS,
            endpoint_macs=END_MACS, n_devices=3))
    if kind == "bridge":
        return orc.Oracle("bridge", orc.BridgeCfg(expiration_time=a["expire_us"],
                                                  dyn_capacity=a["cap"], n_devices=3),
                          statics=[])
    if kind == "pol":
        return orc.Oracle("pol", orc.pol_cfg(lan=1, wan=0, rate=a["rate"], burst=a["burst"],
                                             capacity=a["cap"], n_devices=3))
    c = orc.LbCfg(flow_capacity=a["flow_cap"], flow_expiration_time=a["fexp"],
                  backend_capacity=a["bcap"], cht_height=97,
                  backend_expiration_time=a["bexp"], wan_device=2, n_devices=3)
    for d in range(3):
        c.device_macs[d][:] = list(DEV_MACS[d])
    return orc.Oracle("lb", c)


def dump(kind, o, cap=CAP):
    """The oracle's dump as NF.dump() of the kind returns it."""
    if kind == "nat":
        return o.nat_dump(cap)
    if kind == "fw":
        return o.fw_dump(cap)
    if kind == "bridge":
        return o.bridge_dump(cap)
    if kind == "pol":
        return o.pol_dump(cap)
    return o.lb_dump(cap, LB_BCAP)


def flows_of(kind, d):
    """(alloc, ts, key rows) of the kind's first table in a dump."""
    t = d[0] if kind == "lb" else d
    keys = t[2].reshape(t[0].shape[0], -1)
    if kind == "bridge":
        keys = np.concatenate([keys, t[3].reshape(-1, 1).astype(np.uint8)], axis=1)
    return t[0], t[1], keys


def build(kind, rng, n, n_flows):
    if kind == "nat":
        return mixed_nat_trace(rng, n, n_flows, max_idx=CAP)
    if kind == "fw":
        return mixed_fw_trace(rng, n, n_flows)
    if kind == "bridge":
        return mixed_bridge_trace(rng, n, n_flows)
    if kind == "pol":
        return mixed_pol_trace(rng, n, n_flows, lan_frac=0.1)
    return mixed_lb_trace(rng, n, n_flows, 12, hb_frac=0.05)


def _zero_behind_len(fr, ln):
    """Slots zero behind the frame's last byte: a runt's slot then holds what
    a buffer of len bytes holds, so the entry points that take slots and the
    ones that take frames see the same packet."""
    f = fr.reshape(ln.shape[0], -1)
    f[np.arange(f.shape[1])[None, :] >= ln[:, None]] = 0
    return f.reshape(-1)


def trace(kind, variant):
    """(frames, lens, in_dev, now), the cut: acts 1 and 2 back to back."""
    rng = np.random.default_rng(SEEDS[kind, variant] * 1000 + KINDS.index(kind) * 10 +
                                VARIANTS.index(variant))
    f1, fq, f2 = FLOWS[variant]
    parts = [build(kind, rng, N1 - QUIET, f1), build(kind, rng, QUIET, fq),
             build(kind, rng, N2, f2)]
    fr, ln, dv = (np.concatenate(x) for x in list(zip(*parts))[:3])
    now = T.NOW0 + (np.arange(N1 + N2, dtype=np.int64) // GROUP) * STEP
    return (_zero_behind_len(fr, ln), ln, dv, now), N1


def distinct_trace(kind, n=600, n_flows=100, seed=5):
    """No expiry (run it with expire_us = 60 s) and one stamp per packet:
    every entry's last touch has its own time, so a dump's ts order is the
    LRU order, and the free list is the never-used tail alone."""
    rng = np.random.default_rng(seed + KINDS.index(kind))
    fr, ln, dv, _ = build(kind, rng, n, n_flows)
    return _zero_behind_len(fr, ln), ln, dv, T.NOW0 + 1000 * np.arange(n, dtype=np.int64)


def census(kind, variant):
    """What act 1, the cut and act 2 do to the first table's indices, from
    the oracle's dumps after every packet."""
    (fr, ln, dv, now), cut = trace(kind, variant)
    o = oracle(kind, variant=variant)
    n = ln.shape[0]
    frames = fr.copy().reshape(n, 64)
    out = np.zeros(n, np.uint16)
    used = np.zeros(CAP, bool)        # allocated at some time so far
    freed_once = np.zeros(CAP, bool)  # ... and freed at some time so far
    pa, pt, pk = flows_of(kind, dump(kind, o))
    pa, pk = pa.copy(), pk.copy()
    res = {}
    expired, born = np.zeros(CAP, bool), np.zeros(CAP, bool)
    for p in range(n):
        out[p:p + 1] = o.run(frames[p], ln[p:p + 1], dv[p:p + 1], now[p:p + 1], 64)
        a, ts, k = flows_of(kind, dump(kind, o))
        gone = (pa == 1) & ((a == 0) | (k != pk).any(axis=1))
        new = (a == 1) & ((pa == 0) | (k != pk).any(axis=1))
        if p < cut:
            freed_once |= gone
            used |= (a == 1)
        else:
            expired |= gone & res["live_at_cut"] & ~born
            born |= new
        pa, pk = a.copy(), k.copy()
        if p == cut - 1:
            res.update(live_at_cut=(a == 1), ts_at_cut=ts.copy(), used=used.copy(),
                       freed_before=freed_once.copy(),
                       expired_in_act1=int(freed_once.sum()))
    res.update(expired=expired, born=born, out=out, frames=frames)
    return res


# ------------------------------------------------------ rejected images --

def _edit(state, table, **fields):
    s = {"kind": state["kind"], "last_now": state["last_now"],
         "tables": [dict(t) for t in state["tables"]]}
    s["tables"][table].update(fields)
    return s


def _set(lst, j, v):
    out = list(lst)
    out[j] = v
    return out


def mutations(kind, img):
    """{name: bytes}: one fault each in an image of vignat or viglb whose first
    table has four live entries and two freed indices or more."""
    s = SR.unpack(img)
    t0 = s["tables"][0]
    cap, n, nf = t0["capacity"], len(t0["lru"]), len(t0["freed"])
    assert n >= 4 and nf >= 2
    m = {}
    m["magic"] = SR.pack(s, magic=SR.MAGIC ^ 1)
    m["version"] = SR.pack(s, version=2)
    m["kind"] = SR.pack(dict(s, kind="fw" if kind == "nat" else "nat"))
    m["capacity"] = SR.pack(_edit(s, 0, capacity=cap * 2, fresh_next=t0["fresh_next"] + cap))
    m["short_1"] = img[:-1]
    m["short_section"] = img[:len(img) - 16 * n]
    m["long"] = img + bytes(16)
    m["index_eq_capacity"] = SR.pack(_edit(s, 0, lru=[cap] + t0["lru"][1:]), canon=False)
    m["lru_and_freed"] = SR.pack(_edit(s, 0, freed=[t0["lru"][2]] + t0["freed"][1:]), canon=False)
    m["free_missing"] = SR.pack(_edit(s, 0, freed=t0["freed"][1:]), canon=False)
    m["n_live_gt_capacity"] = SR.pack(_edit(s, 0, n_live=cap + 1), canon=False)
    ts = list(t0["ts"])
    ts[1], ts[-1] = ts[-1] + 1, ts[1]
    m["ts_decreasing"] = SR.pack(_edit(s, 0, ts=ts), canon=False)
    m["ts_after_last_now"] = SR.pack(
        _edit(s, 0, ts=t0["ts"][:-1] + [s["last_now"] + 1]), canon=False)
    m["ts_negative"] = SR.pack(_edit(s, 0, ts=[-5] + t0["ts"][1:]), canon=False)
    m["key_twice"] = SR.pack(_edit(s, 0, key=[t0["key"][3]] + t0["key"][1:]), canon=False)
    m["not_normalised"] = SR.pack(
        _edit(s, 0, freed=t0["freed"] + [t0["fresh_next"]], fresh_next=t0["fresh_next"] + 1),
        canon=False)
    if 4 * n % 16:
        at = 32 + 32 + 4 * n
    else:  # (lru[] ends on a 16-byte boundary: no pad there)
        assert 4 * nf % 16, "no pad byte in the first table's index arrays"
        at = 32 + 32 + 4 * n + 4 * nf
    m["pad_byte"] = img[:at] + b"\x01" + img[at + 1:]
    # two faults in one image: the lower code is reported, wherever it stands
    m["range_0_ts_negative_2"] = SR.pack(
        _edit(s, 0, lru=_set(t0["lru"], 0, cap), ts=_set(t0["ts"], 2, -5)), canon=False)
    m["ts_negative_0_range_2"] = SR.pack(
        _edit(s, 0, lru=_set(t0["lru"], 2, cap), ts=_set(t0["ts"], 0, -5)), canon=False)
    if kind == "lb":
        t1 = s["tables"][1]
        bcap = t1["capacity"]
        m["backend_id_eq_capacity"] = SR.pack(
            _edit(s, 0, value=[bcap.to_bytes(4, "little")] + t0["value"][1:]), canon=False)
        m["backends_capacity"] = SR.pack(
            _edit(s, 1, capacity=bcap * 2, fresh_next=t1["fresh_next"] + bcap))
        m["backends_index"] = SR.pack(_edit(s, 1, lru=[bcap] + t1["lru"][1:]), canon=False)
        m["one_table"] = SR.pack(dict(s, tables=s["tables"][:1]))
    for name, blob in m.items():
        assert blob != img, name
    return m


MUTATIONS = ["magic", "version", "kind", "capacity", "short_1", "short_section", "long",
             "index_eq_capacity", "lru_and_freed", "free_missing", "n_live_gt_capacity",
             "ts_decreasing", "ts_after_last_now", "ts_negative", "key_twice", "not_normalised",
             "pad_byte"]
DOUBLE = ["range_0_ts_negative_2", "ts_negative_0_range_2"]
LB_ONLY = ["backend_id_eq_capacity", "backends_capacity", "backends_index", "one_table"]
# the faults the host finds in the headers and sizes alone, before any upload
HEADER_LEVEL = ["magic", "version", "kind", "capacity", "short_1", "short_section", "long",
                "n_live_gt_capacity", "pad_byte", "one_table", "backends_capacity"]


def names_for(kind):
    return MUTATIONS + DOUBLE + (LB_ONLY if kind == "lb" else [])


def small_state(kind):
    """The smallest case: deltacases.victim's state 0 (eight entries, two freed
    indices; viglb: two backends beside them) as a state of vignat or viglb
    over tables of CAP and LB_BCAP indices, packed on the CPU."""
    s = deltacases.victim("lb", cap=CAP, bcap=LB_BCAP)[0]
    if kind == "lb":
        return s
    assert kind == "nat"
    t = dict(s["tables"][0], value_size=0, value=[b""] * len(s["tables"][0]["lru"]))
    return {"kind": "nat", "last_now": s["last_now"], "tables": [t]}


@functools.lru_cache(None)
def recorded():
    """tests/golden/state_messages.json, as tests/golden/make_state_messages.py
    recorded it: {"image" | "image_small" | "delta": {kind: {name: [return
    code, vp_last_error()]}}} of every refused image and delta of the suites.
    "image": mutations() of the image a context saved after act 1 of the
    "part" trace; "image_small": the HEADER_LEVEL ones of small_state()'s;
    "delta": deltacases.mutations() of deltacases.victim's delta."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "state_messages.json")) as f:
        return json.load(f)
