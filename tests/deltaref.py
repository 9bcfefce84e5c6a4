"""The incremental state image of vp_state_delta_save / vp_state_delta_apply,
version 1, in pure Python: written from the description in include/vigpath.h,
sharing no code with the library. Test infrastructure only.

A delta is a dict {"kind", "last_now", "base": (seq, epoch), "mark": (seq,
epoch), "tables": [table, ...]} and a table a dict
    capacity, n_live, fresh_next, value_size     ints, of the state now
    freed                                        the whole free list before the tail
    idx, ts, key, value                          new[]: lists, entry j belongs to idx[j]
States are tests/stateref.py's. unpack() returns what the bytes say (ValueError
on a structure it cannot walk); pack() writes what it is given; apply() checks
everything the header lists and raises ValueError on the first offence.
"""
import struct

import stateref as SR

MAGIC = 0x44535056
VERSION = 1
HDR = struct.Struct("<IIIIQqQQQQ")
THDR = struct.Struct("<IIIIIIII")
# key bytes that are the key (the rest of the 16 is pad), by kind and table
KEY_BYTES = {"nat": [16], "bridge": [6], "fw": [13], "lb": [13, 4], "pol": [4]}


def _pad(b):
    return b + bytes(-len(b) % 16)


def pack(delta, magic=MAGIC, version=VERSION):
    body = b""
    for t in delta["tables"]:
        n = len(t["idx"])
        assert len(t["ts"]) == len(t["key"]) == len(t["value"]) == n
        body += THDR.pack(t["capacity"], t["n_live"], t["fresh_next"], t["value_size"],
                          t.get("n_freed", len(t["freed"])), t.get("n_new", n), 0, 0)
        body += _pad(struct.pack("<%dI" % n, *t["idx"]))
        body += _pad(struct.pack("<%dI" % len(t["freed"]), *t["freed"]))
        body += _pad(struct.pack("<%dq" % n, *t["ts"]))
        for k in t["key"]:
            assert len(k) == 16
        body += b"".join(t["key"])
        for v in t["value"]:
            assert len(v) == t["value_size"]
        body += _pad(b"".join(t["value"]))
    total = HDR.size + len(body)
    return HDR.pack(magic, version, SR.KINDS[delta["kind"]], len(delta["tables"]), total,
                    delta["last_now"], *delta["base"], *delta["mark"]) + body


def unpack(blob):
    blob = bytes(blob)
    if len(blob) < HDR.size:
        raise ValueError("no header")
    magic, version, kind, nt, total, last_now, bs, be, ms, me = HDR.unpack_from(blob, 0)
    if magic != MAGIC or version != VERSION or total != len(blob):
        raise ValueError("magic, version or size")
    at = HDR.size
    tables = []

    def take(n):
        nonlocal at
        if at + n > len(blob):
            raise ValueError("array past the end")
        b = blob[at:at + n]
        at += n
        if any(blob[at:at + (-n % 16)]):
            raise ValueError("pad byte")
        at += -n % 16
        return b

    for _ in range(nt):
        cap, n_live, fresh, vsz, nf, n, r0, r1 = THDR.unpack(take(THDR.size))
        if r0 | r1:
            raise ValueError("reserved word")
        idx = list(struct.unpack("<%dI" % n, take(4 * n)))
        freed = list(struct.unpack("<%dI" % nf, take(4 * nf)))
        ts = list(struct.unpack("<%dq" % n, take(8 * n)))
        keys = take(16 * n)
        vals = take(vsz * n)
        tables.append({"capacity": cap, "n_live": n_live, "fresh_next": fresh, "value_size": vsz,
                       "freed": freed, "idx": idx, "ts": ts,
                       "key": [keys[16 * j:16 * j + 16] for j in range(n)],
                       "value": [vals[vsz * j:vsz * j + vsz] for j in range(n)]})
    if at != len(blob):
        raise ValueError("bytes behind the last table")
    return {"kind": SR.KIND_NAMES[kind], "last_now": last_now, "base": (bs, be), "mark": (ms, me),
            "tables": tables}


def _value_ok(kind, k, v, tables):
    if kind in ("bridge", "fw"):
        return int.from_bytes(v, "little") <= 0xFFFF
    if kind == "lb" and k == 0:
        return int.from_bytes(v, "little") < tables[1]["capacity"]
    return True


def apply(state0, delta):
    """The state after `delta`, applied to the state it was taken from."""
    kind = state0["kind"]
    if delta["kind"] != kind or len(delta["tables"]) != len(state0["tables"]):
        raise ValueError("kind or table count")
    if delta["last_now"] < state0["last_now"] or delta["last_now"] < -1:
        raise ValueError("last_now below the context's")
    out = []
    for k, (t0, d) in enumerate(zip(state0["tables"], delta["tables"])):
        cap, fresh, n_live = d["capacity"], d["fresh_next"], d["n_live"]
        idx, freed = d["idx"], d["freed"]
        if cap != t0["capacity"] or d["value_size"] != SR.VALUE_SIZE[kind][k]:
            raise ValueError("table %d: capacity or value size" % k)
        if d.get("n_new", len(idx)) != len(idx) or d.get("n_freed", len(freed)) != len(freed):
            raise ValueError("table %d: counts" % k)
        if fresh > cap or n_live + len(freed) + (cap - fresh) != cap:
            raise ValueError("table %d: n_live + n_freed + tail is not the capacity" % k)
        if freed and freed[-1] == fresh - 1:
            raise ValueError("table %d: the tail is not normalised" % k)
        for name, arr in (("idx", idx), ("freed", freed)):
            for j, i in enumerate(arr):
                if not 0 <= i < cap:
                    raise ValueError("table %d: %s[%d] out of range" % (k, name, j))
                if i >= fresh:
                    raise ValueError("table %d: %s[%d] in the tail" % (k, name, j))
            if len(set(arr)) != len(arr):
                raise ValueError("table %d: an index twice in %s[]" % (k, name))
        fset, nset = set(freed), set(idx)
        if fset & nset:
            raise ValueError("table %d: an index in idx[] and freed[]" % k)
        for j, ts in enumerate(d["ts"]):
            if ts < 0 or ts > delta["last_now"] or (j and ts < d["ts"][j - 1]):
                raise ValueError("table %d: ts[%d]" % (k, j))
        for j, (key, v) in enumerate(zip(d["key"], d["value"])):
            if any(key[KEY_BYTES[kind][k]:]):
                raise ValueError("table %d: key[%d] pad byte" % (k, j))
            if not _value_ok(kind, k, v, delta["tables"]):
                raise ValueError("table %d: value[%d] out of range" % (k, j))
        if len(set(d["key"])) != len(idx):
            raise ValueError("table %d: a key twice in new[]" % k)
        at0 = {i: j for j, i in enumerate(t0["lru"])}
        kept = [i for i in t0["lru"] if i < fresh and i not in fset and i not in nset]
        for i in range(fresh):
            if i not in fset and i not in nset and i not in at0:
                raise ValueError("table %d: index %d is neither free, new nor live" % (k, i))
        if len(kept) + len(idx) != n_live:
            raise ValueError("table %d: kept + n_new is not n_live" % k)
        if kept and idx and max(t0["ts"][at0[i]] for i in kept) > d["ts"][0]:
            raise ValueError("table %d: ts[0] below a kept entry's stamp" % k)
        kept_keys = {t0["key"][at0[i]] for i in kept}
        for j, key in enumerate(d["key"]):
            if key in kept_keys:
                raise ValueError("table %d: key[%d] held by a kept entry" % (k, j))
        out.append({"capacity": cap, "fresh_next": fresh, "value_size": d["value_size"],
                    "lru": kept + list(idx), "freed": list(freed),
                    "ts": [t0["ts"][at0[i]] for i in kept] + list(d["ts"]),
                    "key": [t0["key"][at0[i]] for i in kept] + list(d["key"]),
                    "value": [t0["value"][at0[i]] for i in kept] + list(d["value"])})
    return {"kind": kind, "last_now": delta["last_now"], "tables": out}


def diff(state0, state1, touched, base=(0, 0), mark=(0, 0)):
    """The delta that takes state0 to state1. touched: per table, the indices
    whose last touch came after state0 was taken."""
    tables = []
    for t1, tch in zip(state1["tables"], touched):
        t1 = SR.normalise(t1)
        tch = set(int(i) for i in tch)
        js = [j for j, i in enumerate(t1["lru"]) if i in tch]
        tables.append({"capacity": t1["capacity"], "n_live": len(t1["lru"]),
                       "fresh_next": t1["fresh_next"], "value_size": t1["value_size"],
                       "freed": list(t1["freed"]), "idx": [t1["lru"][j] for j in js],
                       "ts": [t1["ts"][j] for j in js], "key": [t1["key"][j] for j in js],
                       "value": [t1["value"][j] for j in js]})
    return {"kind": state1["kind"], "last_now": state1["last_now"], "base": tuple(base),
            "mark": tuple(mark), "tables": tables}
