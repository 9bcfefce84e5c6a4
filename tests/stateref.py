"""The state image of vp_state_save / vp_state_load, version 1, in pure
Python: written from the description in include/vigpath.h, sharing no code
with the library. Test infrastructure only.

A state is a dict {"kind": str, "last_now": int, "tables": [table, ...]} and a
table a dict
    capacity, fresh_next          ints
    lru, freed                    lists of indices (oldest first / hand-out order)
    ts                            list of ints, entry j belongs to lru[j]
    key                           list of 16-byte bytes
    value                         list of value_size-byte bytes
    value_size                    int
unpack() returns exactly what the bytes say (it raises ValueError on a
structure it cannot walk); pack() writes what it is given, after moving a
freed index that belongs to the never-used tail into the tail (canon=True).
"""
import struct

import numpy as np

MAGIC = 0x54535056
VERSION = 1
KINDS = {"nat": 1, "bridge": 2, "lb": 3, "fw": 4, "pol": 5}
KIND_NAMES = {v: k for k, v in KINDS.items()}
HDR = struct.Struct("<IIIIQq")
THDR = struct.Struct("<IIIIIIII")
# value bytes per entry, by kind and table
VALUE_SIZE = {"nat": [0], "bridge": [4], "fw": [4], "lb": [4, 8], "pol": [16]}


def _pad(b):
    return b + bytes(-len(b) % 16)


def normalise(table):
    """The table with the longest ascending run that ends the hand-out order
    at capacity - 1 taken as the tail."""
    t = dict(table)
    freed, fresh = list(t["freed"]), t["fresh_next"]
    while freed and freed[-1] == fresh - 1:
        freed.pop()
        fresh -= 1
    t["freed"], t["fresh_next"] = freed, fresh
    return t


def pack(state, canon=True, magic=MAGIC, version=VERSION):
    body = b""
    for t in state["tables"]:
        if canon:
            t = normalise(t)
        n = len(t["lru"])
        assert len(t["ts"]) == len(t["key"]) == len(t["value"]) == n
        body += THDR.pack(t["capacity"], t.get("n_live", n), t["fresh_next"], t["value_size"],
                          t.get("n_freed", len(t["freed"])), 0, 0, 0)
        body += _pad(struct.pack("<%dI" % n, *t["lru"]))
        body += _pad(struct.pack("<%dI" % len(t["freed"]), *t["freed"]))
        body += _pad(struct.pack("<%dq" % n, *t["ts"]))
        for k in t["key"]:
            assert len(k) == 16
        body += b"".join(t["key"])
        for v in t["value"]:
            assert len(v) == t["value_size"]
        body += _pad(b"".join(t["value"]))
    total = HDR.size + len(body)
    return HDR.pack(magic, version, KINDS[state["kind"]], len(state["tables"]), total,
                    state["last_now"]) + body


def unpack(blob):
    blob = bytes(blob)
    if len(blob) < HDR.size:
        raise ValueError("no header")
    magic, version, kind, nt, total, last_now = HDR.unpack_from(blob, 0)
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
        cap, n, fresh, vsz, nf, r0, r1, r2 = THDR.unpack(take(THDR.size))
        if r0 | r1 | r2:
            raise ValueError("reserved word")
        lru = list(struct.unpack("<%dI" % n, take(4 * n)))
        freed = list(struct.unpack("<%dI" % nf, take(4 * nf)))
        ts = list(struct.unpack("<%dq" % n, take(8 * n)))
        keys = take(16 * n)
        vals = take(vsz * n)
        tables.append({"capacity": cap, "fresh_next": fresh, "value_size": vsz, "lru": lru,
                       "freed": freed, "ts": ts,
                       "key": [keys[16 * j:16 * j + 16] for j in range(n)],
                       "value": [vals[vsz * j:vsz * j + vsz] for j in range(n)]})
    if at != len(blob):
        raise ValueError("bytes behind the last table")
    return {"kind": KIND_NAMES[kind], "last_now": last_now, "tables": tables}


# ------------------------------------------------- a table from a dump --

def table_from_dump(alloc, ts, key16, values, value_size, lru=None, freed=(), fresh_next=None):
    """A table of the image from the arrays of a dump by index. lru: the live
    indices oldest first; None: by ts, which must then be distinct. freed /
    fresh_next: the free list; None: the never-used tail alone, which must
    then be what is not live."""
    cap = int(alloc.shape[0])
    live = np.nonzero(alloc)[0]
    if lru is None:
        assert np.unique(ts[live]).size == live.size, "equal stamps: the dump has no LRU order"
        lru = live[np.argsort(ts[live], kind="stable")]
    if fresh_next is None:
        fresh_next = cap - (cap - live.size - len(freed))
        dead = np.setdiff1d(np.arange(cap), np.concatenate([live, np.asarray(freed, np.int64)]))
        assert np.array_equal(dead, np.arange(fresh_next, cap)), "free indices below the tail"
    return {"capacity": cap, "fresh_next": int(fresh_next), "value_size": value_size,
            "lru": [int(i) for i in lru], "freed": [int(i) for i in freed],
            "ts": [int(ts[i]) for i in lru], "key": [bytes(key16[i]) for i in lru],
            "value": [bytes(values[i]) for i in lru]}


def _pad_keys(a, width):
    """Rows of `width` key bytes zero-padded to 16."""
    out = np.zeros((a.shape[0], 16), np.uint8)
    out[:, :width] = a.reshape(a.shape[0], -1)[:, :width]
    return out


def _le(a, dtype):
    """Per-index little-endian bytes of an integer array."""
    a = np.ascontiguousarray(a.astype(dtype).astype(np.dtype(dtype).newbyteorder("<")))
    return a.view(np.uint8).reshape(a.shape[0], -1)


def tables_from_dump(kind, dump, **order):
    """The image's tables from NF.dump() / Oracle.*_dump() of `kind`. order:
    lru / freed / fresh_next as table_from_dump takes them (viglb: lists of
    two)."""
    if kind == "nat":
        alloc, ts, keys = dump
        return [table_from_dump(alloc, ts, keys, np.zeros((alloc.shape[0], 0), np.uint8), 0,
                                **order)]
    if kind == "bridge":
        alloc, ts, macs, port = dump
        return [table_from_dump(alloc, ts, _pad_keys(macs, 6), _le(port, np.uint32), 4, **order)]
    if kind == "fw":
        alloc, ts, keys, dev = dump
        return [table_from_dump(alloc, ts, _pad_keys(keys, 13), _le(dev, np.uint32), 4, **order)]
    if kind == "pol":
        alloc, ts, keys, size, btime = dump
        val = np.concatenate([_le(size, np.uint64), _le(btime, np.int64)], axis=1)
        return [table_from_dump(alloc, ts, _pad_keys(_le(keys, np.uint32), 4), val, 16, **order)]
    if kind == "lb":
        (fa, ft, fk, fb), (ba, bt, bi, bm, bn) = dump
        o = [{k: v[i] for k, v in order.items()} for i in range(2)]
        bval = np.concatenate([bm.reshape(-1, 6), _le(bn, np.uint16)], axis=1)
        return [table_from_dump(fa, ft, _pad_keys(fk, 13), _le(fb, np.uint32), 4, **o[0]),
                table_from_dump(ba, bt, _pad_keys(_le(bi, np.uint32), 4), bval, 8, **o[1])]
    raise ValueError(kind)


def state_from_dump(kind, dump, last_now, **order):
    return {"kind": kind, "last_now": int(last_now), "tables": tables_from_dump(kind, dump, **order)}
