"""vp_table_lookup / vp_table_entries in pure Python: written from the
description in include/vigpath.h, sharing no code with the library. Test
infrastructure only.

by_key / by_index answer over a stateref state (tests/stateref.py: the image's
tables with 16-byte keys and encoded values). lookup_queries / index_queries
build the query sets the tests use, with fixed seeds, and trace_points walks a
statecases trace with the oracle to the three points at which they look up.
"""
import numpy as np

import statecases as SC
import stateref as SR

MISS = 0xFFFFFFFF
# key bytes that are the libVig key, by kind and table; the rest is pad
KEY_BYTES = {"nat": [16], "bridge": [6], "fw": [13], "lb": [13, 4], "pol": [4]}


def _answers(table, found):
    """The four arrays for per-query positions `found` in the table's lru[]
    (None: a miss)."""
    n, vsz = len(found), table["value_size"]
    out = {"index": np.full(n, MISS, np.uint32), "ts": np.zeros(n, np.int64),
           "key": np.zeros((n, 16), np.uint8), "value": np.zeros((n, vsz), np.uint8)}
    for q, j in enumerate(found):
        if j is None:
            continue
        out["index"][q] = table["lru"][j]
        out["ts"][q] = table["ts"][j]
        out["key"][q] = np.frombuffer(table["key"][j], np.uint8)
        out["value"][q] = np.frombuffer(table["value"][j], np.uint8)
    return out


def by_key(state, table, keys):
    """Query q hits iff a live entry holds exactly the 16 bytes keys[q]."""
    t = state["tables"][table]
    where = {k: j for j, k in enumerate(t["key"])}
    assert len(where) == len(t["key"]), "a key occurs twice"
    keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 16)
    return _answers(t, [where.get(bytes(k)) for k in keys])


def by_index(state, table, idx):
    """An index at or above the capacity, or not allocated, is a miss."""
    t = state["tables"][table]
    where = {i: j for j, i in enumerate(t["lru"])}
    return _answers(t, [where.get(int(i)) if int(i) < t["capacity"] else None
                        for i in np.asarray(idx, np.uint32)])


# ----------------------------------------------------------- query sets --

QUOTA = dict(hits=48, absent=48, gone=16, padded=16, dup=8)


def lookup_queries(kind, state, table=0, gone=(), seed=11):
    """uint8[n, 16] keys in a fixed shuffled order, and what they are: a dict
    of query positions by class --
      hits    keys of live entries
      absent  keys no entry holds (a live key with a key byte changed)
      gone    keys of entries that were live earlier and are not now (`gone`)
      padded  live keys with one pad byte set (none for a key without pad)
      dup     positions that repeat an earlier query of the set
    Up to QUOTA of each, fewer where the state has fewer."""
    rng = np.random.default_rng(seed + 100 * table)
    t = state["tables"][table]
    kb = KEY_BYTES[kind][table]
    live = [np.frombuffer(k, np.uint8) for k in t["key"]]
    held = set(t["key"])
    pick = lambda seq, n: [seq[i] for i in rng.permutation(len(seq))[:n]]  # noqa: E731
    rows, cls = [], []
    for k in pick(live, QUOTA["hits"]):
        rows.append(k.copy())
        cls.append("hits")
    for k in pick(live, QUOTA["absent"]):
        k = k.copy()
        k[int(rng.integers(kb))] ^= 1 << int(rng.integers(8))
        if bytes(k) not in held:
            rows.append(k)
            cls.append("absent")
    zero = np.zeros(16, np.uint8)  # (the all-zero key and an all-ones one)
    for k in (zero, np.where(np.arange(16) < kb, 255, 0).astype(np.uint8)):
        if bytes(k) not in held:
            rows.append(k)
            cls.append("absent")
    for k in pick(sorted(g for g in gone if g not in held), QUOTA["gone"]):
        rows.append(np.frombuffer(k, np.uint8).copy())
        cls.append("gone")
    if kb < 16:
        for k in pick(live, QUOTA["padded"]):
            k = k.copy()
            k[kb + int(rng.integers(16 - kb))] = 1 << int(rng.integers(8))
            rows.append(k)
            cls.append("padded")
    for j in pick(list(range(len(rows))), QUOTA["dup"]):
        rows.append(rows[j].copy())
        cls.append("dup")
    order = rng.permutation(len(rows))
    keys = np.stack(rows)[order] if rows else np.zeros((0, 16), np.uint8)
    cls = [cls[i] for i in order]
    return keys, {c: [q for q, x in enumerate(cls) if x == c] for c in QUOTA}


IQUOTA = dict(live=32, free=32, tail=8)


def index_queries(state, table=0, seed=13):
    """uint32[n] indices in a fixed shuffled order and their classes: live,
    free (not allocated, below fresh_next), tail (never used), and `beyond`:
    the capacity, capacity + 1, 0xFFFFFFFE and 0xFFFFFFFF. Up to IQUOTA of the
    first three, fewer where the state has fewer."""
    rng = np.random.default_rng(seed + 100 * table)
    t = state["tables"][table]
    cap, fresh = t["capacity"], t["fresh_next"]
    live = sorted(t["lru"])
    free = sorted(set(range(fresh)) - set(live))
    tail = list(range(fresh, cap))
    pick = lambda seq, n: [seq[i] for i in rng.permutation(len(seq))[:n]]  # noqa: E731
    vals = [(i, "live") for i in pick(live, IQUOTA["live"])]
    vals += [(i, "free") for i in pick(free, IQUOTA["free"])]
    vals += [(i, "tail") for i in pick(tail, IQUOTA["tail"])]
    vals += [(i, "beyond") for i in (cap, cap + 1, 0xFFFFFFFE, 0xFFFFFFFF)]
    vals = [vals[i] for i in rng.permutation(len(vals))]
    idx = np.array([v for v, _ in vals], np.uint32)
    return idx, {c: [q for q, (_, x) in enumerate(vals) if x == c]
                 for c in ("live", "free", "tail", "beyond")}


# ------------------------------------------------- the three points --

def _tables(kind, d):
    """(alloc, the key bytes by index) of every table of a dump."""
    if kind == "lb":
        return [(d[0][0], d[0][2].reshape(d[0][0].shape[0], -1)[:, :13]),
                (d[1][0], d[1][2].reshape(-1, 1))]
    a, _, k = SC.flows_of(kind, d)
    return [(a, k[:, :KEY_BYTES[kind][0]])]


_points = {}
BEFORE, CUT, INSIDE, END = 0, 1, 2, 3
MID = 600  # packets of act 2 before points[INSIDE]


def trace_points(kind, variant, sample=20):
    """The oracle walked over statecases.trace(kind, variant) one packet at a
    time. Returns (trace, points, the oracle at the end); a point is a dict
      packets  the packets processed so far
      state    the stateref state of the oracle's dump there (lru[]: the live
               indices by stamp, which is not the LRU order among equal
               stamps; freed[] empty: a lookup depends on neither)
      gone     per table, the 16-byte keys that were live at an earlier
               sample (every `sample` packets) and are not live now
      reused   table 0's live indices that held another key before
    points[BEFORE] lies right before the packet that runs table 0's first
    expiry, points[CUT] at the cut between the trace's two acts (after many
    expiries; the "part" variant has freed indices on the stack and never-used
    ones there), points[INSIDE] MID packets into act 2 and points[END] at the
    end. Computed once per case and left unchanged."""
    if (kind, variant) in _points:
        return _points[kind, variant]
    tr, cut = SC.trace(kind, variant)
    fr, ln, dv, now = tr
    n = ln.shape[0]
    assert cut % sample == 0
    o = SC.oracle(kind, variant=variant)
    frames = fr.copy().reshape(n, 64)
    d = SC.dump(kind, o)
    prev = [(a.copy(), k.copy()) for a, k in _tables(kind, d)]
    nt = len(prev)
    fresh = [0] * nt
    seen = [set() for _ in range(nt)]
    first_key = {}  # table 0: index -> the first key it held
    reused = set()
    points = []

    def tables_at(d):
        live = [np.nonzero(a)[0] for a, _ in _tables(kind, d)]
        ts = [d[0][1], d[1][1]] if kind == "lb" else [d[1]]
        lru = [lv[np.argsort(ts[k][lv], kind="stable")] for k, lv in enumerate(live)]
        if kind == "lb":
            return SR.tables_from_dump(kind, d, lru=lru, freed=[(), ()], fresh_next=list(fresh))
        return SR.tables_from_dump(kind, d, lru=lru[0], freed=(), fresh_next=fresh[0])

    def point(p, d):
        tabs = tables_at(d)
        live0 = set(tabs[0]["lru"])
        return {"packets": p,
                "state": {"kind": kind, "last_now": int(now[p - 1]) if p else -1, "tables": tabs},
                "gone": [sorted(seen[k] - set(tabs[k]["key"])) for k in range(nt)],
                "reused": sorted(i for i in reused if i in live0)}

    for p in range(n):
        d_before = d
        o.run(frames[p], ln[p:p + 1], dv[p:p + 1], now[p:p + 1], 64)
        d = SC.dump(kind, o)
        cur = _tables(kind, d)
        a, key = cur[0]
        pa, pk = prev[0]
        changed = (pk != key).any(axis=1)
        if not points and ((pa == 1) & ((a == 0) | changed)).any():
            points.append(point(p, d_before))  # (fresh[]: still as before this packet)
        for i in np.nonzero((a == 1) & ((pa == 0) | changed))[0]:
            kb = bytes(key[i])
            if first_key.setdefault(int(i), kb) != kb:
                reused.add(int(i))
        for k, (a, _) in enumerate(cur):
            if a.any():
                fresh[k] = max(fresh[k], int(np.nonzero(a)[0].max()) + 1)
        prev = [(a.copy(), k.copy()) for a, k in cur]
        if (p + 1) % sample == 0:
            tabs = tables_at(d)
            for k in range(nt):
                seen[k] |= set(tabs[k]["key"])
        if p + 1 in (cut, cut + MID):
            assert len(points) == (1 if p + 1 == cut else 2), "no expiry in act 1"
            points.append(point(p + 1, d))
    assert len(points) == 3, (kind, variant, len(points))
    points.append(point(n, d))
    _points[kind, variant] = (tr, points, o)
    return _points[kind, variant]
