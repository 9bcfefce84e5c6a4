"""vp_table_erase / vp_table_free in pure Python: the loop include/vigpath.h
states, over a stateref state (tests/stateref.py), sharing no code with the
library. Test infrastructure only.

    for q = 0 .. n-1 in order: if the query names a live entry, map_erase its
    key and dchain_free_index its index (onto the front of the free list).

erase() works on a state, erase_image() on an image's bytes: unpack, erase in
query order, normalise, pack.
"""
import copy

import numpy as np

import statecases as SC
import stateref as SR

MISS = 0xFFFFFFFF
# key bytes that are the libVig key, by kind and table; the rest is pad
KEY_BYTES = {"nat": [16], "bridge": [6], "fw": [13], "lb": [13, 4], "pol": [4]}


def erase(state, table, queries, by_key):
    """(the state afterwards, the outputs, n_erased). queries: uint8[n, 16]
    keys, or uint32[n] indices. The outputs are the lookup's four arrays: for
    an erasing query the freed index and the entry as it was, else a miss."""
    s = copy.deepcopy(state)
    t = s["tables"][table]
    cap, vsz = t["capacity"], t["value_size"]
    if by_key:
        queries = np.ascontiguousarray(queries, np.uint8).reshape(-1, 16)
    else:
        queries = np.ascontiguousarray(queries, np.uint32).reshape(-1)
    n = queries.shape[0]
    out = {"index": np.full(n, MISS, np.uint32), "ts": np.zeros(n, np.int64),
           "key": np.zeros((n, 16), np.uint8), "value": np.zeros((n, vsz), np.uint8)}
    index_of = dict(zip(t["key"], t["lru"]))  # the map: key -> index
    assert len(index_of) == len(t["lru"]), "a key occurs twice"
    allocated = set(t["lru"])                 # the dchain's allocated indices
    erased = 0
    for q in range(n):
        if by_key:
            i = index_of.get(queries[q].tobytes())
        else:
            i = int(queries[q])
            if i >= cap or i not in allocated:
                i = None
        if i is None:
            continue
        j = t["lru"].index(i)
        out["index"][q] = i
        out["ts"][q] = t["ts"][j]
        out["key"][q] = np.frombuffer(t["key"][j], np.uint8)
        out["value"][q] = np.frombuffer(t["value"][j], np.uint8)
        del index_of[t["key"][j]]             # map_erase
        allocated.discard(i)                  # dchain_free_index: the front
        t["freed"].insert(0, i)
        for a in ("lru", "ts", "key", "value"):
            del t[a][j]
        erased += 1
    return s, out, erased


def erase_image(img, table, queries, by_key):
    """(the image afterwards, the outputs, n_erased) of an image's bytes."""
    s, out, k = erase(SR.unpack(img), table, queries, by_key)
    return SR.pack(s), out, k


def small(kind):
    """statecases.small_state for every kind: vigbridge, vigfw and vigpol take
    viglb's first table with values of their own size."""
    if kind in ("nat", "lb"):
        return SC.small_state(kind)
    s = SC.small_state("lb")
    vsz = SR.VALUE_SIZE[kind][0]
    t = dict(s["tables"][0], value_size=vsz,
             value=[bytes([1]) + bytes(vsz - 1) for _ in s["tables"][0]["lru"]])
    return {"kind": kind, "last_now": s["last_now"], "tables": [t]}


def key_queries(kind, table_no, t, rng, n_hits, n_twice=4, n_miss=6):
    """uint8[n, 16]: n_hits live keys of table t in random order, n_twice of
    them named twice, n_miss keys no entry holds and, where the key has pad
    bytes, one live key with a pad bit set; shuffled."""
    kb = KEY_BYTES[kind][table_no]
    live = [np.frombuffer(k, np.uint8) for k in t["key"]]
    held = set(t["key"])
    pick = [live[i].copy() for i in rng.permutation(len(live))[:n_hits]]
    rows = list(pick) + [k.copy() for k in pick[:n_twice]]
    for k in live[:n_miss]:
        k = k.copy()
        k[int(rng.integers(kb))] ^= 1 << int(rng.integers(8))
        if k.tobytes() not in held:
            rows.append(k)
    if kb < 16 and live:
        k = live[int(rng.integers(len(live)))].copy()
        k[kb + int(rng.integers(16 - kb))] = 1 << int(rng.integers(8))
        rows.append(k)
    if not rows:
        return np.zeros((0, 16), np.uint8)
    return np.stack(rows)[rng.permutation(len(rows))]


def index_queries(t, rng, n_hits, n_twice=4):
    """uint32[n]: n_hits live indices in random order, n_twice of them named
    twice, a free index and a tail index where the table has them, the
    capacity, capacity + 5 and 0xFFFFFFFF; shuffled."""
    cap, fresh = t["capacity"], t["fresh_next"]
    live = [t["lru"][i] for i in rng.permutation(len(t["lru"]))[:n_hits]]
    vals = live + live[:n_twice]
    free = sorted(set(range(fresh)) - set(t["lru"]))
    if free:
        vals.append(free[int(rng.integers(len(free)))])
    if fresh < cap:
        vals.append(int(rng.integers(fresh, cap)))
    vals += [cap, cap + 5, 0xFFFFFFFF]
    return np.array(vals, np.uint32)[rng.permutation(len(vals))]
