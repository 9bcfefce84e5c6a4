"""Malformed deltas for the refusal tests: one mutation each of a good delta
(tests/deltaref.py dicts), for tests/test_state_delta_ref.py (deltaref.apply
raises) and tests/test_state_delta_gpu.py (vp_state_delta_apply refuses)."""
import copy

import deltaref as DR


def _table(cap, lru, freed, fresh, ts, vsz=0, gen=None):
    """gen: index -> the generation of its key (0: the index's first key)."""
    gen = gen or {}
    return {"capacity": cap, "fresh_next": fresh, "value_size": vsz, "lru": list(lru),
            "freed": list(freed), "ts": list(ts),
            "key": [bytes([i, gen.get(i, 0)]) + bytes(14) for i in lru],
            "value": [bytes([1]) + bytes(vsz - 1) for _ in lru]}


def victim(kind, cap=16, bcap=4):
    """(state 0, state 1, the touched indices per table) of vigfw or viglb.
    State 0: indices 0 .. 9 used; 3 and 7 freed. State 1: 0 and 1 expired, 3
    and 7 taken again by new keys, 1 taken again, 10 and 11 from the tail, 5
    touched, 9 erased out of LRU order. viglb: beside a table of backends that
    gains one and has one touched."""
    t0 = _table(cap, [0, 1, 2, 4, 5, 6, 8, 9], [7, 3], 10,
                [100, 100, 101, 102, 103, 110, 110, 120], vsz=4)
    t1 = _table(cap, [2, 4, 6, 8, 7, 3, 5, 1, 10, 11], [0, 9], 12,
                [101, 102, 110, 110, 130, 130, 131, 135, 140, 140], vsz=4,
                gen={7: 1, 3: 1, 1: 1})
    touched = [{7, 3, 5, 1, 10, 11}]
    if kind == "fw":
        return ({"kind": "fw", "last_now": 120, "tables": [t0]},
                {"kind": "fw", "last_now": 140, "tables": [t1]}, touched)
    assert kind == "lb"
    bk0 = _table(bcap, [0, 1], [], 2, [90, 95], vsz=8)
    bk1 = _table(bcap, [0, 1, 2], [], 3, [90, 125, 139], vsz=8)
    return ({"kind": "lb", "last_now": 120, "tables": [t0, bk0]},
            {"kind": "lb", "last_now": 140, "tables": [t1, bk1]}, touched + [{1, 2}])


def _edit(delta, table, **fields):
    d = copy.deepcopy(delta)
    d["tables"][table].update(fields)
    return d


def _set(lst, j, v):
    out = list(lst)
    out[j] = v
    return out


def mutations(state0, delta):
    """{name: blob}. state0: the state the delta applies to. Needs in table 0:
    four entries in new[], one of them at an index that is not live in state0,
    two freed indices, two kept entries, and fresh_next below the capacity."""
    kind = state0["kind"]
    good = DR.pack(delta)
    t, t0 = delta["tables"][0], state0["tables"][0]
    cap, fresh, idx, freed = t["capacity"], t["fresh_next"], t["idx"], t["freed"]
    live0 = {i: j for j, i in enumerate(t0["lru"])}
    kept = [i for i in t0["lru"] if i < fresh and i not in set(freed) and i not in set(idx)]
    assert len(idx) >= 4 and len(freed) >= 2 and len(kept) >= 2 and fresh < cap
    m = {}
    # sizes, offsets, header fields
    m["magic"] = DR.pack(delta, magic=DR.MAGIC ^ 1)
    m["version"] = DR.pack(delta, version=2)
    m["kind"] = DR.pack(dict(delta, kind="fw" if kind == "nat" else "nat"))
    m["short_1"] = good[:-1]
    m["short_section"] = good[:len(good) - 16 * len(idx)]
    m["long"] = good + bytes(16)
    m["reserved_word"] = good[:64 + 24] + b"\x01" + good[64 + 25:]
    m["capacity"] = DR.pack(_edit(delta, 0, capacity=cap * 2, fresh_next=fresh + cap))
    m["value_size"] = DR.pack(_edit(delta, 0, value_size=t["value_size"] + 4,
                                    value=[v + bytes(4) for v in t["value"]]))
    m["n_new_header"] = DR.pack(_edit(delta, 0, n_new=len(idx) + 1))
    if 4 * len(idx) % 16:
        at = 64 + 32 + 4 * len(idx)
    else:
        assert 4 * len(freed) % 16, "no pad byte in the first table's index arrays"
        at = 64 + 32 + 4 * len(idx) + 4 * len(freed)
    m["pad_byte"] = good[:at] + b"\x01" + good[at + 1:]
    if len(delta["tables"]) > 1:
        m["one_table"] = DR.pack(dict(delta, tables=delta["tables"][:1]))
    # the partition of the indices
    m["sum"] = DR.pack(_edit(delta, 0, n_live=t["n_live"] + 1))
    m["not_normalised"] = DR.pack(_edit(delta, 0, freed=freed + [fresh], fresh_next=fresh + 1))
    m["idx_range"] = DR.pack(_edit(delta, 0, idx=_set(idx, 0, cap)))
    m["freed_range"] = DR.pack(_edit(delta, 0, freed=_set(freed, 0, cap)))
    m["idx_twice"] = DR.pack(_edit(delta, 0, idx=_set(idx, 1, idx[0])))
    m["freed_twice"] = DR.pack(_edit(delta, 0, freed=_set(freed, 1, freed[0])))
    m["idx_and_freed"] = DR.pack(_edit(delta, 0, freed=_set(freed, 0, idx[2])))
    m["idx_in_tail"] = DR.pack(_edit(delta, 0, idx=_set(idx, 0, fresh)))
    m["freed_in_tail"] = DR.pack(_edit(delta, 0, freed=_set(freed, 0, fresh)))
    # an entry of new[] at an index that state0 does not hold is left out: the
    # index is then neither free, new nor kept, and the counts do not add up
    j = next(j for j, i in enumerate(idx) if i not in live0)
    drop = {f: t[f][:j] + t[f][j + 1:] for f in ("idx", "ts", "key", "value")}
    m["kept_count"] = DR.pack(_edit(delta, 0, **drop))
    # stamps
    ts = t["ts"]
    m["ts_negative"] = DR.pack(_edit(delta, 0, ts=_set(ts, 0, -5)))
    m["ts_after_last_now"] = DR.pack(_edit(delta, 0, ts=_set(ts, -1, delta["last_now"] + 1)))
    m["ts_decreasing"] = DR.pack(_edit(delta, 0, ts=_set(_set(ts, 1, ts[-1] + 1), -1, ts[1])))
    top = max(t0["ts"][live0[i]] for i in kept)
    assert top >= 1
    m["ts_below_kept"] = DR.pack(_edit(delta, 0, ts=_set(ts, 0, top - 1)))
    m["last_now_below"] = DR.pack(dict(
        _edit(delta, 0, ts=[min(x, state0["last_now"] - 1) for x in ts]),
        last_now=state0["last_now"] - 1))
    # keys and values
    m["key_twice"] = DR.pack(_edit(delta, 0, key=_set(t["key"], 1, t["key"][0])))
    m["key_of_kept"] = DR.pack(_edit(delta, 0, key=_set(t["key"], 0, t0["key"][live0[kept[1]]])))
    if DR.KEY_BYTES[kind][0] < 16:
        m["key_pad"] = DR.pack(_edit(delta, 0, key=_set(t["key"], 0, t["key"][0][:15] + b"\x01")))
    if kind in ("bridge", "fw", "lb"):
        bad = 0x10000 if kind != "lb" else delta["tables"][1]["capacity"]
        m["value_range"] = DR.pack(_edit(delta, 0, value=_set(t["value"], 0,
                                                              bad.to_bytes(4, "little"))))
    # two faults in one delta: the lower code is reported, wherever it stands,
    # and what sd_check finds before anything sd_check2 would
    m["idx_and_freed_ts_negative"] = DR.pack(
        _edit(delta, 0, freed=_set(freed, 0, idx[2]), ts=_set(ts, 0, -5)))
    m["range_0_ts_negative_2"] = DR.pack(
        _edit(delta, 0, idx=_set(idx, 0, cap), ts=_set(ts, 2, -5)))
    m["ts_negative_0_range_2"] = DR.pack(
        _edit(delta, 0, idx=_set(idx, 2, cap), ts=_set(ts, 0, -5)))
    for name, blob in m.items():
        assert blob != good, name
    return m


# every name mutations() can give, for parametrising
NAMES = ["magic", "version", "kind", "short_1", "short_section", "long", "reserved_word",
         "capacity", "value_size", "n_new_header", "pad_byte", "sum", "not_normalised",
         "idx_range", "freed_range", "idx_twice", "freed_twice", "idx_and_freed", "idx_in_tail",
         "freed_in_tail", "kept_count", "ts_negative", "ts_after_last_now", "ts_decreasing",
         "ts_below_kept", "last_now_below", "key_twice", "key_of_kept",
         "idx_and_freed_ts_negative", "range_0_ts_negative_2", "ts_negative_0_range_2"]
# the faults the host finds in the headers and sizes alone, before any upload
HEADER_LEVEL = ["magic", "version", "kind", "short_1", "short_section", "long", "reserved_word",
                "capacity", "value_size", "n_new_header", "pad_byte", "sum", "one_table"]
NOT_NAT = ["key_pad"]
VALUED = ["value_range"]
LB_ONLY = ["one_table"]


def names_for(kind):
    return (NAMES + (NOT_NAT if kind != "nat" else []) +
            (VALUED if kind in ("bridge", "fw", "lb") else []) + (LB_ONLY if kind == "lb" else []))
