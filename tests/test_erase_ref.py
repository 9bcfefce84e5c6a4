"""tests/eraseref.py, the reference of vp_table_erase / vp_table_free, checked
against what libVig's calls do to the dchain and the map, on the smallest
states (eraseref.small: eight entries, two freed indices). CPU only."""
import numpy as np
import pytest

import eraseref as ER
import statecases as SC
import stateref as SR


def tables(kind):
    return range(len(ER.small(kind)["tables"]))


def accounted(t):
    n = SR.normalise(t)
    return len(n["lru"]) + len(n["freed"]) + (n["capacity"] - n["fresh_next"]) == n["capacity"]


@pytest.mark.parametrize("kind", SC.KINDS)
def test_small_states_are_images(kind):
    s = ER.small(kind)
    assert SR.unpack(SR.pack(s)) == s
    assert [t["value_size"] for t in s["tables"]] == SR.VALUE_SIZE[kind]
    assert all(accounted(t) for t in s["tables"])


@pytest.mark.parametrize("by_key", [True, False])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_erasing_the_oldest_in_order_is_their_expiry(kind, by_key):
    """expire_items_single_map frees the k oldest in LRU order, each onto the
    front of the free list: the youngest of them ends on top."""
    s = ER.small(kind)
    for table in tables(kind):
        t = s["tables"][table]
        for k in range(len(t["lru"]) + 1):
            q = (np.frombuffer(b"".join(t["key"][:k]), np.uint8).reshape(-1, 16) if by_key
                 else np.array(t["lru"][:k], np.uint32))
            after, out, n = ER.erase(s, table, q, by_key)
            a = after["tables"][table]
            assert n == k
            assert a["freed"] == t["lru"][:k][::-1] + t["freed"]
            for name in ("lru", "ts", "key", "value"):
                assert a[name] == t[name][k:]
            assert out["index"].tolist() == t["lru"][:k] and out["ts"].tolist() == t["ts"][:k]
            assert out["key"].tobytes() == b"".join(t["key"][:k])
            assert out["value"].tobytes() == b"".join(t["value"][:k])
            assert accounted(a)
            # the other table and the clock stay
            assert after["last_now"] == s["last_now"]
            assert [x for i, x in enumerate(after["tables"]) if i != table] == \
                [x for i, x in enumerate(s["tables"]) if i != table]


@pytest.mark.parametrize("kind", SC.KINDS)
def test_duplicates_and_misses_are_no_ops(kind):
    s = ER.small(kind)
    for table in tables(kind):
        t = s["tables"][table]
        kb = ER.KEY_BYTES[kind][table]
        k1, k0 = (np.frombuffer(t["key"][j], np.uint8) for j in (1, 0))
        absent = k0.copy()
        absent[0] ^= 0x80
        assert absent.tobytes() not in t["key"]
        rows = [k1, absent, k1, k0, k0]
        if kb < 16:
            padded = k0.copy()
            padded[15] = 1
            rows.insert(0, padded)
        after, out, n = ER.erase(s, table, np.stack(rows), True)
        a = after["tables"][table]
        first = len(rows) - 5
        assert n == 2 and a["freed"] == [t["lru"][0], t["lru"][1]] + t["freed"]
        assert a["lru"] == t["lru"][2:]
        want = [ER.MISS] * len(rows)
        want[first], want[first + 3] = t["lru"][1], t["lru"][0]
        assert out["index"].tolist() == want
        assert not out["key"][[q for q, i in enumerate(want) if i == ER.MISS]].any()
        # by index: a free index, a tail index, the capacity, an index named twice
        free, cap, fresh = t["freed"][0] if t["freed"] else None, t["capacity"], t["fresh_next"]
        idx = [t["lru"][-1], fresh, cap, 0xFFFFFFFF, t["lru"][-1]] + ([free] if free is not None else [])
        after, out, n = ER.erase(s, table, np.array(idx, np.uint32), False)
        assert n == 1 and after["tables"][table]["freed"] == [t["lru"][-1]] + t["freed"]
        assert out["index"].tolist() == [t["lru"][-1]] + [ER.MISS] * (len(idx) - 1)
        assert accounted(after["tables"][table])
        # nothing but no-ops: the image stays
        img = SR.pack(s)
        same, out, n = ER.erase_image(img, table, np.array([fresh, cap], np.uint32), False)
        assert n == 0 and same == img


@pytest.mark.parametrize("kind", SC.KINDS)
def test_an_erased_fresh_next_minus_one_joins_the_tail(kind):
    """The image's tail is the longest run that ends the hand-out order: an
    erased fresh_next - 1 joins it when the free list is empty behind it."""
    s = ER.small(kind)
    t = dict(s["tables"][0])
    for name in ("lru", "ts", "key", "value"):  # indices 0 .. 2 live, nothing freed
        t[name] = t[name][:3]
    assert t["lru"] == [0, 1, 2]
    t["freed"], t["fresh_next"] = [], 3
    s = dict(s, tables=[t] + s["tables"][1:])
    img, _, n = ER.erase_image(SR.pack(s), 0, np.array([2], np.uint32), False)
    a = SR.unpack(img)["tables"][0]
    assert n == 1 and a["freed"] == [] and a["fresh_next"] == 2 and a["lru"] == [0, 1]
    # 1 then 2: 2 on top, then 1 -- the hand-out order 2, 1, 3, 4 .. does not end
    # ascending, so neither joins; 2 then 1: the order 1, 2, 3 .. does, both join
    img, _, n = ER.erase_image(SR.pack(s), 0, np.array([1, 2], np.uint32), False)
    a = SR.unpack(img)["tables"][0]
    assert n == 2 and a["freed"] == [2, 1] and a["fresh_next"] == 3
    img, _, n = ER.erase_image(SR.pack(s), 0, np.array([2, 1], np.uint32), False)
    a = SR.unpack(img)["tables"][0]
    assert n == 2 and a["freed"] == [] and a["fresh_next"] == 1
    assert accounted(a)
    # behind an older freed index the erased fresh_next - 1 stays in freed[]
    t0 = ER.small(kind)["tables"][0]
    top = t0["fresh_next"] - 1
    assert top in t0["lru"] and t0["freed"]
    img, _, _ = ER.erase_image(SR.pack(ER.small(kind)), 0, np.array([top], np.uint32), False)
    a = SR.unpack(img)["tables"][0]
    assert a["freed"] == [top] + t0["freed"] and a["fresh_next"] == t0["fresh_next"]


def test_query_builders_cover_their_classes():
    rng = np.random.default_rng(3)
    s = ER.small("lb")
    t = s["tables"][0]
    keys = ER.key_queries("lb", 0, t, rng, 5)
    rows = [k.tobytes() for k in keys]
    assert len(set(rows)) < len(rows)                      # named twice
    assert any(r not in t["key"] and not any(r[13:]) for r in rows)  # a miss
    assert sum(any(r[13:]) for r in rows) == 1             # one pad bit
    idx = ER.index_queries(t, rng, 5).tolist()
    assert t["capacity"] in idx and 0xFFFFFFFF in idx
    assert any(i in t["freed"] for i in idx) and any(t["fresh_next"] <= i < t["capacity"] for i in idx)
    assert len(set(idx)) < len(idx)
