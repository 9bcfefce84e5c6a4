"""tests/lookupref.py against the oracle's dump, and the census of the query
sets tests/test_lookup_gpu.py relies on. CPU only.

Three points per statecases trace (lookupref.trace_points): right before the
first expiry, at the cut between the two acts, and at the end. The reference
is checked against the dump by index directly: every live key maps to its
index, every index back to its key, a key of an expired flow misses, a re-used
index returns its new key.

The census. The figures are: 32 hits, 32 misses among absent keys, 8 keys of
expired flows, 8 live keys with a pad byte set (vignat's key has no pad), 4
duplicates; 16 live indices, 16 free ones below fresh_next, 4 of the
never-used tail, the capacity and 0xFFFFFFFE. A state cannot supply a class it
does not hold: before the first expiry no flow has expired and no index is
free below fresh_next, and the "full" variant's table has neither a free index
nor a tail. So every figure is asserted in full at the "part" variant's cut,
where statecases guarantees all of them, and everywhere else as the smaller
of the figure and what the state holds (counted here from the dump, not from
the query builder)."""
import numpy as np
import pytest

import lookupref as LR
import statecases as SC

FIG = dict(hits=32, absent=32, gone=8, padded=8, dup=4)
IFIG = dict(live=16, free=16, tail=4)
POINTS = (LR.BEFORE, LR.CUT, LR.END)


def _ntables(kind):
    return 2 if kind == "lb" else 1


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_reference_against_the_dump(kind, variant, point):
    _, pts, _ = LR.trace_points(kind, variant)
    pt = pts[point]
    st = pt["state"]
    for table in range(_ntables(kind)):
        t = st["tables"][table]
        cap, n = t["capacity"], len(t["lru"])
        # every live key maps to its index, stamp and value
        keys = np.stack([np.frombuffer(k, np.uint8) for k in t["key"]]) if n else \
            np.zeros((0, 16), np.uint8)
        r = LR.by_key(st, table, keys)
        assert r["index"].tolist() == t["lru"] and r["ts"].tolist() == t["ts"]
        assert np.array_equal(r["key"], keys)
        assert [bytes(v) for v in r["value"]] == t["value"]
        # every index maps back: the live ones to their key, the others miss
        r = LR.by_index(st, table, np.arange(cap + 2, dtype=np.uint32))
        live = np.zeros(cap + 2, bool)
        live[t["lru"]] = True
        assert np.array_equal(r["index"][live], np.nonzero(live)[0])
        assert (r["index"][~live] == LR.MISS).all()
        assert not r["ts"][~live].any() and not r["key"][~live].any()
        assert not r["value"][~live].any()
        where = {i: j for j, i in enumerate(t["lru"])}
        for i in np.nonzero(live)[0]:
            assert bytes(r["key"][i]) == t["key"][where[int(i)]]
            assert int(r["ts"][i]) == t["ts"][where[int(i)]]
        # a key of an expired flow misses
        gone = pt["gone"][table]
        if gone:
            g = np.stack([np.frombuffer(k, np.uint8) for k in gone])
            r = LR.by_key(st, table, g)
            assert (r["index"] == LR.MISS).all() and not r["key"].any() and not r["ts"].any()
    # a re-used index returns the key it holds now
    t = st["tables"][0]
    where = {i: j for j, i in enumerate(t["lru"])}
    r = LR.by_index(st, 0, np.array(pt["reused"], np.uint32))
    for q, i in enumerate(pt["reused"]):
        assert bytes(r["key"][q]) == t["key"][where[i]]
    if point != LR.BEFORE:
        assert len(pt["reused"]) >= 8, "no index was re-used"


@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_census(kind, variant, point):
    _, pts, _ = LR.trace_points(kind, variant)
    pt = pts[point]
    st = pt["state"]
    t = st["tables"][0]
    full = variant == "part" and point == LR.CUT
    keys, cls = LR.lookup_queries(kind, st, 0, pt["gone"][0])
    n_live, kb = len(t["lru"]), LR.KEY_BYTES[kind][0]
    have = dict(hits=n_live, absent=FIG["absent"], gone=len(pt["gone"][0]),
                padded=n_live if kb < 16 else 0, dup=FIG["dup"])
    fig = {c: len(q) for c, q in cls.items()}
    print(kind, variant, pt["packets"], fig)
    for c, want in FIG.items():
        if c == "padded" and kb == 16:
            assert fig[c] == 0
            continue
        assert fig[c] >= (want if full else min(want, have[c])), (c, fig)
    # the classes are what they say
    r = LR.by_key(st, 0, keys)
    held = set(t["key"])
    assert (r["index"][cls["hits"]] != LR.MISS).all()
    for c in ("absent", "gone", "padded"):
        assert (r["index"][cls[c]] == LR.MISS).all(), c
        assert all(bytes(keys[q]) not in held for q in cls[c])
    for q in cls["padded"]:
        k = keys[q].copy()
        assert k[kb:].any()
        k[kb:] = 0
        assert bytes(k) in held
    for q in cls["dup"]:
        assert any(np.array_equal(keys[q], keys[j]) for j in range(len(keys)) if j != q)
    # the indices
    idx, ic = LR.index_queries(st, 0)
    cap, fresh = t["capacity"], t["fresh_next"]
    ihave = dict(live=n_live, free=fresh - n_live, tail=cap - fresh)
    ifig = {c: len(q) for c, q in ic.items()}
    print(kind, variant, pt["packets"], ifig)
    for c, want in IFIG.items():
        assert ifig[c] >= (want if full else min(want, ihave[c])), (c, ifig)
    assert cap in idx.tolist() and 0xFFFFFFFE in idx.tolist()
    live = set(t["lru"])
    assert all(int(idx[q]) in live for q in ic["live"])
    assert all(int(idx[q]) not in live and int(idx[q]) < fresh for q in ic["free"])
    assert all(fresh <= int(idx[q]) < cap for q in ic["tail"])
    r = LR.by_index(st, 0, idx)
    assert (r["index"][ic["live"]] == idx[ic["live"]]).all()
    for c in ("free", "tail", "beyond"):
        assert (r["index"][ic[c]] == LR.MISS).all()


@pytest.mark.parametrize("variant", SC.VARIANTS)
def test_lb_backends_are_queried_too(variant):
    _, pts, _ = LR.trace_points("lb", variant)
    for pt in pts:
        keys, cls = LR.lookup_queries("lb", pt["state"], 1, pt["gone"][1])
        n = len(pt["state"]["tables"][1]["lru"])
        assert n >= 8 and len(cls["hits"]) == n and len(cls["padded"]) >= 8
        assert len(cls["absent"]) >= 8
