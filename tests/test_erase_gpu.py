"""vp_table_erase / vp_table_free on the GPU (include/vigpath.h, DESIGN.md
§5.17) against tests/eraseref.py: the image after an erase byte for byte, the
outputs and n_erased exactly, for every NF, both variants of the two-act
traces (tests/statecases.py) and viglb's both tables, at the cut between the
acts; the continuation of an erased context against a twin that loaded the
reference's image, through vp_process_device and the resident kernel; the free
order against an expiry's; deltas across an erase; the shapes at which the
rank can go wrong; the purge; the refusals.

The rank's geometry is 512 consecutive queries per wave and 2048 per block
(vp_slots_dev.h), the resolve's 64 lanes per wave and 256 per block with a
grid of at most 2048 blocks: the shape test takes n on both sides of all of
these."""
import ctypes as C

import numpy as np
import pytest
import torch

import eraseref as ER
import statecases as SC
import stateref as SR
import vigor_amd
from test_state_gpu import feed, make_pair, one

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
ARRAYS = ("index", "ts", "key", "value")
CASES = [(k, v) for k in SC.KINDS for v in SC.VARIANTS]


def ntables(kind):
    return 2 if kind == "lb" else 1


_traces = {}


def trace(kind, variant):
    """statecases.trace, made once per case and left unchanged."""
    if (kind, variant) not in _traces:
        _traces[kind, variant] = SC.trace(kind, variant)
    return _traces[kind, variant]


def at_cut(kind, variant):
    """A context after act 1 of the trace."""
    tr, cut = trace(kind, variant)
    nf, _ = make_pair(kind, **SC.pair_args(kind, variant))
    feed(nf, tr, 0, cut)
    return nf


def same(got, exp, what):
    for a in ARRAYS:
        assert got[a].dtype == exp[a].dtype and got[a].shape == exp[a].shape, (what, a)
        bad = np.unique(np.nonzero(got[a] != exp[a])[0])
        assert bad.size == 0, "%s: %s differs at queries %s: %s vs %s" % (
            what, a, bad[:8], got[a][bad[:8]].tolist(), exp[a][bad[:8]].tolist())


def erase_checked(nf, table, q, by_key, what):
    """One call against the reference over the image before it; the image
    afterwards."""
    before = nf.save_state()
    want, out, k = ER.erase_image(before, table, q, by_key)
    got = nf.erase(q, table) if by_key else nf.free(q, table)
    print("%s: n = %d, n_erased %d (reference %d)" % (what, len(q), got["n_erased"], k))
    assert got["n_erased"] == k, what
    same(got, out, what)
    after = nf.save_state()
    assert after == want, "%s: the image is not the reference's" % what
    return after, k


def erase_some(kind, nf, seed=7):
    """By key and then by index on every table, about a third of the live
    entries each, every call checked; the queries sent, and the image."""
    rng = np.random.default_rng(seed)
    sent, img, total = [], None, 0
    for table in range(ntables(kind)):
        for by_key in (True, False):
            t = SR.unpack(nf.save_state())["tables"][table]
            n_hits = max(1, len(t["lru"]) // 3)
            q = (ER.key_queries(kind, table, t, rng, n_hits) if by_key
                 else ER.index_queries(t, rng, n_hits))
            img, k = erase_checked(nf, table, q, by_key,
                                   "%s table %d by %s" % (kind, table, "key" if by_key else "index"))
            assert k == min(n_hits, len(t["lru"]))
            total += k
            sent.append((table, q, by_key))
    return sent, img, total


# ------------------------------------------------------------- 1 image --

@pytest.mark.parametrize("kind,variant", CASES)
def test_image_outputs_and_repeat(kind, variant):
    nf = at_cut(kind, variant)
    live = [nf.table_stats(t)["live"] for t in range(ntables(kind))]
    sent, img, total = erase_some(kind, nf)
    assert sum(nf.table_stats(t)["live"] for t in range(ntables(kind))) == sum(live) - total
    # the same queries again: nothing live is named
    for table, q, by_key in sent:
        got = nf.erase(q, table) if by_key else nf.free(q, table)
        assert got["n_erased"] == 0 and (got["index"] == ER.MISS).all()
        assert not got["ts"].any() and not got["key"].any() and not got["value"].any()
    assert nf.save_state() == img


# ------------------------------------------------------ 2 continuation --

def run_device(nf, tr, cut):
    n = tr[1].shape[0]
    frames, outs = [], []
    for x, y in zip([cut, cut + 1, cut + 7, cut + 500], [cut + 1, cut + 7, cut + 500, n]):
        gf, go = feed(nf, tr, x, y)
        frames.append(gf.reshape(-1, 64))
        outs.append(go)
    return np.concatenate(frames), np.concatenate(outs)


def run_resident(nf, tr, cut):
    fr, ln, dv, now = tr
    F = fr.reshape(-1, 64)
    rows, outs = [], []
    for p in range(cut, ln.shape[0]):
        got, row = one(nf, F[p], ln[p], dv[p], now[p])
        outs.append(got)
        rows.append(row.copy())
    assert nf.serve_stats()["packets_one"] > 0
    return np.stack(rows), np.array(outs)


@pytest.mark.parametrize("path", ["device", "resident"])
@pytest.mark.parametrize("kind,variant", CASES)
def test_continuation_equals_the_loaded_twin(kind, variant, path):
    """The allocation order after an erase, and so vignat's external ports:
    act 2 on the erased context and on a twin that loaded the image the
    reference made."""
    tr, cut = trace(kind, variant)
    a = at_cut(kind, variant)
    before = a.save_state()
    sent, img, total = erase_some(kind, a)
    assert total > 0
    ref = before
    for table, q, by_key in sent:
        ref, _, _ = ER.erase_image(ref, table, q, by_key)
    assert ref == img
    b, _ = make_pair(kind, **SC.pair_args(kind, variant))
    b.load_state(ref)
    run = run_device if path == "device" else run_resident
    fa, oa = run(a, tr, cut)
    fb, ob = run(b, tr, cut)
    bad = np.nonzero(oa != ob)[0]
    assert bad.size == 0, "out ports differ at packets %s" % (bad[:10] + cut)
    badf = np.nonzero((fa != fb).any(axis=1))[0]
    assert badf.size == 0, "frames differ at packets %s" % (badf[:10] + cut)
    assert a.save_state() == b.save_state()


# ----------------------------------------------------- 3 against expiry --

def expire_ns(kind, variant, table):
    return SC.EXPIRE_US[variant] * 1000 * (40 if table == 1 else 1)


def ipv4_packet(tr, cut):
    """The first packet of act 2 that every NF parses to its expiry: IPv4,
    with a whole header."""
    fr, ln, dv, now = tr
    F = fr.reshape(-1, 64)
    for p in range(cut, ln.shape[0]):
        if ln[p] >= 60 and F[p, 12] == 0x08 and F[p, 13] == 0x00 and F[p, 14] == 0x45:
            return p
    raise AssertionError("no IPv4 packet in act 2")


@pytest.mark.parametrize("kind,variant", CASES)
def test_freeing_the_oldest_equals_their_expiry(kind, variant):
    tr, cut = trace(kind, variant)
    p = ipv4_packet(tr, cut)
    fr, ln, dv, now = tr
    for table in range(ntables(kind)):
        a, b = at_cut(kind, variant), at_cut(kind, variant)
        st = SR.unpack(a.save_state())
        t = st["tables"][table]
        E = expire_ns(kind, variant, table)
        # the largest k in the older half with ts[k - 1] < ts[k] whose packet
        # time is not before last_now
        ks = [k for k in range(1, len(t["lru"])) if t["ts"][k - 1] < t["ts"][k] and
              t["ts"][k] + E >= st["last_now"]]
        assert ks, (kind, variant, table)
        k = max([x for x in ks if x <= max(ks[0], len(t["lru"]) // 2)])
        T = t["ts"][k] + E  # cutoff T - E = ts[k]: exactly lru[:k] are older
        got = a.free(np.array(t["lru"][:k], np.uint32), table)
        assert got["n_erased"] == k
        one_tr = (fr[p * 64:(p + 1) * 64], ln[p:p + 1], dv[p:p + 1], np.array([T], np.int64))
        feed(a, one_tr, 0, 1)
        feed(b, one_tr, 0, 1)
        ia, ib = a.save_state(), b.save_state()
        tb = SR.unpack(ib)["tables"][table]
        assert not set(t["lru"][:k]) & set(tb["lru"]) - set(tb["lru"][-1:]), "B did not expire them"
        assert ia == ib, "%s %s table %d: freeing lru[:%d] is not their expiry" % (
            kind, variant, table, k)


# ------------------------------------------------------------ 4 deltas --

def raw_apply(nf, blob):
    buf = np.frombuffer(blob, np.uint8)
    rc = nf.L.vp_state_delta_apply(nf.h, C.c_void_p(buf.ctypes.data), buf.size)
    return rc, nf.L.vp_last_error().decode()


@pytest.mark.parametrize("kind", SC.KINDS)
def test_deltas_across_an_erase(kind):
    args = SC.pair_args(kind, "part")
    p = at_cut(kind, "part")
    m0, img0 = p.state_mark(), p.save_state()

    def standby():
        s, _ = make_pair(kind, **args)
        s.load_state(img0)
        s.follow(m0)
        return s

    s1, s2 = standby(), standby()
    sent, img, total = erase_some(kind, p)
    assert total > 0
    m1 = p.state_mark()
    assert m1[1] == m0[1] and m1[0] == m0[0] + len(sent), (m0, m1)  # one step per erasing call
    blob, end = p.save_delta(m0)
    assert end == m1
    s1.apply_delta(blob)
    assert s1.save_state() == img
    # misses alone change neither mark nor following
    t = SR.unpack(img0)["tables"][0]
    absent = np.frombuffer(t["key"][0], np.uint8).copy()
    absent[0] ^= 0x40
    assert absent.tobytes() not in t["key"]
    mark = s2.state_mark()
    got = s2.erase(absent.reshape(1, 16))
    assert got["n_erased"] == 0 and s2.state_mark() == mark
    got = s2.free(np.array([t["capacity"], 0xFFFFFFFF], np.uint32))
    assert got["n_erased"] == 0 and s2.state_mark() == mark
    s2.apply_delta(blob)
    assert s2.save_state() == img
    # an erase on a following context ends the following
    t = SR.unpack(img)["tables"][0]
    got = s2.free(np.array(t["lru"][:1], np.uint32))
    assert got["n_erased"] == 1
    after = s2.save_state()
    blob2, _ = p.save_delta(m1)
    rc, err = raw_apply(s2, blob2)
    assert rc == EINVAL and err == "state delta apply: the context follows no mark", (rc, err)
    assert s2.save_state() == after


# ------------------------------------------------------------ 5 shapes --

@pytest.fixture(scope="module")
def fw_full():
    """vigfw at the cut of the "full" trace: its image, and a context to load
    it into per case."""
    nf = at_cut("fw", "full")
    img = nf.save_state()
    t = SR.unpack(img)["tables"][0]
    assert len(t["lru"]) >= 200
    return nf, img, t


EDGES = (0, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049)


def shaped_queries(t, n, by_key, rng):
    """n queries: a first occurrence of its own live entry at every edge
    position below n and at n - 1, in random entry order; elsewhere a repeat
    of an earlier winner or a miss, by turns."""
    order = rng.permutation(len(t["lru"]))
    cap = t["capacity"]
    if by_key:
        ent = [np.frombuffer(t["key"][j], np.uint8) for j in order]
        miss = ent[0].copy()
        miss[0] ^= 0x21
        assert miss.tobytes() not in t["key"]
        q = np.zeros((n, 16), np.uint8)
    else:
        ent = [t["lru"][j] for j in order]
        miss = cap + 1
        q = np.zeros(n, np.uint32)
    at = sorted({e for e in EDGES if e < n} | {n - 1})
    used = 0
    for pos in range(n):
        if pos in at:
            q[pos] = ent[used]
            used += 1
        elif used and pos % 2:
            q[pos] = ent[pos % used]
        else:
            q[pos] = miss
    return q, used


@pytest.mark.parametrize("by_key", [True, False])
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 512, 513, 2048, 2049])
def test_shapes(fw_full, n, by_key):
    nf, img, t = fw_full
    nf.load_state(img)
    q, winners = shaped_queries(t, n, by_key, np.random.default_rng(n))
    _, k = erase_checked(nf, 0, q, by_key, "n = %d" % n)
    assert k == winners


@pytest.mark.parametrize("by_key", [True, False])
def test_grid_stride(fw_full, by_key):
    """524,288 + 300 queries, beyond the resolve's 2048 blocks of 256: mostly
    misses and repeats, and the last 300 hold the only first occurrences of a
    few entries."""
    nf, img, t = fw_full
    nf.load_state(img)
    rng = np.random.default_rng(5)
    n0, n1 = 2048 * 256, 300
    order = rng.permutation(len(t["lru"]))
    early, late = order[:100], order[100:108]
    if by_key:
        ent = np.stack([np.frombuffer(k, np.uint8) for k in t["key"]])
        miss = ent[0].copy()
        miss[1] ^= 0x12
        assert miss.tobytes() not in t["key"]
        pool = np.concatenate([ent[early], np.tile(miss, (60, 1))])
    else:
        ent = np.array(t["lru"], np.uint32)
        pool = np.concatenate([ent[early], np.full(60, t["capacity"] + 7, np.uint32)])
    q = np.concatenate([pool[rng.integers(0, pool.shape[0], n0)],
                        pool[rng.integers(0, pool.shape[0], n1)]])
    where = n0 + np.sort(rng.permutation(n1)[:2 * late.size])
    q[where] = np.concatenate([ent[late], ent[late]])[rng.permutation(2 * late.size)]
    _, k = erase_checked(nf, 0, q, by_key, "n = %d" % (n0 + n1))
    assert k == early.size + late.size


# ------------------------------------------------------------- 6 purge --

def purge_bound(stats, cap):
    """tbl_purge_bound: 85 % of the entries of one bucket per index (the power
    of two at or above the capacity, at least 64), or of the table when it is
    smaller; three entries per bucket."""
    base = 64
    while base < cap:
        base *= 2
    return min(stats["buckets"], base) * 3 * 85 // 100


@pytest.mark.parametrize("sparse", [None, "-1"])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_erase_everything_and_purge(kind, sparse, monkeypatch):
    """sparse: VIGPATH_SPARSE=-1 halves the buckets (128 of 3 entries for 256
    indices), which lowers the bound from 652 entries to 326."""
    if sparse:
        monkeypatch.setenv("VIGPATH_SPARSE", sparse)
    tr, cut = trace(kind, "full")
    a = at_cut(kind, "full")
    before = a.save_state()
    t = SR.unpack(before)["tables"][0]
    st0 = a.table_stats()
    assert st0["live"] == len(t["lru"]) == SC.CAP
    rng = np.random.default_rng(9)
    keys = np.stack([np.frombuffer(k, np.uint8) for k in t["key"]])[rng.permutation(SC.CAP)]
    img, k = erase_checked(a, 0, keys, True, "%s: every live entry" % kind)
    st1 = a.table_stats()
    assert k == SC.CAP and st1["live"] == 0 and st1["shard_live"] == 0
    crossed = st0["tombstones"] + SC.CAP > purge_bound(st0, SC.CAP)
    print("%s: %d buckets, tombstones %d + %d erased, bound %d, rebuilds %d -> %d" % (
        kind, st0["buckets"], st0["tombstones"], SC.CAP, purge_bound(st0, SC.CAP), st0["rebuilds"],
        st1["rebuilds"]))
    assert (st1["rebuilds"] > st0["rebuilds"]) == crossed
    assert st1["tombstones"] == (0 if crossed else st0["tombstones"] + SC.CAP)
    b, _ = make_pair(kind, **SC.pair_args(kind, "full"))
    b.load_state(img)
    fa, oa = run_device(a, tr, cut)
    fb, ob = run_device(b, tr, cut)
    assert np.array_equal(oa, ob) and np.array_equal(fa, fb)
    assert a.save_state() == b.save_state()


# ---------------------------------------------------------- 7 refusals --

@pytest.mark.parametrize("by_key", [True, False])
def test_refusals(fw_full, by_key):
    nf, img, t = fw_full
    nf.load_state(img)
    img = nf.save_state()
    d = torch.device("cuda:0")
    n = 8
    name = "vp_table_erase" if by_key else "vp_table_free"
    arg = "keys" if by_key else "idx"
    fn = getattr(nf.L, name)
    # live entries: a call that got through would erase them
    if by_key:
        live = np.frombuffer(b"".join(t["key"][:n]), np.uint8)
    else:
        live = np.array(t["lru"][:n], np.uint32).view(np.uint8)
    src = torch.zeros(16 * n + 64, dtype=torch.uint8, device=d)
    src[:live.size] = torch.from_numpy(live.copy()).to(d)
    shifted = torch.zeros(16 * n + 64, dtype=torch.uint8, device=d)
    off = 8 if by_key else 2
    shifted[off:off + live.size] = torch.from_numpy(live.copy()).to(d)
    bufs = {a: torch.full((16 * n + 64,), 0xA5, dtype=torch.uint8, device=d) for a in ARRAYS}

    def out(**shift):
        return vigor_amd.VpLookupOutC(**{a: bufs[a].data_ptr() + shift.get(a, 0) for a in ARRAYS})

    p = src.data_ptr()
    cases = [
        (dict(table=1, src=p, out=out()), "%s: table 1: this NF has table 0 only" % name),
        (dict(table=-1, src=p, out=out()), "%s: table -1: this NF has table 0 only" % name),
        (dict(table=0, src=None, out=out()), "%s: %s is NULL with n = 8" % (name, arg)),
        (dict(table=0, src=shifted.data_ptr() + off, out=out()),
         "%s: %s is not %d-byte aligned" % (name, arg, 16 if by_key else 4)),
        (dict(table=0, src=p, out=out(index=2)), "%s: out->index is not 4-byte aligned" % name),
        (dict(table=0, src=p, out=out(ts=4)), "%s: out->ts is not 8-byte aligned" % name),
        (dict(table=0, src=p, out=out(key=8)), "%s: out->key is not 16-byte aligned" % name),
        (dict(table=0, src=p, out=out(value=2)), "%s: out->value is not 4-byte aligned" % name),
    ]
    mark = nf.state_mark()
    for kw, text in cases:
        k = C.c_uint32(77)
        rc = fn(nf.h, kw["table"], n, kw["src"], C.byref(kw["out"]), C.byref(k), None)
        err = nf.L.vp_last_error().decode()
        torch.cuda.synchronize()
        assert rc == EINVAL and err == text, (kw, rc, err)
        assert k.value == 77
        for b in bufs.values():
            assert (b == 0xA5).all(), "a refused call wrote an output array"
        assert nf.save_state() == img and nf.state_mark() == mark, text
    k = C.c_uint32(77)
    assert fn(None, 0, n, p, C.byref(out()), C.byref(k), None) == EINVAL
    assert nf.L.vp_last_error().decode() == "%s: ctx is NULL" % name and k.value == 77
    # n == 0: VP_OK, nothing launched, *n_erased = 0; out and n_erased may be NULL
    assert fn(nf.h, 0, 0, None, C.byref(out()), C.byref(k), None) == 0 and k.value == 0
    assert fn(nf.h, 0, 0, None, None, None, None) == 0
    for b in bufs.values():
        assert (b == 0xA5).all()
    assert nf.save_state() == img and nf.state_mark() == mark
    # out == NULL and n_erased == NULL: the erase happens all the same
    assert fn(nf.h, 0, n, p, None, None, None) == 0
    want, _, erased = ER.erase_image(img, 0, live.reshape(n, 16) if by_key else live.view(np.uint32),
                                     by_key)
    assert erased == n and nf.save_state() == want


def test_attached_context_is_not_supported():
    nat, _ = make_pair("nat", max_flows=256)

    def allgather(user, send, recv, nbytes):
        if nbytes:
            C.memmove(recv, send, nbytes)
        return 0

    ag = vigor_amd.ALLGATHER_FN(allgather)
    ar = vigor_amd.ALLREDUCE_FN(lambda user, buf, count: 0)
    ops = vigor_amd.CommOpsC(user=None, allgather=ag, allreduce_max_u64=ar)
    assert nat.L.vp_attach_comm(nat.h, C.byref(ops), 1, 0) == 0
    d = torch.device("cuda:0")
    keys = torch.zeros(32, dtype=torch.uint8, device=d)
    index = torch.full((2,), 0x5A5A5A5A, dtype=torch.int32, device=d)
    o = vigor_amd.VpLookupOutC(index=index.data_ptr())
    k = C.c_uint32(77)
    assert nat.L.vp_table_erase(nat.h, 0, 2, keys.data_ptr(), C.byref(o), C.byref(k), None) == ENOTSUP
    assert nat.L.vp_table_free(nat.h, 0, 2, keys.data_ptr(), C.byref(o), C.byref(k), None) == ENOTSUP
    torch.cuda.synchronize()
    assert (index == 0x5A5A5A5A).all() and k.value == 77
