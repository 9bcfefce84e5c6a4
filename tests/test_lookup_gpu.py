"""vp_table_lookup / vp_table_entries on the GPU (include/vigpath.h, DESIGN.md
§5.16) against tests/lookupref.py over the oracle's dump, array by array and
exactly, for every NF and viglb's both tables; a query changes nothing (the
state image before and after it is the same bytes). The traces, the points at
which the tests look up and the census of the query sets: tests/lookupref.py,
tests/test_lookup_ref.py.

The second point is the cut between the traces' two acts, packet 2000, many
expiries after the first one: the "part" variant's table holds tombstones
there (asserted), so the probe has to pass over erased entries.

One pass of the lookup kernels' grid is 2048 blocks of 256 lanes, so the
largest n of the shape test is 2048 * 256 + 1."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import lookupref as LR
import statecases as SC
import stateref as SR
import vigor_amd
from gpuh import dumps_equal
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
ONE_PASS = 2048 * 256
ARRAYS = ("index", "ts", "key", "value")


def make_pair(kind, **args):
    return importlib.import_module("test_%s_gpu" % kind).make_pair(**args)


def ntables(kind):
    return 2 if kind == "lb" else 1


def feed(nf, tr, a, b, slot=64):
    """Packets [a, b) of a trace as one device batch (nothing waited for
    beyond what vp_process_device itself waits for)."""
    fr, ln, dv, now = tr
    d = torch.device("cuda:0")
    f = torch.from_numpy(fr[a * slot:b * slot].copy()).to(d)
    l_ = torch.from_numpy(ln[a:b].astype(np.uint16).view(np.int16)).to(d)
    i_ = torch.from_numpy(dv[a:b].astype(np.uint16).view(np.int16)).to(d)
    o = torch.zeros(b - a, dtype=torch.int16, device=d)
    nf.process_device(f, l_, i_, o, slot, now=torch.from_numpy(now[a:b].astype(np.int64)).to(d))


def one(nf, row, ln, dv, now):
    """vp_process_one of a frame of ln bytes whose first 64 are `row` (zero
    behind, as the traces' slots are)."""
    buf = np.zeros(max(int(ln), 64), np.uint8)
    buf[:64] = row
    out = C.c_uint16(0)
    nf._ck(nf.L.vp_process_one(nf.h, int(dv), C.c_void_p(buf.ctypes.data), int(ln), int(now),
                               C.byref(out)), "vp_process_one")


def same(got, exp, what):
    for a in ARRAYS:
        assert got[a].dtype == exp[a].dtype and got[a].shape == exp[a].shape, (what, a)
        bad = np.unique(np.nonzero(got[a] != exp[a])[0])
        assert bad.size == 0, "%s: %s differs at queries %s: %s vs %s" % (
            what, a, bad[:8], got[a][bad[:8]].tolist(), exp[a][bad[:8]].tolist())


def check_point(kind, nf, pt, what):
    """Both calls on every table against the reference, and the state image
    unchanged by them."""
    before = nf.save_state()
    for table in range(ntables(kind)):
        st = pt["state"]
        w = "%s, table %d, %s" % (what, table, nf.table_stats(table))
        assert nf.value_size(table) == st["tables"][table]["value_size"]
        keys, _ = LR.lookup_queries(kind, st, table, pt["gone"][table])
        same(nf.lookup(keys, table), LR.by_key(st, table, keys), "lookup " + w)
        idx, _ = LR.index_queries(st, table)
        same(nf.entries(idx, table), LR.by_index(st, table, idx), "entries " + w)
    assert nf.save_state() == before, "%s: the queries changed the state" % what


def dumps_match(kind, nf, o):
    got, exp = nf.dump(), SC.dump(kind, o)
    for g, e in (zip(got, exp) if kind == "lb" else [(got, exp)]):
        dumps_equal(g, e)


# ------------------------------------------------- 1 along the batch path --

@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_lookup_along_the_batch_path(kind, variant):
    tr, pts, o = LR.trace_points(kind, variant)
    nf, _ = make_pair(kind, **SC.pair_args(kind, variant))
    at = 0
    for name in (LR.BEFORE, LR.CUT, LR.END):
        pt = pts[name]
        feed(nf, tr, at, pt["packets"])
        at = pt["packets"]
        if variant == "part" and name == LR.CUT:
            st = nf.table_stats()
            assert st["tombstones"] > 0, st
        check_point(kind, nf, pt, "%s %s at packet %d" % (kind, variant, at))
    dumps_match(kind, nf, o)


# ------------------------------------------------------- 2 after a load --

@pytest.mark.parametrize("kind", SC.KINDS)
def test_lookup_after_load_state(kind):
    tr, pts, _ = LR.trace_points(kind, "part")
    pt = pts[LR.CUT]
    a, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    feed(a, tr, 0, pt["packets"])
    b, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    b.load_state(a.save_state())
    check_point(kind, b, pt, "%s after load_state, layout %d" % (kind, b.table_stats()["layout"]))


# ------------------------------------------------ 3 the resident kernel --

@pytest.mark.parametrize("kind", SC.KINDS)
def test_lookup_between_served_packets(kind):
    tr, pts, o = LR.trace_points(kind, "part")
    fr, ln, dv, now = tr
    F = fr.reshape(-1, 64)
    cut, mid, n = pts[LR.CUT]["packets"], pts[LR.INSIDE]["packets"], ln.shape[0]
    nf, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    feed(nf, tr, 0, cut)
    for p in range(cut, mid):
        one(nf, F[p], ln[p], dv[p], now[p])
    served = nf.serve_stats()
    assert served["packets_one"] > 0, served
    check_point(kind, nf, pts[LR.INSIDE], "%s after %d served packets" % (kind, mid - cut))
    assert nf.serve_stats() == served
    for p in range(mid, n):
        one(nf, F[p], ln[p], dv[p], now[p])
    assert nf.serve_stats()["packets_one"] > served["packets_one"]
    dumps_match(kind, nf, o)
    check_point(kind, nf, pts[LR.END], "%s at the end" % kind)


# ---------------------------------------------------- 4 affine-time fold --

def test_vignat_lookup_straight_after_affine_batches():
    cap, n, flows = 4096, 8192, 1500
    nf, o = make_pair("nat", max_flows=cap)
    fr, ln, dv, _ = T.nat_lan_trace(2 * n, flows)
    d = torch.device("cuda:0")
    step = 100
    for b in range(2):
        sl = slice(b * n, (b + 1) * n)
        now = T.NOW0 + step * np.arange(b * n, (b + 1) * n, dtype=np.int64)
        o.run(fr[b * n * 64:(b + 1) * n * 64].copy(), ln[sl], dv[sl], now, 64)
        f = torch.from_numpy(fr[b * n * 64:(b + 1) * n * 64].copy()).to(d)
        l_ = torch.from_numpy(ln[sl].astype(np.uint16).view(np.int16)).to(d)
        i_ = torch.from_numpy(dv[sl].astype(np.uint16).view(np.int16)).to(d)
        out = torch.zeros(n, dtype=torch.int16, device=d)
        nf.process_device(f, l_, i_, out, 64, now0=int(now[0]), now_step=step)
        # (no synchronisation here: the call's own wait is what is tested)
        alloc, ts, keys = o.nat_dump(cap)
        live = np.nonzero(alloc)[0]
        st = {"kind": "nat", "last_now": int(now[-1]), "tables": SR.tables_from_dump(
            "nat", (alloc, ts, keys), lru=live[np.argsort(ts[live], kind="stable")], freed=(),
            fresh_next=int(live.size))}
        assert live.size == flows
        q, _ = LR.lookup_queries("nat", st, 0, ())
        same(nf.lookup(q), LR.by_key(st, 0, q), "lookup after affine batch %d" % b)
        idx = np.arange(flows + 3, dtype=np.uint32)
        same(nf.entries(idx), LR.by_index(st, 0, idx), "entries after affine batch %d" % b)


# ------------------------------------------------------------- 5 shapes --

@pytest.fixture(scope="module")
def fw_at_cut():
    tr, pts, _ = LR.trace_points("fw", "part")
    pt = pts[LR.CUT]
    nf, _ = make_pair("fw", **SC.pair_args("fw", "part"))
    feed(nf, tr, 0, pt["packets"])
    st = pt["state"]
    keys, _ = LR.lookup_queries("fw", st, 0, pt["gone"][0])
    idx, _ = LR.index_queries(st, 0)
    return nf, keys, LR.by_key(st, 0, keys), idx, LR.by_index(st, 0, idx)


def _device_query(nf, by_key, src, n, want=ARRAYS, shift=16):
    """The device call with every array `shift` bytes into its allocation
    (16-byte but not 64-byte aligned for the default) and 64 guard bytes of
    0xA5 behind it; None for the arrays not in `want`."""
    d = torch.device("cuda:0")
    width = {"index": 4, "ts": 8, "key": 16, "value": nf.value_size(0)}

    def room(nbytes):
        t = torch.full((shift + nbytes + 64,), 0xA5, dtype=torch.uint8, device=d)
        assert t.data_ptr() % 64 == 0
        return t

    raw = np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    s = room(raw.size)
    s[shift:shift + raw.size] = torch.from_numpy(raw.copy()).to(d)
    out = {a: room(n * width[a]) for a in want}
    view = {a: out[a][shift:shift + n * width[a]] for a in want}
    typed = {a: (view[a].view(torch.int32) if a == "index" else
                 view[a].view(torch.int64) if a == "ts" else view[a]) for a in want}
    src_t = s[shift:shift + raw.size]
    if by_key:
        nf.lookup_device(src_t, table=0, **typed)
    else:
        nf.entries_device(src_t.view(torch.int32), table=0, **typed)
    got = {}
    for a in want:
        h = out[a].cpu().numpy()
        assert (h[:shift] == 0xA5).all() and (h[shift + n * width[a]:] == 0xA5).all(), a
        body = h[shift:shift + n * width[a]]
        got[a] = (body.view(np.uint32) if a == "index" else body.view(np.int64) if a == "ts"
                  else body.reshape(n, width[a]))
    return got


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, ONE_PASS + 1])
def test_shapes(fw_at_cut, n):
    nf, keys, kref, idx, iref = fw_at_cut
    for by_key, src, ref in ((True, keys, kref), (False, idx, iref)):
        sel = np.arange(n) % src.shape[0]
        got = _device_query(nf, by_key, src[sel], n)
        same(got, {a: ref[a][sel] for a in ARRAYS}, "n = %d, by_key = %s" % (n, by_key))


@pytest.mark.parametrize("want", [("ts", "key", "value"), ("index", "key", "value"),
                                  ("index", "ts", "value"), ("index", "ts", "key"), ()])
def test_any_output_may_be_null(fw_at_cut, want):
    nf, keys, kref, idx, iref = fw_at_cut
    for by_key, src, ref in ((True, keys, kref), (False, idx, iref)):
        got = _device_query(nf, by_key, src, src.shape[0], want)
        for a in want:
            assert np.array_equal(got[a], ref[a]), a


# ----------------------------------------------------------- 6 refusals --

def _raw(nf, by_key, table, n, src, out, guard):
    L = nf.L
    fn = L.vp_table_lookup if by_key else L.vp_table_entries
    rc = fn(nf.h, table, n, src, C.byref(out) if out is not None else None, None)
    torch.cuda.synchronize()
    for t in guard:
        assert (t == 0xA5).all(), "a refused call wrote an output array"
    return rc, L.vp_last_error().decode()


@pytest.mark.parametrize("by_key", [True, False])
def test_refusals(fw_at_cut, by_key):
    nf = fw_at_cut[0]
    d = torch.device("cuda:0")
    n = 8
    name = "vp_table_lookup" if by_key else "vp_table_entries"
    arg = "keys" if by_key else "idx"
    src = torch.zeros(16 * n + 64, dtype=torch.uint8, device=d)
    bufs = {a: torch.full((16 * n + 64,), 0xA5, dtype=torch.uint8, device=d) for a in ARRAYS}
    guard = list(bufs.values())

    def out(**shift):
        return vigor_amd.VpLookupOutC(**{a: bufs[a].data_ptr() + shift.get(a, 0) for a in ARRAYS})

    p = src.data_ptr()
    rc, _ = _raw(nf, by_key, 0, n, p, out(), [])
    assert rc == 0
    for t in guard:
        t.fill_(0xA5)
    cases = [
        (dict(table=0, n=n, src=p, out=None), "%s: out is NULL" % name),
        (dict(table=1, n=n, src=p, out=out()), "%s: table 1: this NF has table 0 only" % name),
        (dict(table=-1, n=n, src=p, out=out()), "%s: table -1: this NF has table 0 only" % name),
        (dict(table=0, n=n, src=None, out=out()), "%s: %s is NULL with n = 8" % (name, arg)),
        (dict(table=0, n=n, src=p + (8 if by_key else 2), out=out()),
         "%s: %s is not %d-byte aligned" % (name, arg, 16 if by_key else 4)),
        (dict(table=0, n=n, src=p, out=out(index=2)), "%s: out->index is not 4-byte aligned" % name),
        (dict(table=0, n=n, src=p, out=out(ts=4)), "%s: out->ts is not 8-byte aligned" % name),
        (dict(table=0, n=n, src=p, out=out(key=8)), "%s: out->key is not 16-byte aligned" % name),
        (dict(table=0, n=n, src=p, out=out(value=2)), "%s: out->value is not 4-byte aligned" % name),
    ]
    for kw, text in cases:
        rc, err = _raw(nf, by_key, kw["table"], kw["n"], kw["src"], kw["out"], guard)
        assert rc == EINVAL and err == text, (kw, rc, err)
    # n == 0: nothing to read, VP_OK, nothing written
    rc, _ = _raw(nf, by_key, 0, 0, None, out(), guard)
    assert rc == 0


def test_table_numbers():
    lb, _ = make_pair("lb", **SC.pair_args("lb", "part"))
    o = vigor_amd.VpLookupOutC()
    n = C.c_uint32()
    for table, rc in ((0, 0), (1, 0), (2, EINVAL)):
        assert lb.L.vp_table_lookup(lb.h, table, 0, None, C.byref(o), None) == rc
        assert lb.L.vp_table_entries(lb.h, table, 0, None, C.byref(o), None) == rc
        assert lb.L.vp_table_value_size(lb.h, table, C.byref(n)) == rc
    assert lb.L.vp_last_error().decode() == "vp_table_value_size: table 2: this NF has tables 0 and 1"
    assert (lb.value_size(0), lb.value_size(1)) == (4, 8)
    pol, _ = make_pair("pol", **SC.pair_args("pol", "part"))
    assert pol.value_size() == 16 and pol.L.vp_table_value_size(pol.h, 1, C.byref(n)) == EINVAL
    # vigpol's value is one 16-byte store per entry
    d = torch.device("cuda:0")
    val = torch.full((64,), 0xA5, dtype=torch.uint8, device=d)
    idx = torch.zeros(2, dtype=torch.int32, device=d)
    o = vigor_amd.VpLookupOutC(value=val.data_ptr() + 8)
    assert pol.L.vp_table_entries(pol.h, 0, 2, idx.data_ptr(), C.byref(o), None) == EINVAL
    assert pol.L.vp_last_error().decode() == "vp_table_entries: out->value is not 16-byte aligned"
    assert (val == 0xA5).all()
    nat, _ = make_pair("nat", max_flows=256)
    # vignat has no value: the pointer is never looked at
    o = vigor_amd.VpLookupOutC(value=val.data_ptr() + 1)
    assert nat.L.vp_table_entries(nat.h, 0, 2, idx.data_ptr(), C.byref(o), None) == 0
    torch.cuda.synchronize()
    assert (val == 0xA5).all()


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
    assert nat.L.vp_table_lookup(nat.h, 0, 2, keys.data_ptr(), C.byref(o), None) == ENOTSUP
    assert nat.L.vp_table_entries(nat.h, 0, 2, keys.data_ptr(), C.byref(o), None) == ENOTSUP
    torch.cuda.synchronize()
    assert (index == 0x5A5A5A5A).all()
