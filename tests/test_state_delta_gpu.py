"""vp_state_delta_save / vp_state_delta_apply on the GPU (include/vigpath.h,
DESIGN.md §5.15): a standby that loads a primary's image and then applies its
deltas gives, after every apply, the primary's full image byte for byte, for
every NF; the delta is what tests/deltaref.py says it is; a promoted standby
goes on as the oracle does; malformed deltas and misuse are refused with the
state and the followed mark untouched. Traces: tests/statecases.py."""
import ctypes as C

import numpy as np
import pytest

import deltacases as DC
import deltaref as DR
import stateref as SR
import statecases as SC
import vigor_amd
from gpuh import run_gpu
from test_state_gpu import dumps_match, feed, make_pair, one, whole
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95


def standby(kind, img, mark, **args):
    s, _ = make_pair(kind, **args)
    s.load_state(img)
    s.follow(mark)
    return s


def started(kind, variant):
    """A primary after act 1, its mark and image there, the trace and cut."""
    tr, cut, exp, out, o = whole(kind, variant)
    p, _ = make_pair(kind, **SC.pair_args(kind, variant))
    feed(p, tr, 0, cut)
    return p, p.state_mark(), p.save_state(), tr, cut


# ------------------------------------------------- 1 follow, 2 cumulative --

@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_follow(kind, variant):
    p, m0, img0, tr, cut = started(kind, variant)
    args = SC.pair_args(kind, variant)
    s = standby(kind, img0, m0, **args)
    n = tr[1].shape[0]
    bounds = [cut, cut + 1, cut + 7, cut + 333, cut + 500, n]
    mark, img = m0, img0
    left = rekeyed = 0
    for x, y in zip(bounds[:-1], bounds[1:]):
        feed(p, tr, x, y)
        blob, nxt = p.save_delta(mark)
        s.apply_delta(blob)
        want = p.save_state()
        assert s.save_state() == want, "image after the delta of packets %d .. %d" % (x, y)
        before, d = SR.unpack(img), DR.unpack(blob)
        assert d["base"] == mark and d["mark"] == nxt
        assert SR.pack(DR.apply(before, d)) == want
        for t0, t1, td in zip(before["tables"][:1], SR.unpack(want)["tables"], d["tables"]):
            key0, key1 = dict(zip(t0["lru"], t0["key"])), dict(zip(t1["lru"], t1["key"]))
            # (an entry left: its index is free now, or holds another key)
            left += sum(key1.get(i) != k for i, k in key0.items())
            rekeyed += sum(i in key0 and key0[i] != k for i, k in zip(td["idx"], td["key"]))
        mark, img = nxt, want
    # act 2 expired act 1's entries, gave freed indices to new keys and (part:
    # the table was not full at the cut) reached the never-used tail
    f0 = SR.unpack(img0)["tables"][0]["fresh_next"]
    f1 = SR.unpack(img)["tables"][0]["fresh_next"]
    assert left > 0 and rekeyed > 0
    if variant == "part":  # ("full": the table was full at the cut, no tail was left)
        assert f1 > f0
    # cumulative: one delta from the first mark, on a fresh standby
    s2 = standby(kind, img0, m0, **args)
    blob, end = p.save_delta(m0)
    assert end == mark
    s2.apply_delta(blob)
    assert s2.save_state() == img


# ------------------------------------------------------------ 3 promotion --

@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_promotion(kind, variant):
    tr, cut, exp, out, o = whole(kind, variant)
    p, m0, img0, _, _ = started(kind, variant)
    args = SC.pair_args(kind, variant)
    n, at = tr[1].shape[0], cut + 500
    followers = [standby(kind, img0, m0, **args)]
    if variant == "part":
        followers.append(standby(kind, img0, m0, **args))
    mark = m0
    for x, y in ((cut, cut + 7), (cut + 7, at)):
        feed(p, tr, x, y)
        blob, mark = p.save_delta(mark)
        for s in followers:
            s.apply_delta(blob)
    # through the batch path
    s = followers[0]
    gf, go = feed(s, tr, at, n)
    assert np.array_equal(go, out[at:]), np.nonzero(go != out[at:])[0][:10] + at
    assert np.array_equal(gf.reshape(-1, 64), exp[at:])
    dumps_match(kind, s, o)
    # promoted: no delta is taken any more
    feed(p, tr, at, at + 1)
    blob, _ = p.save_delta(mark)
    with pytest.raises(Exception):
        s.apply_delta(blob)
    if variant != "part":
        return
    # per packet through the resident kernel
    s = followers[1]
    fr, ln, dv, now = tr
    F = fr.reshape(-1, 64)
    for q in range(at, n):
        got, row = one(s, F[q], ln[q], dv[q], now[q])
        assert got == out[q], "out port of packet %d" % q
        assert np.array_equal(row, exp[q]), "frame of packet %d" % q
    assert s.serve_stats()["packets_one"] > 0 and s.serve_expiry_stats()["expired"] > 0
    dumps_match(kind, s, o)


# -------------------------------------------------------- 4 exact content --

CUT0 = 200
TARGETS = (0, 1, 63, 64, 65)


def _oracle_cuts(kind, tr, args):
    """The oracle's state after CUT0 packets of the distinct trace, and per
    target the first cut behind which that many entries of table 0 have a
    stamp above the base's last_now, with the state there."""
    _, o = make_pair(kind, **args)
    o.run(tr[0][:CUT0 * 64].copy(), tr[1][:CUT0], tr[2][:CUT0], tr[3][:CUT0], 64)
    s0 = SR.state_from_dump(kind, SC.dump(kind, o), tr[3][CUT0 - 1])
    found = {0: (CUT0, s0)}
    for q in range(CUT0, tr[1].shape[0]):
        o.run(tr[0][q * 64:(q + 1) * 64].copy(), tr[1][q:q + 1], tr[2][q:q + 1], tr[3][q:q + 1], 64)
        s = SR.state_from_dump(kind, SC.dump(kind, o), tr[3][q])
        found.setdefault(sum(t > s0["last_now"] for t in s["tables"][0]["ts"]), (q + 1, s))
        if all(t in found for t in TARGETS):
            break
    return s0, found


def _touched(s0, s1):
    return [{i for i, ts in zip(t["lru"], t["ts"]) if ts > s0["last_now"]} for t in s1["tables"]]


@pytest.mark.parametrize("kind", SC.KINDS)
def test_exact_content(kind):
    tr = SC.distinct_trace(kind)
    args = SC.pair_args(kind, expire_us=60_000_000)
    s0, found = _oracle_cuts(kind, tr, args)
    p, _ = make_pair(kind, **args)
    start = p.state_mark()
    feed(p, tr, 0, CUT0)
    m0, img0 = p.state_mark(), p.save_state()
    assert img0 == SR.pack(s0)
    at = CUT0
    for target in TARGETS:
        cut, s1 = found[target]
        if cut > at:
            feed(p, tr, at, cut)
            at = cut
        blob, mark = p.save_delta(m0)  # (from the same base every time: cumulative)
        want = DR.diff(s0, s1, _touched(s0, s1), base=m0, mark=mark)
        assert len(want["tables"][0]["idx"]) == target
        assert blob == DR.pack(want), "the delta with n_new = %d" % target
        s = standby(kind, img0, m0, **args)
        s.apply_delta(blob)
        assert s.save_state() == SR.pack(s1) == p.save_state()
        if target == 0:  # the empty delta: nothing but the mark changes
            assert mark == m0
            again, mark2 = p.save_delta(mark)
            s.apply_delta(again)
            assert s.save_state() == img0
    # all of n_live: the delta from the context's first moment, on a standby
    # that follows from its own creation
    blob, mark = p.save_delta(start)
    d = DR.unpack(blob)
    now = SR.unpack(p.save_state())
    assert [len(t["idx"]) for t in d["tables"]] == [len(t["lru"]) for t in now["tables"]]
    assert [t["idx"] for t in d["tables"]] == [t["lru"] for t in now["tables"]]
    s, _ = make_pair(kind, **args)
    s.follow(start)
    s.apply_delta(blob)
    assert s.save_state() == p.save_state()


def test_one_touched_flow_is_a_small_delta():
    nat, _ = make_pair("nat", max_flows=256)
    tr = T.nat_lan_trace(200, 200)
    run_gpu(nat, *tr, 64)
    m = nat.state_mark()
    full = nat.save_state()
    assert len(SR.unpack(full)["tables"][0]["lru"]) == 200
    run_gpu(nat, tr[0][:64], tr[1][:1], tr[2][:1], tr[3][:1] + 1000, 64)
    blob, _ = nat.save_delta(m)
    assert len(DR.unpack(blob)["tables"][0]["idx"]) == 1
    assert 10 * len(blob) < len(full), (len(blob), len(full))


# -------------------------------------------------- 5 edges of the grid --

def _lan_flows(first, count, t0):
    k = np.arange(first, first + count)
    fr, ln = T.udp_frames(T.ip4(10, 7, 0, 0) + k, np.full(count, T.ip4(8, 8, 8, 8)),
                          1000 + k % 50000, np.full(count, 53))
    return fr, ln, np.zeros(count, np.uint16), t0 + 10 * np.arange(count, dtype=np.int64)


def test_edges_of_the_grid():
    """vignat at 4096 indices: 2,000 flows, of which 1,100 are touched again
    60 ms later (the 450th to the 1549th: across blocks of 256 and bitmap
    words, at no boundary of either) and 90 are new; then, 150 ms after the
    start, the expiry (100 ms) of the 900 that were not touched again."""
    cap, exp_us = 4096, 100_000
    p, _ = make_pair("nat", max_flows=cap, expire_us=exp_us)
    run_gpu(p, *_lan_flows(0, 2000, T.NOW0), 64)
    m0, img0 = p.state_mark(), p.save_state()
    s = standby("nat", img0, m0, max_flows=cap, expire_us=exp_us)
    run_gpu(p, *_lan_flows(450, 1100, T.NOW0 + 60_000_000), 64)
    run_gpu(p, *_lan_flows(2000, 90, T.NOW0 + 70_000_000), 64)
    blob, m1 = p.save_delta(m0)
    d = DR.unpack(blob)["tables"][0]
    assert len(d["idx"]) == 1190
    s.apply_delta(blob)
    assert s.save_state() == p.save_state()
    run_gpu(p, *_lan_flows(3000, 70, T.NOW0 + 150_000_000), 64)
    blob, m2 = p.save_delta(m1)
    d = DR.unpack(blob)["tables"][0]
    assert len(d["idx"]) == 70 and len(d["freed"]) > 800
    s.apply_delta(blob)
    assert s.save_state() == p.save_state()


# ------------------------------------------------------ 6 viglb's erasure --

def test_lb_erasure_out_of_lru_order():
    """Eight backends and forty flows; 10 ms later every backend has expired
    (5 ms) and none is alive, and a packet of flow 20 erases that flow: it
    leaves from the middle of the LRU list, the flows before it stay."""
    args = dict(flow_cap=256, bcap=32, fexp=60_000_000, bexp=5_000)
    t0 = T.NOW0
    hb = T.lb_heartbeats(8, t0=t0)
    fl = T.lb_traffic(40, 40)
    fl = fl[:3] + (t0 + 1000 + np.arange(40, dtype=np.int64),)
    act1 = tuple(np.concatenate(x) for x in zip(hb, fl))
    pkt = (fl[0][20 * 64:21 * 64], fl[1][20:21], fl[2][20:21],
           np.array([t0 + 10_000_000], np.int64))
    # the oracle, on the CPU: the trace does this
    p, o = make_pair("lb", **args)
    o.run(act1[0].copy(), *act1[1:], 64)
    (fa0, ft0, _, _), (ba0, _, _, _, _) = o.lb_dump(256, 32)
    o.run(pkt[0].copy(), *pkt[1:], 64)
    (fa1, _, _, _), (ba1, _, _, _, _) = o.lb_dump(256, 32)
    gone = np.nonzero((fa0 == 1) & (fa1 == 0))[0]
    assert gone.size == 1 and ba0.sum() == 8 and ba1.sum() == 0
    older = np.nonzero((fa1 == 1) & (ft0 < ft0[gone[0]]))[0]
    assert older.size == 20, "the erased flow was the oldest: in LRU order after all"
    # the follow equality across that packet, for both tables
    run_gpu(p, *act1, 64)
    m0, img0 = p.state_mark(), p.save_state()
    s = standby("lb", img0, m0, **args)
    run_gpu(p, *pkt, 64)
    blob, _ = p.save_delta(m0)
    d = DR.unpack(blob)
    assert [t["n_live"] for t in d["tables"]] == [39, 0]
    assert d["tables"][0]["idx"] == [] and int(gone[0]) in d["tables"][0]["freed"]
    s.apply_delta(blob)
    want = p.save_state()
    assert s.save_state() == want
    assert SR.pack(DR.apply(SR.unpack(img0), d)) == want
    for nf in (p, s):
        got = nf.dump()
        np.testing.assert_array_equal(got[0][0], fa1)
        np.testing.assert_array_equal(got[1][0], ba1)


# ------------------------------------------------------------ 7 refusals --

MARK = (77, 3)  # what the victims follow: a primary's numbering, not theirs


@pytest.fixture(scope="module")
def victims():
    """Per kind (vigfw, viglb): a standby that holds deltacases.victim's state
    0 and follows MARK, that state's image, and the good delta to state 1;
    shared by every refusal (none may change it)."""
    made = {}

    def get(kind):
        if kind not in made:
            s0, s1, touched = DC.victim(kind, cap=SC.CAP, bcap=SC.LB_BCAP)
            good = DR.diff(s0, s1, touched, base=MARK, mark=(MARK[0] + 40, MARK[1]))
            nf = standby(kind, SR.pack(s0), MARK, **SC.pair_args(kind))
            assert nf.save_state() == SR.pack(s0)
            made[kind] = (nf, s0, s1, good)
        return made[kind]
    return get


def _refused(nf, blob, img, want=EINVAL, recorded=None):
    buf = np.frombuffer(blob, np.uint8)
    rc = nf.L.vp_state_delta_apply(nf.h, C.c_void_p(buf.ctypes.data), buf.size)
    assert rc == want, rc
    assert nf.L.vp_last_error().decode().startswith("state delta apply:"), nf.L.vp_last_error()
    if recorded:
        assert [rc, nf.L.vp_last_error().decode()] == recorded
    assert nf.save_state() == img


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("fw", "lb") for n in DC.names_for(k)])
def test_refused_delta(victims, kind, name):
    nf, s0, s1, good = victims(kind)
    _refused(nf, DC.mutations(s0, good)[name], SR.pack(s0),
             recorded=SC.recorded()["delta"][kind][name])


@pytest.mark.parametrize("kind", ["fw", "lb"])
def test_refused_base_then_the_good_delta(victims, kind):
    """Behind every refusal above: a delta of another base is refused too,
    and the good one still applies, so the followed mark is the one it was;
    afterwards it is the delta's, and the same delta no longer applies."""
    nf, s0, s1, good = victims(kind)
    _refused(nf, DR.pack(dict(good, base=(MARK[0] + 1, MARK[1]))), SR.pack(s0))
    _refused(nf, DR.pack(dict(good, base=(MARK[0], MARK[1] + 1))), SR.pack(s0))
    nf.apply_delta(DR.pack(good))
    assert nf.save_state() == SR.pack(s1)
    _refused(nf, DR.pack(good), SR.pack(s1))
    # an empty delta from the new mark
    e = DR.diff(s1, s1, [set() for _ in s1["tables"]], base=good["mark"], mark=good["mark"])
    nf.apply_delta(DR.pack(e))
    assert nf.save_state() == SR.pack(s1)


def test_refused_without_follow_and_after_a_packet():
    p, m0, img0, tr, cut = started("nat", "part")
    args = SC.pair_args("nat", "part")
    feed(p, tr, cut, cut + 7)
    blob, _ = p.save_delta(m0)
    s, _ = make_pair("nat", **args)
    s.load_state(img0)
    _refused(s, blob, img0)  # follows nothing
    s.follow(m0)
    feed(s, tr, cut, cut + 1)  # promoted
    _refused(s, blob, s.save_state())
    s.load_state(img0)  # a load ends the following as well
    _refused(s, blob, img0)
    s.follow(m0)
    s.apply_delta(blob)
    assert s.save_state() == p.save_state()


def test_refused_bases_at_the_saving_side():
    p, m0, img0, tr, cut = started("nat", "part")
    L = p.L
    n, m = C.c_uint64(), vigor_amd.StateMarkC()
    buf = np.full(len(img0) + 4096, 0xA5, np.uint8)

    def save(base, cap=None):
        b = vigor_amd.StateMarkC(*base)
        return L.vp_state_delta_save(p.h, C.byref(b), C.c_void_p(buf.ctypes.data),
                                     buf.size if cap is None else cap, C.byref(n), C.byref(m))
    for base in ((m0[0] + 1, m0[1]), (m0[0], m0[1] + 1)):  # a future seq, another epoch
        assert save(base) == EINVAL
        assert L.vp_last_error().decode().startswith("state delta save:"), L.vp_last_error()
        b = vigor_amd.StateMarkC(*base)
        assert L.vp_state_delta_size(p.h, C.byref(b), C.byref(n)) == EINVAL
    assert (buf == 0xA5).all() and p.save_state() == img0
    # a buffer one byte short: the size only
    assert save(m0) == 0
    size = n.value
    buf[:] = 0xA5
    assert save(m0, size - 1) == EINVAL and n.value == size and (buf == 0xA5).all()
    # a load starts a new epoch: marks taken before it are refused
    p.load_state(img0)
    assert p.state_mark()[1] == m0[1] + 1
    assert save(m0) == EINVAL


def test_attached_context_is_not_supported():
    nat, _ = make_pair("nat", max_flows=256)
    m = vigor_amd.StateMarkC()
    assert nat.L.vp_state_mark(nat.h, C.byref(m)) == 0

    def allgather(user, send, recv, nbytes):
        if nbytes:
            C.memmove(recv, send, nbytes)
        return 0

    ag = vigor_amd.ALLGATHER_FN(allgather)
    ar = vigor_amd.ALLREDUCE_FN(lambda user, buf, count: 0)
    ops = vigor_amd.CommOpsC(user=None, allgather=ag, allreduce_max_u64=ar)
    assert nat.L.vp_attach_comm(nat.h, C.byref(ops), 1, 0) == 0
    n, out = C.c_uint64(), vigor_amd.StateMarkC()
    buf = np.zeros(4096, np.uint8)
    assert nat.L.vp_state_mark(nat.h, C.byref(out)) == ENOTSUP
    assert nat.L.vp_state_delta_size(nat.h, C.byref(m), C.byref(n)) == ENOTSUP
    assert nat.L.vp_state_delta_save(nat.h, C.byref(m), C.c_void_p(buf.ctypes.data), buf.size,
                                     C.byref(n), C.byref(out)) == ENOTSUP
    assert nat.L.vp_state_follow(nat.h, C.byref(m)) == ENOTSUP
    assert nat.L.vp_state_delta_apply(nat.h, C.c_void_p(buf.ctypes.data), 64) == ENOTSUP
