"""vp_state_save / vp_state_load on the GPU (include/vigpath.h, DESIGN.md
§5.14): a context that loads another's image goes on exactly as the saved one
would have, for every NF and entry point; the image is canonical and equals
tests/stateref.py's packing of the oracle's state; malformed images are
refused with the state untouched. The traces and what they guarantee:
tests/statecases.py, tests/test_state_cases.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stateref as SR
import statecases as SC
import vigor_amd
from gpuh import check_batches, dumps_equal, run_gpu
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95


def make_pair(kind, **args):
    return importlib.import_module("test_%s_gpu" % kind).make_pair(**args)


def dumps_match(kind, nf, o, cap=SC.CAP):
    got, exp = nf.dump(), SC.dump(kind, o, cap)
    if kind == "lb":
        for g, e in zip(got, exp):
            dumps_equal(g, e)
    else:
        dumps_equal(got, exp)


def feed(nf, tr, a, b, slot=64):
    """Packets [a, b) of a trace as one device batch; frames and out ports."""
    fr, ln, dv, now = tr
    return run_gpu(nf, fr[a * slot:b * slot], ln[a:b], dv[a:b], now[a:b], slot)


def one(nf, row, ln, dv, now):
    """vp_process_one of a frame whose first 64 bytes are `row` (zero behind,
    as the slots of the traces leave them); the out port and those bytes."""
    buf = np.zeros(max(int(ln), 64), np.uint8)
    buf[:64] = row
    out = C.c_uint16(0)
    nf._ck(nf.L.vp_process_one(nf.h, int(dv), C.c_void_p(buf.ctypes.data), int(ln), int(now),
                               C.byref(out)), "vp_process_one")
    return int(out.value), buf[:64]


def tail(tr, a, slot=64):
    fr, ln, dv, now = tr
    return fr[a * slot:], ln[a:], dv[a:], now[a:]


# The oracle's run over a whole two-act trace, computed once per case and left
# unchanged: (expected frames, out ports, the oracle at the end).
_whole = {}


def whole(kind, variant):
    if (kind, variant) not in _whole:
        tr, cut = SC.trace(kind, variant)
        _, o = make_pair(kind, **SC.pair_args(kind, variant))
        exp = tr[0].copy()
        out = o.run(exp, tr[1], tr[2], tr[3], 64)
        _whole[kind, variant] = (tr, cut, exp.reshape(-1, 64), out, o)
    return _whole[kind, variant]


def saved_after_act1(kind, variant):
    tr, cut, exp, out, o = whole(kind, variant)
    a, _ = make_pair(kind, **SC.pair_args(kind, variant))
    gf, go = feed(a, tr, 0, cut)
    assert np.array_equal(go, out[:cut]) and np.array_equal(gf.reshape(-1, 64), exp[:cut])
    return a.save_state()


# ------------------------------------------------------- 1 continuation --

@pytest.mark.parametrize("variant", SC.VARIANTS)
@pytest.mark.parametrize("kind", SC.KINDS)
def test_continuation(kind, variant):
    tr, cut, exp, out, o = whole(kind, variant)
    img = saved_after_act1(kind, variant)
    n = tr[1].shape[0]
    for cuts in ([cut + 1, cut + 7, cut + 500], [cut + 333]):
        b, _ = make_pair(kind, **SC.pair_args(kind, variant))
        b.load_state(img)
        bounds = [cut] + cuts + [n]
        for x, y in zip(bounds[:-1], bounds[1:]):
            gf, go = feed(b, tr, x, y)
            bad = np.nonzero(go != out[x:y])[0]
            assert bad.size == 0, "out port mismatch at packets %s" % (bad[:10] + x)
            badf = np.nonzero((gf.reshape(-1, 64) != exp[x:y]).any(axis=1))[0]
            assert badf.size == 0, "frame mismatch at packets %s" % (badf[:10] + x)
        dumps_match(kind, b, o)


# ----------------------------------- 2 continuation, the resident kernel --

@pytest.mark.parametrize("kind", SC.KINDS)
def test_continuation_resident_kernel(kind):
    tr, cut, exp, out, o = whole(kind, "part")
    img = saved_after_act1(kind, "part")
    fr, ln, dv, now = tr
    n = ln.shape[0]
    # per packet
    b, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    b.load_state(img)
    F = fr.reshape(-1, 64)
    for p in range(cut, n):
        got, row = one(b, F[p], ln[p], dv[p], now[p])
        assert got == out[p], "out port of packet %d" % p
        assert np.array_equal(row, exp[p]), "frame of packet %d" % p
    st, ex = b.serve_stats(), b.serve_expiry_stats()
    assert st["packets_one"] > 0 and ex["expired"] > 0 and ex["walks"] > 0
    # bursts of 32
    b, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    b.load_state(img)
    for x in range(cut, n, 32):
        y = min(n, x + 32)
        bufs = [bytearray(F[j].tobytes() + bytes(max(int(ln[j]) - 64, 0)))[:max(int(ln[j]), 1)]
                for j in range(x, y)]
        keep = [len(q) == int(ln[j]) for q, j in zip(bufs, range(x, y))]
        if not all(keep):  # (a frame of no bytes has no buffer to stand in)
            go = np.array([one(b, F[j], ln[j], dv[j], now[j])[0] for j in range(x, y)])
        else:
            go = b.process_mbufs(bufs, dv[x:y], now[x:y])
            for j, q in zip(range(x, y), bufs):
                m = min(int(ln[j]), 64)
                assert bytes(q[:m]) == exp[j, :m].tobytes(), "frame %d" % j
        assert np.array_equal(go, out[x:y]), "out ports of burst at %d" % x
    st, ex = b.serve_stats(), b.serve_expiry_stats()
    assert st["bursts"] > 0 and ex["expired"] > 0
    dumps_match(kind, b, o)


# ------------------------------------------------------------ 3 canonical --

@pytest.mark.parametrize("kind", SC.KINDS)
def test_canonical(kind):
    tr, cut, exp, out, o = whole(kind, "part")
    img = saved_after_act1(kind, "part")
    # the same packets, one call each
    fr, ln, dv, now = tr
    b, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    F = fr.reshape(-1, 64)
    for p in range(cut):
        got, _ = one(b, F[p], ln[p], dv[p], now[p])
        assert got == out[p]
    assert b.save_state() == img
    # save(load(save(A))) == save(A)
    c, _ = make_pair(kind, **SC.pair_args(kind, "part"))
    c.load_state(img)
    assert c.save_state() == img
    # and the image is what stateref says it is
    assert SR.pack(SR.unpack(img)) == img
    assert SR.unpack(img)["kind"] == kind


def test_canonical_across_bucket_layouts(monkeypatch):
    """vignat: sequential flows over more than half the table take the
    allocation-order layout (tests/test_layout_gpu.py); the same state reached
    with that layout switched off gives the same bytes, and so does a context
    that loaded them."""
    cap = 1 << 12
    tr = T.nat_lan_trace(3 * cap // 2, 3 * cap // 4)
    imgs, layouts = [], []
    for lin in (None, "0"):
        if lin:
            monkeypatch.setenv("VIGPATH_LIN", lin)
        nat, _ = make_pair("nat", max_flows=cap)
        run_gpu(nat, *tr, 64)
        layouts.append(nat.table_stats()["layout"])
        imgs.append(nat.save_state())
    monkeypatch.delenv("VIGPATH_LIN")
    assert layouts[0] != layouts[1], layouts
    assert imgs[0] == imgs[1]
    nat, _ = make_pair("nat", max_flows=cap)
    nat.load_state(imgs[0])
    assert nat.save_state() == imgs[0]


# ------------------------------------------------ 4 image against oracle --

@pytest.mark.parametrize("kind", SC.KINDS)
def test_image_equals_packed_oracle_dump(kind):
    tr = SC.distinct_trace(kind)
    n, cut = tr[1].shape[0], 400
    args = SC.pair_args(kind, expire_us=60_000_000)
    a, o = make_pair(kind, **args)
    o.run(tr[0][:cut * 64].copy(), tr[1][:cut], tr[2][:cut], tr[3][:cut], 64)
    feed(a, tr, 0, cut)
    want = SR.pack(SR.state_from_dump(kind, SC.dump(kind, o), tr[3][cut - 1]))
    assert a.save_state() == want
    # load without save: the packed oracle dump into a fresh context
    b, _ = make_pair(kind, **args)
    b.load_state(want)
    check_batches(b, o, *tail(tr, cut), 64, [77])
    dumps_match(kind, b, o)


# ---------------------------------------------------- 5 kernel shapes --

def _lan_flows(first, count, t0):
    """One LAN packet per flow first .. first + count - 1, one stamp each."""
    k = np.arange(first, first + count)
    fr, ln = T.udp_frames(T.ip4(10, 7, 0, 0) + k, np.full(count, T.ip4(8, 8, 8, 8)),
                          1000 + k % 50000, np.full(count, 53))
    return fr, ln, np.zeros(count, np.uint16), t0 + 10 * np.arange(count, dtype=np.int64)


@pytest.mark.parametrize("stacked", [False, True])
@pytest.mark.parametrize("cap,n_live", [(c, n) for c in (64, 4096)
                                        for n in sorted({0, 1, 63, 64, 65, c}) if n <= c])
def test_kernel_shape_edges(cap, n_live, stacked):
    """vignat with n_live flows; stacked: the table was full first and the
    other flows expired, so every free index is on the stack."""
    exp_us = 1000
    a, o = make_pair("nat", max_flows=cap, expire_us=exp_us)
    t = T.NOW0
    if stacked:
        # the flows that will expire first, then the survivors (the table is
        # full), then one packet after the first ones' expiry that runs it
        old = _lan_flows(n_live, cap - n_live, t)
        t += 10 * cap + 500_000
        new = _lan_flows(0, n_live, t)
        t += 10 * cap + 600_000
        trig = _lan_flows(0, 1, t)
        if not n_live:
            trig[2][:] = 1  # (from the WAN: dropped, opens no flow)
        parts = [old, new, trig]
    else:
        parts = [_lan_flows(0, n_live, t)]
        t += 10 * cap
    for fr, ln, dv, now in parts:
        if ln.shape[0]:
            e = fr.copy()
            eo = o.run(e, ln, dv, now, 64)
            gf, go = run_gpu(a, fr, ln, dv, now, 64)
            assert np.array_equal(go, eo) and np.array_equal(gf, e)
    img = a.save_state()
    s = SR.unpack(img)["tables"][0]
    assert len(s["lru"]) == n_live
    if stacked and n_live < cap:
        assert len(s["freed"]) == cap - n_live and s["fresh_next"] == cap
    b, _ = make_pair("nat", max_flows=cap, expire_us=exp_us)
    b.load_state(img)
    dumps_equal(b.dump(), o.nat_dump(cap))
    assert b.save_state() == img
    more = _lan_flows(cap // 2, 128, t + 2000)
    check_batches(b, o, *more, 64, [50])
    dumps_equal(b.dump(), o.nat_dump(cap))


# ------------------------------------------------------ 6 rejected images --

@pytest.fixture(scope="module")
def victims():
    """Per kind: a context in the state after act 1, its image, and its
    oracle; shared by every rejected image (none may change it)."""
    made = {}

    def get(kind):
        if kind not in made:
            tr, cut = SC.trace(kind, "part")
            nf, o = make_pair(kind, **SC.pair_args(kind, "part"))
            check_batches(nf, o, tr[0][:cut * 64], tr[1][:cut], tr[2][:cut], tr[3][:cut], 64, [])
            made[kind] = (nf, o, nf.save_state(), tr, cut)
        return made[kind]
    return get


@pytest.mark.parametrize("kind,name", [(k, m) for k in ("nat", "lb") for m in SC.names_for(k)])
def test_rejected_image(victims, kind, name):
    nf, o, img, tr, cut = victims(kind)
    bad = SC.mutations(kind, img)[name]
    buf = np.frombuffer(bad, np.uint8)
    L = nf.L
    rc = L.vp_state_load(nf.h, C.c_void_p(buf.ctypes.data), buf.size)
    assert rc == EINVAL, (name, rc)
    assert L.vp_last_error().decode().startswith("state load:"), L.vp_last_error()
    assert [rc, L.vp_last_error().decode()] == SC.recorded()["image"][kind][name]
    assert nf.save_state() == img


@pytest.mark.parametrize("kind", ["nat", "lb"])
def test_victim_goes_on_matching_the_oracle(victims, kind):
    """After every refused load above (this runs behind them), and a save
    into a buffer one byte short."""
    nf, o, img, tr, cut = victims(kind)
    buf = np.full(len(img) + 16, 0xA5, np.uint8)
    n = C.c_uint64()
    rc = nf.L.vp_state_save(nf.h, C.c_void_p(buf.ctypes.data), len(img) - 1, C.byref(n))
    assert rc == EINVAL and n.value == len(img)
    assert (buf == 0xA5).all()
    rc = nf.L.vp_state_save(nf.h, C.c_void_p(buf.ctypes.data), len(img), C.byref(n))
    assert rc == 0 and n.value == len(img) and buf[:len(img)].tobytes() == img
    assert (buf[len(img):] == 0xA5).all()
    bound = C.c_uint64()
    assert nf.L.vp_state_size(nf.h, C.byref(bound)) == 0 and bound.value >= len(img)
    check_batches(nf, o, *tail(tr, cut), 64, [200])
    dumps_match(kind, nf, o)


def test_empty_image_empties_a_used_context():
    tr, cut = SC.trace("nat", "part")
    fresh, _ = make_pair("nat", **SC.pair_args("nat", "part"))
    empty = fresh.save_state()
    s = SR.unpack(empty)
    assert s["last_now"] == -1 and s["tables"][0]["lru"] == [] and s["tables"][0]["fresh_next"] == 0
    nf, o = make_pair("nat", **SC.pair_args("nat", "part"))
    feed(nf, tr, 0, cut)
    assert nf.live_count() > 0
    nf.load_state(empty)
    assert nf.live_count() == 0 and nf.save_state() == empty
    check_batches(nf, o, tr[0], tr[1], tr[2], tr[3], 64, [cut])


# ------------------------------------------------------- 7 multi-GPU guard --

def test_attached_context_is_not_supported():
    nat, _ = make_pair("nat", max_flows=256)
    img = nat.save_state()

    def allgather(user, send, recv, nbytes):
        if nbytes:
            C.memmove(recv, send, nbytes)
        return 0

    ag = vigor_amd.ALLGATHER_FN(allgather)
    ar = vigor_amd.ALLREDUCE_FN(lambda user, buf, count: 0)
    ops = vigor_amd.CommOpsC(user=None, allgather=ag, allreduce_max_u64=ar)
    assert nat.L.vp_attach_comm(nat.h, C.byref(ops), 1, 0) == 0
    n = C.c_uint64()
    buf = np.zeros(len(img), np.uint8)
    assert nat.L.vp_state_size(nat.h, C.byref(n)) == ENOTSUP
    assert nat.L.vp_state_save(nat.h, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)) == ENOTSUP
    src = np.frombuffer(img, np.uint8)
    assert nat.L.vp_state_load(nat.h, C.c_void_p(src.ctypes.data), src.size) == ENOTSUP
