"""vp_rx_merge on the GPU: several packed streams, one per port, merged by time
into one device batch, byte for byte against rxmergeref.merge_reference (the
contract of include/vigpath.h: a lexsort on (entry, queue, time) over entries
judged by rxunpackref's rules).

Every case fills frames, len, now, in_dev, src, which and count with a canary
first, with a canary tail behind each, compares the buffers whole (the
untouched parts included) and checks that the streams are unchanged. The
streams are made as test_rxunpack_gpu.py makes them: every byte, the padding
included, is neither zero nor the canary. The call reads nothing of its context
but the GPU, so the smallest vigbridge context serves, except in the two
end-to-end cases, where the merged batch goes through vp_process_device and
is compared with the oracle fed the same packets one by one in (time, queue,
entry) order."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import vigor_amd
from rxmergeref import I64_MAX, merge_reference, queue
from test_rxunpack_gpu import (B, CANARY, F, Unpacked, bridge, canary_of, dev, draw_lens, filled,
                               lay, packed)
from tracegen import mixed_bridge_trace, mixed_nat_trace
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

NAMES = ("frames", "len", "now", "in_dev", "src", "which", "count")


def up(q):
    """A host queue (rxmergeref.queue) as rx_merge's dict of device tensors;
    the whole stream is kept beside it to check that it stays unchanged."""
    d_t = dev(q["data"], np.uint8) if q["data"].size else None
    return dict(data=d_t[:q["nbytes"]] if d_t is not None and q["nbytes"] else None,
                lens=dev(q["lens"], np.uint16) if q["lens"].size else None,
                in_port=q["in_port"],
                pos=dev(q["pos"], np.uint64) if q["pos"] is not None else None,
                sel=dev(q["sel"], np.uint32) if q["sel"] is not None else None,
                now=dev(q["now"], np.int64) if q["now"] is not None else None,
                now0=q["now0"], now_step=q["now_step"], n=q["n"], whole=d_t)


class Merged:
    """One vp_rx_merge call over canary-filled buffers, back on the host."""

    def __init__(self, nf, dqs, out_slot, out_cap, with_now=True, with_in=True, stream=None):
        self.out_slot, self.out_cap = out_slot, out_cap
        self.with_now, self.with_in = with_now, with_in
        self.t = [filled(out_cap * out_slot, 1), filled(out_cap, 2), filled(out_cap, 8),
                  filled(out_cap, 2), filled(out_cap, 4), filled(out_cap, 1), filled(1, 4)]
        fr, ln, nw, ind, sr, wh, cnt = self.t
        torch.cuda.synchronize()
        c = out_cap
        nf.rx_merge([{k: v for k, v in q.items() if k != "whole"} for q in dqs],
                    fr[:c * out_slot] if c else None, out_slot, ln[:c] if c else None, cnt[:1],
                    sr[:c] if c else None, wh[:c] if c else None,
                    out_now=nw[:c] if with_now and c else None,
                    out_in_dev=ind[:c] if with_in and c else None, stream=stream)
        torch.cuda.synchronize()
        views = (np.uint8, np.uint16, np.int64, np.uint16, np.uint32, np.uint8, np.uint32)
        for name, t, v in zip(NAMES, self.t, views):
            setattr(self, name, t.cpu().numpy().view(v))

    def same(self, other):
        return all(getattr(self, k).tobytes() == getattr(other, k).tobytes() for k in NAMES)


def compare(got, ref):
    """Every buffer of `got` whole against the reference's: what the call
    owes, and the canary everywhere else."""
    count, r_f, r_l, r_n, r_i, r_s, r_w = ref
    m = min(count, got.out_cap)
    assert r_l.size == m
    assert int(got.count[0]) == count
    assert (got.count[1:] == canary_of(4)).all(), "written past count"
    bad = np.nonzero(got.which[:m] != r_w)[0]
    assert bad.size == 0, "which differs at %s: %s vs %s" % (bad[:8], got.which[bad[:8]],
                                                            r_w[bad[:8]])
    assert (got.which[m:] == CANARY).all(), "which written at or beyond entry %d" % m
    assert got.src[:m].tolist() == r_s.tolist()
    assert (got.src[m:] == canary_of(4)).all(), "src written at or beyond entry %d" % m
    bad = np.nonzero(got.frames[:r_f.size] != r_f)[0]
    assert bad.size == 0, "frames differ at bytes %s: %s vs %s" % (
        bad[:8], got.frames[bad[:8]], r_f[bad[:8]])
    assert (got.frames[r_f.size:] == CANARY).all(), "frames written at or beyond entry %d" % m
    assert got.len[:m].tolist() == r_l.tolist()
    assert (got.len[m:] == canary_of(2)).all(), "len written at or beyond entry %d" % m
    k = m if got.with_now else 0
    assert got.now[:k].tolist() == r_n[:k].tolist()
    assert (got.now[k:].view(np.uint64) == canary_of(8)).all(), "now written beyond entry %d" % k
    k = m if got.with_in else 0
    assert got.in_dev[:k].tolist() == r_i[:k].tolist()
    assert (got.in_dev[k:] == canary_of(2)).all(), "in_dev written beyond entry %d" % k


def check(queues, out_slot, out_cap=None, nf=None, **kw):
    """Host queues through one call. out_cap None: exactly the total.
    Returns (got, reference)."""
    total = sum(q["n"] for q in queues)
    out_cap = total if out_cap is None else out_cap
    ref = merge_reference(queues, out_slot, out_cap)
    dqs = [up(q) for q in queues]
    got = Merged(nf or bridge(), dqs, out_slot, out_cap, **kw)
    compare(got, ref)
    for q, d in zip(queues, dqs):
        if d["whole"] is not None:
            assert d["whole"].cpu().numpy().tobytes() == q["data"].tobytes(), "a stream was written"
    return got, ref


def stream_q(rng, times, in_port, form="pos", lens=None):
    """A queue of len(times) frames of random lengths with the given times."""
    n = len(times)
    lens = draw_lens(rng, n) if lens is None else lens
    data, pos = lay(rng, n, lens, gaps=form == "pos")
    return queue(data, lens, in_port, pos=pos if form == "pos" else None,
                 now=np.asarray(times, np.int64))


def forms(k):
    return ["pos" if (j + k) % 2 else "nopos" for j in range(8)]


def ordered(rng, order, sizes):
    """Times per queue, not decreasing along any, in the given pattern."""
    nq = len(sizes)
    if order == "interleaved":  # one by one while the queues last
        return [np.arange(n) * nq + j for j, n in enumerate(sizes)]
    if order == "blocks":  # queue j wholly after queue j + 1
        return [np.arange(n) + (nq - j) * 10**7 for j, n in enumerate(sizes)]
    if order == "equal":
        return [np.full(n, 777) for n in sizes]
    if order == "ties":  # few values: long runs of equal times across the queues
        return [np.sort(rng.integers(0, 5, n)) for n in sizes]
    assert order == "runs"  # runs of 1 to 700 consecutive packets of one queue
    left, t, out = list(sizes), 0, [[] for _ in sizes]
    while any(left):
        j = int(rng.choice([j for j in range(nq) if left[j]]))
        k = min(left[j], int(rng.integers(1, 701)))
        out[j] += range(t, t + k)
        t, left[j] = t + k, left[j] - k
    return [np.array(x, np.int64) for x in out]


ORDERS = ["interleaved", "blocks", "runs", "equal", "ties"]
SHAPES = [
    (1, 64), (63, 65), (B - 1, B + 1), (B, B),           # two queues around the edges
    (0, B + 1), (65, 0),                                 # an empty queue first, last
    (64, 0, B + 1), (1, B - 1, 63),                      # three, an empty one in the middle
    (0, 1, 63, 64, 65, B - 1, B, B + 1),                 # eight, every length once
    (B + 1, 65, 0, 64, 1, 0, 63, 2 * B + 1),
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("sizes", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_queue_lengths_and_orders(sizes, order):
    rng = np.random.default_rng(9000 + sum(sizes) + 31 * len(sizes))
    times = ordered(rng, order, sizes)
    f = forms(len(sizes))
    qs = [stream_q(rng, t, 10 + j, f[j]) for j, t in enumerate(times)]
    got, ref = check(qs, 64)
    assert ref[0] == sum(sizes) and (np.diff(ref[3]) >= 0).all()
    if order == "equal":  # stability: whole queues in turn, each in entry order
        assert ref[6].tolist() == [j for j, n in enumerate(sizes) for _ in range(n)]
    if order == "blocks":
        assert ref[6].tolist() == [j for j in reversed(range(len(sizes)))
                                   for _ in range(sizes[j])]


def test_ties_that_straddle_a_block_edge_of_another_queue():
    """Queue 1's run of equal times 20 covers queue 0's entries 2000 .. 2099
    and queue 2's; the blocks of each queue end inside the others' runs."""
    rng = np.random.default_rng(9100)
    t0 = np.arange(3 * B) // 100
    t1 = np.sort(np.concatenate([np.full(B + 30, 20), np.full(B - 5, 40), np.arange(61)]))
    t2 = np.repeat(np.arange(0, 62, 2), 70)
    qs = [stream_q(rng, t, j, "pos" if j == 1 else "nopos") for j, t in enumerate((t0, t1, t2))]
    got, ref = check(qs, 64)
    w, t = ref[6], ref[3]
    for v in (20, 40):  # inside a tie the queues stand in turn
        assert (np.diff(w[t == v].astype(int)) >= 0).all() and len(set(w[t == v])) == 3


P31, P32, P63 = 1 << 31, 1 << 32, 1 << 63
EDGE_TIMES = ([-P63, -P63 + 1, -(1 << 40), -P32 - 1, -P32, -P31, -2, -1, 0, 1, P31 - 1, P31,
               P31 + 1, P32 - 1, P32, P32 + 1, P63 - 2, P63 - 1]
              + [k << 32 for k in (2, 3, 5, 1 << 20)]           # differ only above bit 32
              + [(7 << 32) + k for k in (0, 1, 2, P31, P32 - 1)]  # differ only below it
              + [(k << 32) + 5 for k in (-3, -2, 9, 10)])


@pytest.mark.parametrize("nq", [2, 3, 8])
def test_all_64_bits_of_a_time_are_compared_signed(nq):
    rng = np.random.default_rng(9200 + nq)
    sizes = [B + 1, 65, 700, 64, 63, 1, 300, B][:nq]
    f = forms(nq + 1)
    qs = [stream_q(rng, np.sort(rng.choice(np.array(EDGE_TIMES, np.int64), n)), j, f[j])
          for j, n in enumerate(sizes)]
    got, ref = check(qs, 64)
    t = ref[3]
    assert (np.diff(t) >= 0).all() and t[0] < 0 < t[-1] and set(EDGE_TIMES) == set(t.tolist())


def test_affine_time_against_an_array():
    """now == NULL: now0 + m * now_step in 64 bits, from below zero across
    2^32, merged with a queue whose array holds the same values and others."""
    rng = np.random.default_rng(9300)
    n, step = B + 100, (1 << 34) // 1000
    lens = draw_lens(rng, n)
    data, pos = lay(rng, n, lens, gaps=True)
    qa = queue(data, lens, 4, pos=pos, now0=-(1 << 34), now_step=step)
    tb = np.sort(np.concatenate([-(1 << 34) + step * np.arange(0, n, 3),
                                 rng.integers(-(1 << 35), 1 << 36, 900)]))
    qb = stream_q(rng, tb, 5, "nopos")
    got, ref = check([qa, qb], 128)
    assert ref[3][0] < -(1 << 32) and ref[3][-1] > (1 << 32) and (np.diff(ref[3]) >= 0).all()
    got, ref = check([qb, qa], 128)  # (the tie rule the other way round)
    # a step of 0: one time for the whole queue
    check([queue(data, lens, 4, pos=pos, now0=int(tb[400]), now_step=0), qb], 64)


def broken_queue(rng, n, in_port, times, form):
    """A queue with sel (repeats, gaps) into a longer len[] / now[], a few
    entries whose index lies beyond them at its end, and, with pos, some
    positions misaligned, near 2^64 or ending beyond the stream."""
    meta_n = n + 50
    now = np.sort(np.concatenate([times, rng.choice(times, meta_n - len(times))]))[:meta_n]
    k = n - 5
    sel = np.sort(rng.integers(0, meta_n, k)).astype(np.uint32)
    sel = np.concatenate([sel, [meta_n, 0xFFFFFFFF, meta_n + 7, meta_n + (1 << 30), meta_n]])
    sel = sel.astype(np.uint32)
    lens = draw_lens(rng, meta_n)
    lens[lens == 0] = 33
    data, pos = lay(rng, n, lens, sel=sel, gaps=form == "pos")
    nbytes = data.size
    if form == "pos":
        pos = pos.copy()
        for e, off in zip(range(3, k, 29), [1, 2, 4, 8, 15, 17, 3, 5, 7, 9, 11, 12, 13, 14, 6]):
            pos[e] += off
        pos[40:43] = [(1 << 64) - 16, (1 << 64) - 1, (1 << 64) - 4096]
    else:
        nbytes = data.size * 2 // 3 // 16 * 16 + 8  # the last third ends beyond the stream
    return queue(data, lens, in_port, pos=pos if form == "pos" else None, sel=sel, now=now,
                 nbytes=nbytes)


@pytest.mark.parametrize("out_slot", [64, 128, 1536])
def test_streams_of_every_form_mixed_in_one_call(out_slot):
    """pos given and pos == NULL, sel, indices beyond len[], misaligned
    positions, entries ending beyond `bytes`, lengths above the out slot, on
    both paths of the slot mover: every broken entry lands where its time says,
    with a zero slot, len 0 and its own time."""
    rng = np.random.default_rng(9400 + out_slot)
    n = B + 77 if out_slot < 1536 else 300
    base = np.sort(rng.integers(-1000, 5000, n))
    qs = [broken_queue(rng, n, 1, base, "pos"),
          broken_queue(rng, n - 64, 0, base[:-64] + 1, "nopos"),
          stream_q(rng, base[::2], 2, "nopos"),
          broken_queue(rng, 200, 0xFFFF, base[:195], "pos")]
    got, (count, r_f, r_l, r_n, r_i, r_s, r_w) = check(qs, out_slot)
    g = r_f.reshape(count, out_slot)
    dead = r_l == 0
    assert dead.sum() > 100 and not g[dead].any()
    assert (r_n[dead] != 0).all() and (np.diff(r_n) >= 0).all()
    # the entries whose index lies beyond len[] come last, at INT64_MAX, queue by queue
    assert r_n[-15:].tolist() == [I64_MAX] * 15 and r_w[-15:].tolist() == [0] * 5 + [1] * 5 + [3] * 5
    assert r_n[-16] < I64_MAX
    assert r_l.max() > out_slot or out_slot == 1536
    assert 0xFFFF in r_i.tolist()


@pytest.mark.parametrize("short", [0, 1, "total-1", "total"])
@pytest.mark.parametrize("form", ["pos", "nopos"])
def test_out_cap_cuts_the_arrays_not_the_count(short, form):
    rng = np.random.default_rng(9500)
    sizes = (B + 1, 65, 700)
    times = ordered(rng, "runs", sizes)
    qs = [stream_q(rng, t, j, form) for j, t in enumerate(times)]
    total = sum(sizes)
    cap = {"total-1": total - 1, "total": total}.get(short, short)
    got, ref = check(qs, 64, out_cap=cap)
    assert int(got.count[0]) == total
    if short == "total":
        check(qs, 64, out_cap=total + 100)


@pytest.mark.parametrize("form", ["pos", "nopos"])
def test_one_queue_is_rx_unpack(form):
    """One queue, all entries readable: frames, len, now and src are byte for
    byte what vp_rx_unpack writes."""
    rng = np.random.default_rng(9600)
    n = 2 * B + 17
    meta_n = n + 30
    sel = np.sort(rng.choice(meta_n, n, replace=False)).astype(np.uint32)
    lens = draw_lens(rng, meta_n)
    data, pos = lay(rng, n, lens, sel=sel, gaps=form == "pos")
    now = np.sort(rng.integers(-(1 << 40), 1 << 40, meta_n))
    q = queue(data, lens, 3, pos=pos if form == "pos" else None, sel=sel, now=now)
    got, ref = check([q], 128)
    d = up(q)
    one = Unpacked(bridge(), d["data"], n, d["lens"], 128, n, d["pos"], d["sel"], d["now"])
    for k in ("frames", "len", "now", "src"):
        assert getattr(got, k).tobytes() == getattr(one, k).tobytes(), k
    assert (got.which[:n] == 0).all() and (got.in_dev[:n] == 3).all()


def test_optional_outputs_callers_stream_and_repeat():
    rng = np.random.default_rng(9700)
    sizes = (2 * B + 1, B, 65)
    times = ordered(rng, "ties", sizes)
    qs = [stream_q(rng, t, j, "nopos" if j else "pos") for j, t in enumerate(times)]
    a, _ = check(qs, 64)
    b, _ = check(qs, 64, stream=torch.cuda.Stream())
    c, _ = check(qs, 64)
    assert a.same(b) and a.same(c)
    d, _ = check(qs, 64, with_now=False, with_in=False)
    assert all(getattr(a, k).tobytes() == getattr(d, k).tobytes()
               for k in ("frames", "len", "src", "which", "count"))


def test_einval_cases_write_nothing_and_say_why():
    nf = bridge()
    L = nf.L
    L.vp_last_error.restype = C.c_char_p
    d = torch.device("cuda:0")
    n, slot, cap = 64, 64, 128
    data = torch.full((4 * n * slot + 16,), 7, dtype=torch.uint8, device=d)
    lens = torch.full((n,), 60, dtype=torch.int16, device=d)
    pos = (torch.arange(n, dtype=torch.int64, device=d) * 64)
    outs = [filled(cap * slot, 1), filled(cap, 2), filled(cap, 8), filled(cap, 2), filled(cap, 4),
            filled(cap, 1), filled(1, 4)]
    o_f, o_l, o_n, o_i, o_s, o_w, o_c = outs
    torch.cuda.synchronize()

    def rx(**kw):
        a = dict(data=data.data_ptr(), bytes=n * slot, n=n, pos=pos.data_ptr(), sel=None,
                 meta_n=n, len=lens.data_ptr(), now=None, now0=0, now_step=1)
        a.update(kw)
        return vigor_amd.RxStreamC(**a)

    def qs(*streams, ports=None):
        arr = (vigor_amd.RxQueueC * max(1, len(streams)))()
        for j, s in enumerate(streams):
            arr[j].stream = s
            arr[j].in_port = ports[j] if ports else j
        return arr

    def mrg(**kw):
        a = dict(frames=o_f.data_ptr(), slot=slot, cap=cap, len=o_l.data_ptr(),
                 now=o_n.data_ptr(), in_dev=o_i.data_ptr(), key=None, src=o_s.data_ptr(),
                 which=o_w.data_ptr(), count=o_c.data_ptr())
        a.update(kw)
        return vigor_amd.TxMergedC(**a)

    def rc(h, arr, nq, o):
        return L.vp_rx_merge(h, arr, nq, C.byref(o) if o is not None else None, None)

    def refused(h, arr, nq, o, why):
        """VP_EINVAL, and vp_last_error() names the call and this cause"""
        got = rc(h, arr, nq, o)
        text = L.vp_last_error() or b""
        return got == vigor_amd.VP_EINVAL and b"vp_rx_merge" in text and why in text

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == CANARY).all()) for t in outs) \
            and bool((data == 7).all())

    two = qs(rx(), rx())
    assert refused(None, two, 2, mrg(), b"NULL ctx")
    assert refused(nf.h, None, 2, mrg(), b"NULL ctx, queues")
    assert refused(nf.h, two, 2, None, b"or out")
    assert refused(nf.h, two, 2, mrg(count=None), b"count")
    assert refused(nf.h, two, 0, mrg(), b"0 queues")
    nine = qs(*[rx() for _ in range(9)])
    assert refused(nf.h, nine, 9, mrg(), b"9 queues")
    assert rc(nf.h, nine, 8, mrg(cap=0, frames=None, len=None, src=None, which=None)) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == 8 * n
    o_c.view(torch.uint8).fill_(CANARY)
    # per queue what vp_rx_unpack rejects, in the first queue and in the last
    for bad, why in ((rx(data=None), b"data"), (rx(data=data.data_ptr() + 8), b"data"),
                     (rx(len=None), b"a NULL len")):
        assert refused(nf.h, qs(bad, rx()), 2, mrg(), b"queue 0: " + why)
        assert refused(nf.h, qs(rx(), bad), 2, mrg(), b"queue 1: " + why)
    base = data.data_ptr()
    assert refused(nf.h, two, 2, mrg(frames=base), b"queue 0: its data overlaps")
    assert refused(nf.h, two, 2, mrg(frames=base + n * slot - 16), b"overlaps")
    assert refused(nf.h, qs(rx(data=base + cap * slot), rx(data=base + (cap - 1) * slot)), 2,
                   mrg(frames=base), b"queue 1: its data overlaps")
    assert refused(nf.h, qs(rx(), rx(), ports=[0, 0x10000]), 2, mrg(), b"queue 1: in_port")
    assert refused(nf.h, qs(rx(), rx(), ports=[0xFFFFFFFF, 1]), 2, mrg(), b"queue 0: in_port")
    assert refused(nf.h, two, 2, mrg(key=o_s.data_ptr()), b"key")
    for bad_slot in (0, 48, 72, 1000):
        assert refused(nf.h, two, 2, mrg(slot=bad_slot), b"out->slot %d" % bad_slot)
    assert refused(nf.h, two, 2, mrg(frames=o_f.data_ptr() + 8), b"alignment")
    for name in ("frames", "len", "src", "which"):
        assert refused(nf.h, two, 2, mrg(**{name: None}), b"a NULL out->frames, len, src or which")
    o_c.view(torch.uint8).fill_(CANARY)
    assert untouched()
    # what the contract allows: no now and no in_dev, port 0xFFFF, an output
    # right behind the streams
    ok = mrg(now=None, in_dev=None, frames=base + 2 * n * slot)
    assert rc(nf.h, qs(rx(), rx(data=base + n * slot), ports=[0xFFFF, 1]), 2, ok) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == 2 * n and bool((data[:2 * n * slot] == 7).all())
    got = data[2 * n * slot:4 * n * slot].view(2 * n, slot)
    assert bool((got[:, :60] == 7).all()) and not bool(got[:, 60:].any())
    assert o_w[:2 * n].tolist() == [0, 1] * n
    with pytest.raises(vigor_amd.VigpathError):
        nf.rx_merge([dict(data=data[8:n * slot + 8], lens=lens, in_port=0, pos=pos)],
                    o_f[:cap * slot], slot, o_l[:cap], o_c, o_s[:cap], o_w[:cap])


def test_round_trip_bridge_floods_through_pack_and_merge():
    """A vigbridge batch with floods through vp_process_device, vp_tx_build and
    vp_tx_pack; the per-port streams, with sel, pos and the batch's affine time,
    through vp_rx_merge: the forwarded packets in input order, a flooded
    packet's copies adjacent and in port order."""
    rng = np.random.default_rng(9800)
    n, nd, slot = B + 300, 4, 64
    nf = vigor_amd.Bridge(vigor_amd.bridge_config_from_args(["--capacity", "512"], nd), gpu=0)
    frames, lens, ins, _ = mixed_bridge_trace(rng, n, 200, n_dev=nd, slot=slot)
    f_t, l_t, i_t = dev(frames, np.uint8), dev(lens, np.uint16), dev(ins, np.uint16)
    o_t = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    now0, step = 5_000_000_000, 3
    nf.process_device(f_t, l_t, i_t, o_t, slot, now0=now0, now_step=step)
    idx_t, off_t, offset, data_t, port_off, pos_t = packed(nf, nd, f_t, slot, l_t, o_t, i_t, n)
    total = int(offset[nd])
    out = o_t.cpu().numpy().view(np.uint16)
    assert (out == F).sum() > 50 and total > n
    qs = [dict(data=data_t[:int(port_off[nd])], lens=l_t, in_port=20 + p,
               pos=pos_t[int(offset[p]):int(offset[p + 1])],
               sel=idx_t[int(offset[p]):int(offset[p + 1])], now0=now0, now_step=step)
          for p in range(nd)]
    o = [filled(total * slot, 1), filled(total, 2), filled(1, 4), filled(total, 4),
         filled(total, 1), filled(total, 8), filled(total, 2)]
    nf.rx_merge(qs, o[0][:total * slot], slot, o[1][:total], o[2][:1], o[3][:total], o[4][:total],
                out_now=o[5][:total], out_in_dev=o[6][:total])
    torch.cuda.synchronize()
    want = [(i, p) for i in range(n) for p in range(nd)
            if (out[i] == F and p != ins[i]) or (out[i] == p and p != ins[i])]
    assert len(want) == total == int(o[2][0])
    src = o[3].cpu().numpy().view(np.uint32)[:total]
    which = o[4].cpu().numpy()[:total]
    assert list(zip(src.tolist(), which.tolist())) == want
    assert o[5].cpu().numpy()[:total].tolist() == [now0 + i * step for i, _ in want]
    assert o[6].cpu().numpy().view(np.uint16)[:total].tolist() == [20 + p for _, p in want]
    # every copy is the processed frame cut at its length
    img = f_t.cpu().numpy().reshape(n, slot).copy()
    img[np.arange(slot)[None, :] >= np.minimum(lens, slot)[:, None]] = 0
    assert o[0].cpu().numpy()[:total * slot].reshape(total, slot).tobytes() == img[src].tobytes()
    assert o[1].cpu().numpy().view(np.uint16)[:total].tolist() == lens[src].tolist()


def per_port_queues(frames, lens, ins, now, slot, nd, rng):
    """A trace as one queue per port, each in trace order: a self-describing
    stream on even ports, one with pos on odd ones. Returns the host queues and
    the trace's packets in (time, queue, entry) order with every frame cut at
    its length: what the oracle is fed."""
    fr = frames.reshape(-1, slot).copy()
    fr[np.arange(slot)[None, :] >= np.minimum(lens, slot)[:, None]] = 0
    qs = []
    for p in range(nd):
        mine = np.nonzero(ins == p)[0]
        data, pos = lay(rng, mine.size, lens[mine], gaps=p % 2 == 1)
        for e, i in enumerate(mine):
            data[int(pos[e]):int(pos[e]) + int(lens[i])] = fr[i, :lens[i]]
        qs.append(queue(data, lens[mine], p, pos=pos if p % 2 else None, now=now[mine]))
    order = np.lexsort((np.arange(lens.size), ins, now))
    return qs, fr[order].reshape(-1), lens[order], ins[order], now[order]


def merged_through(nf, o, qs, frames, lens, ins, now, slot):
    """vp_rx_merge of the queues, then vp_process_device of the merged batch
    with its in_dev and now, against the oracle over the same packets one by
    one. Returns the oracle's out ports."""
    n = lens.size
    got, ref = check(qs, slot, nf=nf)
    assert ref[1].tobytes() == frames.tobytes() and ref[4].tolist() == ins.tolist()
    fr, ln, nw, ind, sr, wh, cnt = got.t
    out = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    nf.process_device(fr[:n * slot], ln[:n], ind[:n], out, slot, now=nw[:n])
    torch.cuda.synchronize()
    exp = frames.copy()
    exp_out = o.run(exp, lens, ins, now, slot)
    assert out.cpu().numpy().view(np.uint16).tolist() == exp_out.tolist()
    assert fr[:n * slot].cpu().numpy().tobytes() == exp.tobytes()
    return exp_out


def nat_trace_with_replies(rng, n, n_flows, max_flows, expire_us):
    """tracegen's mixed vignat trace, its times spread so that flows expire
    between packets, and most of its WAN packets turned into real replies: a
    first pass of the oracle gives every LAN packet's translated frame, and a
    WAN packet becomes the answer (addresses and ports swapped) to a LAN packet
    up to 30 places before or after it."""
    from test_nat_gpu import DEV_MACS, END_MACS
    frames, lens, ins, now = mixed_nat_trace(rng, n, n_flows, max_idx=max_flows)
    now = T.NOW0 + (now - T.NOW0) * 3
    first = orc.Oracle("nat", orc.nat_cfg(ext_ip=T.ip4(192, 168, 4, 2), expire_us=expire_us,
                                          max_flows=max_flows, device_macs=DEV_MACS[:2],
                                          endpoint_macs=END_MACS[:2]))
    sent = frames.copy()
    out = first.run(sent, lens, ins, now, 64)
    fr, sent = frames.reshape(n, 64), sent.reshape(n, 64)
    for i in np.nonzero(ins == 1)[0]:
        k = int(np.clip(i + rng.integers(-30, 31), 0, n - 1))
        if ins[k] == 0 and out[k] == 1 and rng.random() < 0.8:
            fr[i] = sent[k]
            fr[i, 26:30], fr[i, 30:34] = sent[k, 30:34], sent[k, 26:30]
            fr[i, 34:36], fr[i, 36:38] = sent[k, 36:38], sent[k, 34:36]
            lens[i] = lens[k]
    return frames, lens, ins, now


def test_vignat_lan_and_wan_queues_interleaved_by_time():
    """The point of the call: a LAN queue on port 0 and a WAN queue on port 1.
    Whether a WAN reply is forwarded depends on the LAN packet that opened its
    flow standing before it, and on no expiry in between."""
    from test_nat_gpu import check_state, make_pair
    rng = np.random.default_rng(9900)
    max_flows, expire_us = 64, 40
    frames, lens, ins, now = nat_trace_with_replies(rng, 600, 40, max_flows, expire_us)
    nat, o = make_pair(max_flows=max_flows, expire_us=expire_us)
    qs, fr, ln, dv, nw = per_port_queues(frames, lens, ins, now, 64, 2, rng)
    exp_out = merged_through(nat, o, qs, fr, ln, dv, nw, 64)
    wan = dv == 1
    assert (exp_out[wan] == 0).sum() > 20 and (exp_out[wan] == 1).sum() > 20
    check_state(nat, o, max_flows)


def test_vigbridge_three_ports_learning_and_forwarding():
    from test_bridge_gpu import check_state, make_pair
    rng = np.random.default_rng(9901)
    frames, lens, ins, now = mixed_bridge_trace(rng, 700, 60, n_dev=3)
    br, o = make_pair(cap=128, expire_us=200)
    qs, fr, ln, dv, nw = per_port_queues(frames, lens, ins, now, 64, 3, rng)
    exp_out = merged_through(br, o, qs, fr, ln, dv, nw, 64)
    fwd = (exp_out != F) & (exp_out != dv)
    assert fwd.sum() > 50 and (exp_out == F).sum() > 50  # learned on one port, used from another
    check_state(br, o, 128)
