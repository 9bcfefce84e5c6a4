"""vp_tx_merge on the GPU: several transmit lists as one NF's batch, byte for
byte against txmergeref.merge_reference (the contract of include/vigpath.h as
a stable lexsort).

Every case fills frames, len, now, in_dev, key, src, which and count with a
canary first, with a canary tail behind each, compares the buffers whole (the
untouched parts included) and checks that the source frames are unchanged.
Hand-made lists go through the smallest vigbridge contexts with the wanted
n_devices (the call reads only the batches, the lists and the keys); the flood
and stream cases take their lists from vp_tx_build."""
import ctypes as C

import numpy as np
import pytest
import torch

import vigor_amd
from txbatchref import rebatch_reference
from txmergeref import entries, merge_reference, source
from txref import tx_reference

pytestmark = pytest.mark.gpu

B = 2048  # entries per block of vp_tx_merge's kernels (vp_txmerge.hip)
F = 0xFFFF
CANARY = 0xA5
TAIL = 64  # canary entries kept behind every buffer
BUFS = [("frames", 1), ("len", 2), ("now", 8), ("in_dev", 2), ("key", 4), ("src", 4),
        ("which", 1)]
VIEW = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def canary_of(width):
    return int.from_bytes(bytes([CANARY]) * width, "little")


_ctx = {}


def bridge(nd, k=0):
    """A vigbridge context with nd devices; k tells several of them apart."""
    if (nd, k) not in _ctx:
        _ctx[nd, k] = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)
    return _ctx[nd, k]


def dev(a, dtype):
    """A numpy array as a device tensor of the signed torch type of its width."""
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


def frames_for(rng, n, slot):
    """n slots of random bytes, none of them zero or the canary, so that zero
    fill and untouched bytes cannot pass for frame bytes."""
    f = rng.integers(1, 255, n * slot).astype(np.uint8)
    f[f == CANARY] = 0x11
    return f


def filled(count, width):
    """count + TAIL entries of `width` bytes, every byte the canary."""
    t = torch.full(((count + TAIL) * width,), CANARY, dtype=torch.uint8, device="cuda:0")
    return t if width == 1 else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[width])


def on_device(s, nf):
    """A txmergeref source as the tuple NfBase.tx_merge takes."""
    idx_t = dev(s.idx, np.uint32)[:s.lists_cap] if s.lists_cap else None
    return (nf, dev(s.frames, np.uint8), s.slot, dev(s.lens, np.uint16), idx_t,
            dev(s.offset, np.uint32), s.port, s.in_port,
            dev(s.key, np.uint32) if s.key is not None else None,
            dev(s.now, np.int64) if s.now is not None else None, s.now0, s.now_step)


class Merged:
    """One vp_tx_merge call over canary-filled buffers, back on the host."""

    def __init__(self, nf, dsrcs, out_slot, out_cap, without=(), stream=None, before=None):
        self.out_slot, self.out_cap, self.without = out_slot, out_cap, without
        t = {name: filled(out_cap * (out_slot if name == "frames" else 1), w) for name, w in BUFS}
        cnt = filled(1, 4)
        torch.cuda.synchronize()
        if before is not None:
            before()  # (work that fills the lists, enqueued on the same stream)

        def arg(name):
            k = out_cap * (out_slot if name == "frames" else 1)
            return t[name][:k] if out_cap and name not in without else None

        nf.tx_merge(dsrcs, arg("frames"), out_slot, arg("len"), cnt[:1], arg("src"), arg("which"),
                    out_now=arg("now"), out_in_dev=arg("in_dev"), out_key=arg("key"),
                    stream=stream)
        torch.cuda.synchronize()
        for name, w in BUFS:
            setattr(self, name, t[name].cpu().numpy().view(VIEW[w]))
        self.count = cnt.cpu().numpy().view(np.uint32)


def tails_untouched(got, total):
    """count, and the canary at and beyond entry min(total, cap) of every
    buffer: all that is promised when keys decrease."""
    m = min(total, got.out_cap)
    assert int(got.count[0]) == total
    assert (got.count[1:] == canary_of(4)).all(), "written past count"
    for name, w in BUFS:
        k = m * (got.out_slot if name == "frames" else 1)
        if name in got.without:
            k = 0
        assert (getattr(got, name)[k:] == canary_of(w)).all(), \
            "%s written at or beyond entry %d" % (name, m)
    return m


def compare(got, ref):
    """Every buffer of `got` whole against the reference: what the call owes,
    and the canary everywhere else."""
    m = tails_untouched(got, ref.count)
    assert ref.len.size == m
    for name, w in BUFS:
        if name in got.without:
            continue
        k = m * (got.out_slot if name == "frames" else 1)
        g, r = getattr(got, name)[:k], getattr(ref, name).view(VIEW[w])
        bad = np.nonzero(g != r)[0]
        assert bad.size == 0, "%s differs at %s: %s vs %s" % (name, bad[:8], g[bad[:8]],
                                                                r[bad[:8]])


def check(srcs, out_slot=64, out_cap=None, without=(), stream=None, nfs=None, exact=True):
    """Sources (txmergeref.source) through one call; the receiving context is
    a further one. out_cap None: exactly the total. Returns (got, reference)."""
    nfs = nfs or [bridge(s.n_devices, j % 2) for j, s in enumerate(srcs)]
    if out_cap is None:
        out_cap = sum(entries(s)[0].size for s in srcs)
    ref = merge_reference(srcs, out_slot, out_cap)
    dsrcs = [on_device(s, nf) for s, nf in zip(srcs, nfs)]
    got = Merged(bridge(2, 2), dsrcs, out_slot, out_cap, without, stream)
    if exact:
        compare(got, ref)
    else:
        tails_untouched(got, ref.count)
    for s, d in zip(srcs, dsrcs):
        assert d[1].cpu().numpy().tobytes() == s.frames.tobytes(), "frames written"
    return got, ref


def make(rng, count, keys, slot=64, nd=3, port=1, in_port=0, time="array"):
    """A source whose list `port` names `count` packets of its own batch in
    ascending order, its neighbours not empty. keys: None (the index) or the
    batch's key array (one entry per packet, count + 9 of them)."""
    n = count + 9
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    lens[:4] = [0, 1518, 0xFFFF, slot]
    who = np.sort(rng.choice(n, count, replace=False))
    rest = rng.integers(0, n, 12)
    idx = np.concatenate([rest[:5], who, rest[5:]]).astype(np.uint32)
    offset = [0, 5, 5 + count, 5 + count + 7][:nd + 1]
    offset += [offset[-1]] * (nd + 1 - len(offset))
    now = dict(now=np.cumsum(rng.integers(0, 1000, n)).astype(np.int64) + (1 << 40)) \
        if time == "array" else dict(now0=(1 << 62) // n + 12345, now_step=(1 << 62) // n)
    return source(frames_for(rng, n, slot), slot, lens, idx, offset, nd, port, in_port=in_port,
                  key=keys, **now)


def sorted_keys(rng, n, kmax):
    return np.sort(rng.integers(0, kmax, n)).astype(np.uint32)


COUNTS = [(0,), (1,), (2049,), (63, 64), (65, 0), (0, 0), (2047, 2048), (2048, 2049),
          (1, 63, 3 * B + 5), (64, 65, 2047), (0, 1, 63, 64, 65, 2047, 2048, 2049)]


@pytest.mark.parametrize("counts", COUNTS, ids=lambda c: "-".join(map(str, c)))
def test_counts_around_wave_and_block_edges(counts):
    """n_srcs 1, 2, 3 and 8; explicit key arrays that repeat inside a source
    and collide across sources, the times from arrays and affine in turn."""
    rng = np.random.default_rng(7000 + sum(counts) + len(counts))
    kmax = max(sum(counts) // 3, 4)
    srcs = [make(rng, c, sorted_keys(rng, c + 9, kmax), in_port=100 + j,
                 time="array" if j % 2 else "affine") for j, c in enumerate(counts)]
    got, ref = check(srcs)
    assert ref.count == sum(counts)
    if len(counts) > 1 and min(sorted(counts)[-2:]) > 60:
        assert (np.diff(ref.key) == 0).sum() > 10, "no ties"
        assert len(set(ref.which.tolist())) > 1


def pair(kind):
    rng = np.random.default_rng(7100)
    ca, cb = B + 100, B + 1
    na, nb = ca + 9, cb + 9
    if kind == "alternating":
        ka, kb = 2 * np.arange(na), 2 * np.arange(nb) + 1
    elif kind == "one-before":
        ka, kb = np.arange(na) + nb + 7, np.arange(nb)
    elif kind == "runs":  # runs of 700 and 650 keys in turn: they straddle entry 2048
        ka = np.arange(na) + (np.arange(na) // 700) * 650
        kb = np.arange(nb) + (np.arange(nb) // 650 + 1) * 700
    else:  # all keys equal
        ka, kb = np.full(na, 5), np.full(nb, 5)
    return [make(rng, ca, ka.astype(np.uint32), in_port=1),
            make(rng, cb, kb.astype(np.uint32), in_port=0, time="affine")]


@pytest.mark.parametrize("kind", ["alternating", "one-before", "runs", "equal"])
def test_interleavings(kind):
    got, ref = check(pair(kind))
    w = ref.which
    if kind == "alternating":
        assert (np.diff(w[:2 * B].astype(int)) != 0).mean() > 0.9
    elif kind == "one-before":
        assert w[:B + 1].all() and not w[B + 1:].any()
    elif kind == "runs":
        change = np.nonzero(np.diff(w.astype(int)))[0]
        assert 3 < change.size < 12
    else:
        assert not w[:B + 100].any() and w[B + 100:].all()


def mix(rng, n, nd, p_drop=0.1, p_flood=0.6):
    ins = rng.integers(0, nd, n).astype(np.uint16)
    out = rng.integers(0, nd, n).astype(np.uint16)
    r = rng.random(n)
    out[r < p_flood] = F
    drop = (r >= p_flood) & (r < p_flood + p_drop)
    out[drop] = ins[drop]
    return out, ins


def test_two_ports_of_one_flooded_batch_without_keys():
    """key == NULL: ports 1 and 3 of one batch's lists, built by vp_tx_build
    from out ports that mostly flood, so most packets stand in both lists."""
    rng = np.random.default_rng(7200)
    n, nd, slot = B + 700, 4, 64
    out, ins = mix(rng, n, nd)
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    nf = bridge(nd)
    idx_t = torch.zeros(3 * n, dtype=torch.int32, device="cuda:0")
    off_t = torch.zeros(nd + 1, dtype=torch.int32, device="cuda:0")
    nf.tx_build(dev(out, np.uint16), dev(ins, np.uint16), dev(lens, np.uint16), idx_t, off_t,
                None)
    torch.cuda.synchronize()
    idx = idx_t.cpu().numpy().view(np.uint32)
    offset = off_t.cpu().numpy().view(np.uint32)
    srcs = [source(frames, slot, lens, idx[:offset[nd]], offset, nd, p, in_port=q, now0=5,
                   now_step=3) for p, q in ((1, 0), (3, 1))]
    got, ref = check(srcs, nfs=[nf, nf])
    assert (np.diff(ref.key) == 0).sum() > n // 4, "few packets in both lists"
    assert (np.diff(ref.key) >= 0).all()
    twice = np.nonzero(np.diff(ref.key) == 0)[0]
    assert (ref.which[twice] == 0).all() and (ref.which[twice + 1] == 1).all()


@pytest.mark.parametrize("slots", [((64,), 64), ((64,), 128), ((64,), 80), ((128,), 64),
                                   ((64, 128), 64), ((128, 64), 128), ((64, 128, 80), 80),
                                   ((1536, 64), 256)])
def test_slots_sources_to_destination(slots):
    """Both copy paths (64 and 128: 16-byte units that divide a wave; 80: the
    wave path), widening, narrowing, and sources of different slots."""
    src_slots, out_slot = slots
    rng = np.random.default_rng(7300 + out_slot + len(src_slots))
    counts = [150 + 40 * j if max(src_slots) > 128 else B // 2 + 77 + j
              for j in range(len(src_slots))]
    srcs = [make(rng, c, None if len(src_slots) == 1 else sorted_keys(rng, c + 9, 900), slot=s,
                 in_port=j) for j, (c, s) in enumerate(zip(counts, src_slots))]
    got, ref = check(srcs, out_slot=out_slot)
    g = got.frames[:ref.count * out_slot].reshape(ref.count, out_slot)
    for j, s in enumerate(src_slots):
        rows = g[ref.which == j]
        assert rows[:, :min(s, out_slot)].all()
        if s < out_slot:
            assert not rows[:, s:].any()


def trunc_case():
    rng = np.random.default_rng(7400)
    counts = (B + 17, 900, B)
    return [make(rng, c, sorted_keys(rng, c + 9, 1500), in_port=j) for j, c in enumerate(counts)]


@pytest.mark.parametrize("out_cap", [0, 1, 64, B, 2 * B + 917 - 1, 2 * B + 917, 2 * B + 917 + 5])
def test_out_cap_below_at_and_above_the_total(out_cap):
    got, ref = check(trunc_case(), out_cap=out_cap)
    assert int(got.count[0]) == 2 * B + 917  # the true total, whatever fitted


@pytest.mark.parametrize("lists_cap,want", [(5 + 100, 100), (5 + B, B), (5, 0), (3, 0), (0, 0)])
def test_a_source_clipped_by_its_lists_capacity(lists_cap, want):
    """offset[] holds the true counts of lists that outgrew idx: source 1's
    capacity ends inside its list, at its first entry, and before it."""
    srcs = trunc_case()
    srcs[2].lists_cap = lists_cap
    got, ref = check(srcs)
    assert ref.count == B + 17 + 900 + want and (ref.which == 2).sum() == want


def test_entries_outside_a_batch():
    """Entries >= n (vp_tx_build writes none): their key is the index, their
    slot zero, len and now 0, and nothing is read through them. The lists are
    in ascending key order all the same."""
    rng = np.random.default_rng(7500)
    a = make(rng, 700, None)
    b = make(rng, 800, sorted_keys(rng, 809, 600), in_port=9)
    for s, extra in ((a, [709, 709, 5000, 0xFFFFFFFF]), (b, [809, 1 << 31, 0xFFFFFFFE])):
        lo, hi = int(s.offset[1]), int(s.offset[2])
        s.idx = np.concatenate([s.idx[:hi], np.array(extra, np.uint32), s.idx[hi:]])
        s.offset = s.offset + np.array([0, 0, len(extra), len(extra)], np.uint32)
        s.lists_cap = s.idx.size
    got, ref = check([a, b])
    outside = np.nonzero(((ref.which == 0) & (ref.src >= 709)) |
                         ((ref.which == 1) & (ref.src >= 809)))[0]
    assert outside.size == 7 and ref.src[-1] == 0xFFFFFFFF and ref.key[-1] == 0xFFFFFFFF
    assert not ref.len[outside].any() and not ref.now[outside].any()
    assert not got.frames[:ref.count * 64].reshape(-1, 64)[outside].any()


@pytest.mark.parametrize("out_cap", [None, B + 5])
def test_keys_that_decrease_write_nothing_beyond_the_total(out_cap):
    """The precondition broken: random keys, reversed lists, entries outside
    the batch. Only count and the untouched tails are promised."""
    rng = np.random.default_rng(7600)
    srcs = [make(rng, c, rng.integers(0, 3000, c + 9).astype(np.uint32), in_port=j)
            for j, c in enumerate((B + 300, 2 * B + 1, 77))]
    srcs[1].idx = srcs[1].idx[::-1].copy()
    srcs[1].idx[::13] = 0xFFFFFFF0
    srcs[1].offset = np.array([0, 7, 7 + 2 * B + 1, 7 + 2 * B + 1 + 5], np.uint32)
    srcs[2].key = None
    srcs[2].idx = srcs[2].idx[::-1].copy()
    srcs[2].offset = np.array([0, 7, 7 + 77, 7 + 77 + 5], np.uint32)
    got, ref = check(srcs, out_cap=out_cap, exact=False)
    assert int(got.count[0]) == 3 * B + 378


@pytest.mark.parametrize("without", [("now",), ("in_dev",), ("key",), ("now", "in_dev", "key")])
def test_now_in_dev_and_key_may_be_null(without):
    srcs = pair("runs")
    a, _ = check(srcs)
    b, _ = check(srcs, without=without)
    for name in ("frames", "len", "src", "which"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()


def test_same_bytes_twice():
    srcs = trunc_case()
    a, _ = check(srcs, out_slot=128)
    b, _ = check(srcs, out_slot=128)
    for name, _ in BUFS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()


@pytest.mark.parametrize("count", [0, 65, 2 * B + 17])
def test_one_source_without_keys_is_tx_rebatch(count):
    rng = np.random.default_rng(7700 + count)
    s = make(rng, count, None, slot=128, time="affine")
    got, ref = check([s], out_slot=64)
    nf = bridge(3)
    d = on_device(s, nf)
    o = [filled(count * 64, 1), filled(count, 2), filled(count, 8), filled(count, 4), filled(1, 4)]
    torch.cuda.synchronize()
    nf.tx_rebatch(d[1], 128, d[3], d[4], d[5], 1, o[0][:count * 64] if count else None, 64,
                  o[1][:count] if count else None, o[4][:1],
                  out_now=o[2][:count] if count else None,
                  out_src=o[3][:count] if count else None, now0=s.now0, now_step=s.now_step)
    torch.cuda.synchronize()
    assert o[0].cpu().numpy().tobytes() == got.frames.tobytes()
    assert o[1].cpu().numpy().tobytes() == got.len.tobytes()
    assert o[2].cpu().numpy().tobytes() == got.now.tobytes()
    assert o[3].cpu().numpy().tobytes() == got.src.tobytes()
    assert o[4].cpu().numpy().tobytes() == got.count.tobytes()
    r = rebatch_reference(s.frames, 128, s.lens, s.idx, s.offset, s.idx.size, 3, 1, 64, count,
                          now0=s.now0, now_step=s.now_step)
    assert r[0] == ref.count and r[1].tobytes() == ref.frames.tobytes()
    assert r[3].tobytes() == ref.now.tobytes() and r[4].tobytes() == ref.src.tobytes()


def test_two_tx_builds_and_the_merge_back_to_back_on_one_stream():
    """vp_tx_build for two contexts and vp_tx_merge into a third enqueued on
    one stream that is none of theirs, nothing waited for in between."""
    rng = np.random.default_rng(7800)
    s = torch.cuda.Stream()
    nfs, data, refs = [bridge(4, 0), bridge(2, 1)], [], []
    for nf, nd, n, port, in_port in ((nfs[0], 4, B + 300, 2, 1), (nfs[1], 2, B - 50, 1, 0)):
        out, ins = mix(rng, n, nd, p_flood=0.3)
        lens = rng.integers(0, 65, n).astype(np.uint16)
        frames = frames_for(rng, n, 64)
        key = sorted_keys(rng, n, 2500)
        full, r_off, _ = tx_reference(out, ins, lens, nd, 1 << 32)
        now = np.cumsum(rng.integers(0, 50, n)).astype(np.int64)
        refs.append(source(frames, 64, lens, full, r_off, nd, port, in_port=in_port, key=key,
                           now=now))
        idx_t = torch.full((full.size,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        off_t = torch.zeros(nd + 1, dtype=torch.int32, device="cuda:0")
        data.append((nf, dev(out, np.uint16), dev(ins, np.uint16), dev(lens, np.uint16), idx_t,
                     off_t, dev(frames, np.uint8), dev(key, np.uint32), dev(now, np.int64), port,
                     in_port))
    ref = merge_reference(refs, 64, 1 << 40)

    def builds():
        for nf, o_t, i_t, l_t, idx_t, off_t, *_ in data:
            nf.tx_build(o_t, i_t, l_t, idx_t, off_t, None, stream=s)

    dsrcs = [(nf, f_t, 64, l_t, idx_t, off_t, port, in_port, k_t, n_t, 0, 0)
             for nf, o_t, i_t, l_t, idx_t, off_t, f_t, k_t, n_t, port, in_port in data]
    got = Merged(bridge(2, 2), dsrcs, 64, ref.count, stream=s, before=builds)
    compare(got, ref)
    assert len(set(ref.which.tolist())) == 2


def test_einval_cases_that_need_a_context_write_nothing():
    nf, other = bridge(2, 2), bridge(2, 0)
    L = nf.L
    d = torch.device("cuda:0")
    n, slot, cap = 64, 64, 64
    frames = torch.full((2 * n * slot,), 7, dtype=torch.uint8, device=d)
    lens = torch.full((n,), 60, dtype=torch.int16, device=d)
    idx = torch.arange(cap, dtype=torch.int32, device=d)
    off = torch.tensor([0, 30, cap], dtype=torch.int32, device=d)
    outs = {name: filled(cap * (slot if name == "frames" else 1), w) for name, w in BUFS}
    outs["count"] = filled(1, 4)
    torch.cuda.synchronize()
    keep = []

    def srcs(port=1, n_=n, base=None, ctx=None):
        b = vigor_amd.DevBatchC(frames=base or frames.data_ptr(), slot=slot, n=n_,
                                len=lens.data_ptr())
        a = vigor_amd.TxListsC(idx=idx.data_ptr(), cap=cap, offset=off.data_ptr(), stats=None)
        arr = (vigor_amd.TxSourceC * 1)()
        keep.extend([b, a])
        arr[0].ctx, arr[0].batch, arr[0].lists = ctx or other.h, C.addressof(b), C.addressof(a)
        arr[0].port, arr[0].in_port, arr[0].key = port, 0, None
        return arr

    def merged(**kw):
        a = {name: t.data_ptr() for name, t in outs.items()}
        a.update(slot=slot, cap=cap)
        a.update(kw)
        return vigor_amd.TxMergedC(**a)

    def rc(arr, o):
        return L.vp_tx_merge(nf.h, arr, 1, C.byref(o), None)

    E = vigor_amd.VP_EINVAL
    for port in (2, 3, 32, 0xFFFFFFFF):
        assert rc(srcs(port=port), merged()) == E
    base = frames.data_ptr()
    assert rc(srcs(), merged(frames=base)) == E
    assert rc(srcs(), merged(frames=base + (n - 1) * slot)) == E
    assert rc(srcs(base=base + (cap - 1) * slot), merged(frames=base)) == E
    assert rc(srcs(n_=2 * n), merged(frames=base + n * slot)) == E
    torch.cuda.synchronize()
    assert all(bool((t.view(torch.uint8) == CANARY).all()) for t in outs.values())
    assert bool((frames == 7).all())
    # accepted: a source that is the receiving context itself; cap 0 with the
    # buffers NULL writes the count alone; the output right behind the batch
    assert rc(srcs(ctx=nf.h), merged(frames=None, len=None, src=None, which=None, cap=0)) == 0
    torch.cuda.synchronize()
    assert int(outs["count"][0]) == cap - 30
    assert all(bool((t.view(torch.uint8) == CANARY).all()) for k, t in outs.items()
               if k != "count")
    assert rc(srcs(), merged(frames=base + n * slot)) == 0
    torch.cuda.synchronize()
    assert bool((frames[:n * slot + (cap - 30) * slot] == 7).all())  # (copies of 7s)
    assert outs["which"][:cap - 30].cpu().tolist() == [0] * (cap - 30)
    assert outs["src"][:cap - 30].cpu().tolist() == list(range(30, cap))
