"""vp_tx_rebatch on the GPU: a port's transmit list as the next NF's batch,
byte for byte against txbatchref.rebatch_reference (the contract of
include/vigpath.h as a per-entry loop).

Every case fills frames, len, now, src and count with a canary first, with a
canary tail behind each, compares the buffers whole (the untouched parts
included) and checks that the source frames are unchanged. Hand-made lists go
through the smallest vigbridge context with the wanted n_devices (the call
reads only the batch and the lists); the stream and flood cases take their
lists from vp_tx_build."""
import ctypes as C

import numpy as np
import pytest
import torch

import vigor_amd
from txbatchref import rebatch_reference
from txref import tx_reference
from vigor_amd import traces as TR

pytestmark = pytest.mark.gpu

B = 2048  # entries per block of vp_tx_rebatch's kernel (vp_txbatch.hip)
F = 0xFFFF
CANARY = 0xA5
TAIL = 64  # canary entries kept behind every buffer


def canary_of(width):
    return int.from_bytes(bytes([CANARY]) * width, "little")


_ctx = {}


def bridge(nd):
    if nd not in _ctx:
        _ctx[nd] = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)
    return _ctx[nd]


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


class Rebatched:
    """One vp_tx_rebatch call over canary-filled buffers, back on the host."""

    def __init__(self, nf, f_t, slot, l_t, idx_t, off_t, lists_cap, port, out_slot, out_cap,
                 with_now=True, with_src=True, now_t=None, now0=0, now_step=0, stream=None,
                 before=None):
        self.out_slot, self.out_cap = out_slot, out_cap
        self.with_now, self.with_src = with_now, with_src
        fr = filled(out_cap * out_slot, 1)
        ln, nw, sr, cnt = filled(out_cap, 2), filled(out_cap, 8), filled(out_cap, 4), filled(1, 4)
        torch.cuda.synchronize()
        if before is not None:
            before()  # (work that fills the lists, enqueued on the same stream)
        nf.tx_rebatch(f_t, slot, l_t, idx_t[:lists_cap] if lists_cap else None, off_t, port,
                      fr[:out_cap * out_slot] if out_cap else None, out_slot,
                      ln[:out_cap] if out_cap else None, cnt[:1],
                      out_now=nw[:out_cap] if with_now and out_cap else None,
                      out_src=sr[:out_cap] if with_src and out_cap else None,
                      now=now_t, now0=now0, now_step=now_step, stream=stream)
        torch.cuda.synchronize()
        self.frames = fr.cpu().numpy()
        self.len = ln.cpu().numpy().view(np.uint16)
        self.now = nw.cpu().numpy()
        self.src = sr.cpu().numpy().view(np.uint32)
        self.count = cnt.cpu().numpy().view(np.uint32)

    def same(self, other):
        return all(getattr(self, k).tobytes() == getattr(other, k).tobytes()
                   for k in ("frames", "len", "now", "src", "count"))


def compare(got, ref):
    """Every buffer of `got` whole against the reference's (count, frames, len,
    now, src): what the call owes, and the canary everywhere else."""
    count, r_f, r_l, r_n, r_s = ref
    m = min(count, got.out_cap)
    assert r_l.size == m
    assert int(got.count[0]) == count
    assert (got.count[1:] == canary_of(4)).all(), "written past count"
    bad = np.nonzero(got.frames[:r_f.size] != r_f)[0]
    assert bad.size == 0, "frames differ at bytes %s: %s vs %s" % (
        bad[:8], got.frames[bad[:8]], r_f[bad[:8]])
    assert (got.frames[r_f.size:] == CANARY).all(), "frames written at or beyond entry %d" % m
    assert got.len[:m].tolist() == r_l.tolist()
    assert (got.len[m:] == canary_of(2)).all(), "len written at or beyond entry %d" % m
    k = m if got.with_now else 0
    assert got.now[:k].tolist() == r_n[:k].tolist()
    assert (got.now[k:].view(np.uint64) == canary_of(8)).all(), "now written beyond entry %d" % k
    k = m if got.with_src else 0
    assert got.src[:k].tolist() == r_s[:k].tolist()
    assert (got.src[k:] == canary_of(4)).all(), "src written beyond entry %d" % k


def check(nd, frames, slot, lens, idx, offset, port, out_slot=None, out_cap=None, lists_cap=None,
          now=None, now0=0, now_step=0, with_now=True, with_src=True, stream=None, nf=None):
    """Hand-made lists (numpy) through one call. out_cap None: exactly the
    port's list; lists_cap None: everything idx holds. Returns (got,
    reference)."""
    nf = nf or bridge(nd)
    idx = np.asarray(idx, np.uint32)
    offset = np.asarray(offset, np.uint32)
    out_slot = slot if out_slot is None else out_slot
    lists_cap = idx.size if lists_cap is None else lists_cap
    if out_cap is None:
        out_cap = rebatch_reference(frames, slot, lens, idx, offset, lists_cap, nd, port,
                                    out_slot, 0)[0]
    ref = rebatch_reference(frames, slot, lens, idx, offset, lists_cap, nd, port, out_slot,
                            out_cap, now=now, now0=now0, now_step=now_step)
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    idx_t = dev(idx if idx.size else np.zeros(1, np.uint32), np.uint32)
    off_t = dev(offset, np.uint32)
    now_t = dev(now, np.int64) if now is not None else None
    got = Rebatched(nf, f_t, slot, l_t, idx_t, off_t, lists_cap, port, out_slot, out_cap,
                    with_now, with_src, now_t, now0, now_step, stream)
    compare(got, ref)
    assert f_t.cpu().numpy().tobytes() == np.asarray(frames, np.uint8).tobytes(), "frames written"
    return got, ref


def mixed_lens(slot):
    """Lengths in one batch: the edges of the contract."""
    return [0, 1, 14, 60, 64, 65, slot, 1518, 0xFFFF]


def lists_around(rng, n, count, where):
    """Four ports; port `where` lists `count` packets in ascending order, its
    neighbours are not empty. Returns (idx, offset)."""
    sizes = [37, 5, 70, 21]
    sizes[where] = count
    parts = [np.sort(rng.choice(n, s, replace=False)) if s <= n else
             np.sort(rng.integers(0, n, s)) for s in sizes]
    return np.concatenate(parts).astype(np.uint32), np.concatenate([[0], np.cumsum(sizes)])


COUNTS = [0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17]


@pytest.mark.parametrize("where", [0, 2, 3])
@pytest.mark.parametrize("count", COUNTS)
def test_list_lengths_around_wave_and_block_edges(count, where):
    rng = np.random.default_rng(5000 + 10 * count + where)
    n, slot = max(count + 9, 100), 64
    lens = rng.integers(0, 65, n).astype(np.uint16)
    edge = mixed_lens(slot)
    lens[:len(edge)] = edge
    frames = frames_for(rng, n, slot)
    idx, offset = lists_around(rng, n, count, where)
    got, ref = check(4, frames, slot, lens, idx, offset, where, now0=123456789, now_step=3)
    assert ref[0] == count


@pytest.mark.parametrize("slots", [(64, 64), (128, 128), (64, 128), (1536, 64), (2048, 2048),
                                   (128, 64), (64, 1536), (256, 1024)])
def test_slots_source_to_destination(slots):
    """Equal slots on both copy paths, widening (the zero fill) and narrowing
    (len kept); the list spans a block edge for the narrow slots and several
    turns of a wave for the wide ones."""
    slot, out_slot = slots
    rng = np.random.default_rng(slot * 7 + out_slot)
    count = B + 77 if max(slots) <= 128 else 150
    n = count + 40
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    edge = mixed_lens(slot)
    at = rng.permutation(n)[:len(edge)]
    lens[at] = edge
    frames = frames_for(rng, n, slot)
    who = np.sort(np.concatenate([at, rng.permutation(np.setdiff1d(np.arange(n), at))
                                  [:count - at.size]]))
    rest = rng.integers(0, n, 50)
    idx = np.concatenate([rest[:20], who, rest[20:]]).astype(np.uint32)
    now = np.cumsum(rng.integers(0, 1000, n)).astype(np.int64) + (1 << 40)
    got, ref = check(3, frames, slot, lens, idx, [0, 20, 20 + count, idx.size], 1,
                     out_slot=out_slot, now=now)
    count_, r_f, r_l, r_n, r_s = ref
    assert set(edge) <= set(r_l.tolist()), "a length did not come through unchanged"
    assert (np.diff(r_n) >= 0).all()
    if out_slot > slot:  # every tail is zero, every head is not
        g = got.frames[:count * out_slot].reshape(count, out_slot)
        assert not g[:, slot:].any() and g[:, :slot].all()


def cap_case():
    rng = np.random.default_rng(61)
    n, slot, count = 3 * B, 64, 2 * B + 17
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx, offset = lists_around(rng, n, count, 1)
    return frames, slot, lens, idx, offset, count


@pytest.mark.parametrize("out_cap", [0, 1, 64, B, 2 * B, 2 * B + 16, 2 * B + 17, 2 * B + 18])
def test_out_cap_below_at_and_above_the_list(out_cap):
    frames, slot, lens, idx, offset, count = cap_case()
    got, ref = check(4, frames, slot, lens, idx, offset, 1, out_cap=out_cap, now0=7, now_step=1)
    assert int(got.count[0]) == count  # the true count, whatever fitted


@pytest.mark.parametrize("lists_cap,want", [(5 + 100, 100), (5 + B, B), (5, 0), (3, 0), (0, 0)])
def test_lists_clipped_by_their_capacity(lists_cap, want):
    """offset[] holds the true counts of lists that outgrew idx: the capacity
    ends inside port 1's list, at its first entry, and before it."""
    rng = np.random.default_rng(62)
    n, slot, count = 3 * B, 64, 2 * B + 17
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = rng.integers(0, n, 5 + count + 30).astype(np.uint32)
    got, ref = check(3, frames, slot, lens, idx, [0, 5, 5 + count, 5 + count + 30], 1,
                     out_cap=count, lists_cap=lists_cap, now0=1, now_step=1)
    assert ref[0] == want


def test_garbage_lists_read_nothing_outside_the_batch():
    rng = np.random.default_rng(63)
    n, slot = 500, 128
    lens = rng.integers(1, slot + 1, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = np.concatenate([np.arange(n - 1, -1, -1), np.repeat(np.arange(0, n, 7), 3),
                          rng.integers(0, n, 300)]).astype(np.uint32)
    idx[::11] = n
    idx[5::37] = 0xFFFFFFFF
    idx[9::41] = n + rng.integers(1, 1 << 30, idx[9::41].size)
    now = rng.integers(1, 1 << 50, n).astype(np.int64)
    got, (count, r_f, r_l, r_n, r_s) = check(2, frames, slot, lens, idx, [0, 100, idx.size], 1,
                                             now=now)
    outside = np.nonzero(r_s >= n)[0]
    assert outside.size > 50 and 0xFFFFFFFF in r_s[outside].tolist()
    assert not r_l[outside].any() and not r_n[outside].any()
    assert not got.frames[:count * slot].reshape(count, slot)[outside].any()


def time_case():
    rng = np.random.default_rng(64)
    n, slot, count = B + 300, 64, B + 100
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx, offset = lists_around(rng, n, count, 2)
    return rng, n, frames, slot, lens, idx, offset


def test_time_array_and_negative_times():
    rng, n, frames, slot, lens, idx, offset = time_case()
    now = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    now[:3] = [0, -1, (1 << 63) - 1]
    check(4, frames, slot, lens, idx, offset, 2, now=now)


def test_affine_time_is_a_64_bit_product():
    rng, n, frames, slot, lens, idx, offset = time_case()
    step = (1 << 62) // n  # i * step passes 2^32 and 2^61 inside the batch
    got, (count, r_f, r_l, r_n, r_s) = check(4, frames, slot, lens, idx, offset, 2,
                                             now0=(1 << 62) // n + 12345, now_step=step)
    assert int(r_n.max()) > (1 << 61) and (np.diff(r_n) > 0).all()
    # a sum that wraps is the same 64-bit sum
    check(4, frames, slot, lens, idx, offset, 2, now0=(1 << 63) - 5, now_step=step)
    check(4, frames, slot, lens, idx, offset, 2, now0=-(1 << 40), now_step=0)


@pytest.mark.parametrize("with_now,with_src", [(False, True), (True, False), (False, False)])
def test_now_and_src_may_be_null(with_now, with_src):
    rng, n, frames, slot, lens, idx, offset = time_case()
    a, _ = check(4, frames, slot, lens, idx, offset, 2, now0=5, now_step=2)
    b, _ = check(4, frames, slot, lens, idx, offset, 2, now0=5, now_step=2, with_now=with_now,
                 with_src=with_src)
    assert a.frames.tobytes() == b.frames.tobytes() and a.len.tobytes() == b.len.tobytes()


def test_same_bytes_twice():
    rng = np.random.default_rng(65)
    n, slot = 2 * B + 17, 128
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = rng.integers(0, n + 20, 2 * n).astype(np.uint32)
    a, _ = check(2, frames, slot, lens, idx, [0, n // 2, 2 * n], 1, out_slot=256, now0=9,
                 now_step=4)
    b, _ = check(2, frames, slot, lens, idx, [0, n // 2, 2 * n], 1, out_slot=256, now0=9,
                 now_step=4)
    assert a.same(b)


def mix(rng, n, nd, p_drop=0.15, p_flood=0.1, p_bad=0.05):
    ins = rng.integers(0, nd, n).astype(np.uint16)
    out = rng.integers(0, nd, n).astype(np.uint16)
    r = rng.random(n)
    bad = r < p_bad
    out[bad] = rng.integers(nd, F, int(bad.sum()))
    out[(r >= p_bad) & (r < p_bad + p_flood)] = F
    drop = (r >= p_bad + p_flood) & (r < p_bad + p_flood + p_drop)
    out[drop] = ins[drop]
    return out, ins


def test_non_default_stream_right_after_tx_build():
    """vp_tx_build and vp_tx_rebatch enqueued back to back on one stream that
    is not the context's, nothing waited for in between."""
    rng = np.random.default_rng(66)
    n, nd, slot = 2 * B + 300, 4, 64
    out, ins = mix(rng, n, nd)
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    full, r_off, _ = tx_reference(out, ins, lens, nd, 1 << 32)
    nf = bridge(nd)
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    o_t, i_t = dev(out, np.uint16), dev(ins, np.uint16)
    s = torch.cuda.Stream()
    for port in (0, 3):
        idx_t = torch.full((full.size,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        off_t = torch.zeros(nd + 1, dtype=torch.int32, device="cuda:0")
        count = int(r_off[port + 1] - r_off[port])
        got = Rebatched(nf, f_t, slot, l_t, idx_t, off_t, full.size, port, slot, count,
                        now0=1000, now_step=1, stream=s,
                        before=lambda: nf.tx_build(o_t, i_t, l_t, idx_t, off_t, None, stream=s))
        assert idx_t.cpu().numpy().view(np.uint32).tobytes() == full.tobytes()
        compare(got, rebatch_reference(frames, slot, lens, full, r_off, full.size, nd, port, slot,
                                       count, now0=1000, now_step=1))
    assert f_t.cpu().numpy().tobytes() == frames.tobytes(), "frames written"


def test_real_lists_every_port_holds_the_flooded_frames():
    """vigbridge with 4 ports over broadcast frames from unknown stations:
    every frame floods, and every port's batch holds the frames that arrived
    on the other three."""
    rng = np.random.default_rng(67)
    n, nd, slot = B + 200, 4, 64
    frames = np.zeros((n, slot), np.uint8)
    frames[:, 0:6] = 0xFF  # broadcast: never learned, always flooded
    frames[:, 6] = 0x02
    frames[:, 7:12] = rng.integers(0, 256, (n, 5))
    frames[:, 12:14] = (0x08, 0x00)
    frames[:, 14:60] = rng.integers(1, 255, (n, 46))
    lens = np.full(n, 60, np.uint16)
    ins = rng.integers(0, nd, n).astype(np.uint16)
    br = vigor_amd.Bridge(vigor_amd.bridge_config_from_args(["--capacity", "8192"], nd), gpu=0)
    f_t, l_t, i_t = dev(frames.reshape(-1), np.uint8), dev(lens, np.uint16), dev(ins, np.uint16)
    o_t = torch.zeros(n, dtype=torch.int16, device="cuda:0")
    br.process_device(f_t, l_t, i_t, o_t, slot, now0=1_000_000, now_step=1)
    torch.cuda.synchronize()
    out = o_t.cpu().numpy().view(np.uint16)
    assert (out == F).all(), "the trace does not flood"
    after = f_t.cpu().numpy()
    idx_t = torch.zeros(3 * n, dtype=torch.int32, device="cuda:0")
    off_t = torch.zeros(nd + 1, dtype=torch.int32, device="cuda:0")
    br.tx_build(o_t, i_t, l_t, idx_t, off_t, None)
    torch.cuda.synchronize()
    idx = idx_t.cpu().numpy().view(np.uint32)
    offset = off_t.cpu().numpy().view(np.uint32)
    assert int(offset[nd]) == 3 * n
    for port in range(nd):
        want = np.nonzero(ins != port)[0]
        got = Rebatched(br, f_t, slot, l_t, idx_t, off_t, 3 * n, port, slot, want.size,
                        now0=1_000_000, now_step=1)
        compare(got, rebatch_reference(after, slot, lens, idx, offset, 3 * n, nd, port, slot,
                                       want.size, now0=1_000_000, now_step=1))
        assert got.src[:want.size].tolist() == want.tolist()
        assert got.frames[:want.size * slot].tobytes() == \
            after.reshape(n, slot)[want].tobytes()
    assert f_t.cpu().numpy().tobytes() == after.tobytes(), "frames written"
    br.close()


def test_einval_cases_write_nothing():
    """Every VP_EINVAL of the contract but the device count: no context with
    more than VP_MAX_DEVICES devices can be created."""
    nf = bridge(2)
    L = nf.L
    d = torch.device("cuda:0")
    n, slot, cap = 64, 64, 64
    frames = torch.full((2 * n * slot + 16,), 7, dtype=torch.uint8, device=d)
    lens = torch.full((n,), 60, dtype=torch.int16, device=d)
    idx = torch.arange(cap, dtype=torch.int32, device=d)
    off = torch.tensor([0, 30, cap], dtype=torch.int32, device=d)
    outs = [filled(cap * slot, 1), filled(cap, 2), filled(cap, 8), filled(cap, 4), filled(1, 4)]
    o_f, o_l, o_n, o_s, o_c = outs
    torch.cuda.synchronize()

    def batch(**kw):
        b = dict(frames=frames.data_ptr(), slot=slot, n=n, len=lens.data_ptr())
        b.update(kw)
        return vigor_amd.DevBatchC(**b)

    def lists(**kw):
        a = dict(idx=idx.data_ptr(), cap=cap, offset=off.data_ptr(), stats=None)
        a.update(kw)
        return vigor_amd.TxListsC(**a)

    def nxt(**kw):
        a = dict(frames=o_f.data_ptr(), slot=slot, cap=cap, len=o_l.data_ptr(),
                 now=o_n.data_ptr(), src=o_s.data_ptr(), count=o_c.data_ptr())
        a.update(kw)
        return vigor_amd.TxNextC(**a)

    def rc(h, b, a, o, port=1):
        ref = [C.byref(x) if x is not None else None for x in (b, a, o)]
        return L.vp_tx_rebatch(h, ref[0], ref[1], port, ref[2], None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == CANARY).all()) for t in outs) \
            and bool((frames == 7).all())

    E = vigor_amd.VP_EINVAL
    assert rc(None, batch(), lists(), nxt()) == E
    assert rc(nf.h, None, lists(), nxt()) == E
    assert rc(nf.h, batch(), None, nxt()) == E
    assert rc(nf.h, batch(), lists(), None) == E
    assert rc(nf.h, batch(), lists(offset=None), nxt()) == E
    assert rc(nf.h, batch(), lists(), nxt(count=None)) == E
    assert rc(nf.h, batch(), lists(idx=None), nxt()) == E
    for port in (2, 3, 32, 0xFFFFFFFF):
        assert rc(nf.h, batch(), lists(), nxt(), port=port) == E
    for bad_slot in (0, 48, 72, 1000):
        assert rc(nf.h, batch(slot=bad_slot), lists(), nxt()) == E
        assert rc(nf.h, batch(), lists(), nxt(slot=bad_slot)) == E
    assert rc(nf.h, batch(frames=frames.data_ptr() + 8), lists(), nxt()) == E
    assert rc(nf.h, batch(), lists(), nxt(frames=o_f.data_ptr() + 8)) == E
    assert rc(nf.h, batch(), lists(), nxt(frames=None)) == E
    assert rc(nf.h, batch(), lists(), nxt(len=None)) == E
    assert rc(nf.h, batch(frames=None), lists(), nxt()) == E
    assert rc(nf.h, batch(len=None), lists(), nxt()) == E
    # overlapping slot arrays: the output inside the batch, the batch's last
    # slot under the output's first, and the other way round
    base = frames.data_ptr()
    assert rc(nf.h, batch(), lists(), nxt(frames=base)) == E
    assert rc(nf.h, batch(), lists(), nxt(frames=base + (n - 1) * slot)) == E
    assert rc(nf.h, batch(frames=base + (cap - 1) * slot), lists(), nxt(frames=base)) == E
    assert rc(nf.h, batch(n=2 * n), lists(), nxt(frames=base + n * slot)) == E
    assert untouched()
    # the same arguments are accepted where the contract allows a NULL; the
    # count is written even where nothing else is
    assert rc(nf.h, batch(), lists(), nxt(frames=None, len=None, cap=0)) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == cap - 30 and bool((o_c[1:] == o_c[1]).all())
    o_c.view(torch.uint8).fill_(CANARY)
    assert rc(nf.h, batch(frames=None, len=None), lists(idx=None, cap=0), nxt()) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == 0
    o_c.view(torch.uint8).fill_(CANARY)
    # adjacent, not overlapping: the output right behind the batch
    assert rc(nf.h, batch(), lists(), nxt(frames=base + n * slot)) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == cap - 30
    assert bool((frames[:n * slot] == 7).all())
    assert bool((frames[n * slot:n * slot + (cap - 30) * slot] == 7).all())  # (copies of 7s)
    with pytest.raises(vigor_amd.VigpathError):
        nf.tx_rebatch(frames[8:n * slot + 8], slot, lens, idx, off, 1, o_f[:cap * slot], slot,
                      o_l[:cap], o_c)
