"""vp_rx_unpack on the GPU: a packed stream of frames as a device batch, byte
for byte against rxunpackref.unpack_reference (the contract of
include/vigpath.h as a per-entry loop), with pos[] and without.

Every case fills frames, len, now, src and count with a canary first, with a
canary tail behind each, compares the buffers whole (the untouched parts
included) and checks that the stream is unchanged. The streams are made here:
every byte of them, the padding behind a frame included, is neither zero nor
the canary, so zero fill, cleared padding and untouched bytes cannot pass for
one another. The call reads nothing of its context but the GPU, so the smallest
vigbridge context serves; the round trips take their streams from vp_tx_build
and vp_tx_pack."""
import ctypes as C

import numpy as np
import pytest
import torch

import vigor_amd
from rxunpackref import unpack_reference

pytestmark = pytest.mark.gpu

B = 2048  # entries per block of vp_rx_unpack's kernels (vp_rxunpack.hip)
F = 0xFFFF
CANARY = 0xA5
TAIL = 64  # canary entries kept behind every buffer
LENGTHS = [0, 1, 15, 16, 17, 60, 64, 65, 127, 1518, 65535]
# (the long ones rarer, to keep the streams small)
WEIGHTS = np.array([3, 3, 3, 3, 3, 3, 3, 3, 3, 1, 0.25])
FORMS = ["pos", "nopos"]


def canary_of(width):
    return int.from_bytes(bytes([CANARY]) * width, "little")


_ctx = {}


def bridge(nd=2):
    if nd not in _ctx:
        _ctx[nd] = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)
    return _ctx[nd]


def dev(a, dtype):
    """A numpy array as a device tensor of the signed torch type of its width."""
    a = np.ascontiguousarray(a, dtype)
    signed = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(signed)).to("cuda:0")


def filled(count, width):
    """count + TAIL entries of `width` bytes, every byte the canary."""
    t = torch.full(((count + TAIL) * width,), CANARY, dtype=torch.uint8, device="cuda:0")
    return t if width == 1 else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[width])


def draw_lens(rng, n):
    """n lengths of LENGTHS; the first ones hold every value once, so that
    they meet inside one wave."""
    lens = rng.choice(LENGTHS, n, p=WEIGHTS / WEIGHTS.sum()).astype(np.uint16)
    k = min(n, len(LENGTHS))
    lens[:k] = rng.permutation(LENGTHS)[:k]
    return lens


def ext(x):
    return (int(x) + 15) & ~15


def lay(rng, n, lens, sel=None, gaps=False):
    """A stream of n frames in entry order, entry e's the length of its
    lens[m(e)] (0 where m(e) is outside lens) padded to 16; gaps: with 0 to 3
    unused 16-byte units before each. Returns (data, pos)."""
    lens = np.asarray(lens, np.uint16)
    m = np.asarray(sel, np.int64) if sel is not None else np.arange(n)
    L = np.zeros(n, np.int64)
    inside = m < lens.size
    L[inside] = lens[m[inside]]
    e = (L + 15) & ~15
    g = 16 * rng.integers(0, 4, n) if gaps else np.zeros(n, np.int64)
    pos = np.cumsum(e + g) - e
    total = int((e + g).sum())
    data = rng.integers(1, 255, total + 16).astype(np.uint8)[:total]
    data[data == CANARY] = 0x11
    return data, pos.astype(np.uint64)


class Unpacked:
    """One vp_rx_unpack call over canary-filled buffers, back on the host."""

    def __init__(self, nf, data_t, n, lens_t, out_slot, out_cap, pos_t=None, sel_t=None,
                 now_t=None, now0=0, now_step=0, with_now=True, with_src=True, stream=None,
                 wait=True):
        """wait False: only the buffers are made; run() enqueues the call and
        fetch() waits for it."""
        self.out_slot, self.out_cap = out_slot, out_cap
        self.with_now, self.with_src = with_now, with_src
        self.t = [filled(out_cap * out_slot, 1), filled(out_cap, 2), filled(out_cap, 8),
                  filled(out_cap, 4), filled(1, 4)]
        self.call = (nf, data_t, n, lens_t, pos_t, sel_t, now_t, now0, now_step, stream)
        if wait:
            torch.cuda.synchronize()
            self.run()
            self.fetch()

    def run(self):
        nf, data_t, n, lens_t, pos_t, sel_t, now_t, now0, now_step, stream = self.call
        fr, ln, nw, sr, cnt = self.t
        out_cap, out_slot = self.out_cap, self.out_slot
        nf.rx_unpack(data_t, lens_t, fr[:out_cap * out_slot] if out_cap else None, out_slot,
                     ln[:out_cap] if out_cap else None, cnt[:1], pos=pos_t, sel=sel_t,
                     out_now=nw[:out_cap] if self.with_now and out_cap else None,
                     out_src=sr[:out_cap] if self.with_src and out_cap else None,
                     now=now_t, now0=now0, now_step=now_step, n=n, stream=stream)

    def fetch(self):
        torch.cuda.synchronize()
        fr, ln, nw, sr, cnt = self.t
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


def check(data, n, lens, out_slot, out_cap=None, pos=None, sel=None, nbytes=None, now=None,
          now0=0, now_step=0, with_now=True, with_src=True, stream=None):
    """A hand-made stream (numpy) through one call. out_cap None: exactly n;
    nbytes None: all of data. Returns (got, reference)."""
    nf = bridge()
    out_cap = n if out_cap is None else out_cap
    nbytes = data.size if nbytes is None else nbytes
    ref = unpack_reference(data, nbytes, n, lens, out_slot, out_cap, pos=pos, sel=sel, now=now,
                           now0=now0, now_step=now_step)
    d_t = dev(data, np.uint8) if data.size else None
    got = Unpacked(nf, d_t[:nbytes] if d_t is not None else None, n,
                   dev(lens, np.uint16) if len(lens) else None, out_slot, out_cap,
                   dev(pos, np.uint64) if pos is not None else None,
                   dev(sel, np.uint32) if sel is not None else None,
                   dev(now, np.int64) if now is not None else None, now0, now_step, with_now,
                   with_src, stream)
    compare(got, ref)
    if d_t is not None:
        assert d_t.cpu().numpy().tobytes() == data.tobytes(), "the stream was written"
    return got, ref


def case(seed, n, form, sel=None, meta_n=None):
    """(data, lens, pos or None) of a random stream in the given form."""
    rng = np.random.default_rng(seed)
    lens = draw_lens(rng, n if meta_n is None else meta_n)
    data, pos = lay(rng, n, lens, sel, gaps=form == "pos")
    return data, lens, pos if form == "pos" else None


COUNTS = [0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", COUNTS)
def test_entry_counts_around_wave_and_block_edges(n, form):
    data, lens, pos = case(7000 + n, n, form)
    got, ref = check(data, n, lens, 64, pos=pos, now0=123456789, now_step=3)
    assert ref[0] == n
    if n >= len(LENGTHS):
        assert set(LENGTHS) <= set(ref[2].tolist()), "a length did not come through unchanged"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("out_slot", [64, 128, 2048, 80, 1536])
def test_out_slots_on_both_copy_paths(out_slot, form):
    """64, 128 and 2048 take the sub-wave path, 80 and 1536 the wave path; the
    entries span a block edge for the narrow slots and several turns of a wave
    for the wide ones. Lengths below, at and beyond every slot."""
    n = B + 77 if out_slot <= 128 else 150
    rng = np.random.default_rng(7100 + out_slot)
    lens = draw_lens(rng, n)
    lens[20:26] = [out_slot - 1, out_slot, out_slot + 1, out_slot - 16, out_slot - 15, 1]
    data, pos = lay(rng, n, lens, gaps=form == "pos")
    got, (count, r_f, r_l, r_n, r_s) = check(data, n, lens, out_slot,
                                             pos=pos if form == "pos" else None, now0=5,
                                             now_step=7)
    g = got.frames[:n * out_slot].reshape(n, out_slot)
    for k in range(40):  # the head is frame bytes, the tail zero
        r = min(int(lens[k]), out_slot)
        assert g[k, :r].all() and not g[k, r:].any()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("out_cap", [0, 1, 64, B, 2 * B + 16, 2 * B + 17, 2 * B + 18])
def test_out_cap_below_at_and_above_the_entries(out_cap, form):
    n = 2 * B + 17
    data, lens, pos = case(7200, n, form)
    got, ref = check(data, n, lens, 64, out_cap=out_cap, pos=pos, now0=7, now_step=1)
    assert int(got.count[0]) == n  # the true count, whatever fitted


@pytest.mark.parametrize("form", FORMS)
def test_sel_permutation_and_repeats(form):
    rng = np.random.default_rng(7300)
    meta_n = B + 200
    sel = np.concatenate([rng.permutation(meta_n), np.repeat(np.arange(0, meta_n, 9), 3),
                          rng.integers(0, meta_n, 300)]).astype(np.uint32)
    data, lens, pos = case(7301, sel.size, form, sel=sel, meta_n=meta_n)
    now = rng.integers(1, 1 << 50, meta_n).astype(np.int64)
    got, (count, r_f, r_l, r_n, r_s) = check(data, sel.size, lens, 128, pos=pos, sel=sel, now=now)
    assert r_s.tolist() == sel.tolist() and r_l.tolist() == lens[sel].tolist()


@pytest.mark.parametrize("form", FORMS)
def test_sel_at_and_beyond_meta_n_reads_nothing(form):
    rng = np.random.default_rng(7310)
    meta_n = 500
    sel = rng.integers(0, meta_n, 1500).astype(np.uint32)
    sel[::11] = meta_n
    sel[5::37] = 0xFFFFFFFF
    sel[9::41] = meta_n + rng.integers(1, 1 << 30, sel[9::41].size)
    data, lens, pos = case(7311, sel.size, form, sel=sel, meta_n=meta_n)
    now = rng.integers(1, 1 << 50, meta_n).astype(np.int64)
    got, (count, r_f, r_l, r_n, r_s) = check(data, sel.size, lens, 64, pos=pos, sel=sel, now=now)
    outside = np.nonzero(r_s >= meta_n)[0]
    assert outside.size > 100 and 0xFFFFFFFF in r_s[outside].tolist()
    assert not r_l[outside].any() and not r_n[outside].any()
    assert not got.frames[:count * 64].reshape(count, 64)[outside].any()
    # with no len[] at all every entry is outside
    check(data, 200, np.zeros(0, np.uint16), 64, pos=pos[:200] if pos is not None else None,
          sel=sel[:200], now0=3, now_step=1)


def test_positions_rejected_per_entry():
    """Misaligned positions, positions whose padded frame ends one byte past
    `bytes` (and exactly at it), positions near 2^64."""
    rng = np.random.default_rng(7400)
    n = 300
    lens = draw_lens(rng, n)
    lens[lens == 0] = 33  # (every entry has bytes to refuse)
    lens[lens == 65535] = 700
    data, pos = lay(rng, n, lens, gaps=True)
    pos = pos.copy()
    for k, off in zip(range(3, n, 17), [1, 2, 4, 8, 15, 17, 3, 5, 7, 9, 11, 12, 13, 14, 6, 10, 31]):
        pos[k] += off
    top = 1 << 64
    pos[40:46] = [top - 16, top - 32, top - 48, top - 1, top - ext(lens[44]), top - 15]
    got, (count, r_f, r_l, r_n, r_s) = check(data, n, lens, 128, pos=pos, now0=9, now_step=2)
    refused = np.nonzero(r_l == 0)[0]
    assert set(range(40, 46)) <= set(refused.tolist()) and refused.size >= 6 + 17
    # the last frame ends at `bytes`, one byte less refuses it and nothing else
    last = int(np.argmax(pos[:40]))
    end = int(pos[last]) + ext(min(int(lens[last]), 128))
    a, ra = check(data, 40, lens, 128, pos=pos[:40], nbytes=end, now0=9, now_step=2)
    b, rb = check(data, 40, lens, 128, pos=pos[:40], nbytes=end - 1, now0=9, now_step=2)
    assert int(ra[2][last]) == int(lens[last]) and int(rb[2][last]) == 0
    assert [k for k in range(40) if ra[2][k] != rb[2][k]] == [last]


def test_stream_end_without_pos():
    """A self-describing stream that is cut short: every frame that ends
    beyond `bytes` is refused, an empty frame at the very end is not."""
    rng = np.random.default_rng(7410)
    n = B + 50
    lens = draw_lens(rng, n)
    lens[-3:] = [60, 17, 0]
    data, _ = lay(rng, n, lens)
    check(data, n, lens, 64, now0=1, now_step=1)
    got, ref = check(data, n, lens, 64, nbytes=data.size - 1, now0=1, now_step=1)
    assert ref[2][-3:].tolist() == [60, 0, 0]
    got, ref = check(data, n, lens, 64, nbytes=data.size // 2, now0=1, now_step=1)
    assert 0 < np.count_nonzero(ref[2]) < np.count_nonzero(lens)
    check(data[:0], n, lens, 64, nbytes=0, now0=1, now_step=1)  # (a NULL stream)


@pytest.mark.parametrize("form", FORMS)
def test_time_array_and_affine_time_beyond_32_bits(form):
    rng = np.random.default_rng(7500)
    meta_n = B + 300
    sel = np.sort(rng.choice(meta_n, B + 100, replace=False)).astype(np.uint32)
    data, lens, pos = case(7501, sel.size, form, sel=sel, meta_n=meta_n)
    now = rng.integers(-(1 << 62), 1 << 62, meta_n).astype(np.int64)
    now[:3] = [0, -1, (1 << 63) - 1]
    check(data, sel.size, lens, 64, pos=pos, sel=sel, now=now)
    step = (1 << 62) // meta_n  # m * step passes 2^32 and 2^61 inside the batch
    got, (count, r_f, r_l, r_n, r_s) = check(data, sel.size, lens, 64, pos=pos, sel=sel,
                                             now0=step + 12345, now_step=step)
    assert int(r_n.max()) > (1 << 61) and (np.diff(r_n) > 0).all()
    check(data, sel.size, lens, 64, pos=pos, sel=sel, now0=(1 << 63) - 5, now_step=step)
    check(data, sel.size, lens, 64, pos=pos, sel=sel, now0=-(1 << 40), now_step=0)


@pytest.mark.parametrize("with_now,with_src", [(False, True), (True, False), (False, False)])
def test_now_and_src_may_be_null(with_now, with_src):
    n = B + 100
    data, lens, pos = case(7600, n, "pos")
    a, _ = check(data, n, lens, 64, pos=pos, now0=5, now_step=2)
    b, _ = check(data, n, lens, 64, pos=pos, now0=5, now_step=2, with_now=with_now,
                 with_src=with_src)
    assert a.frames.tobytes() == b.frames.tobytes() and a.len.tobytes() == b.len.tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_callers_stream_gives_the_contexts_bytes(form):
    n = 2 * B + 17
    data, lens, pos = case(7700, n, form)
    a, _ = check(data, n, lens, 128, pos=pos, now0=9, now_step=4)
    b, _ = check(data, n, lens, 128, pos=pos, now0=9, now_step=4, stream=torch.cuda.Stream())
    c, _ = check(data, n, lens, 128, pos=pos, now0=9, now_step=4)
    assert a.same(b) and a.same(c)


def test_two_calls_without_pos_back_to_back_on_two_streams():
    """The context's one workspace of sums is ordered between streams by the
    library: two calls without pos on different streams, nothing waited for in
    between, each give their own stream's bytes."""
    nf = bridge()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for seed, n in ((7800, 8 * B + 5), (7801, 8 * B - 9), (7802, 3 * B)):
        rng = np.random.default_rng(seed)
        lens = draw_lens(rng, n)
        lens[lens > 127] = 99
        data, _ = lay(rng, n, lens)
        jobs.append((data, lens, n, dev(data, np.uint8), dev(lens, np.uint16)))
    runs = [Unpacked(nf, d_t, n, l_t, 64, n, now0=1, now_step=1, stream=s, wait=False)
            for (data, lens, n, d_t, l_t), s in zip(jobs, (s1, s2, s1))]
    torch.cuda.synchronize()
    for got in runs:
        got.run()
    for (data, lens, n, d_t, l_t), got in zip(jobs, runs):
        got.fetch()
        compare(got, unpack_reference(data, data.size, n, lens, 64, n, now0=1, now_step=1))


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


def packed(nf, nd, f_t, slot, l_t, o_t, i_t, n):
    """tx_build and tx_pack with pos over a batch: (idx_t, off_t, offset on
    the host, data_t, port_off on the host, pos_t)."""
    cap = n * max(1, nd - 1)
    idx_t = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
    off_t = torch.zeros(nd + 1, dtype=torch.int32, device="cuda:0")
    nf.tx_build(o_t, i_t, l_t, idx_t, off_t, None)
    data_t = torch.full((cap * slot,), CANARY, dtype=torch.uint8, device="cuda:0")
    po_t = torch.zeros(nd + 1, dtype=torch.int64, device="cuda:0")
    pos_t = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    nf.tx_pack(f_t, slot, l_t, idx_t, off_t, data_t, po_t, pos=pos_t)
    torch.cuda.synchronize()
    return (idx_t, off_t, off_t.cpu().numpy().view(np.uint32), data_t,
            po_t.cpu().numpy().view(np.uint64), pos_t)


def rebatched_and_cut(nf, f_t, slot, l_t, idx_t, off_t, port, cnt, out_slot, now0, now_step):
    """tx_rebatch of a port's list, every slot zeroed past min(len, slot): what
    a stream, which drops the bytes past a frame's length, can deliver."""
    fr = torch.zeros(cnt * out_slot, dtype=torch.uint8, device="cuda:0")
    ln = torch.zeros(cnt, dtype=torch.int16, device="cuda:0")
    nw = torch.zeros(cnt, dtype=torch.int64, device="cuda:0")
    sr = torch.zeros(cnt, dtype=torch.int32, device="cuda:0")
    c = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    nf.tx_rebatch(f_t, slot, l_t, idx_t, off_t, port, fr, out_slot, ln, c, out_now=nw,
                  out_src=sr, now0=now0, now_step=now_step)
    torch.cuda.synchronize()
    g = fr.cpu().numpy().reshape(cnt, out_slot).copy()
    lens = ln.cpu().numpy().view(np.uint16)
    keep = np.minimum(lens.astype(np.int64), min(slot, out_slot))
    g[np.arange(out_slot)[None, :] >= keep[:, None]] = 0
    return g.reshape(-1), lens, nw.cpu().numpy(), sr.cpu().numpy().view(np.uint32)


def round_trip_1(nf, nd, frames, slot, lens, out, ins, out_slot):
    n = lens.size
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    o_t, i_t = dev(out, np.uint16), dev(ins, np.uint16)
    idx_t, off_t, offset, data_t, port_off, pos_t = packed(nf, nd, f_t, slot, l_t, o_t, i_t, n)
    total = int(port_off[nd])
    seen = 0
    for port in range(nd):
        lo, hi = int(offset[port]), int(offset[port + 1])
        cnt = hi - lo
        if cnt == 0:
            continue
        seen += 1
        got = Unpacked(nf, data_t[:total], cnt, l_t, out_slot, cnt, pos_t[lo:hi], idx_t[lo:hi],
                       now0=1_000_000, now_step=3)
        w_f, w_l, w_n, w_s = rebatched_and_cut(nf, f_t, slot, l_t, idx_t, off_t, port, cnt,
                                               out_slot, 1_000_000, 3)
        compare(got, (cnt, w_f, w_l, w_n, w_s))
    assert f_t.cpu().numpy().tobytes() == np.asarray(frames, np.uint8).tobytes()
    return seen


@pytest.mark.parametrize("slots", [(64, 64), (128, 64), (64, 128), (256, 1536)])
def test_round_trip_pack_then_unpack_two_ports(slots):
    """tx_build -> tx_pack with pos -> rx_unpack with sel = idx, per port
    against tx_rebatch of the same list cut at each frame's length. Lengths
    stay inside the source slot, as an NF's do."""
    slot, out_slot = slots
    rng = np.random.default_rng(7900 + slot + out_slot)
    n, nd = 2 * B + 300, 2
    out, ins = mix(rng, n, nd)
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    frames = rng.integers(1, 255, n * slot).astype(np.uint8)
    assert round_trip_1(bridge(2), nd, frames, slot, lens, out, ins, out_slot) == 2


@pytest.mark.parametrize("slots", [(64, 64), (128, 64), (64, 128)])
def test_round_trip_flood_pattern_four_ports(slots):
    """vigbridge's flood pattern on four ports: every frame stands in the
    lists of the three ports it did not arrive on."""
    slot, out_slot = slots
    rng = np.random.default_rng(7950 + slot + out_slot)
    n, nd = B + 200, 4
    ins = rng.integers(0, nd, n).astype(np.uint16)
    out = np.full(n, F, np.uint16)
    lens = np.full(n, 60, np.uint16)
    lens[::7] = rng.integers(0, 65, lens[::7].size)
    frames = rng.integers(1, 255, n * slot).astype(np.uint8)
    assert round_trip_1(bridge(4), nd, frames, slot, lens, out, ins, out_slot) == 4


@pytest.mark.parametrize("slot", [64, 256])
def test_round_trip_without_pos_from_port_off(slot):
    """A list whose lengths all fit the source slot, unpacked without pos from
    data + port_off[d] with the lengths gathered by sel: the same bytes as
    with pos."""
    rng = np.random.default_rng(7980 + slot)
    n, nd = 2 * B + 300, 2
    nf = bridge(2)
    out, ins = mix(rng, n, nd)
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    frames = rng.integers(1, 255, n * slot).astype(np.uint8)
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    idx_t, off_t, offset, data_t, port_off, pos_t = packed(
        nf, nd, f_t, slot, l_t, dev(out, np.uint16), dev(ins, np.uint16), n)
    total = int(port_off[nd])
    for port in range(nd):
        lo, hi = int(offset[port]), int(offset[port + 1])
        a, b = int(port_off[port]), int(port_off[port + 1])
        assert hi > lo and a % 16 == 0
        with_pos = Unpacked(nf, data_t[:total], hi - lo, l_t, slot, hi - lo, pos_t[lo:hi],
                            idx_t[lo:hi], now0=77, now_step=5)
        without = Unpacked(nf, data_t[a:b], hi - lo, l_t, slot, hi - lo, None, idx_t[lo:hi],
                           now0=77, now_step=5)
        assert with_pos.same(without)
        assert with_pos.len[:hi - lo].tolist() == \
            lens[idx_t[lo:hi].cpu().numpy().view(np.uint32)].tolist()


def test_einval_cases_write_nothing():
    nf = bridge()
    L = nf.L
    d = torch.device("cuda:0")
    n, slot, cap = 64, 64, 64
    data = torch.full((2 * n * slot + 16,), 7, dtype=torch.uint8, device=d)
    lens = torch.full((n,), 60, dtype=torch.int16, device=d)
    pos = (torch.arange(n, dtype=torch.int64, device=d) * 64)
    outs = [filled(cap * slot, 1), filled(cap, 2), filled(cap, 8), filled(cap, 4), filled(1, 4)]
    o_f, o_l, o_n, o_s, o_c = outs
    torch.cuda.synchronize()

    def rx(**kw):
        a = dict(data=data.data_ptr(), bytes=n * slot, n=n, pos=pos.data_ptr(), sel=None,
                 meta_n=n, len=lens.data_ptr(), now=None, now0=0, now_step=0)
        a.update(kw)
        return vigor_amd.RxStreamC(**a)

    def nxt(**kw):
        a = dict(frames=o_f.data_ptr(), slot=slot, cap=cap, len=o_l.data_ptr(),
                 now=o_n.data_ptr(), src=o_s.data_ptr(), count=o_c.data_ptr())
        a.update(kw)
        return vigor_amd.TxNextC(**a)

    def rc(h, a, o):
        ref = [C.byref(x) if x is not None else None for x in (a, o)]
        return L.vp_rx_unpack(h, ref[0], ref[1], None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == CANARY).all()) for t in outs) \
            and bool((data == 7).all())

    E = vigor_amd.VP_EINVAL
    assert rc(None, rx(), nxt()) == E
    assert rc(nf.h, None, nxt()) == E
    assert rc(nf.h, rx(), None) == E
    assert rc(nf.h, rx(), nxt(count=None)) == E
    assert rc(nf.h, rx(data=None), nxt()) == E
    assert rc(nf.h, rx(data=data.data_ptr() + 8), nxt()) == E
    assert rc(nf.h, rx(), nxt(frames=o_f.data_ptr() + 8)) == E
    assert rc(nf.h, rx(len=None), nxt()) == E
    for bad_slot in (0, 48, 72, 1000):
        assert rc(nf.h, rx(), nxt(slot=bad_slot)) == E
    assert rc(nf.h, rx(), nxt(frames=None)) == E
    assert rc(nf.h, rx(), nxt(len=None)) == E
    # overlapping byte ranges: the output inside the stream, the stream's last
    # bytes under the output's first, and the other way round
    base = data.data_ptr()
    assert rc(nf.h, rx(), nxt(frames=base)) == E
    assert rc(nf.h, rx(), nxt(frames=base + n * slot - 16)) == E
    assert rc(nf.h, rx(data=base + (cap - 1) * slot), nxt(frames=base)) == E
    assert rc(nf.h, rx(bytes=2 * n * slot), nxt(frames=base + n * slot)) == E
    assert untouched()
    # the same arguments are accepted where the contract allows a NULL; the
    # count is written even where nothing else is
    assert rc(nf.h, rx(), nxt(frames=None, len=None, cap=0)) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == n and bool((o_c[1:] == o_c[1]).all())
    o_c.view(torch.uint8).fill_(CANARY)
    assert rc(nf.h, rx(n=0), nxt()) == 0
    assert rc(nf.h, rx(n=0, pos=None), nxt()) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == 0
    o_c.view(torch.uint8).fill_(CANARY)
    assert untouched()
    # a NULL stream of no bytes and no len[]: every entry is refused
    assert rc(nf.h, rx(data=None, bytes=0, len=None, meta_n=0, pos=None), nxt()) == 0
    torch.cuda.synchronize()
    assert int(o_c[0]) == n and not bool(o_f[:cap * slot].any()) and not bool(o_l[:cap].any())
    # adjacent, not overlapping: the output right behind the stream
    assert rc(nf.h, rx(), nxt(frames=base + n * slot)) == 0
    torch.cuda.synchronize()
    assert bool((data[:n * slot] == 7).all())
    got = data[n * slot:2 * n * slot].view(n, slot)
    assert bool((got[:, :60] == 7).all()) and not bool(got[:, 60:].any())
    with pytest.raises(vigor_amd.VigpathError):
        nf.rx_unpack(data[8:n * slot + 8], lens, o_f[:cap * slot], slot, o_l[:cap], o_c, pos=pos)
