"""vp_tx_pack on the GPU: the per-port byte streams, their bounds and the
entries' positions, byte for byte against txpackref.pack_reference (the
contract of include/vigpath.h as a per-entry loop).

Every case fills data, pos and port_off with a canary first, compares all
three buffers whole (the untouched tails included) and checks that the source
frames are unchanged. Hand-made lists go through the smallest vigbridge
context with the wanted n_devices (the call reads only the batch and the
lists); the flood and end-to-end cases take their lists from vp_tx_build."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import vigor_amd
from tracegen import mixed_bridge_trace, mixed_nat_trace
from txpackref import pack_reference
from txref import tx_reference
from vigor_amd import traces as TR

pytestmark = pytest.mark.gpu

B = 2048  # entries per block of vp_tx_pack's kernels (vp_txpack.hip)
F = 0xFFFF
CANARY = 0xA5
CANARY64 = int.from_bytes(bytes([CANARY]) * 8, "little")
TAIL = 256  # canary bytes / words kept behind every buffer

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
    padding and untouched bytes cannot pass for frame bytes."""
    f = rng.integers(1, 255, n * slot).astype(np.uint8)
    f[f == CANARY] = 0x11
    return f


class Packed:
    """One vp_tx_pack call over canary-filled buffers, back on the host."""

    def __init__(self, nf, nd, f_t, slot, l_t, idx_t, off_t, cap, cap_bytes, with_pos=True,
                 stream=None, before=None):
        d = torch.device("cuda:0")
        self.nd, self.cap, self.cap_bytes = nd, cap, cap_bytes
        data = torch.full((cap_bytes + TAIL,), CANARY, dtype=torch.uint8, device=d)
        po = torch.full((8 * (nd + 1 + TAIL),), CANARY, dtype=torch.uint8,
                        device=d).view(torch.int64)
        pos = torch.full((8 * (cap + TAIL),), CANARY, dtype=torch.uint8, device=d).view(torch.int64)
        torch.cuda.synchronize()
        if before is not None:
            before()  # (work that fills the lists, enqueued on the same stream)
        nf.tx_pack(f_t, slot, l_t, idx_t[:cap] if cap else None, off_t,
                   data[:cap_bytes] if cap_bytes else None, po[:nd + 1],
                   pos[:cap] if with_pos and cap else None, stream=stream)
        torch.cuda.synchronize()
        self.data = data.cpu().numpy()
        self.port_off = po.cpu().numpy().view(np.uint64)
        self.pos = pos.cpu().numpy().view(np.uint64)

    def same(self, other):
        return (self.data.tobytes() == other.data.tobytes()
                and self.port_off.tobytes() == other.port_off.tobytes()
                and self.pos.tobytes() == other.pos.tobytes())


def compare(got, frames, slot, lens, idx, offset, with_pos=True):
    """All three buffers of `got` against the reference; returns (data,
    port_off, pos) of the reference."""
    nd, cap, cap_bytes = got.nd, got.cap, got.cap_bytes
    data, port_off, pos = pack_reference(frames, slot, lens, idx, offset, cap, nd, cap_bytes,
                                         canary=CANARY)
    assert got.port_off[:nd + 1].tolist() == port_off.tolist()
    assert (got.port_off[nd + 1:] == CANARY64).all(), "written past port_off's end"
    k = pos.size if with_pos else 0
    bad = np.nonzero(got.pos[:k] != pos[:k])[0]
    assert bad.size == 0, "pos differs at %s: %s vs %s" % (bad[:8], got.pos[bad[:8]], pos[bad[:8]])
    assert (got.pos[k:] == CANARY64).all(), "pos written at or beyond entry %d" % k
    bad = np.nonzero(got.data[:data.size] != data)[0]
    assert bad.size == 0, "data differs at bytes %s: %s vs %s" % (
        bad[:8], got.data[bad[:8]], data[bad[:8]])
    assert (got.data[data.size:] == CANARY).all(), "data written at or beyond byte %d" % data.size
    return data, port_off, pos


def check(nd, frames, slot, lens, idx, offset, cap=None, cap_bytes=None, with_pos=True,
          stream=None, nf=None):
    """Hand-made lists (numpy) through one call. cap None: the lists' total;
    cap_bytes None: exactly the streams' total. Returns (got, reference)."""
    nf = nf or bridge(nd)
    idx = np.asarray(idx, np.uint32)
    offset = np.asarray(offset, np.uint32)
    cap = int(offset[nd]) if cap is None else cap
    if cap_bytes is None:
        cap_bytes = int(pack_reference(frames, slot, lens, idx, offset, cap, nd, 0)[1][nd])
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    idx_t = dev(idx if idx.size else np.zeros(1, np.uint32), np.uint32)
    off_t = dev(offset, np.uint32)
    got = Packed(nf, nd, f_t, slot, l_t, idx_t, off_t, cap, cap_bytes, with_pos, stream)
    ref = compare(got, frames, slot, lens, idx, offset, with_pos)
    assert f_t.cpu().numpy().tobytes() == np.asarray(frames, np.uint8).tobytes(), "frames written"
    return got, ref


def two_port_lists(rng, count):
    """The first `count` packets on two ports, each list in packet order."""
    port = rng.integers(0, 2, count)
    who = np.arange(count, dtype=np.uint32)
    idx = np.concatenate([who[port == 0], who[port == 1]])
    return idx, [0, int((port == 0).sum()), count]


EDGE_LENS = [0, 1, 15, 16, 17, 48, 49, 63, 64]


@pytest.mark.parametrize("count", [0, 1, 15, 16, 17, 63, 64, 65, B - 1, B, B + 1, 2 * B,
                                   3 * B + 17])
def test_entry_counts_around_block_and_wave_edges(count):
    rng = np.random.default_rng(3000 + count)
    n = max(count, len(EDGE_LENS))
    lens = rng.integers(0, 65, n).astype(np.uint16)
    lens[rng.permutation(n)[:len(EDGE_LENS)]] = EDGE_LENS
    frames = frames_for(rng, n, 64)
    idx, offset = two_port_lists(rng, count)
    if count >= len(EDGE_LENS):  # (every packet is in a list)
        assert set(EDGE_LENS) <= set(lens[idx].tolist())
    check(2, frames, 64, lens, idx, offset)


def wide_lens(rng, slot):
    """Every multiple of 16 up to the slot with its two neighbours, 1514, 1518,
    the slot, lengths beyond the slot (cut to it), and random ones."""
    m = np.arange(0, slot + 1, 16)
    want = np.concatenate([m, m[1:] - 1, m + 1, [1514, 1518, slot, slot + 1, 4 * slot, 65535],
                           rng.integers(0, slot + 1, 200)])
    return want.astype(np.uint16)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("slot", [128, 1536, 2048])
def test_wide_slots_both_copy_paths(slot, mixed):
    """Not mixed: the lean frames (at most 64 bytes padded) fill whole groups
    of 16 entries and the wide ones the groups after them, so every wave turn
    takes one path; mixed: both kinds inside the groups."""
    rng = np.random.default_rng(slot + mixed)
    lens = wide_lens(rng, slot)
    lean = lens[lens <= 64]
    more = (-lean.size) % 16 + 16 * 8  # whole groups of lean frames, and enough to mix
    lens = np.concatenate([lean, rng.integers(0, 65, more).astype(np.uint16), lens[lens > 64]])
    n_lean = lean.size + more
    assert n_lean % 16 == 0 and 300 <= lens.size <= 2100
    if mixed:
        lens = lens[rng.permutation(lens.size)]
        g = np.minimum(lens[:lens.size // 16 * 16], slot).reshape(-1, 16)
        both = ((g <= 64).any(1) & (g > 64).any(1)).sum()
        assert both >= 4, "no group of 16 holds lean and wide frames"
    n = lens.size
    frames = frames_for(rng, n, slot)
    # packet order is entry order here: the groups of 16 are the lists' own
    idx = np.arange(n, dtype=np.uint32)
    got, (data, port_off, pos) = check(2, frames, slot, lens, idx, [0, n // 3, n])
    assert int(port_off[2]) == int(((np.minimum(lens, slot).astype(np.int64) + 15) & ~15).sum())


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


def built_and_packed(nf, nd, frames, slot, lens, out, ins, stream=None, process=None):
    """tx_build then tx_pack on one stream, nothing waited for in between;
    returns (the result, idx, offset, the frames' tensor) with the lists read
    back. process: called first, to fill the out ports (end to end)."""
    d = torch.device("cuda:0")
    n = len(lens)
    full, r_off, _ = tx_reference(out, ins, lens, nd, 1 << 32)
    cap = full.size
    f_t, l_t = dev(frames, np.uint8), dev(lens, np.uint16)
    o_t, i_t = dev(out, np.uint16), dev(ins, np.uint16)
    idx_t = torch.full((cap + 1,), 0x5A5A5A5A, dtype=torch.int32, device=d)
    off_t = torch.zeros(nd + 1, dtype=torch.int32, device=d)
    if process is not None:
        o_t = torch.zeros(n, dtype=torch.int16, device=d)

    def before():
        if process is not None:
            process(f_t, l_t, i_t, o_t)
        nf.tx_build(o_t, i_t, l_t, idx_t[:cap], off_t, None, stream=stream)

    cap_bytes = int(((np.minimum(lens, slot).astype(np.int64)[full] + 15) & ~15).sum())
    got = Packed(nf, nd, f_t, slot, l_t, idx_t, off_t, cap, cap_bytes, stream=stream,
                 before=before)
    idx = idx_t.cpu().numpy().view(np.uint32)[:cap]
    offset = off_t.cpu().numpy().view(np.uint32)
    assert idx.tobytes() == full.tobytes() and offset.tobytes() == r_off.tobytes()
    return got, idx, offset, f_t


def test_floods_from_tx_build_on_the_same_stream():
    rng = np.random.default_rng(41)
    n, nd, slot = B + 300, 4, 64
    out, ins = mix(rng, n, nd)
    lens = rng.integers(0, 65, n).astype(np.uint16)
    lens[:8] = 60
    out[3], ins[3] = F, 1  # a flood that is owed to ports 0, 2 and 3
    frames = frames_for(rng, n, slot)
    got, idx, offset, f_t = built_and_packed(bridge(nd), nd, frames, slot, lens, out, ins)
    data, port_off, pos = compare(got, frames, slot, lens, idx, offset)
    assert f_t.cpu().numpy().tobytes() == frames.tobytes(), "frames written"
    where = np.nonzero(idx == 3)[0]
    assert where.size == 3
    streams = set()
    for e in where:
        p = int(pos[e])
        assert got.data[p:p + 60].tobytes() == frames[3 * slot:3 * slot + 60].tobytes()
        assert not got.data[p + 60:p + 64].any()
        streams.add(int(np.searchsorted(port_off, p, side="right")) - 1)
    assert streams == {0, 2, 3}


def test_port_edges_32_ports_mostly_empty():
    rng = np.random.default_rng(42)
    n, nd, slot = 300, 32, 64
    lens = rng.integers(1, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    # ports 0..3 empty, 4 and 9 and 30 hold entries, 31 and the rest empty
    offset = np.zeros(nd + 1, np.uint32)
    offset[5:] = 40
    offset[10:] = 170
    offset[31:] = n
    idx = np.concatenate([np.sort(rng.permutation(n)[:40]), np.sort(rng.permutation(n)[:130]),
                          np.sort(rng.permutation(n)[:130])]).astype(np.uint32)
    got, (data, port_off, pos) = check(nd, frames, slot, lens, idx, offset)
    assert port_off[0] == port_off[4] == 0 and port_off[31] == port_off[32] == data.size
    assert len(set(port_off.tolist())) == 4


def test_port_boundaries_on_block_edges():
    """Several bounds on entry B (the first of the second block) and the total
    on entry 2 B: the block that owns entry E holds no entry of its own."""
    rng = np.random.default_rng(43)
    n, nd, slot = 2 * B, 4, 64
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    check(nd, frames, slot, lens, np.arange(n, dtype=np.uint32), [0, B, B, B, 2 * B])


def test_hand_made_lists_descending_repeating_and_outside_the_batch():
    rng = np.random.default_rng(44)
    n, slot = 500, 128
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = np.concatenate([np.arange(n - 1, -1, -1), np.repeat(np.arange(0, n, 7), 3),
                          rng.integers(0, n, 300)]).astype(np.uint32)
    idx[::11] = n
    idx[5::37] = 0xFFFFFFFF
    idx[9::41] = n + rng.integers(1, 1 << 30, idx[9::41].size)
    got, (data, port_off, pos) = check(2, frames, slot, lens, idx, [0, 600, idx.size])
    outside = np.nonzero(idx >= n)[0]
    assert outside.size > 50 and (pos[outside[:-1] + 1] == pos[outside[:-1]]).all()


@pytest.mark.parametrize("offset", [[0, 700, 1500], [0, 1200, 1500], [0, 1000, 2 * B + 5]])
def test_overflowed_lists_pack_the_first_cap_entries(offset):
    rng = np.random.default_rng(45)
    n, slot, cap = 1200, 64, 1000
    lens = rng.integers(0, 65, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = rng.integers(0, n, cap).astype(np.uint32)
    got, (data, port_off, pos) = check(2, frames, slot, lens, idx, offset, cap=cap)
    assert pos.size == cap and int(port_off[2]) == data.size
    if offset[1] >= cap:
        assert port_off[1] == port_off[2]


def capacity_case():
    rng = np.random.default_rng(46)
    n, slot = 600, 128
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    lens[:40] = rng.integers(1, 65, 40)
    lens[250] = 100
    frames = frames_for(rng, n, slot)
    idx = np.arange(n, dtype=np.uint32)
    offset = [0, 400, n]
    _, port_off, pos = pack_reference(frames, slot, lens, idx, offset, n, 2, 0)
    return frames, slot, lens, idx, offset, port_off, pos


@pytest.mark.parametrize("which", ["zero", "total", "total-1", "mid-frame"])
def test_cap_bytes(which):
    frames, slot, lens, idx, offset, port_off, pos = capacity_case()
    total = int(port_off[2])
    e = 250  # in the middle of port 0's 400 entries
    assert lens[e] > 16 and offset[0] < e < offset[1]
    cap_bytes = {"zero": 0, "total": total, "total-1": total - 1,
                 "mid-frame": int(pos[e]) + 8}[which]
    got, (data, r_off, r_pos) = check(2, frames, slot, lens, idx, offset, cap_bytes=cap_bytes)
    assert r_off.tolist() == port_off.tolist() and r_pos.tolist() == pos.tolist()
    if which == "total-1":  # the last frame that occupies bytes stays out, whole
        last = int(np.nonzero(lens)[0][-1])
        assert (got.data[int(pos[last]):total] == CANARY).all()
    if which == "mid-frame":
        assert (got.data[int(pos[e]):cap_bytes] == CANARY).all()
        assert got.data[int(pos[e]) - 1] != CANARY


def test_pos_null_gives_the_same_data_and_bounds():
    frames, slot, lens, idx, offset, _, _ = capacity_case()
    a, _ = check(2, frames, slot, lens, idx, offset)
    b, _ = check(2, frames, slot, lens, idx, offset, with_pos=False)
    assert a.data.tobytes() == b.data.tobytes() and a.port_off.tobytes() == b.port_off.tobytes()
    assert (b.pos == CANARY64).all()


def sized_case(rng, count):
    lens = rng.integers(0, 65, count).astype(np.uint16)
    return frames_for(rng, count, 64), 64, lens, np.arange(count, dtype=np.uint32), \
        [0, count // 2, count]


def test_streams_and_workspace_growth_and_reuse():
    rng = np.random.default_rng(47)
    nf = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], 2), gpu=0)  # a fresh workspace
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    small, large = sized_case(rng, 100), sized_case(rng, 3 * B + 17)
    check(2, *small, stream=s1, nf=nf)
    check(2, *large, stream=s1, nf=nf)  # the workspace grows
    check(2, *small, stream=s1, nf=nf)  # and is used again
    check(2, *large, stream=s2, nf=nf)  # another stream after the first
    check(2, *small, nf=nf)             # and the context's own
    # two calls back to back on two streams, nothing waited for in between
    d = torch.device("cuda:0")
    f_t, l_t = dev(large[0], np.uint8), dev(large[2], np.uint16)
    idx_t, off_t = dev(large[3], np.uint32), dev(large[4], np.uint32)
    cap = large[3].size
    bufs = []
    for _ in range(2):
        bufs.append((torch.full((cap * 64,), CANARY, dtype=torch.uint8, device=d),
                     torch.zeros(3, dtype=torch.int64, device=d),
                     torch.zeros(cap, dtype=torch.int64, device=d)))
    torch.cuda.synchronize()
    for s, (data, po, pos) in zip((s1, s2), bufs):
        nf.tx_pack(f_t, 64, l_t, idx_t, off_t, data, po, pos, stream=s)
    torch.cuda.synchronize()
    want, w_off, w_pos = pack_reference(*large[:4], large[4], cap, 2, cap * 64)
    for data, po, pos in bufs:
        assert data.cpu().numpy()[:want.size].tobytes() == want.tobytes()
        assert po.cpu().numpy().view(np.uint64).tolist() == w_off.tolist()
        assert pos.cpu().numpy().view(np.uint64).tolist() == w_pos.tolist()
    nf.close()


def test_same_bytes_twice():
    rng = np.random.default_rng(48)
    n, slot = 3 * B + 17, 128
    lens = rng.integers(0, slot + 1, n).astype(np.uint16)
    frames = frames_for(rng, n, slot)
    idx = rng.integers(0, n, n).astype(np.uint32)
    a, _ = check(2, frames, slot, lens, idx, [0, n // 2, n])
    b, _ = check(2, frames, slot, lens, idx, [0, n // 2, n])
    assert a.same(b)


DEV_MACS = [TR.mac("02:03:04:05:06:07"), TR.mac("12:13:14:15:16:17")]
END_MACS = [TR.mac("01:23:45:67:89:00"), TR.mac("01:23:45:67:89:01")]


def end_to_end(nf, oracle, nd, fr, ln, dv, now):
    """process_device, tx_build, tx_pack on the context's stream; the streams
    against the reference applied to the oracle's frames and out ports."""
    exp = fr.copy()
    exp_out = oracle.run(exp, ln, dv, now, 64)
    n_t = torch.from_numpy(now.astype(np.int64)).to("cuda:0")

    def process(f_t, l_t, i_t, o_t):
        nf.process_device(f_t, l_t, i_t, o_t, 64, now=n_t)

    got, idx, offset, f_t = built_and_packed(nf, nd, fr.reshape(-1), 64, ln, exp_out, dv,
                                             process=process)
    assert f_t.cpu().numpy().tobytes() == exp.tobytes(), "frames differ from the oracle's"
    data, port_off, pos = compare(got, exp.reshape(-1), 64, ln, idx, offset)
    return data, pack_reference(fr.reshape(-1), 64, ln, idx, offset, idx.size, nd, data.size)[0]


def test_end_to_end_nat_rewritten_frames():
    rng = np.random.default_rng(22)
    fr, ln, dv, now = mixed_nat_trace(rng, 5000, 40)
    args = ["--wan", "1", "--expire", "60000000", "--starting-port", "0",
            "--max-flows", "64", "--extip", "192.168.4.2",
            "--eth-dest", "0,01:23:45:67:89:00", "--eth-dest", "1,01:23:45:67:89:01"]
    nat = vigor_amd.Nat(vigor_amd.nat_config_from_args(args, 2, DEV_MACS), gpu=0)
    o = orc.Oracle("nat", orc.nat_cfg(wan=1, start_port=0, ext_ip=TR.ip4(192, 168, 4, 2),
                                      expire_us=60000000, max_flows=64, device_macs=DEV_MACS,
                                      endpoint_macs=END_MACS, n_devices=2))
    data, of_inputs = end_to_end(nat, o, 2, fr, ln, dv, now)
    assert data.size > 0 and data.tobytes() != of_inputs.tobytes()  # the rewritten bytes
    nat.close()


def test_end_to_end_bridge_floods():
    rng = np.random.default_rng(21)
    fr, ln, dv, now = mixed_bridge_trace(rng, 4000, 200)
    br = vigor_amd.Bridge(vigor_amd.bridge_config_from_args(["--capacity", "1024"], 3), gpu=0)
    o = orc.Oracle("bridge", orc.BridgeCfg(expiration_time=300_000_000, dyn_capacity=1024,
                                           n_devices=3), statics=[])
    data, _ = end_to_end(br, o, 3, fr, ln, dv, now)
    assert data.size > 0
    br.close()


def test_einval_cases_write_nothing():
    """Every VP_EINVAL of the contract but the device count: no context with
    more than VP_MAX_DEVICES devices can be created."""
    nf = bridge(2)
    L = nf.L
    d = torch.device("cuda:0")
    n, slot, cap = 64, 64, 64
    frames = torch.full((n * slot + 16,), 7, dtype=torch.uint8, device=d)
    lens = torch.full((n,), 60, dtype=torch.int16, device=d)
    idx = torch.arange(cap, dtype=torch.int32, device=d)
    off = torch.tensor([0, 30, cap], dtype=torch.int32, device=d)
    data = torch.full((cap * slot + 16,), CANARY, dtype=torch.uint8, device=d)
    po = torch.full((3,), CANARY64 - (1 << 64), dtype=torch.int64, device=d)
    pos = torch.full((cap,), CANARY64 - (1 << 64), dtype=torch.int64, device=d)
    torch.cuda.synchronize()

    def batch(**kw):
        b = dict(frames=frames.data_ptr(), slot=slot, n=n, len=lens.data_ptr())
        b.update(kw)
        return vigor_amd.DevBatchC(**b)

    def lists(**kw):
        a = dict(idx=idx.data_ptr(), cap=cap, offset=off.data_ptr(), stats=None)
        a.update(kw)
        return vigor_amd.TxListsC(**a)

    def frames_out(**kw):
        a = dict(data=data.data_ptr(), cap_bytes=cap * slot, port_off=po.data_ptr(),
                 pos=pos.data_ptr())
        a.update(kw)
        return vigor_amd.TxFramesC(**a)

    def rc(h, b, a, o):
        ref = [C.byref(x) if x is not None else None for x in (b, a, o)]
        return L.vp_tx_pack(h, ref[0], ref[1], ref[2], None)

    E = vigor_amd.VP_EINVAL
    assert rc(None, batch(), lists(), frames_out()) == E
    assert rc(nf.h, None, lists(), frames_out()) == E
    assert rc(nf.h, batch(), None, frames_out()) == E
    assert rc(nf.h, batch(), lists(), None) == E
    assert rc(nf.h, batch(), lists(), frames_out(port_off=None)) == E
    assert rc(nf.h, batch(), lists(offset=None), frames_out()) == E
    assert rc(nf.h, batch(), lists(idx=None), frames_out()) == E
    assert rc(nf.h, batch(frames=None), lists(), frames_out()) == E
    assert rc(nf.h, batch(len=None), lists(), frames_out()) == E
    for bad_slot in (0, 48, 72, 1000):
        assert rc(nf.h, batch(slot=bad_slot), lists(), frames_out()) == E
    assert rc(nf.h, batch(frames=frames.data_ptr() + 8), lists(), frames_out()) == E
    assert rc(nf.h, batch(), lists(), frames_out(data=data.data_ptr() + 8)) == E
    assert rc(nf.h, batch(), lists(), frames_out(data=None)) == E
    torch.cuda.synchronize()
    assert (data == CANARY).all() and (po == po[0]).all() and (pos == po[0]).all()
    assert int(po[0]) == CANARY64 - (1 << 64) and (frames == 7).all()
    # the same arguments are accepted where the contract allows a NULL
    assert rc(nf.h, batch(frames=None, len=None), lists(idx=None, cap=0), frames_out()) == 0
    assert rc(nf.h, batch(), lists(), frames_out(data=None, cap_bytes=0)) == 0
    torch.cuda.synchronize()
    assert (data == CANARY).all()
    assert po.cpu().numpy().view(np.uint64).tolist() == [0, 30 * 64, cap * 64]
    with pytest.raises(vigor_amd.VigpathError):
        nf.tx_pack(frames[8:n * slot + 8], slot, lens, idx, off, data, po, pos)
