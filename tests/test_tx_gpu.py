"""vp_tx_build on the GPU: the per-port transmit lists, offsets and stats of a
device-resident batch, byte for byte against txref.tx_reference (nf.c's
transmit decision as a per-packet loop).

Synthetic out_dev / in_dev / len tensors through the smallest vigbridge
context with the wanted n_devices (the call reads no frames), then two traces
end to end: process_device, tx_build, and the lists compared with the
reference applied to the oracle's out ports."""
import ctypes as C

import numpy as np
import pytest
import torch

import orc
import vigor_amd
from tracegen import mixed_bridge_trace, mixed_nat_trace
from txref import STATS_WORDS, tx_reference
from vigor_amd import traces as TR

pytestmark = pytest.mark.gpu

T = vigor_amd.TX_BLOCK_PACKETS
F = 0xFFFF
MARK = 0x5A5A5A5A  # no packet index of these tests
TAIL = 64
# tx_scan scans n_devices x blocks counts in tiles of 8192 with a carry: 32
# ports and 257 blocks put the last port's last block in the second tile
SCAN_TILE = 8192

_ctx = {}


def bridge(nd):
    if nd not in _ctx:
        _ctx[nd] = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)
    return _ctx[nd]


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to("cuda:0")


def run(nf, nd, out, ins, lens, cap, stats=True, stream=None, null_idx=False):
    """One vp_tx_build call; returns (idx buffer of cap + TAIL, offset, stats
    words or None) as numpy after a synchronize."""
    d = torch.device("cuda:0")
    o_t, l_t = dev16(out), dev16(lens)
    i_t = ins if isinstance(ins, int) else dev16(ins)
    buf = torch.full((cap + TAIL,), MARK, dtype=torch.int32, device=d)
    off = torch.full((nd + 1,), MARK, dtype=torch.int32, device=d)
    st = torch.full((8 * STATS_WORDS,), 0xFF, dtype=torch.uint8, device=d) if stats else None
    nf.tx_build(o_t, i_t, l_t, None if null_idx else buf[:cap], off, st, stream=stream)
    torch.cuda.synchronize()
    return (buf.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32),
            st.cpu().numpy().view(np.uint64) if stats else None)


def check(nd, out, ins, lens, cap=None, nf=None):
    """cap None: exactly the total. Returns the reference's total."""
    nf = nf or bridge(nd)
    full, r_off, r_st = tx_reference(out, ins, lens, nd, 1 << 32)
    total = int(r_off[nd])
    assert total == full.size
    cap = total if cap is None else cap
    buf, off, st = run(nf, nd, out, ins, lens, cap)
    k = min(total, cap)
    assert off.tobytes() == r_off.tobytes(), (off, r_off)
    assert st.tobytes() == r_st.tobytes(), (st, r_st)
    bad = np.nonzero(buf[:k] != full[:k])[0]
    assert bad.size == 0, "list entries differ at %s: %s vs %s" % (bad[:8], buf[bad[:8]],
                                                                  full[bad[:8]])
    assert (buf[k:] == MARK).all(), "written past min(total, cap) = %d" % k
    return total


def mix(rng, n, nd, p_drop=0.15, p_flood=0.1, p_bad=0.05, in_max=None):
    ins = rng.integers(0, in_max or nd, n).astype(np.uint16)
    out = rng.integers(0, nd, n).astype(np.uint16)
    r = rng.random(n)
    bad = r < p_bad
    out[bad] = rng.integers(nd, F, int(bad.sum()))
    out[(r >= p_bad) & (r < p_bad + p_flood)] = F
    drop = (r >= p_bad + p_flood) & (r < p_bad + p_flood + p_drop)
    out[drop] = ins[drop]
    lens = rng.integers(0, 65536, n).astype(np.uint16)
    return out, ins, lens


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17])
def test_sizes_random_mix_four_devices(n):
    rng = np.random.default_rng(1000 + n)
    out, ins, lens = mix(rng, n, 4)
    check(4, out, ins, lens)


def test_scan_tile_boundary_32_devices():
    n = (SCAN_TILE // 32) * T + 1  # 257 blocks x 32 ports: 8224 counts
    rng = np.random.default_rng(7)
    out, ins, lens = mix(rng, n, 32, p_flood=0.0005)
    check(32, out, ins, lens)


def test_all_dropped():
    rng = np.random.default_rng(2)
    ins = rng.integers(0, 4, T + 100).astype(np.uint16)
    assert check(4, ins.copy(), ins, np.full(T + 100, 64, np.uint16)) == 0


def test_all_to_one_port():
    n = 2 * T + 5
    out, ins = np.full(n, 2, np.uint16), np.zeros(n, np.uint16)
    assert check(4, out, ins, np.arange(n).astype(np.uint16)) == n


@pytest.mark.parametrize("nd", [1, 2, 3, 32])
def test_all_flood(nd):
    n = T + 65
    rng = np.random.default_rng(nd)
    ins = rng.integers(0, nd, n).astype(np.uint16)
    lens = rng.integers(0, 65536, n).astype(np.uint16)
    assert check(nd, np.full(n, F, np.uint16), ins, lens) == n * (nd - 1)


def test_input_ports_beyond_the_devices():
    n = T + 200
    rng = np.random.default_rng(5)
    out, ins, lens = mix(rng, n, 3, p_flood=0.3, in_max=8)
    ins[::17] = F  # (a flood from port 0xFFFF is out == in: dropped)
    check(3, out, ins, lens)


def test_scalar_in_port_equals_the_array():
    n = T + 77
    rng = np.random.default_rng(6)
    out, _, lens = mix(rng, n, 4)
    nf = bridge(4)
    want = tx_reference(out, 1, lens, 4, 1 << 32)
    total = want[0].size
    a = run(nf, 4, out, 1, lens, total)
    b = run(nf, 4, out, np.full(n, 1, np.uint16), lens, total)
    for got in (a, b):
        assert got[0][:total].tobytes() == want[0].tobytes()
        assert got[1].tobytes() == want[1].tobytes()
        assert got[2].tobytes() == want[2].tobytes()


@pytest.mark.parametrize("short", [0, 1])
def test_capacity_total_and_one_less(short):
    n = 2 * T + 300
    rng = np.random.default_rng(8)
    out, ins, lens = mix(rng, n, 4)
    total = tx_reference(out, ins, lens, 4, 0)[1][4]
    check(4, out, ins, lens, cap=int(total) - short)


def test_capacity_zero_null_idx():
    n = T + 9
    rng = np.random.default_rng(9)
    out, ins, lens = mix(rng, n, 4)
    _, r_off, r_st = tx_reference(out, ins, lens, 4, 0)
    buf, off, st = run(bridge(4), 4, out, ins, lens, 0, null_idx=True)
    assert off.tobytes() == r_off.tobytes() and st.tobytes() == r_st.tobytes()
    assert r_off[4] > 0 and (buf == MARK).all()
    # and without stats (len is then not read)
    buf, off, st = run(bridge(4), 4, out, ins, lens, 16, stats=False)
    assert off.tobytes() == r_off.tobytes()
    assert buf[:16].tobytes() == tx_reference(out, ins, lens, 4, 16)[0].tobytes()
    assert (buf[16:] == MARK).all()


def test_byte_sums_are_64_bit():
    n = 70_000
    out, ins = np.ones(n, np.uint16), np.zeros(n, np.uint16)
    lens = np.full(n, 65535, np.uint16)
    _, _, st = run(bridge(2), 2, out, ins, lens, n)
    assert int(st[32 + 1]) == 4_587_450_000 and int(st[1]) == n
    check(2, out, ins, lens)


def test_same_bytes_twice():
    n = 3 * T + 17
    rng = np.random.default_rng(11)
    out, ins, lens = mix(rng, n, 4)
    total = int(tx_reference(out, ins, lens, 4, 0)[1][4])
    a = run(bridge(4), 4, out, ins, lens, total)
    b = run(bridge(4), 4, out, ins, lens, total)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


DEV_MACS = [TR.mac("02:03:04:05:06:07"), TR.mac("12:13:14:15:16:17")]
END_MACS = [TR.mac("01:23:45:67:89:00"), TR.mac("01:23:45:67:89:01")]


def nat_pair(max_flows=64):
    args = ["--wan", "1", "--expire", "60000000", "--starting-port", "0",
            "--max-flows", str(max_flows), "--extip", "192.168.4.2",
            "--eth-dest", "0,01:23:45:67:89:00", "--eth-dest", "1,01:23:45:67:89:01"]
    cfg = vigor_amd.nat_config_from_args(args, 2, DEV_MACS)
    ocfg = orc.nat_cfg(wan=1, start_port=0, ext_ip=TR.ip4(192, 168, 4, 2),
                       expire_us=60000000, max_flows=max_flows, device_macs=DEV_MACS,
                       endpoint_macs=END_MACS, n_devices=2)
    return vigor_amd.Nat(cfg, gpu=0), orc.Oracle("nat", ocfg)


def end_to_end(nf, oracle, nd, fr, ln, dv, now, stream=None):
    """process_device then tx_build on the device tensors; the lists against
    the reference applied to the oracle's out ports."""
    exp_out = oracle.run(fr.copy(), ln, dv, now, 64)
    full, r_off, r_st = tx_reference(exp_out, dv, ln, nd, 1 << 32)
    d = torch.device("cuda:0")
    n = ln.shape[0]
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(None)
    with ctx:
        f_t = torch.from_numpy(fr.copy()).to(d)
        l_t, i_t = dev16(ln), dev16(dv)
        n_t = torch.from_numpy(now.astype(np.int64)).to(d)
        o_t = torch.zeros(n, dtype=torch.int16, device=d)
        buf = torch.full((full.size + TAIL,), MARK, dtype=torch.int32, device=d)
        off = torch.full((nd + 1,), MARK, dtype=torch.int32, device=d)
        st = torch.full((8 * STATS_WORDS,), 0xFF, dtype=torch.uint8, device=d)
    if stream is not None:
        stream.synchronize()  # (the inputs are there; the two calls are stream-ordered)
    nf.process_device(f_t, l_t, i_t, o_t, 64, now=n_t, stream=stream)
    nf.tx_build(o_t, i_t, l_t, buf[:full.size], off, st, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    assert np.array_equal(o_t.cpu().numpy().view(np.uint16), exp_out)
    got = buf.cpu().numpy().view(np.uint32)
    assert off.cpu().numpy().view(np.uint32).tobytes() == r_off.tobytes()
    assert st.cpu().numpy().view(np.uint64).tobytes() == r_st.tobytes()
    assert got[:full.size].tobytes() == full.tobytes()
    assert (got[full.size:] == MARK).all()
    return r_st


def test_end_to_end_bridge_floods_and_learned_macs():
    rng = np.random.default_rng(21)
    fr, ln, dv, now = mixed_bridge_trace(rng, 4000, 200)
    cfg = vigor_amd.bridge_config_from_args(["--capacity", "1024"], 3)
    br = vigor_amd.Bridge(cfg, gpu=0)
    o = orc.Oracle("bridge", orc.BridgeCfg(expiration_time=300_000_000, dyn_capacity=1024,
                                           n_devices=3), statics=[])
    st = end_to_end(br, o, 3, fr, ln, dv, now)
    assert st[64 + 1] > 0 and st[:3].all()  # floods, and unicast to every port


def test_end_to_end_nat_wan_drops():
    rng = np.random.default_rng(22)
    fr, ln, dv, now = mixed_nat_trace(rng, 5000, 40)
    nat, o = nat_pair()
    st = end_to_end(nat, o, 2, fr, ln, dv, now)
    assert st[64] > 0 and st[0] > 0 and st[1] > 0  # drops, both directions


def test_non_default_stream_after_process_device():
    rng = np.random.default_rng(23)
    fr, ln, dv, now = mixed_nat_trace(rng, 3 * T + 17, 40)
    nat, o = nat_pair()
    end_to_end(nat, o, 2, fr, ln, dv, now, stream=torch.cuda.Stream())


def test_workspace_growth_and_reuse_across_two_streams():
    """The context's one workspace of counts is ordered between streams by the
    library: one block's worth on the context's stream, three blocks and a
    remainder with floods on a second stream (the workspace grows), then the
    small batch again on the first (it waits for the second's launches),
    nothing waited for in between; every call gives the reference's offsets,
    lists and stats."""
    rng = np.random.default_rng(24)
    nd = 4
    nf = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], nd), gpu=0)  # a fresh workspace
    small = mix(rng, T, 2, p_bad=0.0)  # ports 0 and 1 only
    large = mix(rng, 3 * T + 5, nd, p_flood=0.3)
    s2 = torch.cuda.Stream()
    d = torch.device("cuda:0")
    jobs = []
    for (out, ins, lens), stream in ((small, None), (large, s2), (small, None)):
        want = tx_reference(out, ins, lens, nd, 1 << 32)
        total = want[0].size
        assert total == int(want[1][nd]) and total > 0
        jobs.append((want, total, stream, dev16(out), dev16(ins), dev16(lens),
                     torch.full((total + TAIL,), MARK, dtype=torch.int32, device=d),
                     torch.full((nd + 1,), MARK, dtype=torch.int32, device=d),
                     torch.full((8 * STATS_WORDS,), 0xFF, dtype=torch.uint8, device=d)))
    assert jobs[1][1] > jobs[1][3].numel()  # (floods: more entries than packets)
    torch.cuda.synchronize()
    for want, total, stream, o_t, i_t, l_t, buf, off, st in jobs:
        nf.tx_build(o_t, i_t, l_t, buf[:total], off, st, stream=stream)
    torch.cuda.synchronize()
    for (full, r_off, r_st), total, stream, o_t, i_t, l_t, buf, off, st in jobs:
        got = buf.cpu().numpy().view(np.uint32)
        assert off.cpu().numpy().view(np.uint32).tobytes() == r_off.tobytes()
        assert st.cpu().numpy().view(np.uint64).tobytes() == r_st.tobytes()
        assert got[:total].tobytes() == full.tobytes()
        assert (got[total:] == MARK).all()
    nf.close()


def test_einval_cases():
    nf = bridge(32)
    L = nf.L
    d = torch.device("cuda:0")
    out = torch.zeros(64, dtype=torch.int16, device=d)
    idx = torch.zeros(64, dtype=torch.int32, device=d)
    off = torch.zeros(33, dtype=torch.int32, device=d)

    def batch(**kw):
        b = dict(n=64, len=out.data_ptr(), in_dev=out.data_ptr(), out_dev=out.data_ptr())
        b.update(kw)
        return vigor_amd.DevBatchC(**b)

    def lists(**kw):
        a = dict(idx=idx.data_ptr(), cap=64, offset=off.data_ptr(), stats=None)
        a.update(kw)
        return vigor_amd.TxListsC(**a)

    def rc(h, b, a):
        return L.vp_tx_build(h, C.byref(b) if b is not None else None,
                             C.byref(a) if a is not None else None, None)

    assert rc(nf.h, batch(), lists()) == 0
    torch.cuda.synchronize()
    assert rc(None, batch(), lists()) == vigor_amd.VP_EINVAL
    assert rc(nf.h, None, lists()) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(), None) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(out_dev=None), lists()) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(), lists(offset=None)) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(), lists(idx=None)) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(), lists(idx=None, cap=0)) == 0
    assert rc(nf.h, batch(in_dev=None, in_port=0x10000), lists()) == vigor_amd.VP_EINVAL
    assert rc(nf.h, batch(in_dev=None, in_port=0xFFFF), lists()) == 0
    # n * max(1, n_devices - 1) must fit 32 bits: 31 lists' worth of 2^28 does not
    assert rc(nf.h, batch(n=1 << 28), lists()) == vigor_amd.VP_EINVAL
    assert rc(bridge(1).h, batch(n=0), lists()) == 0
    torch.cuda.synchronize()
    with pytest.raises(vigor_amd.VigpathError):
        nf.tx_build(out, 0x10000, out, idx, off)
