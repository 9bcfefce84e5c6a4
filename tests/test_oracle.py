"""Pin the oracle before trusting it (CPU only).

1. Known answers from SURVEY.md (probe runs of the reference itself):
   FlowId_hash KAT and the vignat byte-level frames of
   Appendix A (flow 0, LAN->WAN / WAN->LAN reverse path, anti-spoof drop,
   expiry drop).
2. The restated libVig vs the REFERENCE's own libVig sources on random
   operation streams: dchain (allocation order, LRU order, free-list LIFO,
   timestamps, expiry), the chain-counter map (colliding hash), the CHT table
   + lookups.
3. Whole-NF traces (vignat / vigbridge / viglb / vigfw / vigpol) with the same
   glue over both libVig builds: identical out ports, frame bytes and state.
Parts 2 and 3 run the seeded cases of tests/oracle_cases.py over the
restatement and compare with the reference libVig's answers to the same
cases, stored in tests/golden/ref_libvig.npz (tests/golden/
make_ref_golden.py writes them from oracle/_ref where the reference is
present). The known-answer tests of part 1 also run over oracle/_ref itself
where it can be built.
"""
import os

import numpy as np
import pytest

import oracle_cases as OC
import orc
from oracle_cases import DEV3_MACS, END3_MACS, fw_oracle, pol_oracle
from vigor_amd import traces as T

HAVE_REF = os.path.isdir("/root/reference/libvig/verified")
IMPLS = [False, True] if HAVE_REF else [False]

DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
END_MACS = [T.mac("01:23:45:67:89:00"), T.mac("01:23:45:67:89:01")]


def kat_nat(ref, expire_us=60_000_000):
    cfg = orc.nat_cfg(wan=1, start_port=0, ext_ip=T.ip4(192, 168, 4, 2),
                      expire_us=expire_us, max_flows=65536,
                      device_macs=DEV_MACS, endpoint_macs=END_MACS)
    return orc.Oracle("nat", cfg, ref=ref)


@pytest.mark.parametrize("ref", IMPLS)
def test_flowid_hash_kat(ref):
    assert orc.lib(ref).orc_flowid_hash(1, 2, 3, 4, 5, 6) == 0xAE93F0FF


def test_crc_software_equals_hardware():
    OC.check("crc")


@pytest.mark.parametrize("ref", IMPLS)
def test_appendix_a_flow0(ref):
    o = kat_nat(ref)
    fr, ln, dv, now = T.nat_lan_trace(1, 1)
    out = o.run(fr, ln, dv, now, 64)
    assert out[0] == 1
    assert fr[:42].tobytes().hex() == (
        "012345678901121314151617" "0800"
        "4500002e000000004011cffb0204a8c000000000" "0000" "0000" "001a" "54f6")


def _udp(src, dst, sp, dp, proto=17):
    f, _ = T.udp_frames(np.array([src]), np.array([dst]), np.array([sp]),
                        np.array([dp]), slot=64, proto=proto)
    return bytearray(f.tobytes())


def _rfc768(src, dst, l4):
    b = src + dst + bytes([0, 17, 0, len(l4)]) + l4[:6] + b"\0\0" + l4[8:]
    s = sum((b[i] << 8) | (b[i + 1] if i + 1 < len(b) else 0)
            for i in range(0, len(b), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return (~s) & 0xFFFF or 0xFFFF


@pytest.mark.parametrize("ref", IMPLS)
def test_appendix_a_reverse_path(ref):
    o = kat_nat(ref)
    t = T.NOW0
    for i in range(5):  # indices 0..4
        assert o.process(0, _udp(T.ip4(10, 0, 0, 100 + i), 0, 1, 1), 60, 64,
                         t + i) == 1
    f = _udp(T.ip4(10, 0, 0, 5), T.ip4(8, 8, 8, 8), 80, 53)
    assert o.process(0, f, 60, 64, t + 10) == 1
    assert f[:42].hex() == ("012345678901121314151617" "0800"
                            "4500002e000000004011bfeb" "0204a8c0" "08080808"
                            "0500" "0035" "001a" "3fb1")
    # reply: 8.8.8.8:53 -> 0.0.0.0, dst port bytes 05 00 -> index 5
    r = _udp(T.ip4(8, 8, 8, 8), 0, 53, 0x0500)
    assert o.process(1, r, 60, 64, t + 20) == 0
    assert r[:40].hex() == ("012345678900020304050607" "0800"
                            "4500002e00000000401160ab" "08080808" "0a000005"
                            "0035" "0050" "001a")
    # SURVEY.md prints only the first 42 bytes of its probe frame and UDP
    # checksum e51b. With the 18 B zero payload used here the checksum of
    # these header bytes is e520 (also by an independent RFC 768 sum). The
    # two differ by 0x0500 in the sum, i.e. exactly one payload byte 0x05 at
    # an odd L4 offset: the same reply with payload 00 05 00 ... gives e51b
    # from both the oracle and the RFC 768 sum, so the printed KAT holds for
    # a probe frame with that payload.
    assert r[40:42].hex() == "%04x" % _rfc768(bytes(r[26:30]), bytes(r[30:34]),
                                               bytes(r[34:60]))
    assert r[40:42].hex() == "e520"
    o2 = kat_nat(ref)
    for i in range(5):
        o2.process(0, _udp(T.ip4(10, 0, 0, 100 + i), 0, 1, 1), 60, 64, t + i)
    o2.process(0, _udp(T.ip4(10, 0, 0, 5), T.ip4(8, 8, 8, 8), 80, 53), 60, 64, t + 10)
    rp = _udp(T.ip4(8, 8, 8, 8), 0, 53, 0x0500)
    rp[43] = 0x05  # L4 offset 9: the second payload byte
    assert o2.process(1, rp, 60, 64, t + 20) == 0
    assert rp[40:42].hex() == "e51b"
    assert "%04x" % _rfc768(bytes(rp[26:30]), bytes(rp[30:34]), bytes(rp[34:60])) == "e51b"
    # dst port bytes 00 05 -> index 0x0500 = 1280, not allocated -> drop
    r2 = _udp(T.ip4(8, 8, 8, 8), 0, 53, 0x0005)
    before = bytes(r2)
    assert o.process(1, r2, 60, 64, t + 30) == 1
    assert bytes(r2) == before
    # anti-spoof: wrong source port -> drop
    r3 = _udp(T.ip4(8, 8, 8, 8), 0, 54, 0x0500)
    assert o.process(1, r3, 60, 64, t + 40) == 1


@pytest.mark.parametrize("ref", IMPLS)
def test_appendix_a_expiry(ref):
    o = kat_nat(ref, expire_us=1)
    t = T.NOW0
    f = _udp(T.ip4(10, 0, 0, 5), T.ip4(8, 8, 8, 8), 80, 53)
    assert o.process(0, f, 60, 64, t) == 1
    r = _udp(T.ip4(8, 8, 8, 8), 0, 53, 0x0000)
    assert o.process(1, bytearray(r), 60, 64, t + 1000) == 0  # ts < cutoff? no
    assert o.process(1, bytearray(r), 60, 64, t + 2001) == 1  # expired


# --------------------------------------------------------- libVig vs ref --

@pytest.mark.parametrize("seed", range(6))
def test_dchain_matches_reference(seed):
    OC.check("dchain", seed)


@pytest.mark.parametrize("seed", range(6))
def test_map_matches_reference(seed):
    OC.check("map", seed)


@pytest.mark.parametrize("height,cap", [(97, 32), (257, 256), (7, 4), (13, 1), (521, 512)])
def test_cht_matches_reference(height, cap):
    OC.check("cht", height, cap)


# ------------------------------------------------------ whole-NF vs ref --
# (out ports, frame bytes, and the dumped state: allocation flags, the time
# stamps of allocated indices, keys and values)

@pytest.mark.parametrize("seed,max_flows,expire_us,n_flows",
                         [(0, 64, 60_000_000, 40), (1, 64, 1, 100),
                          (2, 16, 60_000_000, 40), (3, 256, 5, 300)])
def test_nat_trace_matches_reference(seed, max_flows, expire_us, n_flows):
    OC.check("nat", seed, max_flows, expire_us, n_flows)


@pytest.mark.parametrize("seed,cap,expire_us", [(0, 64, 300_000_000),
                                                (1, 16, 2), (2, 1024, 10)])
def test_bridge_trace_matches_reference(seed, cap, expire_us):
    OC.check("bridge", seed, cap, expire_us)


@pytest.mark.parametrize("seed,fexp,bexp", [(0, 60_000_000, 3_600_000_000),
                                            (1, 3, 50), (2, 20, 2)])
def test_lb_trace_matches_reference(seed, fexp, bexp):
    OC.check("lb", seed, fexp, bexp)


@pytest.mark.parametrize("shape,seed,fexp,bexp", [("wide", 10, 2, 3_600_000),
                                                  ("edge", 11, 60_000_000, 2)])
def test_lb_wide_and_edge_traces_match_reference(shape, seed, fexp, bexp):
    """viglb in 256-byte slots (wide_lb_trace: flows expire and return;
    edge_lb_trace: backends expire and are learned again, from heartbeats
    with options too): the restatement's lb logic on the shapes the GPU is
    compared with it on."""
    out, rewritten = OC.check("lb_shape", shape, seed, fexp, bexp)[:2]
    assert rewritten.reshape(-1, 256).any(axis=1).sum() > 300  # (forwarded frames)
    if shape == "edge":  # frames with IPv4 options among them
        assert (rewritten.reshape(-1, 256)[:, 38:].any(axis=1)).sum() > 20


# ---------------------------------------------------------------- vigfw --

@pytest.mark.parametrize("ref", IMPLS)
def test_fw_flowid_hash_is_crc_chain(ref):
    """vigfw's generated FlowId_hash: five crc32c_u32 steps in field order
    (codegen/main.ml:328-401), checked against the chained u32 CRC."""
    L = orc.lib(ref)
    for sp, dp, sip, dip, pr in [(1, 2, 3, 4, 5), (0x3500, 0xE803, 0x0A000001,
                                                   0x08080808, 17)]:
        h = 0
        for v in (sp, dp, sip, dip, pr):
            h = L.orc_crc32c_u32(h, v)
        assert L.orc_fw_flowid_hash(sp, dp, sip, dip, pr) == h


@pytest.mark.parametrize("ref", IMPLS)
def test_fw_semantics_kat(ref):
    """fw_main.c:21-80 by hand: a LAN packet opens the flow and goes out on
    the WAN with its MACs; the reply comes back to the LAN device that opened
    it; an unknown reply is dropped; a non-TCP/UDP packet is dropped; the
    header past the MACs is never touched."""
    o = fw_oracle(ref)
    f, _ = T.udp_frames(np.array([T.ip4(10, 0, 0, 5)]), np.array([T.ip4(8, 8, 8, 8)]),
                        np.array([1234]), np.array([53]))
    lan = bytearray(f.tobytes())
    orig = bytes(lan)
    assert o.process(2, lan, now=T.NOW0) == 1
    assert bytes(lan[0:6]) == END3_MACS[1] and bytes(lan[6:12]) == DEV3_MACS[1]
    assert bytes(lan[12:]) == orig[12:]
    r, _ = T.udp_frames(np.array([T.ip4(8, 8, 8, 8)]), np.array([T.ip4(10, 0, 0, 5)]),
                        np.array([53]), np.array([1234]))
    rep = bytearray(r.tobytes())
    assert o.process(1, rep, now=T.NOW0 + 1) == 2
    assert bytes(rep[0:6]) == END3_MACS[2] and bytes(rep[6:12]) == DEV3_MACS[2]
    u, _ = T.udp_frames(np.array([T.ip4(8, 8, 8, 8)]), np.array([T.ip4(10, 0, 0, 6)]),
                        np.array([53]), np.array([1234]))
    unk = bytearray(u.tobytes())
    assert o.process(1, unk, now=T.NOW0 + 2) == 1 and bytes(unk) == u.tobytes()
    icmp = bytearray(orig)
    icmp[23] = 1
    assert o.process(0, icmp, now=T.NOW0 + 3) == 0
    alloc, ts, keys, dev = o.fw_dump(64)
    assert alloc.sum() == 1 and dev[0] == 2 and ts[0] == T.NOW0 + 1


@pytest.mark.parametrize("seed,max_flows,expire_us,n_flows",
                         [(0, 64, 60_000_000, 40), (1, 64, 1, 100),
                          (2, 16, 60_000_000, 40), (3, 256, 5, 300)])
def test_fw_trace_matches_reference(seed, max_flows, expire_us, n_flows):
    OC.check("fw", seed, max_flows, expire_us, n_flows)


@pytest.mark.parametrize("ref", IMPLS)
def test_pol_semantics_kat(ref):
    """policer_main.c:34-145 by hand (rate 1 B/us, burst 1000 B): a new
    destination takes burst - size; a refill adds time_diff * rate / 1e9;
    a packet passes only while bucket > size; after burst/rate of silence the
    bucket is full again; LAN packets pass unpoliced; frames are untouched."""
    o = pol_oracle(ref)
    f, _ = T.udp_frames(np.array([T.ip4(9, 9, 9, 9)]), np.array([T.ip4(10, 0, 0, 1)]),
                        np.array([53]), np.array([80]))
    fr = bytearray(f.tobytes())
    orig = bytes(fr)
    t = T.NOW0
    assert o.process(0, fr, length=600, now=t) == 1       # new: 1000-600 = 400
    assert o.process(0, fr, length=400, now=t) == 0       # 400 > 400 fails
    assert o.process(0, fr, length=399, now=t) == 1       # 1 left
    assert o.process(0, fr, length=64, now=t + 100_000) == 1  # +100 -> 101 - 64
    alloc, ts, keys, size, btime = o.pol_dump(64)
    assert alloc.sum() == 1 and size[0] == 37 and btime[0] == t + 100_000
    assert keys[0] == 0x0100000A and ts[0] == t + 100_000  # raw (network order)
    assert o.process(0, fr, length=1001, now=t + 100_001) == 0  # hit, > burst
    assert o.process(1, fr, length=64, now=t + 100_002) == 0    # LAN -> WAN
    assert o.process(2, fr, length=64, now=t + 100_003) == 2    # other: drop
    assert bytes(fr) == orig
    # burst/rate = 1 ms after the last touch the entry expires
    g, _ = T.udp_frames(np.array([T.ip4(9, 9, 9, 9)]), np.array([T.ip4(10, 0, 0, 2)]),
                        np.array([53]), np.array([80]))
    fr2 = bytearray(g.tobytes())
    assert o.process(0, fr2, length=1001, now=t + 2_000_000) == 0  # > burst, new
    alloc, ts, keys, size, btime = o.pol_dump(64)
    assert alloc.sum() == 0


@pytest.mark.parametrize("seed,cap,n_dsts,burst,gap", [
    (0, 64, 40, 3000, 500), (1, 16, 60, 1000, 2000), (2, 256, 300, 2000, 50),
    (3, 64, 20, 1000, 10)])
def test_pol_trace_matches_reference(seed, cap, n_dsts, burst, gap):
    out, rewritten = OC.check("pol", seed, cap, n_dsts, burst, gap)[:2]
    assert not rewritten.any()  # vigpol leaves the frames untouched
    assert (out == 1).sum() > 100 and (out == 0).sum() > 100
