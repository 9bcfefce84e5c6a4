"""The checksum's value edges on the oracle alone (CPU).

1. An independent verifier: RFC 1071 in plain Python (big-endian words, the
   pseudo header, arbitrary-precision integers; no code shared with orc.c or
   traces.py) over every frame the oracle forwards from the edge traces of
   tests/cksum_cases.py, vignat and viglb. A correct checksum makes the sum
   over the covered bytes, the stored checksum among them, fold to 0xFFFF; a
   stored L4 checksum of 0xFFFF stands for zero (DPDK 20.08
   rte_ipv4_udptcp_cksum: for TCP as for UDP) and, 0xFFFF being zero in
   ones' complement, verifies the same way.
2. The conditions that keep the GPU tests from passing vacuously: every
   case's oracle output holds at least 32 frames on every edge, and every
   labelled frame is forwarded and sits on its edge.
"""
import pytest

import cksum_cases as CC

CASES = [("nat", k) for k in CC.NAT_CASES] + [("lb", k) for k in CC.LB_CASES]


def get(kind, name):
    return CC.nat_case(name) if kind == "nat" else CC.lb_case(name)


def ones_sum(data):
    """RFC 1071: the 16-bit ones' complement sum of big-endian words, an odd
    last byte padded with a zero byte."""
    if len(data) % 2:
        data = data + b"\0"
    s = sum(int.from_bytes(data[i:i + 2], "big") for i in range(0, len(data), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def verify(frame):
    """(IP header verifies, L4 verifies) for one forwarded frame. The header
    sum covers IHL words. The L4 sum covers what nf-util.c:45-64 covers:
    total_length - 20 bytes from the L4 header on, that length in the pseudo
    header (a frame padded past total_length is verified over total_length;
    under IPv4 options the reference still takes the header for 20 bytes)."""
    ihl = frame[14] & 15
    ip_ok = ones_sum(frame[14:14 + 4 * ihl]) == 0xFFFF
    tl = int.from_bytes(frame[16:18], "big")
    l4 = 14 + 4 * ihl
    n = tl - 20
    pseudo = frame[26:34] + bytes([0, frame[23]]) + n.to_bytes(2, "big")
    l4_ok = ones_sum(pseudo + frame[l4:l4 + n]) == 0xFFFF
    return ip_ok, l4_ok


@pytest.mark.parametrize("kind,name", CASES)
def test_oracle_checksums_verify(kind, name):
    c = get(kind, name)
    slot = c["slot"]
    E = c["exp"].reshape(-1, slot)
    bad = []
    fwd = c["forwarded"].nonzero()[0]
    for i in fwd:
        ok = verify(E[i].tobytes())
        if ok != (True, True):
            bad.append((int(i), ok))
    assert len(fwd) > 256
    assert not bad, "frames that do not verify (packet, (ip, l4)): %s" % bad[:10]


@pytest.mark.parametrize("kind,name", CASES)
def test_edges_are_reached(kind, name):
    c = get(kind, name)
    if kind == "nat":
        print(name, CC.require_edges(c))
        return
    # viglb: in each feeding of the edge batch (first sightings, hits, stale)
    bounds = [0] + [int(x) for x in c["cuts"]] + [len(c["ln"])]
    for seg in (1, 2, 4):
        print(name, seg, CC.require_edges(c, bounds[seg], bounds[seg + 1]))
    assert CC.lb_reassigned(c) >= 100


def test_verifier_rejects_a_wrong_checksum():
    """The verifier is no rubber stamp: one bit of a forwarded frame's IP or
    L4 checksum flipped fails that sum and only that one."""
    c = CC.nat_case("tile64_lean")
    E = c["exp"].reshape(-1, 64)
    i = int(c["forwarded"].nonzero()[0][0])
    f = bytearray(E[i].tobytes())
    assert verify(bytes(f)) == (True, True)
    f[25] ^= 1
    assert verify(bytes(f)) == (False, True)
    f[25] ^= 1
    o = 34 + (16 if f[23] == 6 else 6)
    f[o] ^= 0x80
    assert verify(bytes(f)) == (True, False)
