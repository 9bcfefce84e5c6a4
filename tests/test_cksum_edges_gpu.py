"""The checksum's value edges on every HIP path that computes a checksum
(finish_l4's zero rule, fold16's second fold, the IPv4 checksum stored as
0x0000, and the neighbours of each), against the oracle, bit for bit.

The traces are those of tests/cksum_cases.py; tests/test_cksum_edges.py
verifies the oracle's answers to them with an independent RFC 1071 sum. Each
test re-asserts that the oracle output it compares with holds at least 32
frames on every edge (cksum_cases.require_edges) and that the path it is
about was taken.
"""
import numpy as np
import pytest

import cksum_cases as CC
import test_lb_gpu as LG
import test_mbuf_gpu as MG
import test_nat_gpu as NG
from gpuh import run_gpu

pytestmark = pytest.mark.gpu


def nat_batches(case, cuts):
    """The case through vp_process_device in batches; every batch's out ports
    and frame bytes against the oracle's, the last kernel of each batch."""
    c = CC.nat_case(case)
    CC.require_edges(c)
    slot = c["slot"]
    nat, _ = NG.make_pair(max_flows=c["max_flows"])
    kernels = []
    bounds = [0] + cuts + [len(c["ln"])]
    for a, b in zip(bounds[:-1], bounds[1:]):
        got, out = run_gpu(nat, c["fr"][a * slot:b * slot], c["ln"][a:b], c["dv"][a:b],
                           c["now"][a:b], slot)
        np.testing.assert_array_equal(out, c["exp_out"][a:b])
        bad = (got.reshape(-1, slot) != c["exp"][a * slot:b * slot].reshape(-1, slot)).any(axis=1)
        assert not bad.any(), "frame mismatch at packets %s" % (a + np.nonzero(bad)[0][:10])
        kernels.append(nat.last_kernel())
    o = CC.nat_oracle(c["max_flows"])
    o.run(c["fr"].copy(), c["ln"], c["dv"], c["now"], slot)
    NG.check_state(nat, o, c["max_flows"])
    return c, kernels


@pytest.mark.parametrize("case", ["tile64_lean", "tile64_lanes"])
def test_nat_tile64(case):
    """fast_checksums without a tail: the 64-byte tile kernel's lean tiles
    (LAN only) and its per-lane path (WAN replies, a malformed frame in every
    tile)."""
    c, kernels = nat_batches(case, [2048])
    assert all(k.startswith("nat_classify64") for k in kernels), kernels
    F = c["fr"].reshape(-1, 64)
    lean = (c["dv"] == 0).all() and (F[:, 12] == 8).all() and (F[:, 23] != 1).all()
    assert lean == (case == "tile64_lean")
    if not lean:  # no tile without a frame that leaves the lean path
        odd = (c["dv"] == 1) | (F[:, 12] != 8) | (F[:, 23] == 1)
        assert odd.reshape(-1, 64).any(axis=1).all()


@pytest.mark.parametrize("case", ["wide256", "wide1536"])
def test_nat_wide_tail_sums(case):
    """fast_checksums with tile_tail_sums' tail: the spare word below byte 64
    in some labelled frames and past it in others."""
    c, kernels = nat_batches(case, [700, 700 + 64 * 5])
    assert all(k in ("nat_classify128", "nat_classify_wide") for k in kernels), kernels
    lab = np.nonzero(c["labels"] >= 0)[0]
    assert (c["at"][lab] < 64).sum() >= 256 and (c["at"][lab] >= 64).sum() >= 256
    E, F = c["exp"].reshape(-1, c["slot"]), c["fr"].reshape(-1, c["slot"])
    np.testing.assert_array_equal(E[lab, 64:], F[lab, 64:])  # (bytes past 64 untouched)


@pytest.mark.parametrize("case", ["options64", "options128"])
def test_nat_byte_path(case):
    """set_checksums (raw_sum) over frames with an IPv4 option word."""
    c, _ = nat_batches(case, [1000])
    F = c["fr"].reshape(-1, c["slot"])
    lab = c["labels"] >= 0
    assert ((F[lab, 14] & 15) == 6).all() and lab.sum() >= 8 * CC.MIN_FRAMES


def test_nat_mbuf_header_slots(monkeypatch):
    """mbuf_gather_hdr<true>'s tail sums: registered mbufs, frames of 90-1518
    bytes in 64-byte header slots, every spare word past byte 64."""
    monkeypatch.setenv("VIGPATH_HOST_CHUNK", "700")
    monkeypatch.setenv("VIGPATH_MBUF_MODE", "gpu")
    c = CC.nat_case("mbuf")
    CC.require_edges(c)
    slot = c["slot"]
    lab = c["labels"] >= 0
    assert c["ln"].min() >= 90 and (c["at"][lab] >= 64).sum() >= 8 * CC.MIN_FRAMES
    rng = np.random.default_rng(47)
    nat, o = NG.make_pair(max_flows=c["max_flows"])
    pool, bufs, ptrs = MG.to_pool(c["fr"], c["ln"], slot, rng)
    out = MG.run_mbufs(nat, pool, ptrs, c["ln"], c["dv"], c["now"])
    MG.compare(pool, bufs, c["ln"], c["exp"], c["exp_out"], out, slot)
    o.run(c["fr"].copy(), c["ln"], c["dv"], c["now"], slot)
    NG.check_state(nat, o, c["max_flows"])


def test_nat_resident_kernel_per_packet():
    """nat_serve's one-packet body (vp_process_one)."""
    c = CC.nat_case("serve_one")
    CC.require_edges(c)
    n = len(c["ln"])
    F, E = c["fr"].reshape(n, 64), c["exp"].reshape(n, 64)
    nat, o = NG.make_pair(max_flows=c["max_flows"])
    st0 = nat.serve_stats()
    for i in range(n):
        b = bytearray(F[i, :c["ln"][i]].tobytes())
        assert nat.process(int(c["dv"][i]), b, int(c["now"][i])) == c["exp_out"][i], i
        assert bytes(b) == E[i, :c["ln"][i]].tobytes(), i
    st = nat.serve_stats()
    assert st["packets_one"] - st0["packets_one"] == n, (st0, st)
    o.run(c["fr"].copy(), c["ln"], c["dv"], c["now"], 64)
    NG.check_state(nat, o, c["max_flows"])


def test_nat_resident_kernel_bursts():
    """nat_serve's burst body: vp_process_mbufs calls of 32 packets."""
    c = CC.nat_case("serve_burst")
    CC.require_edges(c)
    n = len(c["ln"])
    F, E = c["fr"].reshape(n, 64), c["exp"].reshape(n, 64)
    nat, o = NG.make_pair(max_flows=c["max_flows"])
    st0 = nat.serve_stats()
    for a in range(0, n, 32):
        bufs = [bytearray(F[j, :c["ln"][j]].tobytes()) for j in range(a, a + 32)]
        out = nat.process_mbufs(bufs, c["dv"][a:a + 32], c["now"][a:a + 32])
        np.testing.assert_array_equal(out, c["exp_out"][a:a + 32])
        for j in range(32):
            assert bytes(bufs[j]) == E[a + j, :c["ln"][a + j]].tobytes(), a + j
    st = nat.serve_stats()
    assert st["burst_packets"] - st0["burst_packets"] == n and st["declined"] == 0, (st0, st)
    assert st["bursts"] - st0["bursts"] == n // 32, (st0, st)
    o.run(c["fr"].copy(), c["ln"], c["dv"], c["now"], 64)
    NG.check_state(nat, o, c["max_flows"])


@pytest.mark.parametrize("case", list(CC.LB_CASES))
def test_lb_rewrite_sites(case):
    """viglb's rewrites: the edge batch as first sightings (lb_resolve's
    byte path), as hits (64-byte slots: the tile kernel, its backends staged
    in LDS or, with bcap 512, lb_rewrite_fast; 256-byte slots: lb_classify),
    and, after the backends expired and fewer returned, as stale flows."""
    c = CC.lb_case(case)
    slot = c["slot"]
    bounds = [0] + [int(x) for x in c["cuts"]] + [len(c["ln"])]
    for seg in (1, 2, 4):
        CC.require_edges(c, bounds[seg], bounds[seg + 1])
    assert CC.lb_reassigned(c) >= 100
    lb, _ = LG.make_pair(flow_cap=CC.LB_FLOW_CAP, bcap=c["bcap"], height=c["height"],
                         bexp=CC.LB_BEXP_US)
    for seg, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        got, out = run_gpu(lb, c["fr"][a * slot:b * slot], c["ln"][a:b], c["dv"][a:b],
                           c["now"][a:b], slot)
        np.testing.assert_array_equal(out, c["exp_out"][a:b], "out ports, segment %d" % seg)
        bad = (got.reshape(-1, slot) != c["exp"][a * slot:b * slot].reshape(-1, slot)).any(axis=1)
        assert not bad.any(), "segment %d: frame mismatch at %s" % (seg, a + np.nonzero(bad)[0][:10])
        if slot == 64:
            assert lb.last_kernel() == "lb_classify64", lb.last_kernel()
    o = CC.lb_oracle(c["bcap"], c["height"])
    o.run(c["fr"].copy(), c["ln"], c["dv"], c["now"], slot)
    LG.check_state(lb, o)
