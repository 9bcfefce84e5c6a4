"""vigfw's batch pipeline (vp_process_device, vp_fw.hip) on the directed
traces of fw_cases.py: every batch bit for bit against the oracle (out ports,
every slot byte), the out ports and frames the traces carry (the Python
model's: only bytes 0-11 of a forwarded frame change; and the ports written
by hand), the full dump behind every batch (alloc and, on live indices,
stamp, FlowId and internal device), the model's table behind every case, and
the classify kernel of the slot size through vp_last_kernel.
test_fw_edges.py checks on the CPU that each trace reaches what it names.
No tolerance anywhere: the operation is integer.
"""
import numpy as np
import pytest

import fw_cases as F
import vigor_amd
from gpuh import dumps_equal, run_gpu

pytestmark = pytest.mark.gpu


def states_equal(fw, oracle, cap):
    """test_fw_gpu.check_state's comparison; returns the GPU's live state."""
    g = fw.dump()
    dumps_equal(g, oracle.fw_dump(cap))
    return F.live_state(g)


def feed(fw, oracle, case, b, affine):
    rows, ln, dv, now = b.arrays()
    exp = rows.reshape(-1).copy()
    exp_out = oracle.run(exp, ln, dv, now, case.slot)
    aff = b.affine() if affine else None
    assert aff is not None or not affine
    got, out = run_gpu(fw, rows.reshape(-1), ln, dv, now, case.slot, affine=aff)
    what = "%s, %s" % (case, b.note)
    np.testing.assert_array_equal(out, exp_out, "out ports: " + what)
    np.testing.assert_array_equal(out, b.out_ports(), "model ports: " + what)
    named = [j for j, w in enumerate(b.want) if w is not None]
    np.testing.assert_array_equal(out[named], np.array([b.want[j] & 0xFF for j in named],
                                                       np.uint16), "named ports: " + what)
    got = got.reshape(rows.shape)
    bad = np.nonzero((got != exp.reshape(rows.shape)).any(axis=1))[0]
    assert bad.size == 0, "frames: %s, packets %s" % (what, bad[:10])
    assert (got == b.frames_after()).all(), "model frames: " + what
    assert (got[:, 12:] == rows[:, 12:]).all(), "bytes 12 on: " + what
    # 64-byte slots take the register tiles, any other slot the byte path
    kernel = "fw_classify64" if case.slot == 64 else "fw_classify"
    assert fw.last_kernel() == kernel, (what, fw.last_kernel())
    states_equal(fw, oracle, case.max_flows)


def run_case(case, affine=False):
    args = ["--wan", str(F.WAN), "--expire", str(case.expire_us), "--max-flows",
            str(case.max_flows)]
    for d in range(F.N_DEV):
        args += ["--eth-dest", "%d,%s" % (d, F.END_MACS[d].hex(":"))]
    fw = vigor_amd.Fw(vigor_amd.fw_config_from_args(args, F.N_DEV, F.DEV_MACS), gpu=0)
    try:
        oracle = F.make_oracle(case)
        for b in case.batches:
            feed(fw, oracle, case, b, affine)
        st = states_equal(fw, oracle, case.max_flows)
        assert {k: (v[2], v[1]) for k, v in st.items()} == case.final(), case
        return st
    finally:
        fw.close()


@pytest.mark.parametrize("affine", [False, True], ids=["times", "affine"])
@pytest.mark.parametrize("slot", [64, 128])
def test_order_in_one_segment(slot, affine):
    """a. A reply is a hit only behind its opener: within a wave, across a
    wave's end, across a block's (255 | 256), at every multiple of 64 in both
    orders and first against last of 4096 packets; one 5-tuple opened from
    devices 2 and 0 in one segment belongs to device 2. With affine times the
    steady batch leaves only the fold pending."""
    run_case(F.order_case(slot), affine=affine)


@pytest.mark.parametrize("slot", [64, 128])
def test_key_word_3(slot):
    """b. Only the protocol byte of key word 3 is compared: a flow opened from
    device 2 is found again, TCP and UDP flows of one 4-tuple stay apart, a
    WAN packet's own 5-tuple does not match."""
    st = run_case(F.word3_case(slot))
    assert st[F.lan_key(1)][2] == F.LAN2 and st[F.lan_key(2, 6)][2] == F.LAN2


def test_table_full():
    """c. max_flows 16, 20 new flows: the LAN packets of the unstored four
    still go out rewritten, their replies come back untouched, in the same
    batch and in the next; after the expiry they are stored."""
    st = run_case(F.table_full_case())
    assert len(st) == 4


@pytest.mark.parametrize("slot", [64, 128])
def test_header_matrix(slot):
    """d. Lengths 0 .. 64 (and past 73 in 128-byte slots) x header variants x
    arrival devices, as openers and as replies to flows that exist: the lean
    parse and the byte path agree with nf-util.h on every edge, and the L4
    offset moves with the options that are borrowed."""
    run_case(F.matrix_case(slot))


def test_expiry():
    """e. An expiry due at packet 70 of 200 with the stamps one below, at and
    one above the cutoff; a flow opened again from another device; a flow
    kept alive by replies alone for 3 E."""
    c = F.expiry_case()
    st = run_case(c)
    assert st[F.lan_key(F.KEEP)][1] == c.t_keep and F.lan_key(F.IDLE) not in st


def test_free_order():
    """e. 40 stamps tied in time by replies, all expired by one packet: the
    dump by index behind the 40 new flows is the oracle's."""
    st = run_case(F.free_order_case())
    assert len(st) == F.N_FREE
