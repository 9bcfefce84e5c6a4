"""vigbridge's batch pipeline (vp_process_device, vp_bridge.hip) on the
directed traces of bridge_cases.py: every batch bit for bit against the oracle
(out ports, every slot byte untouched), the out ports the traces carry (the
Python model's and the hand-written ones), the full dump behind every batch
(alloc and, on live indices, stamp, MAC and port), the model's table behind
every case, and the classify kernel through vp_last_kernel.
test_bridge_edges.py checks on the CPU that each trace reaches what it names.
No tolerance anywhere: the operation is integer.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bridge_cases as B
import vigor_amd
from gpuh import dumps_equal, run_gpu

pytestmark = pytest.mark.gpu


def states_equal(br, oracle, cap):
    """test_bridge_gpu.check_state's comparison; returns the GPU's live state."""
    g = br.dump()
    dumps_equal(g, oracle.bridge_dump(cap))
    return B.live_state(g)


def make_bridge(case):
    """The context, created with the case's layout switches in the
    environment (read once per context)."""
    old = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    try:
        args = ["--expire", str(case.expire_us), "--capacity", str(case.cap)]
        cfg = vigor_amd.bridge_config_from_args(args, B.N_DEV, list(case.statics))
        return vigor_amd.Bridge(cfg, gpu=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def feed(br, oracle, case, b, affine, kernel):
    F, ln, dv, now = b.arrays()
    exp = F.reshape(-1).copy()
    exp_out = oracle.run(exp, ln, dv, now, case.slot)
    aff = b.affine() if affine else None
    assert aff is not None or not affine
    got, out = run_gpu(br, F.reshape(-1), ln, dv, now, case.slot, affine=aff)
    what = "%s, %s" % (case, b.note)
    np.testing.assert_array_equal(out, exp_out, "out ports: " + what)
    np.testing.assert_array_equal(out, np.array(b.exp, np.uint16), "model ports: " + what)
    named = [j for j, t in enumerate(b.tags) if t]
    np.testing.assert_array_equal(out[named], np.array([b.want[j] for j in named], np.uint16),
                                  "named ports: " + what)
    assert (got == F.reshape(-1)).all() and (exp == got).all(), "frames: " + what
    assert br.last_kernel() == kernel, (what, br.last_kernel())
    states_equal(br, oracle, case.cap)
    if b.tombs is not None:
        assert br.table_stats()["tombstones"] >= b.tombs, (what, br.table_stats())


def run_case(case, affine=False, kernel="bridge_classify"):
    br = make_bridge(case)
    try:
        oracle = B.make_oracle(case)
        if case.env:  # the layout the case's MACs were chosen for, or fail loudly
            st = br.table_stats()
            assert (st["layout"], st["buckets"]) == (B.PROBE_LAYOUT, B.PROBE_BUCKETS), st
        for b in case.batches:
            feed(br, oracle, case, b, affine, kernel)
        st = states_equal(br, oracle, case.cap)
        assert {m: (v[2], v[1]) for m, v in st.items()} == case.final(), case
        if case.env:
            assert br.table_stats()["layout"] == B.PROBE_LAYOUT
        return st
    finally:
        br.close()


@pytest.mark.parametrize("affine", [False, True], ids=["times", "affine"])
def test_order_in_one_segment(affine):
    """a. Learn precedes lookup; a dst learned by packet q forwards for p >= q
    and floods for p < q, within a wave, across a wave's end, across a block's
    (255 | 256), at every multiple of 64 and first against last of 4096
    packets; the earliest of two first sightings wins; a known MAC keeps its
    port; the broadcast address is learned. With affine times the steady
    batch leaves only the fold pending."""
    run_case(B.order_case(64), affine=affine)


@pytest.mark.parametrize("slot", [64, 80, 128, 2048])
def test_slots_and_runts(slot):
    """f. The same traffic in 64-, 80-, 128- and 2048-byte slots with lengths
    0 .. 14 mixed in: the 12 MAC bytes are read whatever the length."""
    run_case(B.order_case(slot, runts=True), affine=slot == 80)


def test_table_full():
    """b. Capacity 64, 70 new MACs in one batch: the unlearned six stay
    unknown however often they are seen, and are learned after the expiry."""
    st = run_case(B.table_full_case())
    assert len(st) == 6


def test_statics_against_phase_c():
    """c. -1 and -2 rules for MACs the same segment learns, the same dst from
    a port without a rule, a repeated key, a rule on the MAC's own port."""
    run_case(B.statics_case())


@pytest.mark.parametrize("affine", [False, True], ids=["times", "affine"])
def test_expiry_cuts_inside_a_tile(affine):
    """d. Expiries due at packets 70 and 79 of 200 (704 ns after the 32-bit
    wrap of expiration_time * 1000): the stamp at, one below and one above the
    cutoff; a MAC learned again on its new port; a destination-only MAC
    expires."""
    st = run_case(B.expiry_case(), affine=affine)
    assert B.D not in st and st[B.X][2] == 2


def test_free_order():
    """e. 40 stamps tied in time, all expired by one packet: the dump by
    index behind the 40 new MACs is the oracle's."""
    st = run_case(B.free_order_case())
    assert len(st) == B.N_FREE


def test_probe_past_the_home_bucket():
    """g. Nine MACs of one home bucket (multiplicative layout, 64 buckets):
    src and dst probes that leave the home bucket, across tombstones."""
    run_case(B.probe_case())


def test_hot_src():
    """h. 4096 packets from one src: its stamp is the last packet's time."""
    c = B.hot_src_case()
    st = run_case(c)
    assert st[c.hot][1] == c.t_last


def sixteen_waves():
    """Cases a, d and f through bridge_classify_w."""
    for case, affine in ((B.order_case(64), False), (B.order_case(64), True),
                         (B.expiry_case(), False), (B.expiry_case(), True),
                         (B.order_case(80, runts=True), False),
                         (B.order_case(128, runts=True), True),
                         (B.order_case(2048, runts=True), False)):
        run_case(case, affine=affine, kernel="bridge_classify_w")


def test_sixteen_waves():
    """bridge_classify_w (VIGPATH_BRIDGE_WAVES=16, read once per process: a
    fresh child) on cases a, d and f."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VIGPATH_BRIDGE_WAVES="16")
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    code = "import test_bridge_edges_gpu as M; M.sixteen_waves(); print('CHILD OK')"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
