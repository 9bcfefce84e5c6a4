"""vigpol's batch pipeline (vp_process_device, vp_pol.hip) on the directed
traces of pol_cases.py: every batch bit for bit against the oracle (out
ports, frames untouched), the full dump behind every case (alloc and, on live
indices, ts, address, bucket_size, bucket_time), the literals the traces
carry (computed with Python integers, so the tests do not rest on the oracle
alone), and after every batch the phase-T path that produced it, through
vp_last_kernel: run slots, scan + scatter (VIGPATH_POL_RUNS=0) or the sort.
test_pol_edges.py checks on the CPU that each trace reaches what it names.
No tolerance anywhere: the operation is integer.
Reference behaviour: vigpol/policer_main.c:21-145.
"""
import numpy as np
import pytest
import vigor_amd
import pol_cases as P
from gpuh import run_gpu
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu


def make_pair(case, path, monkeypatch):
    """The context (created with the path's switch in the environment: it is
    read once per context) and a fresh oracle."""
    cap, runs_env = P.PATHS[path]
    cap = case.cap or cap
    if runs_env is None:
        monkeypatch.delenv("VIGPATH_POL_RUNS", raising=False)
    else:
        monkeypatch.setenv("VIGPATH_POL_RUNS", runs_env)
    args = ["--lan", str(P.LAN), "--wan", str(P.WAN), "--rate", str(case.rate),
            "--burst", str(case.burst), "--capacity", str(cap)]
    pol = vigor_amd.Pol(vigor_amd.pol_config_from_args(args, P.N_DEV), gpu=0)
    return pol, P.make_oracle(case, cap), cap


def states_equal(pol, oracle, cap):
    """As test_pol_gpu.check_state; returns the GPU's live state."""
    g, o = pol.dump(), oracle.pol_dump(cap)
    np.testing.assert_array_equal(g[0], o[0])
    live = o[0] == 1
    for a, b in zip(g[1:], o[1:]):
        np.testing.assert_array_equal(a[live], b[live])
    return P.live_state(g)


def feed(pol, oracle, case, b, path, cap):
    F, ln, dv, now = b.arrays()
    exp = F.reshape(-1).copy()
    exp_out = oracle.run(exp, ln, dv, now, case.slot)
    before = P.live_state(pol.dump()) if b.unchanged else None
    got, out = run_gpu(pol, F.reshape(-1), ln, dv, now, case.slot)
    what = "%s, %s (%s)" % (case, b.note, path)
    np.testing.assert_array_equal(out, exp_out, "out ports: " + what)
    assert (got == F.reshape(-1)).all() and (exp == got).all(), "frames: " + what
    lit = np.array(b.exp)
    np.testing.assert_array_equal(out[lit >= 0], lit[lit >= 0], "literal ports: " + what)
    assert pol.last_kernel() == P.kernel_name(path, case.slot, b.want), (what, pol.last_kernel())
    if b.live_after or b.unchanged:
        st = states_equal(pol, oracle, cap)
        for k, live in b.live_after.items():
            assert (P.key(k) in st) == live, (what, k)
        if b.unchanged:
            assert st == before and st, what


def run_case(case, path, monkeypatch):
    pol, oracle, cap = make_pair(case, path, monkeypatch)
    assert pol.last_kernel() == ""
    for b in case.batches:
        feed(pol, oracle, case, b, path, cap)
    st = states_equal(pol, oracle, cap)
    for k, v in (case.final or {}).items():
        if v is None:
            assert P.key(k) not in st, (case, k)
        else:  # (every policed packet rejuvenates: the stamp is the bucket's time)
            assert st[P.key(k)][1:] == (v[1], v[0], v[1]), (case, k, st[P.key(k)], v)
    pol.close()
    return st


@pytest.mark.parametrize("slot", [64, 128])
@pytest.mark.parametrize("path", ["runs", "scatter"])
def test_run_lengths(path, slot, monkeypatch):
    """a. Runs of exactly 1, 2, 7, 8 (registers, odd-even sort), 9, 16, 63 and
    64 packets (insertion sort) interleaved in one steady batch; with a run of
    65 added the segment falls back to pol_buckets."""
    run_case(P.run_lengths_case(slot), path, monkeypatch)


@pytest.mark.parametrize("slot", [64, 128])
@pytest.mark.parametrize("path", ["runs", "scatter"])
def test_state_across_segments(path, slot, monkeypatch):
    """b. grouping -> fallback (run of 65) -> grouping with strictly shorter
    runs (stale run slots and counts would show) -> fallback by misses ->
    grouping -> a batch too short to group -> grouping, in one context."""
    run_case(P.state_case(slot), path, monkeypatch)


@pytest.mark.parametrize("case", P.arith_cases(), ids=repr)
@pytest.mark.parametrize("path", ["runs", "scatter", "sort"])
def test_bucket_arithmetic(path, case, monkeypatch):
    """c. The edges of policer_check_tb's arithmetic, each on all three
    phase-T paths (a batch with a miss reports pol_buckets on every one: the
    grouping attempt falls back)."""
    run_case(case, path, monkeypatch)


@pytest.mark.parametrize("case", P.arith_cases(128), ids=repr)
def test_bucket_arithmetic_slot128(case, monkeypatch):
    """c. The same through pol_classify (128-byte slots), on the run slots."""
    run_case(case, "runs", monkeypatch)


@pytest.mark.parametrize("slot", [64, 128])
def test_header_mix(slot, monkeypatch):
    """d. Lengths 0 .. 64 x header variants x input devices in one batch with
    valid traffic around them."""
    run_case(P.header_mix_case(slot), "runs", monkeypatch)


@pytest.mark.parametrize("slot", [64, 128])
def test_expiry_stops_at_last_ipv4(slot, monkeypatch):
    """d. Each variant as the last packet of a batch, an entry's expiry due
    at that packet alone: the entry is gone exactly when the variant parses
    (pol_last_ipv4 against the classify kernel of the slot); a batch without
    any IPv4 frame leaves the table as it was."""
    run_case(P.expiry_edge_case(slot), "runs", monkeypatch)


@pytest.mark.parametrize("path", ["runs", "scatter"])
def test_segment_cut_inside_a_tile(path, monkeypatch):
    """e. An expiry due at packet 70 of 200: the next segment starts inside a
    64-packet tile."""
    run_case(P.segment_cut_case(), path, monkeypatch)


@pytest.mark.parametrize("path", ["runs", "scatter", "sort"])
def test_free_order(path, monkeypatch):
    """f. 40 stamps tied in time by one steady batch, all expired by one
    packet: the addresses by index behind it show the replay's ts / tseq."""
    st = run_case(P.free_order_case(), path, monkeypatch)
    assert len(st) == P.N_FREE


def test_time_going_back_is_not_supported(monkeypatch):
    case = P.Case("backwards")
    pol, _, _ = make_pair(case, "runs", monkeypatch)
    b = case.batch("sort")
    b.add(1, 100, T.NOW0 + 5).pad()
    F, ln, dv, now = b.arrays()
    now[3] -= 1
    with pytest.raises(vigor_amd.VigpathError) as e:
        run_gpu(pol, F.reshape(-1), ln, dv, now, 64)
    assert e.value.rc == vigor_amd.VP_ENOTSUP
