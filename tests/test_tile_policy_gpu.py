"""The cache policy of vignat's 64-byte tile stream (tile_policy, vp_device.h)
against the oracle, byte for byte: the default policy and the one switch value
that stays, VIGPATH_TILE_POLICY=0 (the policy from before the ladder, reported
as nat_classify64w_pp / nat_classify64ws_pp). The switch is read once per
process, so each case runs in a fresh child (as test_nat_switches_gpu does),
with the resident small-burst kernel off (VIGPATH_SERVE=0) so that batches of
one tile take the tile kernel too. No tolerance: the operation is integer.

vp_probe_slots_p (the bare pass the policies were measured with) is checked in
this process: an unknown policy value is VP_EINVAL, and every policy pair
leaves a 64-tile buffer as it was.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tracegen import lan_tile_trace

pytestmark = pytest.mark.gpu

MAX_FLOWS = 8192
LOADS = (0, 2, 16, 17)   # plain, nt, sc1, sc0 sc1
STORES = (16, 18, 2, 0)  # sc1, sc1 nt, nt, plain
VP_EINVAL = -22


def _tile_kernel(nat):
    want = "_pp" if os.environ.get("VIGPATH_TILE_POLICY") == "0" else ""
    k = nat.last_kernel()
    assert k in ("nat_classify64w" + want, "nat_classify64ws" + want), k


def _lan(seed, n, flows=40):
    """n LAN packets over `flows` flows, every tile a lean one."""
    return lan_tile_trace(np.random.default_rng(seed), n, flows, bad_tiles=0.0)


def case_sizes(n):
    """One batch of n packets over new flows (lean tiles whose misses are
    stored unchanged and rewritten by phase B), then the same flows again
    (hits, rewritten in the tile)."""
    from gpuh import check_batches
    from test_nat_gpu import check_state, make_pair

    nat, o = make_pair(max_flows=MAX_FLOWS)
    fr, ln, dv, now = _lan(3, n)
    check_batches(nat, o, fr, ln, dv, now, 64, [])
    _tile_kernel(nat)
    fr, ln, dv, now2 = _lan(3, n)
    check_batches(nat, o, fr, ln, dv, now2 + (now[-1] - now2[0]) + 1, 64, [])
    _tile_kernel(nat)
    check_state(nat, o, MAX_FLOWS)


def case_mixed():
    """Six tiles: one WAN packet in tile 1 and one non-IPv4 frame in tile 3
    send those tiles down the per-lane path between lean tiles."""
    from gpuh import check_batches
    from test_nat_gpu import check_state, make_pair

    nat, o = make_pair(max_flows=MAX_FLOWS)
    fr, ln, dv, now = _lan(5, 64 * 6)
    check_batches(nat, o, fr, ln, dv, now, 64, [])  # (the flows: hits below)
    fr, ln, dv, now2 = _lan(5, 64 * 6)
    f2 = fr.reshape(-1, 64)
    dv[64 + 17] = 1          # arrives on the WAN port
    f2[3 * 64 + 40, 12] = 0x86  # not IPv4
    check_batches(nat, o, f2.reshape(-1), ln, dv, now2 + (now[-1] - now2[0]) + 1, 64, [])
    _tile_kernel(nat)
    check_state(nat, o, MAX_FLOWS)


def case_unaligned_segment():
    """Flows that expire at packet 100 of the next batch (its time jumps past
    their expiry there) cut it into the segments [0, 100) and [100, n): the
    second one's p0 is no multiple of 64, its first tile starts at packet 64."""
    from gpuh import check_batches
    from test_nat_gpu import check_state, make_pair

    expire = 1000
    nat, o = make_pair(max_flows=MAX_FLOWS, expire_us=expire)
    fr, ln, dv, now = _lan(7, 64 * 5)
    check_batches(nat, o, fr, ln, dv, now, 64, [])
    live = nat.live_count()
    fr, ln, dv, _ = _lan(8, 64 * 5 + 9, flows=60)
    t = now[-1] + 1 + np.arange(ln.shape[0], dtype=np.int64) // 8
    t[100:] += 5 * expire
    assert t[-1] - t[100] < expire  # no later cut
    check_batches(nat, o, fr, ln, dv, t, 64, [])
    _tile_kernel(nat)
    check_state(nat, o, MAX_FLOWS)
    assert 30 < live <= 40 and nat.live_count() <= 60  # (the first call's flows expired)


def case_twice():
    """The same device buffer processed twice. The first call allocates the
    flows (the tile stores the misses unchanged, phase B rewrites them); the
    second call reads what the first left: frames whose source is now the
    external address, new flows of their own."""
    import torch

    from test_nat_gpu import check_state, make_pair

    nat, o = make_pair(max_flows=MAX_FLOWS)
    n = 64 * 9 + 5
    fr, ln, dv, now = _lan(11, n, flows=200)
    d = torch.device("cuda:0")
    f = torch.from_numpy(fr.copy()).to(d)
    l_ = torch.from_numpy(ln.astype(np.uint16).view(np.int16)).to(d)
    i_ = torch.from_numpy(dv.astype(np.uint16).view(np.int16)).to(d)
    exp = fr.copy()
    for k in range(2):
        t = now + k * (now[-1] - now[0] + 1)
        exp_out = o.run(exp, ln, dv, t, 64)
        out = torch.zeros(n, dtype=torch.int16, device=d)
        nat.process_device(f, l_, i_, out, 64, now=torch.from_numpy(t).to(d))
        torch.cuda.synchronize()
        _tile_kernel(nat)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), exp_out), k
        bad = np.nonzero((f.cpu().numpy().reshape(n, 64) != exp.reshape(n, 64)).any(axis=1))[0]
        assert bad.size == 0, (k, bad[:10])
    check_state(nat, o, MAX_FLOWS)
    assert nat.live_count() > 200  # (the second call's flows are new ones)


def case_long_ranges():
    """Every CU's block with 20 tiles (some waves a second, prefetched tile),
    lean, per-lane and mixed tiles, a clipped last block and a partial last
    tile: test_nat_switches_gpu's batch under this policy."""
    import test_nat_switches_gpu as M

    want = "_pp" if os.environ.get("VIGPATH_TILE_POLICY") == "0" else ""
    M.child("nat_classify64w" + want)


CASES = {
    "n64": (case_sizes, 64),           # one whole tile
    "n63": (case_sizes, 63),           # the guarded partial-tile loads
    "n65": (case_sizes, 65),           # a whole tile and one packet
    "n1089": (case_sizes, 64 * 17 + 1),  # two blocks of nine tiles, a ragged end
    "mixed": (case_mixed,),
    "unaligned_segment": (case_unaligned_segment,),
    "twice": (case_twice,),
    "long_ranges": (case_long_ranges,),
}


def child(name):
    fn, *args = CASES[name]
    fn(*args)


@pytest.mark.parametrize("policy", [None, "0"], ids=["default", "parent"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_tile_policy_matches_oracle(case, policy):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for v in ("VIGPATH_TILE_POLICY", "VIGPATH_SPLIT", "VIGPATH_BLOCK_WAVES"):
        env.pop(v, None)
    if policy is not None:
        env["VIGPATH_TILE_POLICY"] = policy
    env["VIGPATH_SERVE"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    code = "import test_tile_policy_gpu as M; M.child(%r); print('CHILD DONE')" % case
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "CHILD DONE" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def _probe(buf, n, store, waves, lp, sp):
    import vigor_amd

    ms = ctypes.c_float(-1.0)
    rc = vigor_amd.lib().vp_probe_slots_p(ctypes.c_void_p(buf.data_ptr()), n, 64, store, waves,
                                          lp, sp, 1, ctypes.byref(ms))
    return rc, ms.value


def test_probe_rejects_unknown_policy():
    import torch

    n = 64 * 64
    buf = torch.zeros(n * 64, dtype=torch.uint8, device="cuda:0")
    for lp, sp in ((1, 16), (3, 16), (18, 16), (-1, 16), (32, 16),
                   (0, 1), (0, 17), (0, 3), (2, -2), (2, 64)):
        rc, ms = _probe(buf, n, 1, 16, lp, sp)
        assert rc == VP_EINVAL and ms == -1.0, (lp, sp, rc)
    # pairs other than the tile kernels' own: 64-byte slots at 4 or 16 waves only
    assert _probe(buf, n, 1, 8, 17, 0)[0] == VP_EINVAL
    assert _probe(buf, n, 1, 16, 2, 18)[0] == 0


@pytest.mark.parametrize("waves", [16, 4])
def test_probe_leaves_the_buffer_unchanged(waves):
    import torch

    n = 64 * 64  # 64 tiles
    rng = np.random.default_rng(13)
    ref = rng.integers(0, 256, n * 64, dtype=np.uint8)
    buf = torch.from_numpy(ref).to("cuda:0")
    for lp in LOADS:
        for sp in STORES:
            for store in (1, 0):
                rc, ms = _probe(buf, n, store, waves, lp, sp)
                assert rc == 0 and ms > 0, (lp, sp, store, rc)
            torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), ref), (lp, sp)
