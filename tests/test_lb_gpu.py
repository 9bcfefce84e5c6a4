"""viglb on the GPU vs the oracle (bit-exact out ports, rewritten frames,
flow and backend state).

Every test calls the product through the C-ABI (libvigpath.so via
vigor_amd); the oracle (oracle/liborc.so) is only the checker.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import vigor_amd
from gpuh import check_batches, run_gpu
from tracegen import edge_lb_trace, mixed_lb_trace, wide_lb_trace
from vigor_amd import traces as T

pytestmark = pytest.mark.gpu

DEV_MACS = [bytes([0x10 * d + i for i in range(6)]) for d in range(3)]


def make_pair(flow_cap=1024, bcap=32, height=97, fexp=60_000_000,
              bexp=3_600_000_000, wan=2, n_dev=3):
    args = ["--flow-capacity", str(flow_cap), "--backend-capacity", str(bcap),
            "--cht-height", str(height), "--flow-expiration", str(fexp),
            "--backend-expiration", str(bexp), "--wan", str(wan)]
    cfg = vigor_amd.lb_config_from_args(args, n_dev, DEV_MACS[:n_dev])
    gpu = vigor_amd.Lb(cfg, gpu=0)
    ocfg = orc.LbCfg(flow_capacity=flow_cap, flow_expiration_time=fexp,
                     backend_capacity=bcap, cht_height=height,
                     backend_expiration_time=bexp, wan_device=wan,
                     n_devices=n_dev)
    for d in range(n_dev):
        ocfg.device_macs[d][:] = list(DEV_MACS[d])
    return gpu, orc.Oracle("lb", ocfg)


def check_state(lb, oracle):
    g = lb.dump()
    o = oracle.lb_dump(lb.cfg.flow_capacity, lb.cfg.backend_capacity)
    for x, y in zip(g, o):  # flows, then backends
        np.testing.assert_array_equal(x[0], y[0])
        live = y[0] == 1
        for a, b in zip(x[1:], y[1:]):
            np.testing.assert_array_equal(a[live], b[live])


def concat(*traces):
    return tuple(np.concatenate(x) for x in zip(*traces))


def test_config4_heartbeats_then_traffic():
    lb, o = make_pair(flow_cap=4096, bcap=256, height=257)
    hb = T.lb_heartbeats(256)
    tr = T.lb_traffic(30_000, 3000)
    fr, ln, dv, now = concat(hb, tr)
    check_batches(lb, o, fr, ln, dv, now, 64, [100, 256, 5000])
    check_state(lb, o)


@pytest.mark.parametrize("seed,fcap,fexp,bexp,quiet,cuts", [
    (0, 1024, 60_000_000, 3_600_000, None, [100, 2000]),   # steady + hb mix
    (1, 64, 60_000_000, 3_600_000, None, [2500]),          # flow table full
    (2, 256, 2, 3_600_000, None, [1, 2, 500, 4000]),       # flow expiry
    (3, 1024, 60_000_000, 2, (1000, 3500), [1500, 3600]),  # backends die
    (4, 1024, 3, 2, (500, 4500), []),                      # both, one batch
])
def test_mixed_traces(seed, fcap, fexp, bexp, quiet, cuts):
    rng = np.random.default_rng(seed)
    fr, ln, dv, now = mixed_lb_trace(rng, 6000, 300, 20, quiet=quiet)
    lb, o = make_pair(flow_cap=fcap, fexp=fexp, bexp=bexp)
    check_batches(lb, o, fr, ln, dv, now, 64, cuts)
    check_state(lb, o)


def test_burst_port():
    """vp_dev_batch.in_port: bursts of heartbeats (LAN ports) and WAN
    traffic, each passed with its one port instead of a port array (the
    64-byte tile and the queue rounds read it), state compared at the end."""
    rng = np.random.default_rng(31)
    fr, ln, dv, now = mixed_lb_trace(rng, 3000, 200, 20)
    cuts = [i for i in range(1, len(dv)) if dv[i] != dv[i - 1]]
    lb, o = make_pair(flow_cap=256, fexp=40)
    check_batches(lb, o, fr, ln, dv, now, 64, cuts, one_port=True)
    check_state(lb, o)


def test_backend_table_full_and_generic_slots():
    rng = np.random.default_rng(8)
    fr, ln, dv, now = mixed_lb_trace(rng, 4000, 200, 40, hb_frac=0.1,
                                     slot=128)
    lb, o = make_pair(bcap=16, height=17)
    check_batches(lb, o, fr, ln, dv, now, 128, [333, 2000])
    check_state(lb, o)


def test_config4_256_backends_1m_flows_full_size():
    """BASELINE config 4 at full size: 256 backends, CHT height 257, flow
    capacity 2^20, 1M flows."""
    nf = 1 << 20
    lb, o = make_pair(flow_cap=nf, bcap=256, height=257)
    hb = T.lb_heartbeats(256)
    exp = hb[0].copy()
    exp_out = o.run(exp, hb[1], hb[2], hb[3], 64)
    got, out = run_gpu(lb, *hb, 64)
    assert np.array_equal(out, exp_out) and np.array_equal(got, exp)
    B = 1 << 21
    for j in range(2):
        fr, ln, dv, now = T.lb_traffic(B, nf, start=j * B)
        exp = fr.copy()
        exp_out = o.run(exp, ln, dv, now, 64)
        got, out = run_gpu(lb, fr, ln, dv, now, 64, affine=(int(now[0]), 1))
        assert np.array_equal(out, exp_out)
        assert orc.digest(got, 64, ln, out) == orc.digest(exp, 64, ln, exp_out)
    assert lb.live_count() == nf + 256


def test_rejects_bad_config():
    with pytest.raises(vigor_amd.VigpathError):
        make_pair(height=96)  # not prime
    with pytest.raises(vigor_amd.VigpathError):
        make_pair(bcap=128, height=97)  # backends >= height
    with pytest.raises(vigor_amd.VigpathError):
        make_pair(flow_cap=1000)


def test_stale_frees_keep_shard_count():
    """Flows whose backend died while no backend is alive are erased and
    their indices freed (lb_stale_free_seq) — cycle after cycle. The bucket
    bookkeeping must follow (shard_live == live: the layout and rebuild
    checks count it), so the table does not rebuild on every check; outputs
    and state equal the oracle's throughout."""
    nb, nfl = 20, 200
    lb, o = make_pair(flow_cap=256, bexp=5_000)  # backends expire after 5 ms
    for c in range(12):
        t = T.NOW0 + c * 10_000_000
        stale = T.lb_traffic(nfl, nfl)            # backends expired: stale frees
        hb = T.lb_heartbeats(nb, t0=t + 1_000)
        fresh = T.lb_traffic(2 * nfl, nfl)        # re-balanced, new indices
        stale = stale[:3] + (t + np.arange(nfl, dtype=np.int64),)
        fresh = fresh[:3] + (t + 2_000 + np.arange(2 * nfl, dtype=np.int64),)
        fr, ln, dv, now = concat(stale, hb, fresh)
        check_batches(lb, o, fr, ln, dv, now, 64, [nfl + 7])
        st = lb.table_stats(0)
        assert st["shard_live"] == st["live"], (c, st)
    check_state(lb, o)
    assert lb.table_stats(0)["rebuilds"] <= 4, lb.table_stats(0)


@pytest.mark.parametrize("slot,max_len", [(80, 80), (128, 128), (256, 256), (1536, 1518),
                                          (2048, 1518)])
def test_wide_slots(slot, max_len):
    """Frames of 60..1518 bytes in wide slots (lb_classify, set_checksums'
    raw_sum over real payload): TCP and UDP, odd lengths, frames padded past
    total_length, heartbeats mixed in, malformed frames, flows that expire
    and return; several batches, one cut at packet 1."""
    rng = np.random.default_rng(slot)
    fr, ln, dv, now = wide_lb_trace(rng, 3000, 200, 12, slot, max_len=max_len)
    now = T.NOW0 + (now - T.NOW0) * 5
    lb, o = make_pair(flow_cap=256, fexp=1)  # (1 us: some 200 packets of the trace)
    check_batches(lb, o, fr, ln, dv, now, slot, [1, 700, 2100])
    assert (o.lb_dump(256, 32)[0][0] == 1).sum() < 200  # (some flows are gone)
    check_state(lb, o)


@pytest.mark.parametrize("slot,long_frames", [(64, False), (128, False), (256, True)])
def test_header_edge_cases(slot, long_frames):
    """edge_lb_trace: IPv4 options (a TCP checksum as far out as bytes 90-91),
    IHL < 5, total_length below 20 and past the frame, frames shorter than
    their headers or than 14 bytes, on WAN packets and heartbeats. In 64-byte
    slots they take the tile kernel's byte path (LbPend.kind 1), in wide slots
    parse_l34."""
    rng = np.random.default_rng(100 + slot)
    fr, ln, dv, now = edge_lb_trace(rng, 3000, 100, 12, slot, long_frames=long_frames)
    now = T.NOW0 + (now - T.NOW0) * 10
    lb, o = make_pair(flow_cap=256, bexp=1)  # (1 us: some 100 packets of the trace)
    check_batches(lb, o, fr, ln, dv, now, slot, [1, 900])
    if slot == 64:
        assert lb.last_kernel().startswith("lb_classify64"), lb.last_kernel()
    check_state(lb, o)


def beyond_the_lds_stage(want_kernel):
    """bcap 512 (above kLbLdsBackends: the tile kernel stages no backend in
    LDS), CHT height 521: 400 heartbeats, 2000 flows twice (the second batch
    all hits: lb_flow_found -> lb_rewrite_fast reads be_rec from global
    memory), then the backends expire, the flows go stale, and heartbeats
    and traffic come again."""
    nb, nfl, bexp_us = 400, 2000, 1000
    lb, o = make_pair(flow_cap=4096, bcap=512, height=521, bexp=bexp_us)
    hb = T.lb_heartbeats(nb)
    tr = T.lb_traffic(nfl, nfl)
    t1 = T.NOW0 + 5 * bexp_us * 1000  # (every backend has expired)
    at = lambda t: (t + np.arange(nfl, dtype=np.int64),)  # noqa: E731
    segs = [hb, tr, tr[:3] + at(T.NOW0 + 10_000),
            tr[:3] + at(t1),                       # no backend alive: dropped, erased
            T.lb_heartbeats(nb // 2, t0=t1 + 5_000),
            tr[:3] + at(t1 + 10_000), tr[:3] + at(t1 + 20_000)]
    for k, (fr, ln, dv, now) in enumerate(segs):
        exp = fr.copy()
        exp_out = o.run(exp, ln, dv, now, 64)
        got, out = run_gpu(lb, fr, ln, dv, now, 64)
        np.testing.assert_array_equal(out, exp_out, "out ports, segment %d" % k)
        np.testing.assert_array_equal(got, exp, "frames, segment %d" % k)
        assert lb.last_kernel() == want_kernel, lb.last_kernel()
        if k == 2:  # the all-hit batch: forwarded, and to backends past 255
            assert (exp_out != 2).all()
            (fa, _, _, fb), _ = o.lb_dump(4096, 512)
            assert ((fa == 1) & (fb >= 256)).sum() >= 100
        if k == 3:
            assert (exp_out == 2).all()
    check_state(lb, o)


def test_backends_beyond_the_lds_stage():
    beyond_the_lds_stage("lb_classify64")


def test_backends_beyond_the_lds_stage_16_waves():
    """The same through lb_classify64w (VIGPATH_LB_WAVES=16, read once per
    process: a fresh child)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VIGPATH_LB_WAVES="16")
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    code = "import test_lb_gpu as M; M.beyond_the_lds_stage('lb_classify64w'); print('CHILD OK')"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
