"""The two path-selecting switches vignat's classify keeps, each against the
oracle: VIGPATH_SPLIT (2, 4: the 1024-thread tile's block range cut into
sub-ranges, nat_classify64w) and VIGPATH_BLOCK_WAVES=4 (the 256-thread tile,
nat_classify64). Both are read once per process, so each case runs in a fresh
child (as test_bridge_edges_gpu.test_sixteen_waves does); the child compares
out ports, every frame byte and the dumped table with the oracle and asserts
the kernel through vp_last_kernel. No tolerance: the operation is integer.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tracegen import lan_tile_trace, mixed_nat_trace

pytestmark = pytest.mark.gpu

MAX_FLOWS = 8192
N_HOT = 63  # flows of the setup call: below one tile, so it leaves the
            # kernel choice (run tiles seen) as a new context has it


PER_B = 20  # tiles per block of the 1024-thread kernel's grid


def batch_size(cus):
    """A batch whose 1024-thread classify launch (nat_segment's layout) has
    every CU's block own PER_B tiles but the last, one short, with a partial
    last tile: tiles = PER_B cus - 1. The grid is resident_grid's
    min(ceil(tiles / 16), cus blocks) = cus, one block per CU; a block owns
    per_b = ceil(tiles / grid) = PER_B tiles and, at split k, sub-range s the
    tiles [s per_s, min(per_b, (s + 1) per_s)) of them, per_s = ceil(per_b /
    k), with 16 / k waves interleaved over it. PER_B = 20 is the least
    multiple of 4 with per_s > 16 / k for k = 1, 2 and 4 (20 > 16, 10 > 8, 5 >
    4), so under every split some wave of every sub-range takes a second tile
    (the `tile += tstep` step and the next tile's prefetch); the last block
    owns 19 tiles, at split 4 in sub-ranges of 5, 5, 5 and 4 with its end
    clipped (tend)."""
    tiles = PER_B * cus - 1
    return (tiles - 1) * 64 + 37


def layout(n, cus, split):
    """nat_segment's and nat_tiles' arithmetic for n packets from packet 0:
    (grid, per_b, per_s, tiles of the last block's last sub-range)."""
    tiles = (n + 63) // 64
    grid = min((tiles + 15) // 16, cus)
    per_b = (tiles + grid - 1) // grid
    per_s = (per_b + split - 1) // split
    last = tiles - (grid - 1) * per_b
    return grid, per_b, per_s, min(last, split * per_s) - (split - 1) * per_s


def trace(n):
    """One batch of n packets over a few thousand flows: tiles of LAN-only
    traffic (lean tiles, a tenth with one malformed packet) interleaved at
    random with tiles of mixed LAN / WAN traffic, half of the LAN-only tiles'
    packets from the N_HOT flows the setup call allocated (hits beside the
    misses of flows first seen anywhere in the batch, so in every sub-range),
    and WAN replies to indices in and beyond the allocated ones."""
    rng = np.random.default_rng(29)
    fa, la, da, _ = lan_tile_trace(rng, n, 3000)
    fh, lh, dh, _ = lan_tile_trace(rng, n, N_HOT, bad_tiles=0.0)
    fb, lb, db, now = mixed_nat_trace(rng, n, 2500, max_idx=MAX_FLOWS)
    fa, fh, fb = fa.reshape(n, 64), fh.reshape(n, 64), fb.reshape(n, 64)
    hot = rng.random(n) < 0.5
    fa[hot], la[hot], da[hot] = fh[hot], lh[hot], dh[hot]
    mixed = np.repeat(rng.random((n + 63) // 64) < 0.3, 64)[:n]
    fa[mixed], la[mixed], da[mixed] = fb[mixed], lb[mixed], db[mixed]
    return fa.reshape(-1), la, da, now


def child(kernel):
    """In the child, with the switch in the environment."""
    import torch

    import vigor_amd
    from gpuh import check_batches
    from test_nat_gpu import check_state, make_pair

    split = int(os.environ.get("VIGPATH_SPLIT", "1"))
    # one 1024-thread block per CU (nat_classify64w: __launch_bounds__(1024, 1)
    # and 89 KB of LDS), which resident_grid caps at the launch's work blocks
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = batch_size(cus)
    for k in (1, 2, 4):
        grid, per_b, per_s, last = layout(n, cus, k)
        assert grid == cus and per_b == PER_B and per_s > 16 // k and last >= 2, (k, grid, per_b)
    assert n % 64 and (n + 63) // 64 < cus * PER_B  # a partial tile; tend clips
    nat, o = make_pair(max_flows=MAX_FLOWS)
    rng = np.random.default_rng(7)
    fr, ln, dv, now = lan_tile_trace(rng, 4096, N_HOT, bad_tiles=0.0)
    first = np.unique(fr.reshape(-1, 64), axis=0, return_index=True)[1]
    first = np.sort(first)[:N_HOT]
    assert first.size == N_HOT
    fr = fr.reshape(-1, 64)[first].reshape(-1)
    check_batches(nat, o, fr, ln[first], dv[first], now[first], 64, [])
    fr, ln, dv, now2 = trace(n)
    check_batches(nat, o, fr, ln, dv, now2 + (now[-1] - now2[0]) + 1, 64, [])
    assert nat.last_kernel() == kernel, (nat.last_kernel(), split)
    check_state(nat, o, MAX_FLOWS)
    live = nat.live_count()
    assert 3000 < live < MAX_FLOWS, live  # (new flows; the table never full)
    print("CHILD OK", vigor_amd.lib().vp_version().decode())


@pytest.mark.parametrize("var,val,kernel", [
    ("VIGPATH_SPLIT", "2", "nat_classify64w"),
    ("VIGPATH_SPLIT", "4", "nat_classify64w"),
    ("VIGPATH_BLOCK_WAVES", "4", "nat_classify64"),
])
def test_switch_matches_oracle(var, val, kernel):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("VIGPATH_SPLIT", None)
    env.pop("VIGPATH_BLOCK_WAVES", None)
    env[var] = val
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] +
                                        [p for p in [env.get("PYTHONPATH")] if p])
    code = "import test_nat_switches_gpu as M; M.child(%r); print('CHILD DONE')" % kernel
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "CHILD DONE" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
