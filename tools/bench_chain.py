"""The firewall -> NAT chain over one device-resident batch: the C-ABI chain
object (vigor_amd.CChain, vp_chain_process_device) beside the Python chain
(vigor_amd.Chain.process_device) on twin contexts, in the same run. Run by
hand; not part of bench.py.

  python3 tools/bench_chain.py [--packets 1048576] [--flows N] [--reps 10]

The batch has bench.py's trace shape: 64-byte slots of LAN packets, `flows`
flows round robin (default: one packet per flow), affine time. Every packet
passes the firewall to its WAN port, crosses the link to the NAT's LAN port and
leaves on the NAT's WAN port, so both stages and the way home see the whole
batch. Both chains get the same batches in the same order, a C call and a
Python call alternating; the tables are warm (two untimed batches each). A
call is timed on the host's clock from its entry to its return -- both return
only after the results are in device memory -- because the host's own work is
what the two differ in. The frames are restored from a pristine copy before
each call, outside the timed region. Per cable ("slots", "stream"): medians,
minima and maxima over `reps` calls. One JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vigor_amd  # noqa: E402
from vigor_amd import traces as T  # noqa: E402

DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
SLOT = 64
EXITS = {(0, 0): 0, (1, 1): 1}
LINKS = [(0, 1, 1, 0)]


def make_stages(flows):
    eth = ["--eth-dest", "0,01:23:45:67:89:00", "--eth-dest", "1,01:23:45:67:89:01"]
    fw = vigor_amd.Fw(vigor_amd.fw_config_from_args(
        ["--wan", "1", "--expire", "60000000", "--max-flows", str(flows)] + eth, 2, DEV_MACS),
        gpu=0)
    nat = vigor_amd.Nat(vigor_amd.nat_config_from_args(
        ["--wan", "1", "--expire", "60000000", "--starting-port", "0", "--max-flows", str(flows),
         "--extip", "192.168.4.2"] + eth, 2, DEV_MACS), gpu=0)
    return [fw, nat]


def stats(ms):
    ms = sorted(ms)
    return {"ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4),
            "ms_max": round(ms[-1], 4)}


def measure(cable, n, flows, reps, dev, pristine, lens):
    c_nfs, p_nfs = make_stages(flows), make_stages(flows)
    c_chain = vigor_amd.CChain(c_nfs, LINKS, cable=cable, exits=EXITS)
    p_chain = vigor_amd.Chain(p_nfs, LINKS, cable=cable, exits=EXITS)
    frames = torch.empty_like(pristine)
    outs = [torch.empty(n, dtype=torch.int16, device=dev) for _ in range(2)]
    times = ([], [])
    last = [None, None]
    for k in range(2 + reps):
        now0 = int(T.NOW0) + k * n
        for which, chain in enumerate((c_chain, p_chain)):
            frames.copy_(pristine)
            outs[which].fill_(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[which] = chain.process_device(frames, lens, 0, outs[which], SLOT, now0=now0,
                                               now_step=1)
            t1 = time.perf_counter()
            if k >= 2:
                times[which].append((t1 - t0) * 1e3)
    # a sanity check of the run, not the test (tests/test_cchain_gpu.py)
    assert last[0] == last[1], (last[0], last[1])
    assert bool((outs[0] == outs[1]).all()) and bool((outs[0] == 1).all())
    r = {"c": stats(times[0]), "python": stats(times[1]), "returned": last[0]["returned"]}
    r["python_over_c"] = round(r["python"]["ms_median"] / r["c"]["ms_median"], 3)
    c_chain.close()
    for nf in c_nfs + p_nfs:
        nf.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--flows", type=int, default=None,
                    help="flows, round robin (default: the packets, one packet per flow; the "
                         "tables hold the next power of two)")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.packets
    flows = args.flows or n
    cap = 1 << max(10, (flows - 1).bit_length())
    fr, ln, _, _ = T.fw_trace(n, flows)
    pristine = torch.from_numpy(fr).to(dev)
    lens = torch.from_numpy(np.ascontiguousarray(ln).view(np.int16)).to(dev)
    line = {"tool": "bench_chain", "chain": "fw -> nat", "packets": n, "flows": flows,
            "slot": SLOT, "reps": args.reps, "version": vigor_amd.lib().vp_version().decode()}
    for cable in ("slots", "stream"):
        line[cable] = measure(cable, n, cap, args.reps, dev, pristine, lens)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
