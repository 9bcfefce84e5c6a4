"""vp_tx_build over one headline-sized batch: the time of its three launches
beside the bytes the algorithm has to move. Run by hand; not part of bench.py.

  python3 tools/bench_tx.py [--packets 16777216] [--reps 20] [--step-ms MS]

Three cases:
  two-port         vignat's headline outputs: every packet from port 0 (one
                   port per burst, vp_dev_batch.in_port) to port 1
  two-port-drop16  the same with one packet in 16 dropped (out == in)
  four-port-flood  vigbridge with 4 devices over its flood pattern
                   (traces.bridge_trace(..., flood_pattern=True)): the out
                   ports of a 2^20-packet trace through vp_process_device,
                   repeated to the batch size, with the trace's port array

Algorithmic bytes: two passes (tx_count, tx_scatter) over out_dev, the port
array and len, 6 B per packet (4 B with in_port: no port array), plus 4 B per
list entry written. (tx_scatter does not read len, so the figure is an upper
bound of what the kernels request.) Each call is timed between two events on
the stream it is enqueued on, the calls back to back.
--step-ms: the headline step (bench.py's ms_per_step of the same session);
every time is then also given as a fraction of it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vigor_amd  # noqa: E402
from vigor_amd import traces as T  # noqa: E402


def dev16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).to(dev)


def bridge_flood_outputs(n, dev):
    """(out, in_dev, len) device tensors of n packets: vigbridge (4 devices)
    over its flood pattern, a 2^20-packet trace repeated."""
    base = min(n, 1 << 20)
    cfg = vigor_amd.bridge_config_from_args(["--capacity", "65536"], 4)
    br = vigor_amd.Bridge(cfg, gpu=dev.index or 0)
    fr, ln, dv, now = T.bridge_trace(base, 32768, flood_pattern=True)
    f_t = torch.from_numpy(fr).to(dev)
    l_t, i_t = dev16(ln, dev), dev16(dv, dev)
    o_t = torch.zeros(base, dtype=torch.int16, device=dev)
    br.process_device(f_t, l_t, i_t, o_t, 64, now0=int(now[0]), now_step=1)
    torch.cuda.synchronize()
    br.close()
    reps = (n + base - 1) // base
    return tuple(t.repeat(reps)[:n].contiguous() for t in (o_t, i_t, l_t))


def measure(nf, nd, out, in_dev, lens, reps, dev):
    n = out.numel()
    off = torch.zeros(nd + 1, dtype=torch.int32, device=dev)
    st = torch.zeros(C.sizeof(vigor_amd.TxStatsC), dtype=torch.uint8, device=dev)
    nf.tx_build(out, in_dev, lens, None, off, st)  # the total, to size idx
    torch.cuda.synchronize()
    total = int(off.cpu().numpy().view(np.uint32)[nd])
    idx = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with torch.cuda.stream(s):
        for _ in range(3):
            nf.tx_build(out, in_dev, lens, idx, off, st, stream=s)
        ev[0].record(s)
        for k in range(reps):
            nf.tx_build(out, in_dev, lens, idx, off, st, stream=s)
            ev[k + 1].record(s)
    s.synchronize()
    ms = sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))
    words = st.cpu().numpy().view(np.uint64)
    per_pkt = 4 if isinstance(in_dev, int) else 6
    alg = 2 * per_pkt * n + 4 * total
    return {"packets": n, "n_devices": nd, "entries": total,
            "dropped": int(words[64]), "flooded": int(words[65]),
            "ms_median": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4),
            "ms_max": round(ms[-1], 4), "reps": reps,
            "alg_bytes": alg, "alg_bytes_per_packet": round(alg / max(n, 1), 2),
            "alg_gb_per_s": round(alg / (ms[len(ms) // 2] * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=None,
                    help="the headline step of the same session (bench.py ms_per_step)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.packets
    macs = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
    nat = vigor_amd.Nat(vigor_amd.nat_config_from_args(
        ["--wan", "1", "--max-flows", "1024", "--extip", "192.168.4.2"], 2, macs), gpu=0)
    br4 = vigor_amd.Bridge(vigor_amd.bridge_config_from_args([], 4), gpu=0)
    lens = torch.full((n,), 60, dtype=torch.int16, device=dev)
    out1 = torch.ones(n, dtype=torch.int16, device=dev)
    out2 = out1.clone()
    out2[::16] = 0
    cases = [("two-port", nat, 2, out1, 0, lens),
             ("two-port-drop16", nat, 2, out2, 0, lens),
             ("four-port-flood", br4, 4) + bridge_flood_outputs(n, dev)]
    for name, nf, nd, out, in_dev, ln in cases:
        r = {"case": name, **measure(nf, nd, out, in_dev, ln, args.reps, dev)}
        if args.step_ms:
            r["headline_step_ms"] = args.step_ms
            r["fraction_of_step"] = round(r["ms_median"] / args.step_ms, 4)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
