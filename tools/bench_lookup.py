#!/usr/bin/env python3
"""vp_table_lookup / vp_table_entries of vignat at 1M live flows (BASELINE
config 1's table): lookup_device of 2^10, 2^16 and 2^20 keys -- all hits in
random order, then all misses -- and entries_device of as many random live
indices, every output array asked for. Wall time around the call in ms,
medians of 10 with min-max. The yardsticks, in the same run: a plain
device-to-device copy of as many bytes as the call's arrays hold (what it
reads plus what it writes: 44 bytes per key, 32 per index) on the stream the
call runs on, and save_state of the whole table. No threshold is set. One
JSON line per query count.

  python tools/bench_lookup.py [--flows 1048576] [--queries Q] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vigor_amd  # noqa: E402
from vigor_amd import traces as T  # noqa: E402

DEV_MACS = [T.mac("02:03:04:05:06:07"), T.mac("12:13:14:15:16:17")]
NAT_ARGS = ["--wan", "1", "--expire", "60000000", "--starting-port", "0", "--extip",
            "192.168.4.2", "--eth-dest", "0,01:23:45:67:89:00", "--eth-dest",
            "1,01:23:45:67:89:01"]


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, default=0, help="one query count (default: 2^10, 2^16, 2^20)")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    cfg = vigor_amd.nat_config_from_args(NAT_ARGS + ["--max-flows", str(a.flows)], 2, DEV_MACS)
    nat = vigor_amd.Nat(cfg, gpu=0)
    d = torch.device("cuda:0")
    step = 1 << 18
    for s in range(0, a.flows, step):  # every flow once: the table full of live flows
        n = min(step, a.flows - s)
        fr, ln, dv, now = T.nat_lan_trace(n, a.flows, start=s)
        nat.process_device(torch.from_numpy(fr).to(d), torch.from_numpy(ln.view(np.int16)).to(d),
                           torch.from_numpy(dv.view(np.int16)).to(d),
                           torch.zeros(n, dtype=torch.int16, device=d), 64,
                           now=torch.from_numpy(now).to(d))
    torch.cuda.synchronize()
    assert nat.live_count() == a.flows
    save = timed(nat.save_state, a.reps)
    image_bytes = len(nat.save_state())
    # every live key, from the table itself
    all_idx = torch.arange(a.flows, dtype=torch.int32, device=d)
    live_keys = torch.empty(a.flows * 16, dtype=torch.uint8, device=d)
    nat.entries_device(all_idx, key=live_keys)
    live_keys = live_keys.view(a.flows, 16)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    st = torch.cuda.Stream()
    sp = C.c_void_p(st.cuda_stream)
    gen = torch.Generator(device="cpu").manual_seed(7)
    for q in ([a.queries] if a.queries else [1 << 10, 1 << 16, 1 << 20]):
        pick = torch.randint(0, a.flows, (q,), generator=gen).to(d)
        hits = live_keys[pick].contiguous().view(-1)
        miss = live_keys[pick].clone()
        miss[:, 8:12] = 0xFF  # (no flow of the trace has this destination address)
        miss = miss.contiguous().view(-1)
        idx = pick.to(torch.int32)
        index = torch.empty(q, dtype=torch.int32, device=d)
        ts = torch.empty(q, dtype=torch.int64, device=d)
        key = torch.empty(q * 16, dtype=torch.uint8, device=d)
        look = lambda k: nat.lookup_device(k, index=index, ts=ts, key=key, stream=st)  # noqa: E731
        torch.cuda.synchronize()  # (the queries were built on another stream than st)
        look(hits)
        assert bool((index == idx).all()) and bool((key == hits).all())
        look(miss)
        assert bool((index == -1).all()) and not bool(key.any()) and not bool(ts.any())
        nat.entries_device(idx, index=index, ts=ts, key=key, stream=st)
        assert bool((index == idx).all()) and bool((key == hits).all())
        t_hit = timed(lambda: look(hits), a.reps)
        t_miss = timed(lambda: look(miss), a.reps)
        t_ent = timed(lambda: nat.entries_device(idx, index=index, ts=ts, key=key, stream=st),
                      a.reps)
        res = {"tool": "bench_lookup", "nf": "vignat", "flows": a.flows, "queries": q,
               "reps": a.reps, "lookup_hits_ms": stats(t_hit), "lookup_misses_ms": stats(t_miss),
               "entries_ms": stats(t_ent)}
        for name, per in (("copy_d2d_44B_per_key_ms", 44), ("copy_d2d_32B_per_index_ms", 32)):
            src = torch.empty(q * per, dtype=torch.uint8, device=d)
            dst = torch.empty(q * per, dtype=torch.uint8, device=d)

            def copy():
                assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                          q * per, 3, sp) == 0  # hipMemcpyDeviceToDevice
                assert hip.hipStreamSynchronize(sp) == 0
            copy()
            res[name] = stats(timed(copy, a.reps))
        res["save_state_ms"] = stats(save)
        res["image_bytes"] = image_bytes
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
