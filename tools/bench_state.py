#!/usr/bin/env python3
"""vp_state_save / vp_state_load of vignat at 1M live flows (BASELINE config
1's table) beside plain hipMemcpy of the same number of bytes in each
direction on the same stream: medians of 10 with min-max, wall time in ms.
One JSON line. The copies are the yardstick; no threshold is set.

  python tools/bench_state.py [--flows 1048576] [--reps 10]

--delta: after that, per share of the flows (1 %, 10 %, 100 %): mark, touch
that share in one batch, then save_delta on the primary and apply_delta on a
twin that follows it, beside plain copies of the delta's bytes each way. The
twin is brought back to the mark by load_state and follow before every
apply; that is outside the timed region. One more JSON line per share.

  python tools/bench_state.py --delta [--flows 1048576] [--reps 10]
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
    return {"median": round(float(np.median(ms)), 3), "min": round(min(ms), 3),
            "max": round(max(ms), 3)}


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--delta", action="store_true")
    a = ap.parse_args()
    cfg = vigor_amd.nat_config_from_args(NAT_ARGS + ["--max-flows", str(a.flows)], 2, DEV_MACS)
    nat = vigor_amd.Nat(cfg, gpu=0)
    twin = vigor_amd.Nat(cfg, gpu=0)
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
    img = nat.save_state()
    twin.load_state(img)
    assert twin.save_state() == img
    save = timed(nat.save_state, a.reps)
    load = timed(lambda: twin.load_state(img), a.reps)
    layout = twin.table_stats()["layout"]
    # the yardstick: one plain copy of as many bytes, pageable host memory as
    # the calls' buffers are, on a stream of its own kind
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    st = torch.cuda.Stream()
    host = np.frombuffer(img, np.uint8).copy()
    devbuf = torch.empty(len(img), dtype=torch.uint8, device=d)
    sp, hp, dp = C.c_void_p(st.cuda_stream), C.c_void_p(host.ctypes.data), C.c_void_p(devbuf.data_ptr())

    def copy(dst, src, kind, nbytes=len(img)):
        assert hip.hipMemcpyAsync(dst, src, nbytes, kind, sp) == 0
        assert hip.hipStreamSynchronize(sp) == 0

    copy(dp, hp, 1)
    h2d = timed(lambda: copy(dp, hp, 1), a.reps)   # hipMemcpyHostToDevice
    d2h = timed(lambda: copy(hp, dp, 2), a.reps)   # hipMemcpyDeviceToHost
    res = {"tool": "bench_state", "nf": "vignat", "flows": a.flows, "image_bytes": len(img),
           "reps": a.reps, "save_ms": stats(save), "load_ms": stats(load),
           "copy_d2h_ms": stats(d2h), "copy_h2d_ms": stats(h2d),
           "save_over_d2h": round(float(np.median(save) / np.median(d2h)), 2),
           "load_over_h2d": round(float(np.median(load) / np.median(h2d)), 2),
           "layout_after_load": layout}
    print(json.dumps(res))
    if not a.delta:
        return
    t_next = int(T.NOW0) + 2 * a.flows
    for share in (0.01, 0.1, 1.0):
        k = max(1, int(a.flows * share))
        mark, base_img = nat.state_mark(), nat.save_state()
        fr, ln, dv, now = T.nat_lan_trace(k, a.flows)  # flows 0 .. k - 1, once each
        now = t_next + np.arange(k, dtype=np.int64)
        t_next += k
        nat.process_device(torch.from_numpy(fr).to(d), torch.from_numpy(ln.view(np.int16)).to(d),
                           torch.from_numpy(dv.view(np.int16)).to(d),
                           torch.zeros(k, dtype=torch.int16, device=d), 64,
                           now=torch.from_numpy(now).to(d))
        torch.cuda.synchronize()
        blob, _ = nat.save_delta(mark)
        sv = timed(lambda: nat.save_delta(mark), a.reps)
        ap_ms = []
        for _ in range(a.reps):
            twin.load_state(base_img)
            twin.follow(mark)
            ap_ms += timed(lambda: twin.apply_delta(blob), 1)
        assert twin.save_state() == nat.save_state()
        dh2d = timed(lambda: copy(dp, hp, 1, len(blob)), a.reps)
        dd2h = timed(lambda: copy(hp, dp, 2, len(blob)), a.reps)
        print(json.dumps({"tool": "bench_state", "mode": "delta", "flows": a.flows, "touched": k,
                          "delta_bytes": len(blob), "image_bytes": len(base_img), "reps": a.reps,
                          "save_delta_ms": stats(sv), "apply_delta_ms": stats(ap_ms),
                          "save_ms": stats(save), "load_ms": stats(load),
                          "copy_d2h_ms": stats(dd2h), "copy_h2d_ms": stats(dh2d)}))


if __name__ == "__main__":
    main()
