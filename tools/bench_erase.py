#!/usr/bin/env python3
"""vp_table_erase / vp_table_free of vignat at 1M live flows (BASELINE config
1's table), the table rebuilt from a saved image (load_state, not timed) before
every repetition: erase_device of 2^10, 2^16 and 2^20 distinct live keys in
random order, of 2^20 keys that all miss, and free_device of 2^20 distinct live
indices in random order, every output array asked for. Wall time around the
call in ms, medians of 10 with min-max. The yardsticks, in the same run:
lookup_device of the same keys, a plain device-to-device copy of as many bytes
as the call's arrays hold (44 bytes per key, 32 per index) on the stream the
call runs on, and the path an erase replaces -- save_state, the entries taken
out of the image on the host with numpy, load_state -- each step timed. No
threshold is set. One JSON line per case.

  python tools/bench_erase.py [--flows 1048576] [--reps 10]
"""
import argparse
import ctypes as C
import json
import os
import struct
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
HDR, THDR = struct.Struct("<IIIIQq"), struct.Struct("<IIIIIIII")


def stats(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4),
            "max": round(max(ms), 4)}


def pad16(n):
    return (n + 15) & ~15


def edit_image(img, gone):
    """vignat's image (one table, no values) with the indices `gone` erased in
    that order, as the host has to do it without the call: lru[] and its ts[]
    and key[] rows filtered, the indices put before freed[] in reverse order,
    the tail normalised."""
    buf = np.frombuffer(img, np.uint8)
    magic, version, kind, nt, total, last_now = HDR.unpack_from(img, 0)
    cap, n, fresh, vsz, nf, _, _, _ = THDR.unpack_from(img, HDR.size)
    assert nt == 1 and vsz == 0
    at = HDR.size + THDR.size
    lru = buf[at:at + 4 * n].view(np.uint32)
    at += pad16(4 * n)
    freed = buf[at:at + 4 * nf].view(np.uint32)
    at += pad16(4 * nf)
    ts = buf[at:at + 8 * n].view(np.int64)
    at += pad16(8 * n)
    key = buf[at:at + 16 * n].reshape(n, 16)
    dead = np.zeros(cap, bool)
    dead[gone] = True
    keep = ~dead[lru]
    freed = np.concatenate([gone[::-1], freed])
    while freed.size and freed[-1] == fresh - 1:
        freed, fresh = freed[:-1], fresh - 1
    lru, ts, key = lru[keep], ts[keep], key[keep]
    n, nf = lru.size, freed.size
    body = [THDR.pack(cap, n, fresh, 0, nf, 0, 0, 0)]
    for arr in (lru, freed, ts, key):
        b = arr.tobytes()
        body.append(b + bytes(-len(b) % 16))
    body = b"".join(body)
    return HDR.pack(magic, version, kind, 1, HDR.size + len(body), last_now) + body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flows", type=int, default=1 << 20)
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
    img = nat.save_state()
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

    def timed_fresh(fn):
        """fn on the table as the image has it, every repetition."""
        out = []
        for _ in range(a.reps):
            nat.load_state(img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out, k

    def timed(fn):
        out = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=d)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=d)

        def copy():
            assert hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()),
                                      nbytes, 3, sp) == 0  # hipMemcpyDeviceToDevice
            assert hip.hipStreamSynchronize(sp) == 0
        copy()
        return stats(timed(copy))

    cases = [("erase_hits", 1 << 10), ("erase_hits", 1 << 16), ("erase_hits", min(1 << 20, a.flows)),
             ("erase_misses", 1 << 20), ("free_hits", min(1 << 20, a.flows))]
    for what, q in cases:
        pick = torch.randperm(a.flows, generator=gen)[:q] if what != "erase_misses" else \
            torch.randint(0, a.flows, (q,), generator=gen)
        pick = pick.to(d)
        keys = live_keys[pick].clone()
        if what == "erase_misses":
            keys[:, 8:12] = 0xFF  # (no flow of the trace has this destination address)
        keys = keys.contiguous().view(-1)
        idx = pick.to(torch.int32)
        index = torch.empty(q, dtype=torch.int32, device=d)
        ts = torch.empty(q, dtype=torch.int64, device=d)
        key = torch.empty(q * 16, dtype=torch.uint8, device=d)
        torch.cuda.synchronize()  # (the queries were built on another stream than st)
        if what == "free_hits":
            call = lambda: nat.free_device(idx, index=index, ts=ts, key=key, stream=st)  # noqa: E731
        else:
            call = lambda: nat.erase_device(keys, index=index, ts=ts, key=key, stream=st)  # noqa: E731
        t_call, k = timed_fresh(call)
        want = 0 if what == "erase_misses" else q
        assert k == want and nat.live_count() == a.flows - want, (what, q, k)
        if want:
            assert bool((index == idx).all()) and bool((key == keys).all())
        else:
            assert bool((index == -1).all()) and not bool(key.any()) and not bool(ts.any())
        res = {"tool": "bench_erase", "nf": "vignat", "flows": a.flows, "case": what, "queries": q,
               "reps": a.reps, "n_erased": k, "call_ms": stats(t_call)}
        nat.load_state(img)
        if what == "free_hits":
            look = lambda: nat.entries_device(idx, index=index, ts=ts, key=key, stream=st)  # noqa: E731
            res["entries_same_indices_ms"] = stats(timed(look))
            res["copy_d2d_32B_per_index_ms"] = copy_ms(32 * q)
        else:
            look = lambda: nat.lookup_device(keys, index=index, ts=ts, key=key, stream=st)  # noqa: E731
            res["lookup_same_keys_ms"] = stats(timed(look))
            res["copy_d2d_44B_per_key_ms"] = copy_ms(44 * q)
        if want:  # the path the call replaces, on the same indices
            gone = pick.cpu().numpy().astype(np.uint32)
            t_save, t_edit, t_load = [], [], []
            for _ in range(a.reps):
                nat.load_state(img)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cur = nat.save_state()
                t1 = time.perf_counter()
                new = edit_image(cur, gone)
                t2 = time.perf_counter()
                nat.load_state(new)
                t3 = time.perf_counter()
                t_save.append((t1 - t0) * 1e3)
                t_edit.append((t2 - t1) * 1e3)
                t_load.append((t3 - t2) * 1e3)
            assert nat.live_count() == a.flows - q
            nat.load_state(img)
            call()
            assert nat.save_state() == new, "the host's edit is not the call's image"
            res["save_edit_load_ms"] = stats([x + y + z for x, y, z in zip(t_save, t_edit, t_load)])
            res["save_state_ms"], res["host_edit_ms"], res["load_state_ms"] = (
                stats(t_save), stats(t_edit), stats(t_load))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
