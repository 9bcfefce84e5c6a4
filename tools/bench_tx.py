"""vp_tx_build over one headline-sized batch: the time of its three launches
beside the bytes the algorithm has to move. Run by hand; not part of bench.py.

  python3 tools/bench_tx.py [--packets 16777216] [--reps 20] [--step-ms MS] [--pack]
                             [--rebatch] [--merge] [--unpack] [--return] [--rxmerge]

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
--pack: after a case's lists are built, vp_tx_pack over them
is timed the same way, with and without pos[], and in the same run on the same
stream a plain device-to-device copy (torch's copy_, one hipMemcpyAsync) of
the streams' total bytes. The frames are 64-byte slots of random bytes.
Algorithmic bytes of a pack: idx and len read in two passes (12 B per entry),
the payload read and written, and 8 B per entry of pos[].
--rebatch: after a case's lists are built, vp_tx_rebatch of one port's list
(port 1, the fullest in every case) into 64-byte slots with
len[], now[] and src[] is timed the same way, beside a plain device-to-device
copy of the same number of slot bytes on the same stream. Algorithmic bytes of
a rebatch: each listed slot read and written, 14 B per entry read (idx, len,
now) and 14 B written (len, now, src).
--merge: vp_tx_merge of (a) the two lists of the two-port
case and (b) three lists (ports 1 to 3) of the four-port flood pattern, keyed
by packet index (key NULL), into 64-byte slots with len[], now[], in_dev[],
key[], src[] and which[]; beside it, in the same run and on the same stream,
vp_tx_rebatch of a single list holding the same number of entries (the same
stretch of idx[] read as one list) and a plain device-to-device copy of the
same slot bytes. Algorithmic bytes of a merge: each listed slot read and
written; per entry idx read (4), in_dev, key, src and which written (11),
which and src read back (5), len and now read and written (20): 40 B; the
binary searches' reads come on top and are not counted.
--unpack: after a case's lists are built and packed (vp_tx_pack with pos, 64-
byte slots of random bytes), vp_rx_unpack of port 1's stream
into 64-byte slots with len[], now[] and src[] is timed the same way, once with
pos and sel and once without pos from the port's first byte (sizes and scan
launches included); beside them, in the same run and on the same stream,
vp_tx_rebatch of the same entries and a plain device-to-device copy of the
same slot bytes. Algorithmic bytes of an unpack: the port's stream read, each
slot written, 22 B per entry read (sel, len, now, pos) and 14 B written (len,
now, src); without pos the sizes pass reads sel and len once more.
--return: after a case's lists are built and port 1's list is rebatched into
64-byte slots with src[], vp_tx_return of that batch into the
source batch's slots (home = src[], every packet sent on to an exit) is timed
the same way, with stats and without; beside it, in the same run and on the
same stream, vp_tx_rebatch of the same entries and a plain device-to-device
copy of the same slot bytes. Algorithmic bytes of a return: each slot read and
written, 6 B per entry read (home, out) and 2 B written (the home out port):
the rebatch's slot bytes with the index on the write side, and 8 B of
per-entry arrays where the rebatch has 28.
--rxmerge: after a case's lists are built and packed as for --unpack,
vp_rx_merge of (a) the two port streams of the two-port case
and (b) the streams of ports 1 to 3 of the four-port flood pattern, each with
sel and the batch's time array (so the merge is by packet index, a flooded
packet's three copies tying), into 64-byte slots with len[], now[], in_dev[],
src[] and which[], once with pos and once without (every queue's sizes and
scan launches included); beside them, in the same run and on the same stream,
vp_rx_unpack of the same entries as one stream (with pos) and a plain
device-to-device copy of the same slot bytes. Algorithmic bytes of a merge:
the streams read, each slot written; per entry sel, now and pos read (20),
which, src, in_dev, now and the position record written (23), which, src and
the record read back (13), len read and written (4): 60 B; the binary
searches' reads come on top and are not counted.
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
    """(result, (idx, offset, total)): the timed vp_tx_build and its lists."""
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
            "alg_gb_per_s": round(alg / (ms[len(ms) // 2] * 1e-3) / 1e9, 1)}, (idx, off, total)


def timed(s, reps, call):
    """ms of `reps` calls back to back on stream s, each between two events,
    after 3 untimed ones; sorted."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    with torch.cuda.stream(s):
        for _ in range(3):
            call()
        ev[0].record(s)
        for k in range(reps):
            call()
            ev[k + 1].record(s)
    s.synchronize()
    return sorted(ev[k].elapsed_time(ev[k + 1]) for k in range(reps))


def measure_pack(nf, nd, lens, idx, off, total, reps, dev):
    """vp_tx_pack over built lists and 64-byte slots, and a plain copy of the
    same payload on the same stream."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    po = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    pos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    idx = idx[:total] if total else None
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
    nf.tx_pack(frames, slot, lens, idx, off, None, po)  # the total, to size data
    torch.cuda.synchronize()
    payload = int(po.cpu().numpy().view(np.uint64)[nd])
    data = torch.zeros(max(payload, 16), dtype=torch.uint8, device=dev)[:payload]
    src = torch.randint(0, 256, (max(payload, 16),), dtype=torch.uint8, device=dev)[:payload]
    dst = torch.empty_like(src)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ms = timed(s, reps, lambda: nf.tx_pack(frames, slot, lens, idx, off, data, po,
                                           pos[:total] if total else None, stream=s))
    ms_np = timed(s, reps, lambda: nf.tx_pack(frames, slot, lens, idx, off, data, po, None,
                                              stream=s))
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    # the first entries against a gather made with torch (a sanity check of the
    # run, not the test: tests/test_txpack_gpu.py)
    k = min(total, 4096)
    if k:
        i = idx[:k].long()
        want = frames.view(n, slot)[i].clone()
        cl = lens[i].long().clamp(max=slot)
        want[torch.arange(slot, device=dev)[None, :] >= cl[:, None]] = 0
        p = pos[:k]
        assert bool((p == torch.cumsum((cl + 15) // 16 * 16, 0) - (cl + 15) // 16 * 16).all())
        if bool((cl > 48).all()):  # every frame fills its four units
            assert bool((data[:k * slot].view(k, slot) == want).all())
    alg = 12 * total + 2 * payload + 8 * total
    med = ms[len(ms) // 2]
    med_cp = ms_cp[len(ms_cp) // 2]
    return {"payload_bytes": payload, "pack_ms_median": round(med, 4),
            "pack_ms_min": round(ms[0], 4), "pack_ms_max": round(ms[-1], 4),
            "pack_no_pos_ms_median": round(ms_np[len(ms_np) // 2], 4),
            "copy_ms_median": round(med_cp, 4), "copy_ms_min": round(ms_cp[0], 4),
            "copy_ms_max": round(ms_cp[-1], 4),
            "pack_over_copy": round(med / med_cp, 3) if med_cp else None,
            "pack_alg_bytes": alg, "pack_alg_gb_per_s": round(alg / (med * 1e-3) / 1e9, 1),
            "copy_gb_per_s": round(2 * payload / (med_cp * 1e-3) / 1e9, 1) if med_cp else None}


def measure_rebatch(nf, nd, lens, idx, off, total, port, reps, dev):
    """vp_tx_rebatch of list `port` over built lists and 64-byte slots, and a
    plain copy of the same slot bytes on the same stream."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    now = torch.arange(n, dtype=torch.int64, device=dev) + T.NOW0
    bounds = off.cpu().numpy().view(np.uint32)
    lo, count = int(bounds[port]), int(bounds[port + 1] - bounds[port])
    idx = idx[:total] if total else None
    cap = max(count, 1)
    o_f = torch.zeros(cap * slot, dtype=torch.uint8, device=dev)
    o_l = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_n = torch.zeros(cap, dtype=torch.int64, device=dev)
    o_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    src = torch.randint(0, 256, (cap * slot,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)

    def call():
        nf.tx_rebatch(frames, slot, lens, idx, off, port, o_f, slot, o_l, cnt, out_now=o_n,
                      out_src=o_s, now=now, stream=s)

    ms = timed(s, reps, call)
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    # the first entries against a gather made with torch (a sanity check of the
    # run, not the test: tests/test_txbatch_gpu.py)
    assert int(cnt.cpu()[0]) == count
    k = min(count, 4096)
    if k:
        i = idx[lo:lo + k].long()
        assert bool((o_f[:k * slot].view(k, slot) == frames.view(n, slot)[i]).all())
        assert bool((o_l[:k] == lens[i]).all()) and bool((o_n[:k] == now[i]).all())
        assert bool((o_s[:k].long() == i).all())
    alg = 2 * count * slot + 28 * count
    med, med_cp = ms[len(ms) // 2], ms_cp[len(ms_cp) // 2]
    return {"port": port, "list_entries": count, "slot_bytes": count * slot,
            "rebatch_ms_median": round(med, 4), "rebatch_ms_min": round(ms[0], 4),
            "rebatch_ms_max": round(ms[-1], 4), "copy_ms_median": round(med_cp, 4),
            "copy_ms_min": round(ms_cp[0], 4), "copy_ms_max": round(ms_cp[-1], 4),
            "rebatch_over_copy": round(med / med_cp, 3) if med_cp else None,
            "bytes_over_copy_bytes": round(alg / (2 * count * slot), 3) if count else None,
            "rebatch_alg_bytes": alg,
            "rebatch_alg_gb_per_s": round(alg / (med * 1e-3) / 1e9, 1),
            "copy_gb_per_s": round(2 * count * slot / (med_cp * 1e-3) / 1e9, 1)
            if med_cp else None}


def measure_merge(nf, nd, lens, idx, off, total, ports, reps, dev):
    """vp_tx_merge of the lists `ports` of one batch (64-byte slots, keyed by
    packet index), vp_tx_rebatch of the same stretch of idx[] as one list, and
    a plain copy of the same slot bytes, all on one stream."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    now = torch.arange(n, dtype=torch.int64, device=dev) + T.NOW0
    bounds = off.cpu().numpy().view(np.uint32)
    assert list(ports) == list(range(ports[0], ports[-1] + 1))
    lo, hi = int(bounds[ports[0]]), int(bounds[ports[-1] + 1])
    count = hi - lo
    cap = max(count, 1)
    o_f = torch.zeros(cap * slot, dtype=torch.uint8, device=dev)
    o_l = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_n = torch.zeros(cap, dtype=torch.int64, device=dev)
    o_i = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_k = torch.zeros(cap, dtype=torch.int32, device=dev)
    o_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    o_w = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    # the same entries as one list: the stretch of idx[] the ports' lists fill
    one = idx[lo:hi] if count else None
    one_off = torch.tensor([0] + [count] * nd, dtype=torch.int32, device=dev)
    src = torch.randint(0, 256, (cap * slot,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    s = torch.cuda.Stream(device=dev)
    lists = idx[:total] if total else None
    sources = [(nf, frames, slot, lens, lists, off, p, k, None, now, 0, 0)
               for k, p in enumerate(ports)]
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
    ms = timed(s, reps, lambda: nf.tx_merge(sources, o_f, slot, o_l, cnt, o_s, o_w, out_now=o_n,
                                            out_in_dev=o_i, out_key=o_k, stream=s))
    assert int(cnt.cpu()[0]) == count
    # a sanity check of the run, not the test (tests/test_txmerge_gpu.py): the
    # keys ascend, and the first entries hold the slots src[] names
    k = min(count, 4096)
    if k:
        assert bool((o_k[1:count] >= o_k[:count - 1]).all())
        i = o_s[:k].long()
        assert bool((o_k[:k].long() == i).all())
        assert bool((o_f[:k * slot].view(k, slot) == frames.view(n, slot)[i]).all())
        assert bool((o_l[:k] == lens[i]).all()) and bool((o_n[:k] == now[i]).all())
    ms_rb = timed(s, reps, lambda: nf.tx_rebatch(frames, slot, lens, one, one_off, 0, o_f, slot,
                                                 o_l, cnt, out_now=o_n, out_src=o_s, now=now,
                                                 stream=s))
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    alg = 2 * count * slot + 40 * count
    med, med_rb, med_cp = (x[len(x) // 2] for x in (ms, ms_rb, ms_cp))
    return {"ports": list(ports), "entries_merged": count, "slot_bytes": count * slot,
            "merge_ms_median": round(med, 4), "merge_ms_min": round(ms[0], 4),
            "merge_ms_max": round(ms[-1], 4), "rebatch_ms_median": round(med_rb, 4),
            "rebatch_ms_min": round(ms_rb[0], 4), "rebatch_ms_max": round(ms_rb[-1], 4),
            "copy_ms_median": round(med_cp, 4), "copy_ms_min": round(ms_cp[0], 4),
            "copy_ms_max": round(ms_cp[-1], 4),
            "merge_over_rebatch": round(med / med_rb, 3) if med_rb else None,
            "merge_over_copy": round(med / med_cp, 3) if med_cp else None,
            "merge_alg_bytes": alg,
            "bytes_over_copy_bytes": round(alg / (2 * count * slot), 3) if count else None}


def measure_unpack(nf, nd, lens, idx, off, total, port, reps, dev):
    """vp_rx_unpack of list `port`'s packed stream (vp_tx_pack with pos over
    64-byte slots) into 64-byte slots with len[], now[] and src[]: with pos and
    sel, and without pos from the port's first byte; beside them, on the same
    stream, vp_tx_rebatch of the same entries and a plain copy of the same slot
    bytes."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    now = torch.arange(n, dtype=torch.int64, device=dev) + T.NOW0
    bounds = off.cpu().numpy().view(np.uint32)
    lo, count = int(bounds[port]), int(bounds[port + 1] - bounds[port])
    idx = idx[:total] if total else None
    po = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    pos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    data = torch.zeros(max(total, 1) * slot, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
    nf.tx_pack(frames, slot, lens, idx, off, data, po, pos[:total] if total else None)
    torch.cuda.synchronize()
    p_off = po.cpu().numpy().view(np.uint64)
    payload, a, b = int(p_off[nd]), int(p_off[port]), int(p_off[port + 1])
    assert payload <= data.numel() and int(lens.max()) <= slot
    cap = max(count, 1)
    o_f = torch.zeros(cap * slot, dtype=torch.uint8, device=dev)
    o_l = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_n = torch.zeros(cap, dtype=torch.int64, device=dev)
    o_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    src = torch.randint(0, 256, (cap * slot,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    sel = idx[lo:lo + count] if count else None
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def verify():
        # the first entries against a gather made with torch (a sanity check
        # of the run, not the test: tests/test_rxunpack_gpu.py)
        assert int(cnt.cpu()[0]) == count
        k = min(count, 4096)
        if k:
            i = sel[:k].long()
            want = frames.view(n, slot)[i].clone()
            want[torch.arange(slot, device=dev)[None, :] >= lens[i].long()[:, None]] = 0
            assert bool((o_f[:k * slot].view(k, slot) == want).all())
            assert bool((o_l[:k] == lens[i]).all()) and bool((o_n[:k] == now[i]).all())
            assert bool((o_s[:k].long() == i).all())
        o_f.zero_()
        torch.cuda.synchronize()

    d_all, d_port = data[:payload], data[a:b]
    p_port = pos[lo:lo + count] if count else None
    ms = timed(s, reps, lambda: nf.rx_unpack(
        d_all, lens, o_f, slot, o_l, cnt, pos=p_port, sel=sel, out_now=o_n, out_src=o_s,
        now=now, n=count, stream=s))
    verify()
    ms_np = timed(s, reps, lambda: nf.rx_unpack(
        d_port, lens, o_f, slot, o_l, cnt, sel=sel, out_now=o_n, out_src=o_s, now=now,
        n=count, stream=s))
    verify()
    ms_rb = timed(s, reps, lambda: nf.tx_rebatch(frames, slot, lens, idx, off, port, o_f, slot,
                                                 o_l, cnt, out_now=o_n, out_src=o_s, now=now,
                                                 stream=s))
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    # per entry: sel, len, now and pos read (22 B), len, now and src written (14 B)
    alg = (b - a) + count * slot + 36 * count
    med, med_np, med_rb, med_cp = (x[len(x) // 2] for x in (ms, ms_np, ms_rb, ms_cp))
    return {"port": port, "list_entries": count, "slot_bytes": count * slot,
            "stream_bytes": b - a,
            "unpack_ms_median": round(med, 4), "unpack_ms_min": round(ms[0], 4),
            "unpack_ms_max": round(ms[-1], 4),
            "unpack_no_pos_ms_median": round(med_np, 4), "unpack_no_pos_ms_min": round(ms_np[0], 4),
            "unpack_no_pos_ms_max": round(ms_np[-1], 4),
            "rebatch_ms_median": round(med_rb, 4), "rebatch_ms_min": round(ms_rb[0], 4),
            "rebatch_ms_max": round(ms_rb[-1], 4),
            "copy_ms_median": round(med_cp, 4), "copy_ms_min": round(ms_cp[0], 4),
            "copy_ms_max": round(ms_cp[-1], 4),
            "unpack_over_copy": round(med / med_cp, 3) if med_cp else None,
            "unpack_no_pos_over_copy": round(med_np / med_cp, 3) if med_cp else None,
            "unpack_over_rebatch": round(med / med_rb, 3) if med_rb else None,
            "unpack_no_pos_over_rebatch": round(med_np / med_rb, 3) if med_rb else None,
            "rebatch_over_copy": round(med_rb / med_cp, 3) if med_cp else None,
            "unpack_alg_bytes": alg,
            "bytes_over_copy_bytes": round(alg / (2 * count * slot), 3) if count else None}


def measure_rxmerge(nf, nd, lens, idx, off, total, ports, reps, dev):
    """vp_rx_merge of the packed streams of `ports` (vp_tx_pack with pos over
    64-byte slots; sel and the batch's time array per queue) into 64-byte slots,
    with pos and without; beside them, on the same stream, vp_rx_unpack of the
    same entries as one stream and a plain copy of the same slot bytes."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    now = torch.arange(n, dtype=torch.int64, device=dev) + T.NOW0
    bounds = off.cpu().numpy().view(np.uint32)
    assert list(ports) == list(range(ports[0], ports[-1] + 1))
    lo, hi = int(bounds[ports[0]]), int(bounds[ports[-1] + 1])
    count = hi - lo
    idx = idx[:total] if total else None
    po = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    pos = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
    data = torch.zeros(max(total, 1) * slot, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)
    nf.tx_pack(frames, slot, lens, idx, off, data, po, pos[:total] if total else None)
    torch.cuda.synchronize()
    p_off = po.cpu().numpy().view(np.uint64)
    payload = int(p_off[nd])
    assert payload <= data.numel() and int(lens.max()) <= slot
    cap = max(count, 1)
    o_f = torch.zeros(cap * slot, dtype=torch.uint8, device=dev)
    o_l = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_n = torch.zeros(cap, dtype=torch.int64, device=dev)
    o_i = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    o_w = torch.zeros(cap, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    src = torch.randint(0, 256, (cap * slot,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def queues(with_pos):
        qs = []
        for k, p in enumerate(ports):
            a, b = int(bounds[p]), int(bounds[p + 1])
            d = data[:payload] if with_pos else data[int(p_off[p]):int(p_off[p + 1])]
            qs.append(dict(data=d, lens=lens, in_port=k, now=now, n=b - a,
                           sel=idx[a:b] if b > a else None,
                           pos=pos[a:b] if with_pos and b > a else None))
        return qs

    def verify():
        # a sanity check of the run, not the test (tests/test_rxmerge_gpu.py):
        # the times ascend, and the first entries hold the frames src[] names
        assert int(cnt.cpu()[0]) == count
        k = min(count, 4096)
        if k:
            assert bool((o_n[1:count] >= o_n[:count - 1]).all())
            i = o_s[:k].long()
            want = frames.view(n, slot)[i].clone()
            want[torch.arange(slot, device=dev)[None, :] >= lens[i].long()[:, None]] = 0
            assert bool((o_f[:k * slot].view(k, slot) == want).all())
            assert bool((o_l[:k] == lens[i]).all()) and bool((o_n[:k] == now[i]).all())
        o_f.zero_()
        o_n.zero_()
        torch.cuda.synchronize()

    s = torch.cuda.Stream(device=dev)
    q_pos, q_np = queues(True), queues(False)
    torch.cuda.synchronize()
    ms = timed(s, reps, lambda: nf.rx_merge(q_pos, o_f, slot, o_l, cnt, o_s, o_w, out_now=o_n,
                                            out_in_dev=o_i, stream=s))
    verify()
    ms_np = timed(s, reps, lambda: nf.rx_merge(q_np, o_f, slot, o_l, cnt, o_s, o_w, out_now=o_n,
                                               out_in_dev=o_i, stream=s))
    verify()
    # the same entries as one stream: the stretch of idx[] and pos[] the ports fill
    ms_up = timed(s, reps, lambda: nf.rx_unpack(
        data[:payload], lens, o_f, slot, o_l, cnt, pos=pos[lo:hi] if count else None,
        sel=idx[lo:hi] if count else None, out_now=o_n, out_src=o_s, now=now, n=count, stream=s))
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    stream_bytes = int(p_off[ports[-1] + 1] - p_off[ports[0]])
    alg = stream_bytes + count * slot + 60 * count
    med, med_np, med_up, med_cp = (x[len(x) // 2] for x in (ms, ms_np, ms_up, ms_cp))
    return {"ports": list(ports), "entries_merged": count, "slot_bytes": count * slot,
            "stream_bytes": stream_bytes,
            "rxmerge_ms_median": round(med, 4), "rxmerge_ms_min": round(ms[0], 4),
            "rxmerge_ms_max": round(ms[-1], 4),
            "rxmerge_no_pos_ms_median": round(med_np, 4),
            "rxmerge_no_pos_ms_min": round(ms_np[0], 4),
            "rxmerge_no_pos_ms_max": round(ms_np[-1], 4),
            "unpack_ms_median": round(med_up, 4), "unpack_ms_min": round(ms_up[0], 4),
            "unpack_ms_max": round(ms_up[-1], 4),
            "copy_ms_median": round(med_cp, 4), "copy_ms_min": round(ms_cp[0], 4),
            "copy_ms_max": round(ms_cp[-1], 4),
            "rxmerge_over_unpack": round(med / med_up, 3) if med_up else None,
            "rxmerge_no_pos_over_unpack": round(med_np / med_up, 3) if med_up else None,
            "rxmerge_over_copy": round(med / med_cp, 3) if med_cp else None,
            "rxmerge_no_pos_over_copy": round(med_np / med_cp, 3) if med_cp else None,
            "unpack_over_copy": round(med_up / med_cp, 3) if med_cp else None,
            "rxmerge_alg_bytes": alg,
            "bytes_over_copy_bytes": round(alg / (2 * count * slot), 3) if count else None}


def measure_return(nf, nd, lens, idx, off, total, port, reps, dev):
    """vp_tx_return of list `port`'s rebatched batch (64-byte slots) into the
    source batch's slots, home = the rebatch's src[]; beside it, on the same
    stream, vp_tx_rebatch of the same entries and a plain copy of the same slot
    bytes."""
    n, slot = lens.numel(), 64
    frames = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device=dev)
    now = torch.arange(n, dtype=torch.int64, device=dev) + T.NOW0
    bounds = off.cpu().numpy().view(np.uint32)
    lo, count = int(bounds[port]), int(bounds[port + 1] - bounds[port])
    idx = idx[:total] if total else None
    cap = max(count, 1)
    o_f = torch.zeros(cap * slot, dtype=torch.uint8, device=dev)
    o_l = torch.zeros(cap, dtype=torch.int16, device=dev)
    o_n = torch.zeros(cap, dtype=torch.int64, device=dev)
    o_s = torch.zeros(cap, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    # the stage behind the cable sent every packet on to its port 1, the
    # composite's port 7
    o_out = torch.ones(cap, dtype=torch.int16, device=dev)
    h_out = torch.zeros(n, dtype=torch.int16, device=dev)
    st = torch.zeros(C.sizeof(vigor_amd.TxReturnStatsC), dtype=torch.uint8, device=dev)
    ports = [vigor_amd.RET_DROP] * nd
    ports[1] = 7
    src = torch.randint(0, 256, (cap * slot,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # (torch filled the buffers on its own stream)

    def rebatch():
        nf.tx_rebatch(frames, slot, lens, idx, off, port, o_f, slot, o_l, cnt, out_now=o_n,
                      out_src=o_s, now=now, stream=s)

    with torch.cuda.stream(s):
        rebatch()
        o_f[:count * slot] ^= 0xFF  # (the stage rewrote its frames: the return shows)
    s.synchronize()
    ms = timed(s, reps, lambda: nf.tx_return(
        o_f[:count * slot], slot, o_out[:count], 0, frames, slot, h_out, 0, ports,
        vigor_amd.RET_DROP, vigor_amd.RET_DROP, vigor_amd.RET_DROP, home=o_s[:count], stats=st,
        stream=s))
    # the first entries against a scatter made with torch (a sanity check of
    # the run, not the test: tests/test_txreturn_gpu.py)
    words = st.cpu().numpy().view(np.uint64)
    assert words.tolist() == [count, 0, 0, 0, 0]
    k = min(count, 4096)
    if k:
        i = idx[lo:lo + k].long()
        assert bool((frames.view(n, slot)[i] == o_f[:k * slot].view(k, slot)).all())
        assert bool((h_out[i] == 7).all()) and int((h_out == 7).sum()) == count
    ms_ns = timed(s, reps, lambda: nf.tx_return(
        o_f[:count * slot], slot, o_out[:count], 0, frames, slot, h_out, 0, ports,
        vigor_amd.RET_DROP, vigor_amd.RET_DROP, vigor_amd.RET_DROP, home=o_s[:count], stream=s))
    ms_rb = timed(s, reps, rebatch)
    ms_cp = timed(s, reps, lambda: dst.copy_(src))
    # per entry: home (4) and out (2) read, home out (2) written
    alg, alg_rb = 2 * count * slot + 8 * count, 2 * count * slot + 28 * count
    med, med_rb, med_cp = (x[len(x) // 2] for x in (ms, ms_rb, ms_cp))
    return {"port": port, "list_entries": count, "slot_bytes": count * slot,
            "return_ms_median": round(med, 4), "return_ms_min": round(ms[0], 4),
            "return_ms_max": round(ms[-1], 4),
            "return_no_stats_ms_median": round(ms_ns[len(ms_ns) // 2], 4),
            "return_no_stats_ms_min": round(ms_ns[0], 4),
            "return_no_stats_ms_max": round(ms_ns[-1], 4),
            "rebatch_ms_median": round(med_rb, 4), "rebatch_ms_min": round(ms_rb[0], 4),
            "rebatch_ms_max": round(ms_rb[-1], 4),
            "copy_ms_median": round(med_cp, 4), "copy_ms_min": round(ms_cp[0], 4),
            "copy_ms_max": round(ms_cp[-1], 4),
            "return_over_rebatch": round(med / med_rb, 3) if med_rb else None,
            "return_over_copy": round(med / med_cp, 3) if med_cp else None,
            "rebatch_over_copy": round(med_rb / med_cp, 3) if med_cp else None,
            "return_alg_bytes": alg,
            "bytes_over_rebatch_bytes": round(alg / alg_rb, 3) if count else None,
            "bytes_over_copy_bytes": round(alg / (2 * count * slot), 3) if count else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=None,
                    help="the headline step of the same session (bench.py ms_per_step)")
    ap.add_argument("--pack", action="store_true",
                    help="also time vp_tx_pack over each case's lists, beside a plain copy")
    ap.add_argument("--rebatch", action="store_true",
                    help="also time vp_tx_rebatch of port 1's list, beside a plain copy")
    ap.add_argument("--merge", action="store_true",
                    help="also time vp_tx_merge of the two-port case's two lists and of three "
                         "lists of the flood pattern, beside vp_tx_rebatch and a plain copy")
    ap.add_argument("--unpack", action="store_true",
                    help="also time vp_rx_unpack of port 1's packed stream, with and without "
                         "pos, beside vp_tx_rebatch and a plain copy")
    ap.add_argument("--return", action="store_true",
                    help="also time vp_tx_return of port 1's rebatched batch into the source "
                         "batch's slots, beside vp_tx_rebatch and a plain copy")
    ap.add_argument("--rxmerge", action="store_true",
                    help="also time vp_rx_merge of the two-port case's two packed streams and "
                         "of three streams of the flood pattern, with and without pos, beside "
                         "vp_rx_unpack of the same entries and a plain copy")
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
        r, lists = measure(nf, nd, out, in_dev, ln, args.reps, dev)
        r = {"case": name, **r}
        if args.step_ms:
            r["headline_step_ms"] = args.step_ms
            r["fraction_of_step"] = round(r["ms_median"] / args.step_ms, 4)
        print(json.dumps(r), flush=True)
        if args.pack:
            idx, off, total = lists
            p = {"case": name + "-pack", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps, **measure_pack(nf, nd, ln, idx, off, total, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["pack_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        if args.rebatch:
            idx, off, total = lists
            p = {"case": name + "-rebatch", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps,
                 **measure_rebatch(nf, nd, ln, idx, off, total, 1, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["rebatch_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        if args.merge and name != "two-port-drop16":
            idx, off, total = lists
            ports = [0, 1] if nd == 2 else [1, 2, 3]
            p = {"case": name + "-merge", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps,
                 **measure_merge(nf, nd, ln, idx, off, total, ports, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["merge_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        if args.unpack:
            idx, off, total = lists
            p = {"case": name + "-unpack", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps,
                 **measure_unpack(nf, nd, ln, idx, off, total, 1, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["unpack_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        if getattr(args, "return"):
            idx, off, total = lists
            p = {"case": name + "-return", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps,
                 **measure_return(nf, nd, ln, idx, off, total, 1, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["return_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        if args.rxmerge and name != "two-port-drop16":
            idx, off, total = lists
            ports = [0, 1] if nd == 2 else [1, 2, 3]
            p = {"case": name + "-rxmerge", "packets": n, "n_devices": nd, "entries": total,
                 "reps": args.reps,
                 **measure_rxmerge(nf, nd, ln, idx, off, total, ports, args.reps, dev)}
            if args.step_ms:
                p["headline_step_ms"] = args.step_ms
                p["fraction_of_step"] = round(p["rxmerge_ms_median"] / args.step_ms, 4)
            print(json.dumps(p), flush=True)
        del lists
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
