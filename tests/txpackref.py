"""Reference for vp_tx_pack (include/vigpath.h, "transmit"): the per-port byte
streams of a device-resident batch's transmit lists as a plain loop over the
list entries. Shares no code with the library; the tests compare the GPU's
bytes with it."""
import numpy as np


def pack_reference(frames, slot, lens, idx, offset, cap, n_devices, cap_bytes, canary=0):
    """(data, port_off, pos): data the first min(total, cap_bytes) bytes of the
    streams (u8), where the bytes of an entry that did not fit whole hold
    `canary` (what the buffer held before the call); port_off the
    n_devices + 1 stream bounds (u64) and pos the E = min(offset[n_devices],
    cap) entry positions (u64), the true ones whatever cap_bytes is. frames: u8
    of n * slot bytes; idx holds at least E entries."""
    frames = np.asarray(frames, np.uint8).reshape(-1)
    lens = np.asarray(lens).astype(np.uint16).tolist()
    offset = [int(x) for x in np.asarray(offset).astype(np.uint32)]
    n = len(lens)
    entries = min(offset[n_devices], cap)
    idx = [int(x) for x in np.asarray(idx).astype(np.uint32)[:entries]]
    pos = np.zeros(entries, np.uint64)
    pieces = []  # (position, clen, pad, packet) of the entries that occupy bytes
    at = 0
    for e in range(entries):
        i = idx[e]
        clen = min(lens[i], slot) if i < n else 0
        pad = (clen + 15) & ~15
        pos[e] = at
        if pad:
            pieces.append((at, clen, pad, i))
        at += pad
    total = at
    every = [int(p) for p in pos] + [total]
    port_off = np.array([every[min(offset[d], cap, entries)] for d in range(n_devices + 1)],
                        np.uint64)
    size = min(total, cap_bytes)
    data = np.full(size, canary, np.uint8)
    for at, clen, pad, i in pieces:
        if at + pad > cap_bytes:  # an entry is written whole or not at all
            continue
        data[at:at + clen] = frames[i * slot:i * slot + clen]
        data[at + clen:at + pad] = 0
    return data, port_off, pos
