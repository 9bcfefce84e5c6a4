"""Reference for vp_tx_rebatch (include/vigpath.h, "transmit"): one port's
transmit list as the next NF's batch, as a plain loop over the list's entries.
Shares no code with the library; the tests compare the GPU's bytes with it."""
import numpy as np

M64 = (1 << 64) - 1


def rebatch_reference(frames, slot, lens, idx, offset, lists_cap, n_devices, port, out_slot,
                      out_cap, now=None, now0=0, now_step=0):
    """(count, frames, len, now, src) of the call: count the list's true
    length C, the arrays what the first min(C, out_cap) entries of the output
    buffers hold (u8 of min(C, out_cap) * out_slot bytes, u16, i64, u32).
    frames: u8 of n * slot bytes; now: None for now0 + i * now_step."""
    frames = np.asarray(frames, np.uint8).reshape(-1)
    lens = [int(x) for x in np.asarray(lens).astype(np.uint16)]
    offset = [int(x) for x in np.asarray(offset).astype(np.uint32)]
    idx = [int(x) for x in np.asarray(idx).astype(np.uint32)]
    n = len(lens)
    entries = min(offset[n_devices], lists_cap)
    lo, hi = min(offset[port], entries), min(offset[port + 1], entries)
    count = hi - lo
    m = min(count, out_cap)
    w = min(slot, out_slot)
    o_frames = np.zeros(m * out_slot, np.uint8)
    o_len = np.zeros(m, np.uint16)
    o_now = np.zeros(m, np.int64)
    o_src = np.zeros(m, np.uint32)
    for k in range(m):
        i = idx[lo + k]
        o_src[k] = i
        if i >= n:
            continue  # a zero slot, length 0, time 0
        o_frames[k * out_slot:k * out_slot + w] = frames[i * slot:i * slot + w]
        o_len[k] = lens[i]
        t = int(now[i]) if now is not None else now0 + i * now_step
        t &= M64  # (64-bit arithmetic)
        o_now[k] = t - (1 << 64) if t >> 63 else t
    return count, o_frames, o_len, o_now, o_src
