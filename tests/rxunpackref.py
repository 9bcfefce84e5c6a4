"""Reference for vp_rx_unpack (include/vigpath.h, "receive"): a packed stream of
frames as a device batch, as a plain loop over the stream's entries. Shares no
code with the library; the tests compare the GPU's bytes with it."""
import numpy as np

M64 = (1 << 64) - 1


def unpack_reference(data, nbytes, n, lens, out_slot, out_cap, pos=None, sel=None, now=None,
                     now0=0, now_step=0):
    """(count, frames, len, now, src) of the call: count is n, the arrays what
    the first min(n, out_cap) entries of the output buffers hold (u8 of
    min(n, out_cap) * out_slot bytes, u16, i64, u32). data: u8, of which the
    first nbytes may be read; lens (and now, when given): meta_n entries; pos,
    sel: None or at least n entries."""
    data = np.asarray(data, np.uint8).reshape(-1)
    lens = [int(x) for x in np.asarray(lens).astype(np.uint16)]
    meta_n = len(lens)
    m_out = min(n, out_cap)
    o_frames = np.zeros(m_out * out_slot, np.uint8)
    o_len = np.zeros(m_out, np.uint16)
    o_now = np.zeros(m_out, np.int64)
    o_src = np.zeros(m_out, np.uint32)
    run = 0  # pos is None: the sum of ext(k) over k < e
    for e in range(m_out):
        m = int(sel[e]) if sel is not None else e
        L = lens[m] if m < meta_n else 0
        p = int(pos[e]) & M64 if pos is not None else run
        run += (L + 15) & ~15
        r = min(L, out_slot)
        o_src[e] = m
        if not (m < meta_n and p % 16 == 0 and p + ((r + 15) & ~15) <= nbytes):
            continue  # a zero slot, length 0, time 0
        o_frames[e * out_slot:e * out_slot + r] = data[p:p + r]
        o_len[e] = L
        t = int(now[m]) if now is not None else now0 + m * now_step
        t &= M64  # (64-bit arithmetic)
        o_now[e] = t - (1 << 64) if t >> 63 else t
    return n, o_frames, o_len, o_now, o_src
