"""Reference for vp_rx_merge (include/vigpath.h, "receive"): several packed
streams merged by time into one batch, in numpy: every entry's m, L, p and
readability by rxunpackref's rules, one np.lexsort on (entry, queue, time), and
the outputs built position by position. Shares no code with the library; the
tests compare the GPU's bytes with it."""
import numpy as np

M64 = (1 << 64) - 1
I64_MAX = (1 << 63) - 1


def queue(data, lens, in_port, pos=None, sel=None, now=None, now0=0, now_step=0, n=None,
          nbytes=None):
    """One queue of a call, host side: data u8 (the first nbytes may be read,
    by default all), lens (and now, when given) meta_n entries, pos and sel None
    or at least n entries; n by default sel's length, else pos's, else meta_n."""
    data = np.asarray(data, np.uint8).reshape(-1)
    lens = np.asarray(lens).astype(np.uint16).reshape(-1)
    if n is None:
        n = len(sel) if sel is not None else len(pos) if pos is not None else len(lens)
    return dict(data=data, nbytes=len(data) if nbytes is None else nbytes, lens=lens,
                in_port=in_port, pos=pos, sel=sel, now=now, now0=now0, now_step=now_step, n=n)


def _signed(t):
    t &= M64  # (64-bit arithmetic)
    return t - (1 << 64) if t >> 63 else t


def _entries(q):
    """Per entry (m, L, p, time) of one queue"""
    lens = [int(x) for x in q["lens"]]
    meta_n = len(lens)
    out = []
    run = 0  # pos is None: the sum of ext(k) over k < e
    for e in range(q["n"]):
        m = int(q["sel"][e]) if q["sel"] is not None else e
        L = lens[m] if m < meta_n else 0
        p = int(q["pos"][e]) & M64 if q["pos"] is not None else run
        run += (L + 15) & ~15
        if m >= meta_n:
            t = I64_MAX
        elif q["now"] is not None:
            t = _signed(int(q["now"][m]))
        else:
            t = _signed(q["now0"] + m * q["now_step"])
        out.append((m, L, p, t))
    return out


def merge_reference(queues, out_slot, out_cap):
    """(count, frames, len, now, in_dev, src, which) of the call: count is the
    sum of all n (0xFFFFFFFF past 32 bits), the arrays what the first
    min(total, out_cap) entries of the output buffers hold (u8 of that many
    slots, u16, i64, u16, u32, u8)."""
    ents = [_entries(q) for q in queues]
    jj = np.array([j for j, es in enumerate(ents) for _ in es], np.int64)
    ee = np.array([e for es in ents for e in range(len(es))], np.int64)
    tt = np.array([x[3] for es in ents for x in es], np.int64)
    order = np.lexsort((ee, jj, tt))  # by time, then queue, then entry
    total = len(order)
    m_out = min(total, out_cap)
    o_frames = np.zeros(m_out * out_slot, np.uint8)
    o_len = np.zeros(m_out, np.uint16)
    o_now = np.zeros(m_out, np.int64)
    o_in = np.zeros(m_out, np.uint16)
    o_src = np.zeros(m_out, np.uint32)
    o_which = np.zeros(m_out, np.uint8)
    for k in range(m_out):
        j, e = int(jj[order[k]]), int(ee[order[k]])
        q = queues[j]
        m, L, p, t = ents[j][e]
        o_now[k] = t  # (also where the frame is not readable)
        o_in[k] = q["in_port"]
        o_src[k] = m
        o_which[k] = j
        r = min(L, out_slot)
        if not (m < len(q["lens"]) and p % 16 == 0 and p + ((r + 15) & ~15) <= q["nbytes"]):
            continue  # a zero slot, length 0
        o_frames[k * out_slot:k * out_slot + r] = q["data"][p:p + r]
        o_len[k] = L
    return min(total, 0xFFFFFFFF), o_frames, o_len, o_now, o_in, o_src, o_which
