"""Reference for vp_tx_merge (include/vigpath.h, "transmit"): several
transmit lists as one NF's batch, ordered by (key, source number, place in the
list) with a stable numpy lexsort, the slots by vp_tx_rebatch's rules. Shares
no code with the library; the tests compare the GPU's bytes with it."""
from types import SimpleNamespace

import numpy as np

M64 = (1 << 64) - 1


def source(frames, slot, lens, idx, offset, n_devices, port, in_port=0, key=None, now=None,
           now0=0, now_step=0, lists_cap=None):
    """One source of a merge as numpy data. lists_cap None: all idx holds."""
    idx = np.asarray(idx, np.uint32)
    return SimpleNamespace(
        frames=np.asarray(frames, np.uint8).reshape(-1), slot=slot,
        lens=np.asarray(lens).astype(np.uint16), idx=idx,
        offset=np.asarray(offset).astype(np.uint32), n_devices=n_devices, port=port,
        in_port=in_port, key=None if key is None else np.asarray(key).astype(np.uint32),
        now=None if now is None else np.asarray(now, np.int64), now0=now0, now_step=now_step,
        lists_cap=idx.size if lists_cap is None else lists_cap)


def entries(s):
    """The packets source s's list really holds, and their keys."""
    e = min(int(s.offset[s.n_devices]), s.lists_cap)
    lo, hi = min(int(s.offset[s.port]), e), min(int(s.offset[s.port + 1]), e)
    i = s.idx[lo:max(hi, lo)].astype(np.uint32)
    n = s.lens.size
    k = i.copy()
    if s.key is not None:
        inside = i < n
        k[inside] = s.key[i[inside]]
    return i, k


def merge_reference(sources, out_slot, out_cap):
    """What the call leaves in the first min(total, out_cap) entries of every
    output buffer, and count = total: a namespace of count, frames (u8), len
    (u16), now (i64), in_dev (u16), key (u32), src (u32), which (u8)."""
    pk, ky, jj, mm = [], [], [], []
    for j, s in enumerate(sources):
        i, k = entries(s)
        pk.append(i)
        ky.append(k)
        jj.append(np.full(i.size, j, np.int64))
        mm.append(np.arange(i.size, dtype=np.int64))
    pk, ky, jj, mm = (np.concatenate(x) for x in (pk, ky, jj, mm))
    total = pk.size
    order = np.lexsort((mm, jj, ky))  # by key, then source, then place in the list
    m = min(total, out_cap)
    order = order[:m]
    o = SimpleNamespace(count=total, frames=np.zeros(m * out_slot, np.uint8),
                        len=np.zeros(m, np.uint16), now=np.zeros(m, np.int64),
                        in_dev=np.zeros(m, np.uint16), key=ky[order].astype(np.uint32),
                        src=pk[order].astype(np.uint32), which=jj[order].astype(np.uint8))
    for p, e in enumerate(order):
        s = sources[int(jj[e])]
        i = int(pk[e])
        o.in_dev[p] = s.in_port
        if i >= s.lens.size:
            continue  # a zero slot, length 0, time 0
        w = min(s.slot, out_slot)
        o.frames[p * out_slot:p * out_slot + w] = s.frames[i * s.slot:i * s.slot + w]
        o.len[p] = s.lens[i]
        t = (int(s.now[i]) if s.now is not None else s.now0 + i * s.now_step) & M64
        o.now[p] = t - (1 << 64) if t >> 63 else t
    return o
