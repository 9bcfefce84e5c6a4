"""Reference for vp_tx_build (include/vigpath.h, "transmit"): nf.c's per-packet
transmit decision (nf.c:159-174) as a plain loop over the packets. Shares no
code with the library; the tests compare the GPU's bytes with it."""
import numpy as np

MAX_DEV = 32
FLOOD = 0xFFFF
# vp_tx_stats as u64 words: packets[32], bytes[32], dropped, flooded, bad_port
STATS_WORDS = 2 * MAX_DEV + 3


def tx_reference(out, in_dev, lens, n_devices, cap):
    """(idx, offset, stats): idx the first min(total, cap) list entries (u32;
    port 0's list first, each list in packet order), offset the n_devices + 1
    list bounds (u32, the true ones whatever cap is), stats the vp_tx_stats
    words (u64). in_dev: an array, or an int for every packet."""
    out = np.asarray(out).astype(np.uint16).tolist()
    n = len(out)
    one = isinstance(in_dev, int)
    ins = None if one else np.asarray(in_dev).astype(np.uint16).tolist()
    lens = np.asarray(lens).astype(np.uint16).tolist()
    lists = [[] for _ in range(n_devices)]
    nbytes = [0] * n_devices
    dropped = flooded = bad = 0
    for i in range(n):
        o, src, ln = out[i], (in_dev if one else ins[i]), lens[i]
        if o == src:
            dropped += 1
        elif o == FLOOD:
            flooded += 1
            for d in range(n_devices):
                if d != src:
                    lists[d].append(i)
                    nbytes[d] += ln
        elif o < n_devices:
            lists[o].append(i)
            nbytes[o] += ln
        else:
            bad += 1
    offset = np.zeros(n_devices + 1, np.uint32)
    stats = np.zeros(STATS_WORDS, np.uint64)
    for d in range(n_devices):
        offset[d + 1] = offset[d] + len(lists[d])
        stats[d] = len(lists[d])
        stats[MAX_DEV + d] = nbytes[d]
    stats[2 * MAX_DEV:] = (dropped, flooded, bad)
    idx = np.array([i for lst in lists for i in lst], np.uint32)
    return idx[:cap], offset, stats
