"""Numpy model of vp_tx_return (include/vigpath.h): the contract as a loop over
the entries, one after another, on copies of the home batch. Shares no code
with the library. For home[] that does not decrease (what the contract calls
deterministic) the result is the call's, byte for byte."""
import numpy as np

FLOOD = 0xFFFF
RET_SKIP, RET_DROP = 0x10000, 0x10001
STATS = ("returned", "dropped", "skipped", "dup", "bad_home")


def action_of(out, inp, n_devices, ports, on_drop, on_flood, on_bad):
    """The action for one entry, chosen in vp_tx_build's order."""
    if out == inp:
        return on_drop
    if out == FLOOD:
        return on_flood
    if out < n_devices:
        return ports[out]
    return on_bad


def return_reference(frames, slot, out, in_dev, home_frames, home_slot, home_out, home_in_dev,
                     n_devices, ports, on_drop, on_flood, on_bad, home=None, in_place=False):
    """(home frames, home out_dev, stats) after the call. frames / out /
    in_dev: the returning batch (in_dev an int: every packet on that port);
    home_*: the home batch before the call, its n that of home_out; home:
    None (entry k's home is k) or one index per entry. in_place: the batch is
    its own home (frames are home_frames): no frame byte moves."""
    out = np.asarray(out, np.uint16)
    n, hn = out.size, np.asarray(home_out).size
    src = np.asarray(frames, np.uint8).reshape(n, slot) if n else np.zeros((0, slot), np.uint8)
    hf = np.array(home_frames, np.uint8).reshape(hn, home_slot)
    ho = np.array(home_out, np.uint16)
    w = min(slot, home_slot)
    st = dict.fromkeys(STATS, 0)
    before = None
    for k in range(n):
        h = k if home is None else int(home[k])
        first = k == 0 or h != before
        before = h
        if not first:
            st["dup"] += 1
            continue
        inp = in_dev if isinstance(in_dev, int) else int(in_dev[k])
        a = action_of(int(out[k]), inp, n_devices, ports, on_drop, on_flood, on_bad)
        if a == RET_SKIP:
            st["skipped"] += 1
        if h >= hn:
            st["bad_home"] += 1
        if a == RET_SKIP or h >= hn:
            continue
        st["returned"] += 1
        if a == RET_DROP:
            st["dropped"] += 1
            a = home_in_dev if isinstance(home_in_dev, int) else int(home_in_dev[h])
        ho[h] = a
        if not in_place:
            hf[h, :w] = src[k, :w]
            hf[h, w:] = 0
    return hf.reshape(-1), ho, st
