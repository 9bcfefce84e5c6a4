"""Reference for vigor_amd.Chain.process_device: what the caller's batch holds
after a chain stood where one NF stands. Built from the per-stage results of
chainref.chain_reference by the rules of the composite box, restated here in
this file's own code (nothing of vigor_amd.Chain or txreturnref is used):

  * stages come home in ascending order, a later one overriding an earlier
    one's word on the same packet; of the copies one stage holds of a packet
    (consecutive, equal origins) the first counts;
  * a stage's out port is translated: a linked port leaves the packet alone,
    an exit becomes its external number, any other port is a drop; out == the
    entry's in port and a port the stage does not have are drops; a flood is
    a flood where every port of the stage is an exit, else it leaves the
    packet alone at stage 0 and is a drop later;
  * a drop comes home as the packet's own in port of the caller's batch;
  * a packet nobody writes keeps what the caller put into out (stage 0's
    frame bytes are there all the same: it rewrote the batch in place).

The chains are chainref.cases()'s, each with the exits that name its composite
box; the CPU test checks the conditions the GPU test relies on."""
import numpy as np

import chainref as CR

FLOOD = 0xFFFF
KEEP, DROP = "keep", "drop"
STATS = ("returned", "dropped", "skipped", "dup", "bad_home")

# per case: {(stage, port): external port}, and the composite box's port count
EXITS = {
    # LAN 0 -> firewall -> NAT -> WAN 1; accepted replies leave on the LAN
    "fw-nat": ({(0, 0): 0, (1, 1): 1}, 2),
    # the same, and the NAT's WAN side is the balancer's WAN port: the backends
    # sit on the balancer's ports 0 and 1, the box's 1 and 2
    "fw-nat-lb": ({(0, 0): 0, (2, 0): 1, (2, 1): 2}, 3),
    # the bridge's port 2 is policed on its way out; the policer's LAN side is
    # the box's port 2
    "bridge-pol": ({(0, 0): 0, (0, 1): 1, (0, 3): 3, (1, 1): 2}, 4),
}
NAMES = ["fw-nat", "fw-nat-lb", "bridge-pol"]


def cases():
    """{name: (chainref.Case, exits, composite port count)}."""
    base = CR.cases()
    return {name: (base[name],) + EXITS[name] for name in NAMES}


def translate(s, out, inp, n_devices, linked, exits):
    """Stage s's word on a packet it sent to `out` after receiving it on
    `inp`: KEEP, DROP or a port number of the composite box."""
    if out == inp:
        return DROP
    if out == FLOOD:
        if all((s, d) in exits for d in range(n_devices)):
            return FLOOD
        return KEEP if s == 0 else DROP
    if out >= n_devices:
        return DROP
    if out in linked:
        return KEEP
    return exits.get((s, out), DROP)


def home_reference(case, exits, res, in_dev, slot, out_before, stream=False):
    """(frames, out, stats, last) of the caller's batch after process_device.
    res: chain_reference's per-stage (origin, out, frames, lens) for the batch;
    in_dev: the batch's in ports; out_before: what out held (u16, n). stream:
    the chain's cable is "stream", so behind a link a frame's bytes past
    min(len, slot) are zero. last[i]: the stage that had the last word on
    packet i, -1 where nobody wrote it."""
    n = len(in_dev)
    origin0, _, frames0, _ = res[0]
    assert origin0.tolist() == list(range(n))
    frames = np.array(frames0, np.uint8).reshape(n, slot)  # stage 0, in place
    out = np.array(out_before, np.uint16)
    last = np.full(n, -1, np.int64)
    st = dict.fromkeys(STATS, 0)
    for s, (origin, outs, slots, lens) in enumerate(res):
        inbound = [(a, p, q) for a, p, t, q in case.links if t == s]
        assert s == 0 or len(inbound) == 1  # (one cable into every stage here)
        linked = {p for a, p, t, q in case.links if a == s}
        nd = case.stages[s].n_devices
        image = np.asarray(slots, np.uint8).reshape(-1, slot)
        if stream and s > 0:
            past = np.arange(slot)[None, :] >= np.minimum(lens.astype(np.int64), slot)[:, None]
            image = np.where(past, 0, image).astype(np.uint8)
        prev = None
        for k, i in enumerate(origin.tolist()):
            if k and i == prev:
                st["dup"] += 1
                continue
            prev = i
            inp = int(in_dev[i]) if s == 0 else inbound[0][2]
            word = translate(s, int(outs[k]), inp, nd, linked, exits)
            if word == KEEP:
                st["skipped"] += 1
                continue
            st["returned"] += 1
            if word == DROP:
                st["dropped"] += 1
                word = int(in_dev[i])
            out[i] = word
            frames[i] = image[k]
            last[i] = s
    return frames.reshape(-1), out, st, last


def conditions(case, exits, res, in_dev, slot):
    """What the GPU test relies on, as {name: count}: per stage the packets it
    has the last word on, the packets that come home dropped, and per exit the
    packets that come home on it."""
    n = len(in_dev)
    before = np.full(n, 0xABCD, np.uint16)
    _, out, _, last = home_reference(case, exits, res, in_dev, slot, before)
    written = last >= 0
    got = {"last word of stage %d" % s: int((last == s).sum()) for s in range(len(res))}
    got["dropped"] = int((written & (out == np.asarray(in_dev, np.uint16))).sum())
    for (s, p), ext in sorted(exits.items()):
        on = written & (out == ext) & (out != np.asarray(in_dev, np.uint16))
        got["exit %d (stage %d port %d)" % (ext, s, p)] = int(on.sum())
    return got
