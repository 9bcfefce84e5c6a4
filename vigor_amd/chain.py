"""NF chains on one GPU: what the reference runs as one box per NF with a
cable between each pair (firewall -> NAT, bridge -> policer, ...), as contexts
whose batches stay in device memory. A link hands one port's transmit list of
a stage to a later stage as that stage's input batch: vp_tx_build, then
vp_tx_rebatch, then vp_process_device. Several links into one
stage are merged by the packets' positions in the chain's input: vp_tx_merge
(DESIGN.md §5.8). No frame byte crosses to the host.

With cable="stream" a link into a stage with one inbound link is rehearsed as a
byte stream that could cross a device boundary: vp_tx_pack of the source
stage's lists, then vp_rx_unpack of each linked port.
"""
from __future__ import annotations

import numpy as np
import torch

from . import FLOOD_FRAME, RET_DROP, RET_SKIP, TX_MERGE_MAX, TxReturnStatsC


class Chain:
    """`stages`: NF objects (vigor_amd.Nat, Fw, ...) on one GPU. `links`:
    (s, out_port, t, in_port) tuples with t > s: what stage s sends to its
    port out_port arrives at stage t on port in_port. Every stage but 0 has
    one to TX_MERGE_MAX inbound links; anything else raises ValueError.
    Packets a stage sends to a port without a link stay in that stage's
    result with their out port: they have left the chain.

    A stage with several inbound links sees their packets merged by origin
    (each packet's index in the chain's input), as cables into one box would
    deliver them: an NF's state depends on the order and the times of its
    packets. The tie rule: copies of one input packet (floods, or a packet
    that reaches the stage through two branches) arrive in the order of the
    stage's inbound links in `links`. That is the order in which boxes pushing
    each packet through all its cables before the next would deliver them
    whenever `links` is written in depth-first order -- every link of a
    stage's subtree before the stage's next link -- and only then: the limit
    of the rule. An out port that feeds a stage with several inbound links
    carries that one link: a port named by another link as well raises
    ValueError.

    inbound[t]: the (s, out_port, in_port) of stage t's first inbound link in
    `links` order (None for stage 0); inbounds[t]: all of them, in `links`
    order.

    cable: "slots" (the default) hands a port's list over with tx_rebatch;
    "stream" feeds every stage that has one inbound link through a packed
    stream instead: one tx_pack of the source stage's lists, with pos, into a
    buffer the chain owns, then one rx_unpack per linked port. The stream
    carries min(len, slot) bytes of a frame, so the target sees zeros where the
    source slot held bytes past the frame's length. Stages with several
    inbound links keep tx_merge. Any other value raises ValueError.

    exits: {(stage, port): external_port}, the ports of the composite box that
    process_device reports: what stage `stage` sends to its unlinked port
    `port` leaves the box on external_port. An unlinked port that is no exit
    has no cable: its packets come home as drops. An exit that names a linked
    port, a port its stage does not have, or a value above 0xFFFF raises
    ValueError. `run` does not read it."""

    def __init__(self, stages, links, cable="slots", exits=None):
        if cable not in ("slots", "stream"):
            raise ValueError("cable %r is neither 'slots' nor 'stream'" % (cable,))
        self.cable = cable
        self.stages = list(stages)
        if not self.stages:
            raise ValueError("a chain needs a stage")
        k = len(self.stages)
        self.inbound = [None] * k
        self.inbounds = [[] for _ in range(k)]
        self.outbound = [[] for _ in range(k)]
        for link in links:
            s, out_port, t, in_port = (int(x) for x in link)
            if not (0 <= s < k and 0 <= t < k):
                raise ValueError("link %r names a stage outside the chain" % (link,))
            if t <= s:
                raise ValueError("link %r goes backward" % (link,))
            if not 0 <= out_port < self.stages[s].cfg.n_devices:
                raise ValueError("link %r leaves from a port stage %d does not have" % (link, s))
            if not 0 <= in_port <= 0xFFFF:
                raise ValueError("link %r arrives on a port beyond 16 bits" % (link,))
            if len(self.inbounds[t]) == TX_MERGE_MAX:
                raise ValueError("stage %d has more than %d inbound links" % (t, TX_MERGE_MAX))
            if self.inbound[t] is None:
                self.inbound[t] = (s, out_port, in_port)
            self.inbounds[t].append((s, out_port, in_port))
            self.outbound[s].append((out_port, t))
        for t in range(1, k):
            if self.inbound[t] is None:
                raise ValueError("stage %d has no inbound link" % t)
            if len(self.inbounds[t]) > 1:
                for s, out_port, _ in self.inbounds[t]:
                    if [p for p, _ in self.outbound[s]].count(out_port) > 1:
                        raise ValueError("port %d of stage %d feeds stage %d, which merges, and "
                                         "has another link" % (out_port, s, t))
        self.exits = {}
        for key, ext in (exits or {}).items():
            s, port = (int(x) for x in key)
            if not 0 <= s < k or not 0 <= port < self.stages[s].cfg.n_devices:
                raise ValueError("exit %r names a port its stage does not have" % (key,))
            if port in [p for p, _ in self.outbound[s]]:
                raise ValueError("exit %r names a linked port" % (key,))
            if not 0 <= int(ext) <= 0xFFFF:
                raise ValueError("exit %r: port %r is beyond 16 bits" % (key, ext))
            self.exits[(s, port)] = int(ext)
        self._home_stats = None  # process_device: one vp_tx_return_stats per stage
        self.stream = None
        self._lists = [None] * k  # per stage: (idx, offset)
        self._bufs = [None] * k   # per stage >= 1: its input batch's buffers
        self._packs = [None] * k  # per stage, cable "stream": (data, pos, port_off)

    def _grown(self, t, n, slot, dev, merged=False):
        """Stage t's input buffers for n packets: kept from call to call,
        replaced by larger ones on demand. merged: with the per-packet port,
        key and source number of vp_tx_merge."""
        b = self._bufs[t]
        if b is None or b["cap"] < n or b["slot"] != slot:
            cap = max(n, 2 * b["cap"] if b and b["slot"] == slot else 0, 64)
            b = {"cap": cap, "slot": slot,
                 "frames": torch.empty(cap * slot, dtype=torch.uint8, device=dev),
                 "lens": torch.empty(cap, dtype=torch.int16, device=dev),
                 "now": torch.empty(cap, dtype=torch.int64, device=dev),
                 "src": torch.empty(cap, dtype=torch.int32, device=dev),
                 "out": torch.empty(cap, dtype=torch.int16, device=dev),
                 "count": torch.zeros(1, dtype=torch.int32, device=dev)}
            if merged:
                b["in"] = torch.empty(cap, dtype=torch.int16, device=dev)
                b["key"] = torch.empty(cap, dtype=torch.int32, device=dev)
                b["which"] = torch.empty(cap, dtype=torch.uint8, device=dev)
            self._bufs[t] = b
        return b

    def run(self, frames, lens, in_dev, slot: int, now=None, now0: int = 0, now_step: int = 0):
        """One batch through the chain. frames / lens / in_dev / now / now0 /
        now_step: stage 0's batch, as for process_device (frames are rewritten
        in place). Stage 0 processes the caller's batch; then, for every stage
        in order that has a link: tx_build over its out ports, one small
        device-to-host read of offset[] to size the next batches (the one host
        synchronisation per stage), tx_rebatch of each linked port into buffers
        the chain owns (cable "stream": one tx_pack of all the lists, then
        rx_unpack of each linked port), and process_device of the target stage with every
        packet on the link's in_port and the gathered per-packet times. A
        stage with several inbound links gets its input when it is reached,
        after every earlier stage ran: one tx_merge over its links' lists (in
        `links` order, each keyed by its source stage's origins), sized from
        the offset[] reads already made, then process_device with the merged
        per-packet ports and times. All of it is enqueued on one stream of the
        chain's, which is waited for once more before the call returns.

        Returns one dict per stage: n (packets the stage received), frames
        (n * slot bytes, as the stage left them), lens, out (its out ports)
        and origin (int64: each packet's index in the caller's batch, composed
        from the links' src arrays; at a merged stage the merged keys), and at
        a merged stage in_dev (the per-packet in port). The tensors of the
        stages after 0 are the chain's own buffers: valid until the next run.
        State persists across calls in the stages' contexts."""
        dev = frames.device
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)
        S = self.stream
        S.wait_stream(torch.cuda.current_stream(dev))
        k = len(self.stages)
        n0 = lens.numel()
        res = [None] * k
        with torch.cuda.stream(S):
            out0 = torch.zeros(n0, dtype=torch.int16, device=dev)
            if n0:
                self.stages[0].process_device(frames, lens, in_dev, out0, slot, now=now,
                                              now0=now0, now_step=now_step, stream=S)
            res[0] = {"n": n0, "frames": frames, "lens": lens, "out": out0,
                      "origin": torch.arange(n0, dtype=torch.int64, device=dev)}
            time = [(now, now0, now_step)] + [None] * (k - 1)
            ports = [in_dev] + [None] * (k - 1)
            offsets = [None] * k  # per stage with built lists: offset[] on the host
            merges = [len(x) > 1 for x in self.inbounds]
            for s in range(k):
                if merges[s]:
                    res[s] = self._merge(s, res, offsets, time, ports, slot, dev)
                r = res[s]
                if not self.outbound[s] or r["n"] == 0:
                    for _, t in self.outbound[s]:
                        if not merges[t]:
                            res[t] = self._empty(slot, dev)
                    continue
                nf = self.stages[s]
                nd = nf.cfg.n_devices
                offset = offsets[s] = self._build(s, nf, nd, r, ports[s], dev)
                idx = self._lists[s][0]
                t_now, t_now0, t_step = time[s]
                packed = None  # cable "stream": this stage's lists, packed once
                for out_port, t in self.outbound[s]:
                    if merges[t]:
                        continue  # (assembled when stage t is reached)
                    cnt = int(offset[out_port + 1]) - int(offset[out_port])
                    if cnt == 0:
                        res[t] = self._empty(slot, dev)
                        continue
                    b = self._grown(t, cnt, slot, dev)
                    if self.cable == "stream":
                        if packed is None:
                            packed = self._pack(s, nf, nd, r, int(offset[nd]), slot, dev)
                        lo = int(offset[out_port])
                        nf.rx_unpack(packed[0], r["lens"], b["frames"][:cnt * slot], slot,
                                     b["lens"][:cnt], b["count"], pos=packed[1][lo:lo + cnt],
                                     sel=idx[lo:lo + cnt], out_now=b["now"][:cnt],
                                     out_src=b["src"][:cnt], now=t_now, now0=t_now0,
                                     now_step=t_step, stream=S)
                    else:
                        nf.tx_rebatch(r["frames"], slot, r["lens"], idx, self._lists[s][1],
                                      out_port, b["frames"][:cnt * slot], slot, b["lens"][:cnt],
                                      b["count"], out_now=b["now"][:cnt], out_src=b["src"][:cnt],
                                      now=t_now, now0=t_now0, now_step=t_step, stream=S)
                    in_port = self.inbound[t][2]
                    self.stages[t].process_device(b["frames"][:cnt * slot], b["lens"][:cnt],
                                                  in_port, b["out"][:cnt], slot,
                                                  now=b["now"][:cnt], stream=S)
                    time[t] = (b["now"][:cnt], 0, 0)
                    ports[t] = in_port
                    res[t] = {"n": cnt, "frames": b["frames"][:cnt * slot],
                              "lens": b["lens"][:cnt], "out": b["out"][:cnt],
                              "origin": r["origin"][b["src"][:cnt].long()]}
        S.synchronize()
        return res

    def way_home(self, s):
        """Stage s's actions for tx_return, as (ports, on_drop, on_flood,
        on_bad): a linked port is RET_SKIP (the packet travelled on; the stage
        it reached has the later word), an exit its external number, any other
        port RET_DROP (no cable); a drop and an out port the stage does not
        have are RET_DROP. A flood's copies take different ways and a home
        slot holds one out port, so: where every port of the stage is an exit
        the flood is the composite's own (FLOOD_FRAME); otherwise stage 0
        leaves the packet alone (RET_SKIP), for a stage that a copy reached to
        decide, and a later stage drops it."""
        nd = self.stages[s].cfg.n_devices
        linked = {p for p, _ in self.outbound[s]}
        ports = [RET_SKIP if d in linked else self.exits.get((s, d), RET_DROP) for d in range(nd)]
        if all((s, d) in self.exits for d in range(nd)):
            on_flood = FLOOD_FRAME
        else:
            on_flood = RET_SKIP if s == 0 else RET_DROP
        return ports, RET_DROP, on_flood, RET_DROP

    def process_device(self, frames, lens, in_dev, out, slot: int, now=None, now0: int = 0,
                       now_step: int = 0):
        """The chain where one NF stands: an NF's process_device signature, and
        afterwards the caller's batch as one box holding the whole chain would
        leave it -- frames rewritten in place, out[i] a port of the composite
        box (`exits`) or, for a drop, packet i's own in port.

        Calls run, then, for every stage in ascending order that received
        packets, one tx_return into the caller's batch: home = the stage's
        origins (stage 0: the in-place form), the actions way_home's. A later
        stage's return overrides an earlier one's for the same packet; of the
        copies one stage holds of a packet (floods merged back together) the
        first counts. A packet that stage 0 flooded and no copy of which
        reached a later stage is not written: out keeps the caller's value
        there (way_home's rule). All returns go on the chain's stream, which is
        waited for once at the end. Returns the stages' vp_tx_return_stats
        summed, as a dict."""
        res = self.run(frames, lens, in_dev, slot, now=now, now0=now0, now_step=now_step)
        dev, S, k = frames.device, self.stream, len(self.stages)
        names = [f for f, _ in TxReturnStatsC._fields_]
        if self._home_stats is None or self._home_stats.device != dev:
            self._home_stats = torch.zeros(k, len(names), dtype=torch.int64, device=dev)
        stats = self._home_stats
        with torch.cuda.stream(S):
            stats.zero_()
            for s, r in enumerate(res):
                if r is None or r["n"] == 0:
                    continue
                ports, on_drop, on_flood, on_bad = self.way_home(s)
                if s == 0:
                    s_in, home = in_dev, None
                else:
                    s_in = r["in_dev"] if "in_dev" in r else self.inbound[s][2]
                    home = r["key"] if "key" in r else r["origin"].to(torch.int32)
                self.stages[s].tx_return(r["frames"], slot, r["out"], s_in, frames, slot, out,
                                         in_dev, ports, on_drop, on_flood, on_bad, home=home,
                                         stats=stats[s], stream=S)
        S.synchronize()
        total = stats.sum(dim=0).cpu().tolist()
        return dict(zip(names, total))

    def _merge(self, t, res, offsets, time, ports, slot, dev):
        """Stage t's input from its several inbound links, and its run: one
        tx_merge over the links' lists in `links` order, each source keyed by
        its stage's origins (stage 0's are the packet indices: no key array),
        then process_device with the merged per-packet ports and times."""
        sources, cnt = [], 0
        for s, out_port, in_port in self.inbounds[t]:
            r = res[s]
            if r["n"] == 0 or offsets[s] is None:
                continue
            c = int(offsets[s][out_port + 1]) - int(offsets[s][out_port])
            if c == 0:
                continue
            cnt += c
            if s and "key" not in r:
                r["key"] = r["origin"].to(torch.int32)
            idx, off_t = self._lists[s]
            sources.append((self.stages[s], r["frames"], slot, r["lens"], idx, off_t, out_port,
                            in_port, r["key"] if s else None) + tuple(time[s]))
        if cnt == 0:
            res_t = self._empty(slot, dev)
            res_t["in_dev"] = res_t["lens"].clone()
            return res_t
        b = self._grown(t, cnt, slot, dev, merged=True)
        S = self.stream
        self.stages[t].tx_merge(sources, b["frames"][:cnt * slot], slot, b["lens"][:cnt],
                                b["count"], b["src"][:cnt], b["which"][:cnt],
                                out_now=b["now"][:cnt], out_in_dev=b["in"][:cnt],
                                out_key=b["key"][:cnt], stream=S)
        self.stages[t].process_device(b["frames"][:cnt * slot], b["lens"][:cnt], b["in"][:cnt],
                                      b["out"][:cnt], slot, now=b["now"][:cnt], stream=S)
        time[t] = (b["now"][:cnt], 0, 0)
        ports[t] = b["in"][:cnt]
        return {"n": cnt, "frames": b["frames"][:cnt * slot], "lens": b["lens"][:cnt],
                "out": b["out"][:cnt], "origin": b["key"][:cnt].long(),
                "in_dev": b["in"][:cnt], "key": b["key"][:cnt]}

    def _pack(self, s, nf, nd, r, total, slot, dev):
        """Stage s's lists as one packed stream (cable "stream"): tx_pack with
        pos into a buffer of total * slot bytes, which holds every listed frame
        at its padded length. Returns (data, pos); the buffers are kept from
        call to call and replaced by larger ones on demand."""
        idx, off_t = self._lists[s]
        p = self._packs[s]
        if p is None or p[0].numel() < total * slot or p[1].numel() < idx.numel():
            p = self._packs[s] = (torch.empty(total * slot, dtype=torch.uint8, device=dev),
                                  torch.empty(idx.numel(), dtype=torch.int64, device=dev),
                                  torch.zeros(nd + 1, dtype=torch.int64, device=dev))
        data = p[0][:total * slot]
        nf.tx_pack(r["frames"], slot, r["lens"], idx, off_t, data, p[2], pos=p[1],
                   stream=self.stream)
        return data, p[1]

    @staticmethod
    def _empty(slot, dev):
        z16 = torch.zeros(0, dtype=torch.int16, device=dev)
        return {"n": 0, "frames": torch.zeros(0, dtype=torch.uint8, device=dev), "lens": z16,
                "out": z16.clone(), "origin": torch.zeros(0, dtype=torch.int64, device=dev)}

    def _build(self, s, nf, nd, r, in_dev, dev):
        """Stage s's transmit lists over its result; returns offset[] on the
        host. A list that outgrew idx (floods) is built again with room."""
        n = r["n"]
        if self._lists[s] is None or self._lists[s][0].numel() < n:
            self._lists[s] = (torch.empty(n, dtype=torch.int32, device=dev),
                              torch.zeros(nd + 1, dtype=torch.int32, device=dev))
        while True:
            idx, off_t = self._lists[s]
            nf.tx_build(r["out"], in_dev, r["lens"], idx, off_t, None, stream=self.stream)
            offset = off_t.cpu().numpy().view(np.uint32)  # (waits for the stream)
            if int(offset[nd]) <= idx.numel():
                return offset
            self._lists[s] = (torch.empty(int(offset[nd]), dtype=torch.int32, device=dev), off_t)
