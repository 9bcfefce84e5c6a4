"""The C-ABI chain object (vp_chain_*, include/vigpath.h) as
a class with vigor_amd.Chain's interface: the graph checks, the buffers, the
per-stage sequence, the origins and the way home all happen behind
vp_chain_create / vp_chain_run / vp_chain_process_device. This file only
builds the configuration, passes tensors' addresses in and wraps the views'
device pointers as tensors on the way out.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import (CABLE_SLOTS, CABLE_STREAM, VP_EINVAL, ChainConfigC, ChainExitC, ChainLinkC,
               ChainViewC, DevBatchC, TxReturnStatsC, _check)

_CABLES = {"slots": CABLE_SLOTS, "stream": CABLE_STREAM}


class _DevArray:
    """`n` items of a numpy `typestr` at a device address, for torch.as_tensor;
    keeps `owner` (whose memory it is) alive as long as the tensor."""

    def __init__(self, ptr, n, typestr, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr,
                                         "data": (ptr, False), "version": 2}


def _u32(x, what):
    x = int(x)
    if not 0 <= x <= 0xFFFFFFFF:
        raise ValueError("%s: %d is no 32-bit unsigned value" % (what, x))
    return x


class CChain:
    """vigor_amd.Chain's arguments and results (see there), the work done by
    the library: `stages` NF objects on one GPU, `links` (s, out_port, t,
    in_port) tuples, cable "slots" or "stream", exits {(stage, port):
    external_port}. Raises ValueError carrying vp_last_error() for every
    configuration vp_chain_create refuses with VP_EINVAL. The stages must stay
    open for as long as the chain is used; close() frees the chain only."""

    def __init__(self, stages, links, cable="slots", exits=None):
        if cable not in _CABLES:
            raise ValueError("cable %r is neither 'slots' nor 'stream'" % (cable,))
        self.cable = cable
        self.stages = list(stages)
        self.h = C.c_void_p()
        if not self.stages:
            raise ValueError("a chain needs a stage")
        self.L = self.stages[0].L
        k = len(self.stages)
        links = [tuple(_u32(x, "link %r" % (link,)) for x in link) for link in links]
        self.inbound = [None] * k  # per stage: (s, out_port, in_port) of its first link
        self._n_in = [0] * k       # per stage: its inbound links
        for s, out_port, t, in_port in links:
            if t < k:
                self._n_in[t] += 1
                if self.inbound[t] is None:
                    self.inbound[t] = (s, out_port, in_port)
        hs = (C.c_void_p * k)(*[nf.h.value for nf in self.stages])
        ls = (ChainLinkC * max(1, len(links)))(*[ChainLinkC(*link) for link in links])
        ex = [(_u32(s, "exit"), _u32(p, "exit"), _u32(e, "exit %r" % ((s, p),)))
              for (s, p), e in (exits or {}).items()]
        es = (ChainExitC * max(1, len(ex)))(*[ChainExitC(*e) for e in ex])
        cfg = ChainConfigC(stages=hs, n_stages=k, links=ls, n_links=len(links), exits=es,
                           n_exits=len(ex), cable=_CABLES[cable])
        rc = self.L.vp_chain_create(C.byref(cfg), C.byref(self.h))
        if rc == VP_EINVAL:
            raise ValueError((self.L.vp_last_error() or b"").decode(errors="replace")
                             or "vp_chain_create: EINVAL")
        _check(rc, "vp_chain_create", self.L)
        self.stream = None
        self._stats = TxReturnStatsC()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.vp_chain_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _batch(self, frames, lens, in_dev, out, slot, now, now0, now_step):
        n = lens.numel()
        assert frames.numel() == n * slot and frames.is_cuda
        port = isinstance(in_dev, int)
        return DevBatchC(frames=frames.data_ptr() if n else None, slot=slot, n=n,
                         len=lens.data_ptr() if n else None,
                         in_dev=None if port or not n else in_dev.data_ptr(),
                         now=now.data_ptr() if now is not None and n else None,
                         now0=now0, now_step=now_step,
                         out_dev=out.data_ptr() if out is not None and n else None,
                         in_port=in_dev if port else 0)

    def _enter(self, dev):
        """The chain's stream, ordered after the caller's current one."""
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        return C.c_void_p(self.stream.cuda_stream)

    def _views(self, frames, lens, dev):
        res = []
        v = ChainViewC()
        for s in range(len(self.stages)):
            _check(self.L.vp_chain_view_get(self.h, s, C.byref(v)), "vp_chain_view_get", self.L)
            n = v.n

            def t(ptr, typestr, count=n):
                if not count:
                    dtype = {"|u1": torch.uint8, "<i2": torch.int16, "<i4": torch.int32}[typestr]
                    return torch.zeros(0, dtype=dtype, device=dev)
                return torch.as_tensor(_DevArray(ptr, count, typestr, self), device=dev)

            if s == 0:
                r = {"n": n, "frames": frames, "lens": lens, "out": t(v.out_dev, "<i2"),
                     "origin": torch.arange(n, dtype=torch.int64, device=dev)}
            else:
                r = {"n": n, "frames": t(v.frames, "|u1", n * v.slot), "lens": t(v.len, "<i2"),
                     "out": t(v.out_dev, "<i2"),
                     "origin": t(v.origin, "<i4").to(torch.int64) & 0xFFFFFFFF}
                if self._n_in[s] > 1:  # (merged: the per-packet in port)
                    r["in_dev"] = t(v.in_dev, "<i2")
            res.append(r)
        return res

    def run(self, frames, lens, in_dev, slot: int, now=None, now0: int = 0, now_step: int = 0):
        """vp_chain_run: one batch through the chain; frames are rewritten in
        place. Returns one dict per stage as vigor_amd.Chain.run does: n,
        frames, lens, out, origin (int64) and, at a stage with several inbound
        links, in_dev. The tensors of the stages after 0 (and stage 0's out)
        wrap the chain's own buffers: valid until the next run or close()."""
        dev = frames.device
        b = self._batch(frames, lens, in_dev, None, slot, now, now0, now_step)
        _check(self.L.vp_chain_run(self.h, C.byref(b), self._enter(dev)), "vp_chain_run", self.L)
        return self._views(frames, lens, dev)

    def process_device(self, frames, lens, in_dev, out, slot: int, now=None, now0: int = 0,
                       now_step: int = 0):
        """vp_chain_process_device: the chain where one NF stands. Frames are
        rewritten in place, out[i] is a port of the composite box (`exits`)
        or, for a drop, packet i's own in port. Returns the stages'
        vp_tx_return_stats summed, as a dict."""
        b = self._batch(frames, lens, in_dev, out, slot, now, now0, now_step)
        st = self._stats
        _check(self.L.vp_chain_process_device(self.h, C.byref(b), C.byref(st),
                                              self._enter(frames.device)),
               "vp_chain_process_device", self.L)
        return {f: int(getattr(st, f)) for f, _ in TxReturnStatsC._fields_}
