"""NF instances on the GPU: the batch form of the reference operator
`int nf_process(uint16_t device, uint8_t *buffer, uint16_t len, vigor_time_t
now)` (nf.h:13), driven the way nf.c's loop drives it (nf.c:150-176).

`process_device` takes torch tensors already in HBM; `process_host` takes
numpy arrays and stages them through pinned memory (hipMemcpyAsync);
`process` is the per-packet nf_process equivalent (one-packet batch).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import (BridgeConfigC, DevBatchC, FwConfigC, LbConfigC, MAX_DEV, MbufBatchC,
               NatConfigC, PolConfigC, RX_MERGE_MAX, RxQueueC, RxStreamC, ServeExpiryStatsC, ServeStatsC, StateMarkC, TableStatsC,
               TX_MERGE_MAX, TxFramesC, TxListsC, TxMergedC, TxNextC, TxReturnStatsC, TxSourceC,
               TxStatsC, TxWayHomeC, VpLookupOutC, _check, lib)


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _rx_stream(data, lens, pos, sel, now, now0, now_step, n):
    """vp_rx_stream of rx_unpack's arguments of these names (one queue of
    rx_merge's)."""
    meta_n = lens.numel() if lens is not None else 0
    nbytes = data.numel() if data is not None else 0
    if n is None:
        n = sel.numel() if sel is not None else pos.numel() if pos is not None else meta_n
    if nbytes:
        assert data.is_cuda and data.element_size() == 1
    if meta_n:
        assert lens.is_cuda and lens.element_size() == 2
    if pos is not None:
        assert pos.is_cuda and pos.element_size() == 8 and pos.numel() >= n
    if sel is not None:
        assert sel.is_cuda and sel.element_size() == 4 and sel.numel() >= n
    if now is not None:
        assert now.is_cuda and now.element_size() == 8 and now.numel() == meta_n
    return RxStreamC(data=_dptr(data) if nbytes else None, bytes=nbytes, n=n,
                     pos=_dptr(pos) if n else None, sel=_dptr(sel) if n else None,
                     meta_n=meta_n, len=_dptr(lens) if meta_n else None,
                     now=_dptr(now) if meta_n else None, now0=now0, now_step=now_step)


class NfBase:
    kind = "?"
    gpu = 0

    def __init__(self, libpath=None):
        self.h = C.c_void_p()
        self.L = lib(libpath)

    def _ck(self, rc: int, what: str):
        _check(rc, what, self.L)  # vp_last_error() of this instance's library

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.vp_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --------------------------------------------------------- device --
    def process_device(self, frames, lens, in_dev, out, slot: int, now=None,
                       now0: int = 0, now_step: int = 0, stream=None):
        """frames: uint8 CUDA tensor of n*slot bytes (mutated in place);
        lens/in_dev/out: int16/uint16-sized CUDA tensors of n (in_dev an int:
        every packet on that port, vp_dev_batch.in_port); now: int64 CUDA
        tensor of n, or None for now0 + i*now_step."""
        n = lens.numel()
        assert frames.numel() == n * slot and frames.is_cuda
        port = isinstance(in_dev, int)
        b = DevBatchC(frames=frames.data_ptr(), slot=slot, n=n,
                      len=lens.data_ptr(), in_dev=None if port else in_dev.data_ptr(),
                      now=now.data_ptr() if now is not None else None,
                      now0=now0, now_step=now_step, out_dev=out.data_ptr(),
                      in_port=in_dev if port else 0)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_process_device(self.h, C.byref(b), s),
               "vp_process_device")

    def device_step(self, frames, lens, in_dev, out, slot: int):
        """A prepared vp_process_device call over fixed device buffers with
        affine time: returns f(now0, now_step). The batch descriptor and its
        pointers are built once (a C caller's per-burst cost), so a loop of
        calls pays only the C-ABI call itself. The callable keeps the tensors
        alive: the descriptor holds their raw device pointers. in_dev: as for
        process_device (an int: the burst's one port)."""
        n = lens.numel()
        assert frames.numel() == n * slot and frames.is_cuda
        port = isinstance(in_dev, int)
        b = DevBatchC(frames=frames.data_ptr(), slot=slot, n=n,
                      len=lens.data_ptr(), in_dev=None if port else in_dev.data_ptr(),
                      now=None, now0=0, now_step=0, out_dev=out.data_ptr(),
                      in_port=in_dev if port else 0)
        ref, fn, h, L = C.byref(b), self.L.vp_process_device, self.h, self.L
        keep = (frames, lens, in_dev, out)

        def step(now0: int, now_step: int):
            b.now0, b.now_step = now0, now_step
            rc = fn(h, ref, None)
            if rc:
                _check(rc, "vp_process_device", L)
        step.tensors = keep
        return step

    def device_steps(self, frames_list, lens, in_dev, out, slot: int):
        """The loop of device_step calls in C (host/steps.c,
        libvp_steps.so): one vp_process_device per buffer of frames_list, in
        order, as nf.c's loop makes one call per burst. Returns
        f(now0s, now_step) that runs them all (now0s: each batch's first time
        stamp). Measurement infrastructure: no interpreter between the
        calls."""
        import os
        n = lens.numel()
        port = isinstance(in_dev, int)
        arr = (DevBatchC * len(frames_list))()
        for k, fr in enumerate(frames_list):
            assert fr.numel() == n * slot and fr.is_cuda
            arr[k] = DevBatchC(frames=fr.data_ptr(), slot=slot, n=n, len=lens.data_ptr(),
                               in_dev=None if port else in_dev.data_ptr(), now=None,
                               now0=0, now_step=0, out_dev=out.data_ptr(),
                               in_port=in_dev if port else 0)
        S = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(self.L._name)),
                                "libvp_steps.so"))
        S.vp_steps_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_int)]
        keep = (list(frames_list), lens, in_dev, out)

        def run(now0s, now_step: int):
            assert len(now0s) == len(arr)
            for k, t0 in enumerate(now0s):
                arr[k].now0, arr[k].now_step = t0, now_step
            done = C.c_int()
            rc = S.vp_steps_device(self.h, C.cast(arr, C.c_void_p), len(arr),
                                   C.byref(done))
            if rc:
                _check(rc, "vp_process_device (call %d)" % done.value, self.L)
        run.tensors = keep
        return run

    def tx_build(self, out, in_dev, lens, idx, offset, stats=None, stream=None):
        """vp_tx_build: the per-port transmit lists of a device-resident batch
        from its out ports (what nf.c does with nf_process's return value,
        nf.c:159-174). out / lens: 16-bit CUDA tensors of n; in_dev: the same,
        or an int (every packet on that port), as for process_device. idx:
        int32/uint32 CUDA tensor whose length is the capacity (None: capacity
        0, only offsets and stats); offset: the same kind, n_devices + 1
        entries; stats: None or a CUDA tensor of at least
        sizeof(vigor_amd.TxStatsC) bytes. Enqueued on `stream` (the context's
        own for None) and not waited for: synchronize before reading."""
        port = isinstance(in_dev, int)
        n = out.numel()
        # (an empty tensor has no address and a NULL out_dev is VP_EINVAL: with
        # n == 0 nothing is read through it, any device address serves)
        b = DevBatchC(n=n, len=_dptr(lens),
                      in_dev=None if port else in_dev.data_ptr(),
                      out_dev=out.data_ptr() if n else offset.data_ptr(),
                      in_port=in_dev if port else 0)
        if idx is not None:
            assert idx.is_cuda and idx.element_size() == 4
        assert offset.is_cuda and offset.element_size() == 4
        if stats is not None:
            assert stats.is_cuda and stats.numel() * stats.element_size() >= C.sizeof(TxStatsC)
        lists = TxListsC(idx=_dptr(idx), cap=idx.numel() if idx is not None else 0,
                         offset=offset.data_ptr(), stats=_dptr(stats))
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_tx_build(self.h, C.byref(b), C.byref(lists), s), "vp_tx_build")

    def tx_pack(self, frames, slot, lens, idx, offset, data, port_off, pos=None, stream=None):
        """vp_tx_pack: the frames that tx_build's lists name, packed into one
        byte stream per port (each frame at min(len, slot) bytes, zero-padded
        to 16). frames: uint8 CUDA tensor of n * slot bytes (only read); lens:
        16-bit CUDA tensor of n; idx / offset: as tx_build wrote them (idx
        None: capacity 0); data: uint8 CUDA tensor whose size is the capacity
        in bytes (None: 0); port_off: 64-bit CUDA tensor of n_devices + 1;
        pos: None or a 64-bit CUDA tensor of at least idx's length. Enqueued
        on `stream` (the context's own for None) and not waited for."""
        n = lens.numel()
        assert frames.numel() == n * slot
        b = DevBatchC(frames=_dptr(frames) if n else None, slot=slot, n=n,
                      len=_dptr(lens) if n else None)
        cap = idx.numel() if idx is not None else 0
        if idx is not None:
            assert idx.is_cuda and idx.element_size() == 4
        assert offset.is_cuda and offset.element_size() == 4
        assert port_off.is_cuda and port_off.element_size() == 8
        if data is not None:
            assert data.is_cuda and data.element_size() == 1
        if pos is not None:
            assert pos.is_cuda and pos.element_size() == 8 and pos.numel() >= cap
        cap_bytes = data.numel() if data is not None else 0
        lists = TxListsC(idx=_dptr(idx) if cap else None, cap=cap, offset=offset.data_ptr(),
                         stats=None)
        out = TxFramesC(data=_dptr(data) if cap_bytes else None, cap_bytes=cap_bytes,
                        port_off=port_off.data_ptr(), pos=_dptr(pos) if cap else None)
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_tx_pack(self.h, C.byref(b), C.byref(lists), C.byref(out), s),
                 "vp_tx_pack")

    def tx_rebatch(self, frames, slot, lens, idx, offset, port, out_frames, out_slot, out_lens,
                   count, out_now=None, out_src=None, now=None, now0: int = 0,
                   now_step: int = 0, stream=None):
        """vp_tx_rebatch: list `port` of tx_build's lists as the next NF's
        device batch -- the listed slots gathered into consecutive slots of
        out_frames (out_slot bytes each, zero-filled past the narrower slot),
        with len[], the per-packet time and the index of origin carried along.
        frames: uint8 CUDA tensor of n * slot bytes (only read); lens: 16-bit
        CUDA tensor of n; now: None (now0 + i * now_step) or a 64-bit CUDA
        tensor of n; idx / offset: as tx_build wrote them (idx None: capacity
        0). out_lens: 16-bit CUDA tensor whose length is the capacity in
        packets (None: 0); out_frames: uint8 CUDA tensor of capacity *
        out_slot bytes; out_now: None or a 64-bit tensor, out_src: None or a
        32-bit tensor, each of at least the capacity; count: 32-bit CUDA
        tensor of one word, the list's true length afterwards. Enqueued on
        `stream` (the context's own for None) and not waited for."""
        n = lens.numel()
        assert frames.numel() == n * slot
        cap = out_lens.numel() if out_lens is not None else 0
        if idx is not None:
            assert idx.is_cuda and idx.element_size() == 4
        assert offset.is_cuda and offset.element_size() == 4
        assert count.is_cuda and count.element_size() == 4 and count.numel() >= 1
        if cap:
            assert out_lens.is_cuda and out_lens.element_size() == 2
            assert out_frames.is_cuda and out_frames.element_size() == 1
            assert out_frames.numel() == cap * out_slot
        if out_now is not None:
            assert out_now.is_cuda and out_now.element_size() == 8 and out_now.numel() >= cap
        if out_src is not None:
            assert out_src.is_cuda and out_src.element_size() == 4 and out_src.numel() >= cap
        if now is not None:
            assert now.is_cuda and now.element_size() == 8 and now.numel() == n
        b = DevBatchC(frames=_dptr(frames) if n else None, slot=slot, n=n,
                      len=_dptr(lens) if n else None,
                      now=_dptr(now) if n else None, now0=now0, now_step=now_step)
        lcap = idx.numel() if idx is not None else 0
        lists = TxListsC(idx=_dptr(idx) if lcap else None, cap=lcap, offset=offset.data_ptr(),
                         stats=None)
        out = TxNextC(frames=_dptr(out_frames) if cap else None, slot=out_slot, cap=cap,
                      len=_dptr(out_lens) if cap else None,
                      now=_dptr(out_now) if cap else None,
                      src=_dptr(out_src) if cap else None, count=count.data_ptr())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_tx_rebatch(self.h, C.byref(b), C.byref(lists), port, C.byref(out), s),
                 "vp_tx_rebatch")

    def tx_merge(self, sources, out_frames, out_slot, out_lens, count, out_src, out_which,
                 out_now=None, out_in_dev=None, out_key=None, stream=None):
        """vp_tx_merge: several lists of tx_build's as this NF's device batch,
        merged by a 32-bit key per packet (stable: equal keys in the order of
        `sources`, inside a source in list order). sources: 1 to TX_MERGE_MAX
        tuples (nf, frames, slot, lens, idx, offset, port, in_port, key, now,
        now0, now_step), the tail from `key` on optional (None, None, 0, 0):
        nf the NF whose tx_build wrote idx / offset over that batch, frames /
        slot / lens / now / now0 / now_step the batch as for tx_rebatch, port
        the list, in_port the port its packets arrive on here, key None (the
        packet's index) or a 32-bit CUDA tensor of n that does not decrease
        along the list. out_lens: 16-bit CUDA tensor whose length is the
        capacity in packets (None: 0); out_frames: uint8 CUDA tensor of
        capacity * out_slot bytes; out_src (32-bit) and out_which (8-bit) are
        needed with a capacity; out_now (64-bit), out_in_dev (16-bit) and
        out_key (32-bit) may be None; count: 32-bit CUDA tensor of one word,
        the lists' true total afterwards. Enqueued on `stream` (this
        context's own for None) and not waited for."""
        sources = [tuple(s) + (None, None, 0, 0)[len(tuple(s)) - 8:] for s in sources]
        assert 1 <= len(sources) <= TX_MERGE_MAX
        cap = out_lens.numel() if out_lens is not None else 0
        assert count.is_cuda and count.element_size() == 4 and count.numel() >= 1
        if cap:
            assert out_lens.is_cuda and out_lens.element_size() == 2
            assert out_frames.is_cuda and out_frames.element_size() == 1
            assert out_frames.numel() == cap * out_slot
            assert out_src.is_cuda and out_src.element_size() == 4 and out_src.numel() >= cap
            assert out_which.is_cuda and out_which.element_size() == 1
            assert out_which.numel() >= cap
        for t, width in ((out_now, 8), (out_in_dev, 2), (out_key, 4)):
            if t is not None:
                assert t.is_cuda and t.element_size() == width and t.numel() >= cap
        arr = (TxSourceC * len(sources))()
        keep = []  # (the structs the array points to)
        for a, (nf, frames, slot, lens, idx, offset, port, in_port, key, now, now0,
                now_step) in zip(arr, sources):
            n = lens.numel()
            assert frames.numel() == n * slot
            if idx is not None:
                assert idx.is_cuda and idx.element_size() == 4
            assert offset.is_cuda and offset.element_size() == 4
            if now is not None:
                assert now.is_cuda and now.element_size() == 8 and now.numel() == n
            if key is not None:
                assert key.is_cuda and key.element_size() == 4 and key.numel() == n
            b = DevBatchC(frames=_dptr(frames) if n else None, slot=slot, n=n,
                          len=_dptr(lens) if n else None,
                          now=_dptr(now) if n else None, now0=now0, now_step=now_step)
            lcap = idx.numel() if idx is not None else 0
            lists = TxListsC(idx=_dptr(idx) if lcap else None, cap=lcap,
                             offset=offset.data_ptr(), stats=None)
            keep += [b, lists]
            a.ctx, a.batch, a.lists = nf.h, C.addressof(b), C.addressof(lists)
            a.port, a.in_port = port, in_port
            a.key = _dptr(key) if n else None
        out = TxMergedC(frames=_dptr(out_frames) if cap else None, slot=out_slot, cap=cap,
                        len=_dptr(out_lens) if cap else None,
                        now=_dptr(out_now) if cap else None,
                        in_dev=_dptr(out_in_dev) if cap else None,
                        key=_dptr(out_key) if cap else None,
                        src=_dptr(out_src) if cap else None,
                        which=_dptr(out_which) if cap else None, count=count.data_ptr())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_tx_merge(self.h, arr, len(sources), C.byref(out), s), "vp_tx_merge")

    def rx_unpack(self, data, lens, out_frames, out_slot, out_lens, count, pos=None, sel=None,
                  out_now=None, out_src=None, now=None, now0: int = 0, now_step: int = 0,
                  n=None, stream=None):
        """vp_rx_unpack: a packed stream of frames (tx_pack's, a capture, a
        buffer another device wrote) as a device batch -- entry e's frame,
        r = min(len, out_slot) bytes at a 16-byte aligned position of `data`,
        into slot e of out_frames, zero-filled behind, with len[], the time and
        the index m(e) into lens / now carried along. data: uint8 CUDA tensor
        whose size is the readable bytes (None: 0); lens: 16-bit CUDA tensor of
        meta_n entries (None: 0); now: None (now0 + m * now_step) or a 64-bit
        CUDA tensor of meta_n; pos: None (the frames lie back to back at their
        lengths rounded up to 16) or a 64-bit CUDA tensor of byte offsets; sel:
        None (m(e) = e) or a 32-bit CUDA tensor. n: the entries, by default
        sel's length, else pos's, else meta_n; pos and sel hold at least n.
        out_lens: 16-bit CUDA tensor whose length is the capacity in packets
        (None: 0); out_frames: uint8 CUDA tensor of capacity * out_slot bytes;
        out_now: None or a 64-bit tensor, out_src: None or a 32-bit tensor,
        each of at least the capacity; count: 32-bit CUDA tensor of one word,
        n afterwards. Enqueued on `stream` (the context's own for None) and
        not waited for."""
        cap = out_lens.numel() if out_lens is not None else 0
        rx = _rx_stream(data, lens, pos, sel, now, now0, now_step, n)
        assert count.is_cuda and count.element_size() == 4 and count.numel() >= 1
        if cap:
            assert out_lens.is_cuda and out_lens.element_size() == 2
            assert out_frames.is_cuda and out_frames.element_size() == 1
            assert out_frames.numel() == cap * out_slot
        if out_now is not None:
            assert out_now.is_cuda and out_now.element_size() == 8 and out_now.numel() >= cap
        if out_src is not None:
            assert out_src.is_cuda and out_src.element_size() == 4 and out_src.numel() >= cap
        out = TxNextC(frames=_dptr(out_frames) if cap else None, slot=out_slot, cap=cap,
                      len=_dptr(out_lens) if cap else None,
                      now=_dptr(out_now) if cap else None,
                      src=_dptr(out_src) if cap else None, count=count.data_ptr())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_rx_unpack(self.h, C.byref(rx), C.byref(out), s), "vp_rx_unpack")

    def rx_merge(self, queues, out_frames, out_slot, out_lens, count, out_src, out_which,
                 out_now=None, out_in_dev=None, stream=None):
        """vp_rx_merge: several packed streams, one per port, as this NF's
        device batch, merged by each frame's signed 64-bit time (stable: equal
        times in the order of `queues`, inside a queue in entry order), every
        slot, len and src as rx_unpack writes them; an entry that is not
        readable keeps its time. queues: 1 to RX_MERGE_MAX dicts with the keys
        data, lens, in_port and optionally pos, sel, now, now0, now_step, n --
        rx_unpack's arguments of those names -- or tuples (data, lens, in_port,
        pos, sel, now, now0, now_step, n), the tail from `pos` on optional.
        Every queue's times must not decrease along its entries. out_lens:
        16-bit CUDA tensor whose length is the capacity in packets (None: 0);
        out_frames: uint8 CUDA tensor of capacity * out_slot bytes; out_src
        (32-bit) and out_which (8-bit) are needed with a capacity; out_now
        (64-bit) and out_in_dev (16-bit) may be None; count: 32-bit CUDA tensor
        of one word, the queues' true total afterwards. Enqueued on `stream`
        (this context's own for None) and not waited for."""
        names = ("data", "lens", "in_port", "pos", "sel", "now", "now0", "now_step", "n")
        queues = [q if isinstance(q, dict) else dict(zip(names, q)) for q in queues]
        assert 1 <= len(queues) <= RX_MERGE_MAX
        cap = out_lens.numel() if out_lens is not None else 0
        assert count.is_cuda and count.element_size() == 4 and count.numel() >= 1
        if cap:
            assert out_lens.is_cuda and out_lens.element_size() == 2
            assert out_frames.is_cuda and out_frames.element_size() == 1
            assert out_frames.numel() == cap * out_slot
            assert out_src.is_cuda and out_src.element_size() == 4 and out_src.numel() >= cap
            assert out_which.is_cuda and out_which.element_size() == 1
            assert out_which.numel() >= cap
        for t, width in ((out_now, 8), (out_in_dev, 2)):
            if t is not None:
                assert t.is_cuda and t.element_size() == width and t.numel() >= cap
        arr = (RxQueueC * len(queues))()
        for a, q in zip(arr, queues):
            a.stream = _rx_stream(q["data"], q["lens"], q.get("pos"), q.get("sel"), q.get("now"),
                                  q.get("now0") or 0, q.get("now_step") or 0, q.get("n"))
            a.in_port = q["in_port"]
        out = TxMergedC(frames=_dptr(out_frames) if cap else None, slot=out_slot, cap=cap,
                        len=_dptr(out_lens) if cap else None,
                        now=_dptr(out_now) if cap else None,
                        in_dev=_dptr(out_in_dev) if cap else None, key=None,
                        src=_dptr(out_src) if cap else None,
                        which=_dptr(out_which) if cap else None, count=count.data_ptr())
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_rx_merge(self.h, arr, len(queues), C.byref(out), s), "vp_rx_merge")

    def tx_return(self, frames, slot, out, in_dev, home_frames, home_slot, home_out, home_in_dev,
                  ports, on_drop, on_flood, on_bad, home=None, stats=None, stream=None):
        """vp_tx_return: this NF's batch back in the slots its packets started
        from -- the inverse of tx_rebatch. Entry k goes to slot home[k] of
        home_frames (k itself for home None) if it is the first of its run of
        equal homes, and its out port, translated, to home_out[home[k]]:
        ports[d] for out == d, on_drop for out == the entry's in port, on_flood
        for FLOOD_FRAME, on_bad for anything else; each a port number up to
        0xFFFF, RET_SKIP (leave the home packet alone) or RET_DROP (the home
        packet's own in port). frames: uint8 CUDA tensor of n * slot bytes
        (only read); out: 16-bit CUDA tensor of n; in_dev: the same, or an int
        (every packet on that port); home_frames / home_out / home_in_dev: the
        same of the home batch, its n that of home_out; ports: n_devices
        values; home: None or a 32-bit CUDA tensor of n that does not decrease;
        stats: None or a CUDA tensor of at least sizeof(vigor_amd.
        TxReturnStatsC) bytes. frames and home_frames the same memory with
        equal slots and home None: the batch is its own home, only the out
        ports are translated (out and home_out may then be one tensor).
        Enqueued on `stream` (the context's own for None) and not waited for."""
        n, hn = out.numel(), home_out.numel()
        assert frames.numel() == n * slot and home_frames.numel() == hn * home_slot
        assert len(ports) <= MAX_DEV
        port, hport = isinstance(in_dev, int), isinstance(home_in_dev, int)
        for t, width, count in ((frames, 1, n * slot), (out, 2, n), (None if port else in_dev, 2, n),
                                (home_frames, 1, hn * home_slot), (home_out, 2, hn),
                                (None if hport else home_in_dev, 2, hn), (home, 4, n)):
            if t is not None and count:
                assert t.is_cuda and t.element_size() == width and t.numel() >= count
        if stats is not None:
            assert stats.is_cuda
            assert stats.numel() * stats.element_size() >= C.sizeof(TxReturnStatsC)
        b = DevBatchC(frames=_dptr(frames) if n else None, slot=slot, n=n,
                      in_dev=None if port or not n else in_dev.data_ptr(),
                      out_dev=_dptr(out) if n else None, in_port=in_dev if port else 0)
        hb = DevBatchC(frames=_dptr(home_frames) if hn else None, slot=home_slot, n=hn,
                       in_dev=None if hport or not hn else home_in_dev.data_ptr(),
                       out_dev=_dptr(home_out) if hn else None,
                       in_port=home_in_dev if hport else 0)
        way = TxWayHomeC(home=_dptr(home) if n else None, on_drop=on_drop, on_flood=on_flood,
                         on_bad=on_bad, stats=_dptr(stats))
        for d, a in enumerate(ports):
            way.port[d] = a
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(self.L.vp_tx_return(self.h, C.byref(b), C.byref(hb), C.byref(way), s),
                 "vp_tx_return")

    def sync_state(self):
        """Multi-GPU: merge the ranks' timestamps (collective)."""
        self._ck(self.L.vp_sync_state(self.h), "vp_sync_state")

    def kernel_timing(self, on: bool = True):
        """Bracket every classification kernel launch with HIP events
        (vp_kernel_timing; off by default: the events cost a step about 6 us),
        so that last_kernel_ms() reports its time."""
        self._ck(self.L.vp_kernel_timing(self.h, 1 if on else 0), "vp_kernel_timing")

    def last_kernel_ms(self):
        if not hasattr(self, "_kms"):  # (built once: called every batch)
            ms, k = C.c_float(), C.c_int()
            self._kms = (ms, k, C.byref(ms), C.byref(k))
        ms, k, rms, rk = self._kms
        self._ck(self.L.vp_last_kernel_ms(self.h, rms, rk), "vp_last_kernel_ms")
        return ms.value, k.value

    def last_kernel(self) -> str:
        """vp_last_kernel: the tile kernel the last call launched ("" if none).
        vigpol: the classify kernel plus the phase-T path of the call's last
        segment, e.g. "pol_classify64+pol_runs", "pol_classify+pol_scatter+pol_runs"
        or "pol_classify64+pol_buckets". vigfw: "fw_classify64" (64-byte slots) or
        "fw_classify"."""
        return (self.L.vp_last_kernel(self.h) or b"").decode()

    STAGES = ("pass1", "offsets", "a2a_keys", "probe", "a2a_answers", "pass2", "fold",
              "pipeline")

    def last_stage_ms(self) -> dict:
        """vp_stage_ms: owner mode with kernel timing on, the last call's
        phase-A stage times (ms) by stage name ({} if none); the chunked
        pipeline reports "pipeline" (its overlapped chunks) and "fold"
        only."""
        cap = len(self.STAGES)
        ms, k = (C.c_float * cap)(), C.c_int()
        self._ck(self.L.vp_stage_ms(self.h, ms, cap, C.byref(k)), "vp_stage_ms")
        d = {self.STAGES[i]: ms[i] for i in range(min(cap, k.value))}
        if d.get("pipeline"):
            d = {"pipeline": d["pipeline"], "fold": d["fold"]}
        return d

    def table_stats(self, table: int = 0) -> dict:
        """vp_table_stats_get: live / shard_live / tombstones / buckets /
        rebuilds / layout of table 0 (flows) or 1 (viglb backends)."""
        st = TableStatsC()
        self._ck(self.L.vp_table_stats_get(self.h, table, C.byref(st)), "vp_table_stats_get")
        return {k: int(getattr(st, k)) for k, _ in TableStatsC._fields_ if k != "pad"}

    def save_state(self) -> bytes:
        """vp_state_save: the context's table state (both tables for viglb),
        the LRU order among equal stamps and the free list's order included,
        as the canonical image include/vigpath.h describes. Stops the
        resident kernel."""
        n = C.c_uint64()
        self._ck(self.L.vp_state_size(self.h, C.byref(n)), "vp_state_size")
        buf = np.empty(max(int(n.value), 1), np.uint8)
        self._ck(self.L.vp_state_save(self.h, C.c_void_p(buf.ctypes.data), buf.size, C.byref(n)),
                 "vp_state_save")
        return buf[:int(n.value)].tobytes()

    def load_state(self, data):
        """vp_state_load: replace this context's whole table state with an
        image (bytes-like) saved from a context of the same NF and
        capacities; the configuration stays this context's. A malformed image
        raises (vp_last_error names the first offending field) and leaves the
        state as it was."""
        buf = np.frombuffer(data, np.uint8)
        if not buf.size:
            buf = np.zeros(1, np.uint8)
            size = 0
        else:
            size = buf.size
        self._ck(self.L.vp_state_load(self.h, C.c_void_p(buf.ctypes.data), size), "vp_state_load")

    def state_mark(self):
        """vp_state_mark: (seq, epoch), the name of the present state; a
        save_state() taken now, with no packet in between, is its image."""
        m = StateMarkC()
        self._ck(self.L.vp_state_mark(self.h, C.byref(m)), "vp_state_mark")
        return int(m.seq), int(m.epoch)

    def save_delta(self, base):
        """vp_state_delta_save: (the delta from the mark `base` to now as
        bytes, the mark of now). Any earlier mark of this context since its
        last load_state will do as the base."""
        b, m, n = StateMarkC(*base), StateMarkC(), C.c_uint64()
        self._ck(self.L.vp_state_delta_size(self.h, C.byref(b), C.byref(n)), "vp_state_delta_size")
        buf = np.empty(max(int(n.value), 1), np.uint8)
        self._ck(self.L.vp_state_delta_save(self.h, C.byref(b), C.c_void_p(buf.ctypes.data),
                                            buf.size, C.byref(n), C.byref(m)),
                 "vp_state_delta_save")
        return buf[:int(n.value)].tobytes(), (int(m.seq), int(m.epoch))

    def follow(self, mark):
        """vp_state_follow: this context holds the state its primary named
        `mark` (call it after load_state of the image taken at that mark)."""
        m = StateMarkC(*mark)
        self._ck(self.L.vp_state_follow(self.h, C.byref(m)), "vp_state_follow")

    def apply_delta(self, data):
        """vp_state_delta_apply: bring this following context from the mark
        it follows to the delta's. A delta of another base, a malformed one or
        a context that changed since it followed raises (vp_last_error says
        why) and leaves the state and the followed mark as they were."""
        buf = np.frombuffer(data, np.uint8)
        size = buf.size
        if not size:
            buf = np.zeros(1, np.uint8)
        self._ck(self.L.vp_state_delta_apply(self.h, C.c_void_p(buf.ctypes.data), size),
                 "vp_state_delta_apply")

    def value_size(self, table: int = 0) -> int:
        """vp_table_value_size: bytes per entry of `table`'s values (0 the
        NF's flow table, 1 viglb's backends), as in the state image."""
        n = C.c_uint32()
        self._ck(self.L.vp_table_value_size(self.h, table, C.byref(n)), "vp_table_value_size")
        return int(n.value)

    def _table_query(self, call, what, n, src, index, ts, key, value, table, stream):
        for t, width, count in ((index, 4, n), (ts, 8, n), (key, 1, 16 * n)):
            if t is not None:
                assert t.is_cuda and t.element_size() == width and t.numel() >= count
        if value is not None:
            assert value.is_cuda and value.numel() * value.element_size() >= n * self.value_size(table)
        out = VpLookupOutC(index=_dptr(index), ts=_dptr(ts), key=_dptr(key), value=_dptr(value))
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._ck(call(self.h, table, n, _dptr(src) if n else None, C.byref(out), s), what)

    def lookup_device(self, keys, index=None, ts=None, key=None, value=None, table: int = 0,
                      stream=None):
        """vp_table_lookup: for each 16-byte key of `keys` (uint8 CUDA tensor
        of n * 16 bytes, zero-padded as the state image's keys) the live entry
        that holds it -- its index (LOOKUP_MISS: none) into `index` (32-bit
        CUDA tensor of n), its stamp into `ts` (64-bit), its key into `key`
        (uint8, n * 16) and its value into `value` (n * value_size(table)
        bytes); a miss writes zeros. Any output may be None. Read-only: no
        entry is rejuvenated. Stops the resident kernel, runs on `stream` (the
        context's own for None) and returns with the results written."""
        assert keys.is_cuda and keys.element_size() == 1 and keys.numel() % 16 == 0
        self._table_query(self.L.vp_table_lookup, "vp_table_lookup", keys.numel() // 16, keys,
                          index, ts, key, value, table, stream)

    def entries_device(self, idx, index=None, ts=None, key=None, value=None, table: int = 0,
                       stream=None):
        """vp_table_entries: the same answers for each index of `idx` (32-bit
        CUDA tensor of n); an index that is not allocated, or not below the
        capacity, is a miss. vignat's index is the external port minus
        start_port: the reverse NAT lookup."""
        assert idx.is_cuda and idx.element_size() == 4
        self._table_query(self.L.vp_table_entries, "vp_table_entries", idx.numel(), idx,
                          index, ts, key, value, table, stream)

    def _table_query_host(self, query, src, n, table):
        import torch
        d = src.device
        vsz = self.value_size(table)
        index = torch.empty(n, dtype=torch.int32, device=d)
        ts = torch.empty(n, dtype=torch.int64, device=d)
        key = torch.empty(n * 16, dtype=torch.uint8, device=d)
        value = torch.empty(n * vsz, dtype=torch.uint8, device=d) if vsz else None
        query(src, index, ts, key, value, table)
        return {"index": index.cpu().numpy().view(np.uint32), "ts": ts.cpu().numpy(),
                "key": key.cpu().numpy().reshape(n, 16),
                "value": (value.cpu().numpy() if vsz else np.zeros(0, np.uint8)).reshape(n, vsz)}

    def lookup(self, keys: np.ndarray, table: int = 0) -> dict:
        """lookup_device of uint8[n, 16] keys in host memory: a dict of numpy
        arrays index (uint32[n]), ts (int64[n]), key (uint8[n, 16]) and value
        (uint8[n, value_size])."""
        import torch
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 16)
        src = torch.from_numpy(keys.reshape(-1).copy()).to("cuda:%d" % self.gpu)
        return self._table_query_host(self.lookup_device, src, keys.shape[0], table)

    def entries(self, indices: np.ndarray, table: int = 0) -> dict:
        """entries_device of uint32[n] indices in host memory; the dict lookup
        returns."""
        import torch
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        src = torch.from_numpy(idx.view(np.int32).copy()).to("cuda:%d" % self.gpu)
        return self._table_query_host(self.entries_device, src, idx.shape[0], table)

    def _table_erase(self, call, what, n, src, index, ts, key, value, table, stream) -> int:
        for t, width, count in ((index, 4, n), (ts, 8, n), (key, 1, 16 * n)):
            if t is not None:
                assert t.is_cuda and t.element_size() == width and t.numel() >= count
        if value is not None:
            assert value.is_cuda and value.numel() * value.element_size() >= n * self.value_size(table)
        out = VpLookupOutC(index=_dptr(index), ts=_dptr(ts), key=_dptr(key), value=_dptr(value))
        s = C.c_void_p(stream.cuda_stream) if stream is not None else None
        k = C.c_uint32()
        self._ck(call(self.h, table, n, _dptr(src) if n else None, C.byref(out), C.byref(k), s), what)
        return int(k.value)

    def erase_device(self, keys, index=None, ts=None, key=None, value=None, table: int = 0,
                     stream=None) -> int:
        """vp_table_erase: take out the live entry that holds each 16-byte key
        of `keys` (as lookup_device takes them), in query order: the index of
        the last erasing query is the first the allocator hands out again. A
        query that names nothing live (a miss, a pad byte set, a key an
        earlier query of the call erased) is a no-op. The outputs are
        lookup_device's: for an erasing query the freed index and the entry as
        it was, for any other a miss. Returns the number of entries erased. An
        erase ends a follow() and moves the context's mark. Stops the resident
        kernel, runs on `stream` and returns when done."""
        assert keys.is_cuda and keys.element_size() == 1 and keys.numel() % 16 == 0
        return self._table_erase(self.L.vp_table_erase, "vp_table_erase", keys.numel() // 16, keys,
                                 index, ts, key, value, table, stream)

    def free_device(self, idx, index=None, ts=None, key=None, value=None, table: int = 0,
                    stream=None) -> int:
        """vp_table_free: erase_device by index (32-bit CUDA tensor of n); an
        index that is not allocated, or not below the capacity, is a no-op."""
        assert idx.is_cuda and idx.element_size() == 4
        return self._table_erase(self.L.vp_table_free, "vp_table_free", idx.numel(), idx,
                                 index, ts, key, value, table, stream)

    def _table_erase_host(self, call, src, n, table):
        got = {}

        def query(src, index, ts, key, value, table):
            got["n_erased"] = call(src, index, ts, key, value, table)

        out = self._table_query_host(query, src, n, table)
        out["n_erased"] = got["n_erased"]
        return out

    def erase(self, keys: np.ndarray, table: int = 0) -> dict:
        """erase_device of uint8[n, 16] keys in host memory: lookup's dict of
        numpy arrays plus "n_erased"."""
        import torch
        keys = np.ascontiguousarray(keys, np.uint8).reshape(-1, 16)
        src = torch.from_numpy(keys.reshape(-1).copy()).to("cuda:%d" % self.gpu)
        return self._table_erase_host(self.erase_device, src, keys.shape[0], table)

    def free(self, indices: np.ndarray, table: int = 0) -> dict:
        """free_device of uint32[n] indices in host memory; the dict erase
        returns."""
        import torch
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        src = torch.from_numpy(idx.view(np.int32).copy()).to("cuda:%d" % self.gpu)
        return self._table_erase_host(self.free_device, src, idx.shape[0], table)

    def live_count(self) -> int:
        v = self.L.vp_live_count(self.h)
        if v < 0:
            self._ck(int(v), "vp_live_count")
        return int(v)

    # ----------------------------------------------------------- host --
    def process_host(self, frames: np.ndarray, lens, in_dev, now, slot: int):
        """Contiguous host batch; frames (u8, n*slot) rewritten in place.
        Returns out_dev (u16)."""
        n = int(lens.shape[0])
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        assert frames.size == n * slot
        lens = np.ascontiguousarray(lens, np.uint16)
        in_dev = np.ascontiguousarray(in_dev, np.uint16)
        now = np.ascontiguousarray(now, np.int64)
        out = np.zeros(n, np.uint16)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_process_host(self.h, n, P(in_dev), P(frames), slot,
                                     P(lens), P(now), P(out)),
               "vp_process_host")
        return out

    def process_host_batch(self, frames: np.ndarray, lens, in_dev, out, slot: int,
                           now=None, now0: int = 0, now_step: int = 0):
        """vp_process_host_batch: host numpy arrays (page-locked ones, e.g.
        torch.pin_memory() views, are DMA'd in place), rewritten in place;
        out (u16/i16, n) receives the out ports. now: int64 array, or None
        for now0 + i * now_step."""
        n = int(lens.shape[0])
        assert frames.dtype == np.uint8 and frames.flags.c_contiguous
        assert frames.size == n * slot and out.shape[0] == n
        for a in (lens, in_dev, out):
            assert a.flags.c_contiguous and a.itemsize == 2
        if now is not None:
            assert now.dtype == np.int64 and now.flags.c_contiguous
        b = DevBatchC(frames=frames.ctypes.data, slot=slot, n=n, len=lens.ctypes.data,
                      in_dev=in_dev.ctypes.data,
                      now=now.ctypes.data if now is not None else None,
                      now0=now0, now_step=now_step, out_dev=out.ctypes.data)
        self._ck(self.L.vp_process_host_batch(self.h, C.byref(b)), "vp_process_host_batch")

    def process_mbufs(self, bufs, in_dev, now):
        """Per-frame host buffers (bytearray each, mbuf-like), rewritten in
        place. Returns out_dev."""
        n = len(bufs)
        ptrs = (C.c_void_p * n)()
        arrs = []
        lens = np.zeros(n, np.uint16)
        for i, b in enumerate(bufs):
            a = (C.c_uint8 * len(b)).from_buffer(b)
            arrs.append(a)
            ptrs[i] = C.cast(a, C.c_void_p)
            lens[i] = len(b)
        in_dev = np.ascontiguousarray(in_dev, np.uint16)
        now = np.ascontiguousarray(now, np.int64)
        out = np.zeros(n, np.uint16)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_process_batch(self.h, n, P(in_dev), ptrs, P(lens),
                                      P(now), P(out)), "vp_process_batch")
        return out

    def register_host(self, arr: np.ndarray):
        """vp_register_host: the GPU reads and writes frames inside `arr`
        (e.g. an mbuf pool) in place from now on (vp_process_mbufs)."""
        assert arr.flags.c_contiguous
        self._ck(self.L.vp_register_host(self.h, C.c_void_p(arr.ctypes.data), arr.nbytes),
                 "vp_register_host")
        self._hostmaps = getattr(self, "_hostmaps", []) + [arr]

    def unregister_host(self, arr: np.ndarray):
        self._ck(self.L.vp_unregister_host(self.h, C.c_void_p(arr.ctypes.data)),
                 "vp_unregister_host")
        self._hostmaps = [a for a in getattr(self, "_hostmaps", []) if a is not arr]

    def process_mbuf_batch(self, ptrs: np.ndarray, lens, in_dev, out, now=None,
                           now0: int = 0, now_step: int = 0):
        """vp_process_mbufs: ptrs (u64, n) = each frame's host address (the
        mbuf data pointers of an rx burst), lens / in_dev (u16, n), out (u16,
        n) receives the out ports; now (i64, n) or None for affine time.
        Arrays in page-locked memory are DMA'd in place."""
        n = int(ptrs.shape[0])
        assert ptrs.dtype == np.uint64 and ptrs.flags.c_contiguous
        for a in (lens, in_dev, out):
            assert a.flags.c_contiguous and a.itemsize == 2 and a.shape[0] == n
        if now is not None:
            assert now.dtype == np.int64 and now.flags.c_contiguous
        b = MbufBatchC(n=n, frames=ptrs.ctypes.data, len=lens.ctypes.data,
                       in_dev=in_dev.ctypes.data,
                       now=now.ctypes.data if now is not None else None,
                       now0=now0, now_step=now_step, out_dev=out.ctypes.data)
        self._ck(self.L.vp_process_mbufs(self.h, C.byref(b)), "vp_process_mbufs")

    def mbuf_step(self, ptrs, lens, in_dev, out):
        """A prepared vp_process_mbufs call over fixed host arrays with affine
        time: returns f(now0, now_step) (the batch descriptor built once, as
        device_step)."""
        n = int(ptrs.shape[0])
        b = MbufBatchC(n=n, frames=ptrs.ctypes.data, len=lens.ctypes.data,
                       in_dev=in_dev.ctypes.data, now=None, now0=0, now_step=0,
                       out_dev=out.ctypes.data)
        ref, fn, h, L = C.byref(b), self.L.vp_process_mbufs, self.h, self.L

        def step(now0: int, now_step: int):
            b.now0, b.now_step = now0, now_step
            rc = fn(h, ref)
            if rc:
                _check(rc, "vp_process_mbufs", L)
        step.arrays = (ptrs, lens, in_dev, out)
        return step

    def process(self, device: int, buffer: bytearray, now: int) -> int:
        """nf_process for one packet (nf.h:13): vp_process_one (on one GPU the
        NF's persistent kernel's mailbox, no launch per packet; a one-packet
        batch where an expiry is due, and for the packet viglb's kernel hands
        back: the erasure of a flow while no backend is alive)."""
        a = (C.c_uint8 * len(buffer)).from_buffer(buffer)
        out = C.c_uint16(device)
        self._ck(self.L.vp_process_one(self.h, device, C.cast(a, C.c_void_p), len(buffer),
                                       now, C.byref(out)), "vp_process_one")
        return int(out.value)

    def serve_stats(self) -> dict:
        """vp_serve_stats_get: what the NF's resident kernel served so far --
        packets_one (vp_process_one), bursts / burst_packets (small
        vp_process_batch / vp_process_mbufs calls), declined (requests handed
        back to the pipeline: a burst with IPv4 options, viglb's erasure of a
        flow), launches. A host-side counter read: the kernel stays."""
        st = ServeStatsC()
        self._ck(self.L.vp_serve_stats_get(self.h, C.byref(st)), "vp_serve_stats_get")
        return {k: int(getattr(st, k)) for k, _ in ServeStatsC._fields_}

    def serve_expiry_stats(self) -> dict:
        """vp_serve_expiry_stats_get: expiry inside the resident kernel
        (every served NF) -- seeds (journal builds, one per table: a viglb
        seeding builds the flows' and the backends' and counts 2),
        expired (entries the kernel expired; viglb: flows and backends
        together), walks (requests that expired at least one), handed
        (requests that took the pipeline because an expiry was due, on either
        table), splits (bursts served in part, the rest posted again). A
        host-side counter read: the kernel stays."""
        st = ServeExpiryStatsC()
        self._ck(self.L.vp_serve_expiry_stats_get(self.h, C.byref(st)),
                 "vp_serve_expiry_stats_get")
        return {k: int(getattr(st, k)) for k, _ in ServeExpiryStatsC._fields_}


class Nat(NfBase):
    kind = "nat"

    def __init__(self, cfg: NatConfigC, gpu: int = 0, libpath=None):
        super().__init__(libpath)
        self.cfg = cfg
        self.gpu = gpu
        self._ck(self.L.vp_nat_create(C.byref(cfg), gpu, C.byref(self.h)),
               "vp_nat_create")

    def dump(self):
        n = self.cfg.max_flows
        alloc = np.zeros(n, np.uint8)
        ts = np.zeros(n, np.int64)
        keys = np.zeros(n * 16, np.uint8)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_nat_dump(self.h, P(alloc), P(ts), P(keys)),
               "vp_nat_dump")
        return alloc, ts, keys.reshape(n, 16)


class Bridge(NfBase):
    kind = "bridge"

    def __init__(self, cfg: BridgeConfigC, gpu: int = 0, libpath=None):
        super().__init__(libpath)
        self.cfg = cfg
        self.gpu = gpu
        self._ck(self.L.vp_bridge_create(C.byref(cfg), gpu, C.byref(self.h)),
               "vp_bridge_create")

    def dump(self):
        """Dynamic table by index: alloc, ts, MAC (6 B), learned port."""
        n = self.cfg.dyn_capacity
        alloc = np.zeros(n, np.uint8)
        ts = np.zeros(n, np.int64)
        macs = np.zeros(n * 6, np.uint8)
        port = np.zeros(n, np.uint16)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_bridge_dump(self.h, P(alloc), P(ts), P(macs), P(port)),
               "vp_bridge_dump")
        return alloc, ts, macs.reshape(n, 6), port


class Lb(NfBase):
    kind = "lb"

    def __init__(self, cfg: LbConfigC, gpu: int = 0, libpath=None):
        super().__init__(libpath)
        self.cfg = cfg
        self.gpu = gpu
        self._ck(self.L.vp_lb_create(C.byref(cfg), gpu, C.byref(self.h)),
               "vp_lb_create")

    def dump(self):
        """(flow alloc, ts, keys[16], backend id), (backend alloc, ts, ip,
        mac[6], nic) by index."""
        nf_, nb = self.cfg.flow_capacity, self.cfg.backend_capacity
        fa, ft = np.zeros(nf_, np.uint8), np.zeros(nf_, np.int64)
        fk, fb = np.zeros(nf_ * 16, np.uint8), np.zeros(nf_, np.uint32)
        ba, bt = np.zeros(nb, np.uint8), np.zeros(nb, np.int64)
        bi, bm = np.zeros(nb, np.uint32), np.zeros(nb * 6, np.uint8)
        bn = np.zeros(nb, np.uint16)
        self._ck(self.L.vp_lb_dump(self.h, *[C.c_void_p(x.ctypes.data) for x in
                                           (fa, ft, fk, fb, ba, bt, bi, bm, bn)]),
               "vp_lb_dump")
        return ((fa, ft, fk.reshape(nf_, 16), fb),
                (ba, bt, bi, bm.reshape(nb, 6), bn))


class Fw(NfBase):
    kind = "fw"

    def __init__(self, cfg: FwConfigC, gpu: int = 0, libpath=None):
        super().__init__(libpath)
        self.cfg = cfg
        self.gpu = gpu
        self._ck(self.L.vp_fw_create(C.byref(cfg), gpu, C.byref(self.h)),
               "vp_fw_create")

    def dump(self):
        """By flow index: alloc, ts, FlowId bytes (16), int_devices."""
        n = self.cfg.max_flows
        alloc = np.zeros(n, np.uint8)
        ts = np.zeros(n, np.int64)
        keys = np.zeros(n * 16, np.uint8)
        dev = np.zeros(n, np.uint32)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_fw_dump(self.h, P(alloc), P(ts), P(keys), P(dev)),
               "vp_fw_dump")
        return alloc, ts, keys.reshape(n, 16), dev


class Pol(NfBase):
    """vigpol (vigpol/policer_main.c): per-destination token buckets on the
    WAN device; frames are never rewritten."""
    kind = "pol"

    def __init__(self, cfg: PolConfigC, gpu: int = 0, libpath=None):
        super().__init__(libpath)
        self.cfg = cfg
        self.gpu = gpu
        self._ck(self.L.vp_pol_create(C.byref(cfg), gpu, C.byref(self.h)),
               "vp_pol_create")

    def dump(self):
        """By index: alloc, ts, dyn_keys (raw u32 address), bucket_size,
        bucket_time."""
        n = self.cfg.dyn_capacity
        alloc = np.zeros(n, np.uint8)
        ts = np.zeros(n, np.int64)
        keys = np.zeros(n, np.uint32)
        size = np.zeros(n, np.uint64)
        btime = np.zeros(n, np.int64)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        self._ck(self.L.vp_pol_dump(self.h, P(alloc), P(ts), P(keys), P(size),
                                  P(btime)), "vp_pol_dump")
        return alloc, ts, keys, size, btime
