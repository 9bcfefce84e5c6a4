// Several receive queues as one NF's device batch (vp_rx_merge,
// include/vigpath.h): up to VP_RX_MERGE_MAX packed streams, one per port, each
// exactly vp_rx_unpack's input, merged by each frame's signed 64-bit time into
// consecutive slots with a per-packet in_dev -- what nf.c's poll over its
// devices hands the NF, for streams that already lie in device memory. Two
// launches:
//
//   rxm_rank    each block takes kSlotBlockEntries consecutive entries of one
//               queue, a wave 64 of them per turn as rxu_scatter does. A few
//               lanes narrow, by two binary searches per other queue, the
//               window the block's first and last time fall in; every lane then
//               ranks its own entry inside those windows (upper bound in the
//               queues before its own, lower bound in those after: the stable
//               order) and scatters the small records which[p], src[p],
//               in_dev[p], now[p] and, into the workspace, the frame's byte
//               position in its stream: pos[e] read coalesced here, or the
//               running sum of the padded lengths. Block 0 writes the count.
//   rxm_scatter which[], src[] and the positions read coalesced, len[] stored
//               coalesced, the frames through the slot mover (vp_slots_dev.h)
//               with a stream address and a kept length per entry.
//
// A queue without pos[] first gets vp_rx_unpack's two launches, rxu_sizes and
// txp_scan, over all its entries into its own region of the workspace: every
// wave's first position. A queue with pos[] adds no launch.
//
// No block waits for another: the order between the launches is the stream's.
// The queues' records travel as kernel arguments and are staged in LDS, where a
// lane may index them by its entry's queue without a private segment.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(rxmerge)

constexpr uint32_t kRxmMax = VP_RX_MERGE_MAX;
static_assert(2 * kRxmMax <= kSlotThreads, "a lane per window end");

struct RxmQueue {
  const uint8_t *data;  // the stream
  uint64_t bytes;
  const uint64_t *pos;
  const uint32_t *sel;
  const uint16_t *len;
  const int64_t *now;
  int64_t now0, now_step;
  const uint64_t *base;  // pos == NULL: every wave's first position (scanned sums)
  uint32_t n, meta_n;
  uint32_t in_port;
  uint32_t chunk0;  // the queue's first block in rxm_rank's grid
};

struct RxmArgs {
  RxmQueue q[kRxmMax];
  uint32_t nq;
  uint32_t m;      // min(total, cap): the positions that are written
  uint32_t total;  // (0xFFFFFFFF where the sum passes 32 bits)
  uint32_t oslot;
  uint8_t *oframes;  // the merged batch
  uint16_t *olen;
  int64_t *onow;
  uint16_t *oin;
  uint32_t *osrc;
  uint8_t *owhich;
  uint32_t *count;
  uint64_t *fpos;  // workspace, m words: position p's frame lies at fpos[p] of its stream
};

// Stages the records (static indices into the kernel arguments: nothing of
// them is copied to scratch memory)
__device__ __forceinline__ void rxm_stage(const RxmArgs &a, RxmQueue *sh, uint32_t tid) {
#pragma unroll
  for (uint32_t j = 0; j < kRxmMax; j++)
    if (tid == j && j < a.nq) {
      const RxmQueue Q = a.q[j];
      sh[j] = Q;
    }
  __syncthreads();
}

// Entry e's index into len[] / now[] and its time: INT64_MAX where the index is
// outside them, and nothing is read through such an index
__device__ __forceinline__ int64_t rxm_time(const RxmQueue &Q, uint32_t e, uint32_t &mm) {
  mm = Q.sel ? Q.sel[e] : e;
  return mm < Q.meta_n ? (int64_t)batch_time(Q.now, Q.now0, Q.now_step, mm) : INT64_MAX;
}

// How many of the queue's entries lo .. hi - 1 stand before time x: those with
// a time <= x (upper) or < x, compared as signed 64-bit values. With times that
// do not decrease along the queue and the answer inside the window it is the
// queue's bound; with any times it is a number in lo .. hi.
__device__ __forceinline__ uint32_t rxm_bound(const RxmQueue &Q, int64_t x, bool upper,
                                              uint32_t lo, uint32_t hi) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    uint32_t mm;
    const int64_t t = rxm_time(Q, mid, mm);
    if (upper ? t <= x : t < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kSlotThreads) void rxm_rank(const RxmArgs a) {
  __shared__ RxmQueue sh[kRxmMax];
  __shared__ uint32_t win[2][kRxmMax];  // per other queue: the block's window
  const uint32_t tid = threadIdx.x, lane = tid & 63, nq = a.nq;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  rxm_stage(a, sh, tid);
  if (blockIdx.x == 0 && tid == 0) *a.count = a.total;
  if (a.m == 0) return;  // (nothing to rank into; the grid is one block)
  // this block is chunk c - chunk0 of queue j (an empty queue has no chunk)
  const uint32_t c = blockIdx.x;
  uint32_t j = 0;
  for (; j + 1 < nq; j++)
    if (c < sh[j + 1].chunk0) break;
  const RxmQueue &Q = sh[j];
  const uint32_t cj = c - Q.chunk0, nj = Q.n;
  const uint32_t e0 = cj * kSlotBlockEntries;  // < n_j
  const uint32_t cnt = nj - e0 < kSlotBlockEntries ? nj - e0 : kSlotBlockEntries;
  if (tid < 2 * nq) {
    const uint32_t jp = tid >> 1, end = tid & 1;
    if (jp != j) {
      uint32_t mm;
      const int64_t x = rxm_time(Q, e0 + (end ? cnt - 1 : 0), mm);
      win[end][jp] = rxm_bound(sh[jp], x, jp < j, 0, sh[jp].n);
    }
  }
  __syncthreads();
  const uint64_t w0 = (uint64_t)e0 + wv * kSlotPerWave;
  if (w0 >= nj) return;
  uint64_t run = 0;  // pos == NULL: this turn's first position
  if (!Q.pos) run = Q.base[(size_t)cj * kSlotWaves + wv];
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k0 = w0 + it * 64;  // (may pass 2^32)
    if (k0 >= nj) break;
    const bool mine = k0 + lane < nj;
    const uint32_t e = (uint32_t)(k0 + lane);
    uint32_t mm = 0;
    int64_t t = INT64_MAX;
    if (mine) t = rxm_time(Q, e, mm);
    uint64_t fp = 0;
    if (Q.pos) {
      if (mine) fp = Q.pos[e];
    } else {
      const uint32_t ext = mine && mm < Q.meta_n ? pad16(Q.len[mm]) : 0u;
      const uint32_t x = wave_scan(ext, lane);
      fp = run + (x - ext);
      run += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    if (mine) {
      uint64_t p = e;
      for (uint32_t jp = 0; jp < nq; jp++) {
        if (jp == j) continue;
        const uint32_t lo = win[0][jp];
        const uint32_t hi = win[1][jp] > lo ? win[1][jp] : lo;  // (times that decrease)
        p += rxm_bound(sh[jp], t, jp < j, lo, hi);
      }
      // p < total whatever the times: e < n_j and every bound is at most its n
      if (p < a.m) {
        a.owhich[p] = (uint8_t)j;
        a.osrc[p] = mm;
        if (a.oin) a.oin[p] = (uint16_t)Q.in_port;
        if (a.onow) a.onow[p] = t;
        a.fpos[p] = fp;
      }
    }
  }
}

// What a lane holds of its entry for the slot mover: the frame lies at `from`
// with `r` bytes to keep; r is 0 for an entry that is not readable, and then
// nothing is read
struct RxmFrame {
  const uint8_t *from;
  uint32_t r;
  __device__ __forceinline__ RxmFrame at(uint32_t e) const {
    return {(const uint8_t *)(uintptr_t)shfl64((uint64_t)(uintptr_t)from, e),
            (uint32_t)__shfl((int)r, (int)e)};
  }
  __device__ __forceinline__ RxmFrame at_uniform(uint32_t e) const {
    return {(const uint8_t *)(uintptr_t)readlane64((uint64_t)(uintptr_t)from, e),
            (uint32_t)__builtin_amdgcn_readlane((int)r, (int)e)};
  }
  __device__ __forceinline__ uint4 unit(uint32_t u, bool on) const {
    const uint32_t keep = on ? r : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (u < keep) v = unit_clear(*(const uint4 *)(from + u), keep - u);
    return v;
  }
};

__global__ __launch_bounds__(kSlotThreads) void rxm_scatter(const RxmArgs a) {
  __shared__ RxmQueue sh[kRxmMax];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  rxm_stage(a, sh, tid);
  const uint64_t w0 = (uint64_t)blockIdx.x * kSlotBlockEntries + wv * kSlotPerWave;
  if (w0 >= a.m) return;
  const SlotPath path = slot_path(a.oslot);
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k0 = w0 + it * 64;  // (may pass 2^32)
    if (k0 >= a.m) break;
    const uint32_t left = a.m - k0 < 64 ? (uint32_t)(a.m - k0) : 64;
    const bool mine = lane < left;
    uint32_t j = ~0u, mm = ~0u;
    uint64_t fp = 0;
    if (mine) {
      j = a.owhich[k0 + lane];
      mm = a.osrc[k0 + lane];
      fp = a.fpos[k0 + lane];
    }
    // after times that decrease a position may hold records no lane of
    // rxm_rank wrote: nothing is read through a queue that does not exist, an
    // index outside len[] or a position outside the stream
    const uint32_t jj = j < a.nq ? j : 0;
    const RxmQueue &Q = sh[jj];
    const bool in = mine && j < a.nq && mm < Q.meta_n;
    uint32_t l = in ? Q.len[mm] : 0u;
    // readable: inside len[], aligned, and its kept bytes' units inside the
    // stream; compared without a sum that could wrap
    uint32_t r = l < a.oslot ? l : a.oslot;
    const bool ok = in && (fp & 15) == 0 && fp <= Q.bytes && pad16(r) <= Q.bytes - fp;
    const uint8_t *from = nullptr;
    if (ok)
      from = Q.data + fp;
    else
      l = r = 0;
    if (mine) a.olen[k0 + lane] = (uint16_t)l;
    slot_move(path, RxmFrame{from, r}, a.oframes, a.oslot, k0, lane, left);
  }
}

// vp_last_error()'s text for a refused call
static int rxm_refuse(const char *fmt, ...) {
  char text[200];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  state_fail("vp_rx_merge: %s", text);  // (records the text)
  return VP_EINVAL;
}

}  // namespace vp

using namespace vp;

extern "C" int vp_rx_merge(vp_ctx *c, const vp_rx_queue *queues, uint32_t n_queues,
                           const vp_tx_merged *o, void *stream) {
  if (!c || !queues || !o) return rxm_refuse("a NULL ctx, queues or out");
  if (!o->count) return rxm_refuse("a NULL out->count");
  if (n_queues == 0 || n_queues > VP_RX_MERGE_MAX)
    return rxm_refuse("%u queues (1 to %d)", n_queues, VP_RX_MERGE_MAX);
  if (o->key) return rxm_refuse("out->key must be NULL: the 64-bit time comes out in out->now");
  if (!slots_ok(o->frames, o->slot))
    return rxm_refuse("out->slot %u or the alignment of out->frames", o->slot);
  if ((!o->frames || !o->len || !o->src || !o->which) && o->cap)
    return rxm_refuse("a NULL out->frames, len, src or which with cap %u", o->cap);
  RxmArgs a = {};
  uint64_t total = 0;
  uint32_t chunks = 0;
  size_t words = 0;  // of all queues without pos[]: their waves' sums
  for (uint32_t j = 0; j < n_queues; j++) {
    const vp_rx_stream &in = queues[j].stream;
    if ((!in.data && in.bytes) || ((uintptr_t)in.data & 15))
      return rxm_refuse("queue %u: data NULL with bytes, or not 16-byte aligned", j);
    if (!in.len && in.meta_n) return rxm_refuse("queue %u: a NULL len with meta_n %u", j, in.meta_n);
    if (bytes_overlap(in.data, in.bytes, o->frames, (uint64_t)o->cap * o->slot))
      return rxm_refuse("queue %u: its data overlaps out->frames", j);
    if (queues[j].in_port > 0xFFFF)
      return rxm_refuse("queue %u: in_port %u above 0xFFFF", j, queues[j].in_port);
    RxmQueue &q = a.q[j];
    q.data = in.data;
    q.bytes = in.bytes;
    q.pos = in.pos;
    q.sel = in.sel;
    q.len = in.len;
    q.now = in.now;
    q.now0 = in.now0;
    q.now_step = in.now_step;
    q.n = in.n;
    q.meta_n = in.meta_n;
    q.in_port = queues[j].in_port;
    q.chunk0 = chunks;
    const uint32_t blocks = in.n ? (in.n - 1) / kSlotBlockEntries + 1 : 0;
    chunks += blocks;  // (at most 8 * 2^21)
    if (!in.pos) words += (size_t)blocks * kSlotWaves;
    total += in.n;
  }
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  a.nq = n_queues;
  a.total = total < 0xFFFFFFFFull ? (uint32_t)total : ~0u;
  a.m = total < o->cap ? (uint32_t)total : o->cap;
  a.oslot = o->slot;
  a.oframes = o->frames;
  a.olen = o->len;
  a.onow = o->now;
  a.oin = o->in_dev;
  a.osrc = o->src;
  a.owhich = o->which;
  a.count = o->count;
  if (a.m == 0) {  // one block, so that count is written
    rxm_rank<<<1, kSlotThreads, 0, s>>>(a);
    VP_HIP(hipGetLastError());
    return 0;
  }
  // the workspace: the positions' records, then the sums of each queue
  // without pos[]
  CallBuf &w = c->ws.rxm_rec;
  VP_TRY(callbuf_reserve(w, 8 * ((size_t)a.m + words), s));
  a.fpos = (uint64_t *)w.p;
  uint64_t *sums = a.fpos + a.m;
  for (uint32_t j = 0; j < n_queues; j++) {
    RxmQueue &q = a.q[j];
    if (q.pos || !q.n) continue;
    const uint32_t blocks = (q.n - 1) / kSlotBlockEntries + 1;
    RxuArgs u = {};
    u.sel = q.sel;
    u.len = q.len;
    u.meta_n = q.meta_n;
    u.n = u.m = q.n;  // (every entry: any of them may stand below cap)
    rxu_sizes<<<blocks, kSlotThreads, 0, s>>>(u, sums);
    VP_HIP(hipGetLastError());
    txp_scan<<<1, kTxpScanThreads, 0, s>>>(sums, blocks * kSlotWaves);
    VP_HIP(hipGetLastError());
    q.base = sums;
    sums += (size_t)blocks * kSlotWaves;
  }
  rxm_rank<<<chunks, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  rxm_scatter<<<(a.m - 1) / kSlotBlockEntries + 1, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  return callbuf_done(w, s);
}
