// Several transmit lists as one NF's device batch (vp_tx_merge,
// include/vigpath.h): the lists that vp_tx_build wrote for up to
// VP_TX_MERGE_MAX (context, batch, port) sources, merged by a 32-bit key per
// packet -- its position in the chain's input -- into consecutive slots, as the
// cables of several boxes into one would deliver them. Two launches
// (DESIGN.md §5.8):
//
//   txm_rank    each block takes kSlotBlockEntries consecutive entries of one
//               source's list. A few lanes narrow, by two binary searches per
//               other source, the window the block's first and last key fall
//               in; every lane then ranks its own entries inside those windows
//               (upper bound in the sources before its own, lower bound in
//               those after: the stable order) and scatters the small records
//               which[p], src[p], key[p], in_dev[p]. Block 0 writes the count.
//   txm_gather  which[] and src[] read coalesced, len[] and the time stored
//               coalesced, the slots through the slot mover (vp_slots_dev.h)
//               with a source slot's address and width per entry.
//
// No block waits for another and there is no workspace: every block reads the
// lists' bounds from the sources' offset[]. The sources' records travel as
// kernel arguments and are staged in LDS, where a lane may index them by its
// entry's source without a private segment.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(txmerge)

constexpr uint32_t kTxmPerLane = kSlotBlockEntries / kSlotThreads;
constexpr uint32_t kTxmMax = VP_TX_MERGE_MAX;
static_assert(2 * kTxmMax <= kSlotThreads, "a lane per window end");

struct TxmSrc {
  const uint8_t *frames;  // the source batch
  const uint16_t *len;
  const int64_t *now;
  int64_t now0, now_step;
  const uint32_t *idx;  // its lists
  const uint32_t *offset;
  const uint32_t *key;  // or NULL
  uint32_t n;           // packets anything may be gathered through (0: frames or len NULL)
  uint32_t nkey;        // entries of key[]
  uint32_t slot, lcap, nd, port, in_port, pad;
};

struct TxmArgs {
  TxmSrc s[kTxmMax];
  uint32_t n_srcs;
  uint8_t *oframes;  // the merged batch
  uint32_t oslot, ocap;
  uint16_t *olen;
  int64_t *onow;
  uint16_t *oin;
  uint32_t *okey;
  uint32_t *osrc;
  uint8_t *owhich;
  uint32_t *count;
};

// What both kernels keep in LDS: the sources' records, and of every source's
// list where it starts in idx[] and how many entries idx[] holds of it.
struct TxmShared {
  TxmSrc s[kTxmMax];
  uint32_t lo[kTxmMax], C[kTxmMax];
};

// Stages the records (static indices into the kernel arguments: nothing of
// them is copied to scratch memory) and the bounds, as vp_tx_rebatch defines
// them; returns the total of all lists.
__device__ __forceinline__ uint64_t txm_stage(const TxmArgs &a, TxmShared &sh, uint32_t tid) {
#pragma unroll
  for (uint32_t j = 0; j < kTxmMax; j++)
    if (tid == j && j < a.n_srcs) {
      const TxmSrc S = a.s[j];
      sh.s[j] = S;
      uint32_t lo;
      const uint32_t C = list_port(S.offset, S.port, list_entries(S.offset, S.nd, S.lcap), lo);
      sh.lo[j] = lo;
      sh.C[j] = C;
    }
  __syncthreads();
  uint64_t total = 0;
  for (uint32_t j = 0; j < a.n_srcs; j++) total += sh.C[j];
  return total;
}

// Entry m of source j's list (m < C_j): its packet, and that packet's key.
// Nothing is read through a packet outside the batch: its key is the index.
__device__ __forceinline__ uint32_t txm_entry(const TxmShared &sh, uint32_t j, uint32_t m) {
  return sh.s[j].idx[(size_t)sh.lo[j] + m];
}
__device__ __forceinline__ uint32_t txm_key(const TxmShared &sh, uint32_t j, uint32_t i) {
  const uint32_t *key = sh.s[j].key;
  return key && i < sh.s[j].nkey ? key[i] : i;
}

// How many of source j's entries lo .. hi - 1 stand before key x: those with a
// key <= x (upper) or < x. With keys that do not decrease along the list and
// the answer inside the window it is the list's bound; with any keys it is a
// number in lo .. hi.
__device__ __forceinline__ uint32_t txm_bound(const TxmShared &sh, uint32_t j, uint32_t x,
                                              bool upper, uint32_t lo, uint32_t hi) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    const uint32_t k = txm_key(sh, j, txm_entry(sh, j, mid));
    if (upper ? k <= x : k < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kSlotThreads) void txm_rank(const TxmArgs a) {
  __shared__ TxmShared sh;
  __shared__ uint32_t win[2][kTxmMax];  // per other source: the block's window
  const uint32_t tid = threadIdx.x, ns = a.n_srcs;
  const uint64_t total = txm_stage(a, sh, tid);
  if (blockIdx.x == 0 && tid == 0) *a.count = total < 0xFFFFFFFFull ? (uint32_t)total : ~0u;
  if (a.ocap == 0) return;  // (nothing to rank into)
  uint64_t chunks = 0;
  for (uint32_t j = 0; j < ns; j++)
    chunks += ((uint64_t)sh.C[j] + kSlotBlockEntries - 1) / kSlotBlockEntries;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    // chunk c is chunk c - base of source j
    uint32_t j = 0;
    uint64_t base = 0;
    for (; j + 1 < ns; j++) {
      const uint64_t nb = ((uint64_t)sh.C[j] + kSlotBlockEntries - 1) / kSlotBlockEntries;
      if (c < base + nb) break;
      base += nb;
    }
    const uint64_t m0 = (c - base) * kSlotBlockEntries;  // < C_j
    const uint32_t Cj = sh.C[j];
    const uint32_t cnt = Cj - m0 < kSlotBlockEntries ? (uint32_t)(Cj - m0) : kSlotBlockEntries;
    if (tid < 2 * ns) {
      const uint32_t jp = tid >> 1, end = tid & 1;
      if (jp != j) {
        const uint32_t m = (uint32_t)m0 + (end ? cnt - 1 : 0);
        const uint32_t x = txm_key(sh, j, txm_entry(sh, j, m));
        win[end][jp] = txm_bound(sh, jp, x, jp < j, 0, sh.C[jp]);
      }
    }
    __syncthreads();
    for (uint32_t it = 0; it < kTxmPerLane; it++) {
      const uint32_t e = it * kSlotThreads + tid;
      if (e >= cnt) break;
      const uint32_t m = (uint32_t)m0 + e;
      const uint32_t i = txm_entry(sh, j, m), x = txm_key(sh, j, i);
      uint64_t p = m;
      for (uint32_t jp = 0; jp < ns; jp++) {
        if (jp == j) continue;
        const uint32_t lo = win[0][jp];
        const uint32_t hi = win[1][jp] > lo ? win[1][jp] : lo;  // (keys that decrease)
        p += txm_bound(sh, jp, x, jp < j, lo, hi);
      }
      // p < total whatever the keys: m < C_j and every bound is at most its C
      if (p < a.ocap) {
        a.owhich[p] = (uint8_t)j;
        a.osrc[p] = i;
        if (a.okey) a.okey[p] = x;
        if (a.oin) a.oin[p] = (uint16_t)sh.s[j].in_port;
      }
    }
    __syncthreads();  // (the next chunk's windows)
  }
}

// What a lane holds of its entry for the slot mover: `from` the source slot,
// `w` the bytes to take of it (0: nothing may be read, the slot is zero)
struct TxmFrom {
  const uint8_t *from;
  uint32_t w;
  __device__ __forceinline__ TxmFrom at(uint32_t e) const {
    return {(const uint8_t *)(uintptr_t)shfl64((uint64_t)(uintptr_t)from, e),
            (uint32_t)__shfl((int)w, (int)e)};
  }
  __device__ __forceinline__ TxmFrom at_uniform(uint32_t e) const {
    return {(const uint8_t *)(uintptr_t)readlane64((uint64_t)(uintptr_t)from, e),
            (uint32_t)__builtin_amdgcn_readlane((int)w, (int)e)};
  }
  __device__ __forceinline__ uint4 unit(uint32_t u, bool on) const {
    uint4 v = make_uint4(0, 0, 0, 0);  // an entry nothing is read through, and the bytes past w
    if (on && u < w) v = *(const uint4 *)(from + u);
    return v;
  }
};

__global__ __launch_bounds__(kSlotThreads) void txm_gather(const TxmArgs a) {
  __shared__ TxmShared sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t total = txm_stage(a, sh, tid);
  const uint32_t m = total < a.ocap ? (uint32_t)total : a.ocap;
  const uint32_t first = blockIdx.x * kSlotBlockEntries;
  if (first >= m) return;
  const SlotPath path = slot_path(a.oslot);
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k0 = (uint64_t)first + wv * kSlotPerWave + it * 64;  // (may pass 2^32)
    if (k0 >= m) break;
    const uint32_t left = m - k0 < 64 ? (uint32_t)(m - k0) : 64;
    const bool mine = lane < left;
    uint32_t j = ~0u, i = ~0u;
    if (mine) {
      j = a.owhich[k0 + lane];
      i = a.osrc[k0 + lane];
    }
    // after keys that decrease a position may hold a record no lane of
    // txm_rank wrote: nothing is read through a source or a packet that does
    // not exist
    const uint32_t jj = j < a.n_srcs ? j : 0;
    const bool ok = mine && j < a.n_srcs && i < sh.s[jj].n;
    uint32_t l = 0, w = 0;
    uint64_t at = 0;
    const uint8_t *from = nullptr;
    if (ok) {
      const TxmSrc &S = sh.s[jj];
      l = S.len[i];
      at = batch_time(S.now, S.now0, S.now_step, i);
      from = S.frames + (size_t)i * S.slot;
      w = S.slot < a.oslot ? S.slot : a.oslot;
    }
    if (mine) {
      const size_t k = k0 + lane;
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
    }
    slot_move(path, TxmFrom{from, w}, a.oframes, a.oslot, k0, lane, left);
  }
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_merge(vp_ctx *c, const vp_tx_source *srcs, uint32_t n_srcs,
                           const vp_tx_merged *o, void *stream) {
  if (!c || !srcs || !o || !o->count) return VP_EINVAL;
  if (n_srcs == 0 || n_srcs > VP_TX_MERGE_MAX) return VP_EINVAL;
  if (!slot_dest_ok(o) || ((!o->src || !o->which) && o->cap)) return VP_EINVAL;
  TxmArgs a = {};
  for (uint32_t j = 0; j < n_srcs; j++) {
    const vp_tx_source &s = srcs[j];
    const vp_dev_batch *b = s.batch;
    const vp_tx_lists *l = s.lists;
    if (!s.ctx || s.ctx->gpu != c->gpu || s.in_port > 0xFFFF) return VP_EINVAL;
    uint32_t nd;
    VP_TRY(tx_source_check(s.ctx, b, l, s.port, o->frames, o->slot, o->cap, &nd));
    TxmSrc &t = a.s[j];
    t.frames = b->frames;
    t.len = b->len;
    t.now = b->now;
    t.now0 = b->now0;
    t.now_step = b->now_step;
    t.idx = l->idx;
    t.offset = l->offset;
    t.key = s.key;
    t.n = b->frames && b->len ? b->n : 0;  // (allowed NULL only where nothing is gathered)
    t.nkey = b->n;
    t.slot = b->slot;
    t.lcap = l->cap;
    t.nd = nd;
    t.port = s.port;
    t.in_port = s.in_port;
  }
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernels hold the contexts' streams)
  for (uint32_t j = 0; j < n_srcs; j++)
    if (srcs[j].ctx != c) VP_TRY(serve_stop(srcs[j].ctx));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  a.n_srcs = n_srcs;
  a.oframes = o->frames;
  a.oslot = o->slot;
  a.ocap = o->cap;
  a.olen = o->len;
  a.onow = o->now;
  a.oin = o->in_dev;
  a.okey = o->key;
  a.osrc = o->src;
  a.owhich = o->which;
  a.count = o->count;
  // grids from cap. txm_rank's blocks walk the chunks of all lists in strides
  // (a list's last chunk may be short: one more block per source); at least
  // one block, so that count is written when cap == 0
  const uint32_t full = o->cap ? (o->cap - 1) / kSlotBlockEntries + 1 : 0;
  txm_rank<<<full + n_srcs, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  if (full) {
    txm_gather<<<full, kSlotThreads, 0, s>>>(a);
    VP_HIP(hipGetLastError());
  }
  return 0;
}
