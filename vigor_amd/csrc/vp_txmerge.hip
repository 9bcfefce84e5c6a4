// Several transmit lists as one NF's device batch (vp_tx_merge,
// include/vigpath.h): the lists that vp_tx_build wrote for up to
// VP_TX_MERGE_MAX (context, batch, port) sources, merged by a 32-bit key per
// packet -- its position in the chain's input -- into consecutive slots, as the
// cables of several boxes into one would deliver them. Two launches
// (DESIGN.md §5.8):
//
//   txm_rank    each block takes kTxmBlockEntries consecutive entries of one
//               source's list. A few lanes narrow, by two binary searches per
//               other source, the window the block's first and last key fall
//               in; every lane then ranks its own entries inside those windows
//               (upper bound in the sources before its own, lower bound in
//               those after: the stable order) and scatters the small records
//               which[p], src[p], key[p], in_dev[p]. Block 0 writes the count.
//   txm_gather  txr_gather's movement (vp_txbatch.hip) with a source per
//               entry: which[] and src[] read coalesced, len[] and the time
//               stored coalesced, the slots moved in 16-byte units.
//
// No block waits for another and there is no workspace: every block reads the
// lists' bounds from the sources' offset[]. The sources' records travel as
// kernel arguments and are staged in LDS, where a lane may index them by its
// entry's source without a private segment.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"

namespace vp {

VP_PRELOAD_UNIT(txmerge)

constexpr uint32_t kTxmBlockEntries = 2048;
constexpr uint32_t kTxmThreads = 256, kTxmWaves = kTxmThreads / 64;
constexpr uint32_t kTxmPerLane = kTxmBlockEntries / kTxmThreads;
constexpr uint32_t kTxmPerWave = kTxmBlockEntries / kTxmWaves;
constexpr uint32_t kTxmTurns = kTxmPerWave / 64;  // 64 entries, one per lane, per turn
constexpr uint32_t kTxmMax = VP_TX_MERGE_MAX;
static_assert(kTxmBlockEntries % (64 * kTxmWaves) == 0, "whole waves");
static_assert(2 * kTxmMax <= kTxmThreads, "a lane per window end");

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
      // E = min(offset[n_devices], cap) entries are in idx[]; the port's are lo .. hi
      const uint32_t t = S.offset[S.nd], E = t < S.lcap ? t : S.lcap;
      const uint32_t o0 = S.offset[S.port], o1 = S.offset[S.port + 1];
      const uint32_t lo = o0 < E ? o0 : E, hi = o1 < E ? o1 : E;
      sh.lo[j] = lo;
      sh.C[j] = hi > lo ? hi - lo : 0u;  // (bad bounds: 0)
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

__global__ __launch_bounds__(kTxmThreads) void txm_rank(const TxmArgs a) {
  __shared__ TxmShared sh;
  __shared__ uint32_t win[2][kTxmMax];  // per other source: the block's window
  const uint32_t tid = threadIdx.x, ns = a.n_srcs;
  const uint64_t total = txm_stage(a, sh, tid);
  if (blockIdx.x == 0 && tid == 0) *a.count = total < 0xFFFFFFFFull ? (uint32_t)total : ~0u;
  if (a.ocap == 0) return;  // (nothing to rank into)
  uint64_t chunks = 0;
  for (uint32_t j = 0; j < ns; j++)
    chunks += ((uint64_t)sh.C[j] + kTxmBlockEntries - 1) / kTxmBlockEntries;
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    // chunk c is chunk c - base of source j
    uint32_t j = 0;
    uint64_t base = 0;
    for (; j + 1 < ns; j++) {
      const uint64_t nb = ((uint64_t)sh.C[j] + kTxmBlockEntries - 1) / kTxmBlockEntries;
      if (c < base + nb) break;
      base += nb;
    }
    const uint64_t m0 = (c - base) * kTxmBlockEntries;  // < C_j
    const uint32_t Cj = sh.C[j];
    const uint32_t cnt = Cj - m0 < kTxmBlockEntries ? (uint32_t)(Cj - m0) : kTxmBlockEntries;
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
      const uint32_t e = it * kTxmThreads + tid;
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

// The slot movement of vp_txbatch.hip, with the address and the width of every
// entry's source slot in its lane: `from` the slot, `w` the bytes to take of it
// (0: nothing may be read, the slot is zero).
struct TxmUnit {
  uint4 v;
  bool on;
};

__device__ __forceinline__ const uint8_t *txm_shfl_ptr(const uint8_t *p, uint32_t e) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)e);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)e);
  return (const uint8_t *)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ TxmUnit txm_sub_load(uint32_t lg, uint32_t g, uint32_t lane,
                                                const uint8_t *from, uint32_t w, uint32_t left) {
  // U = 1 << lg units a slot: lanes U f .. U f + U - 1 move entry (64 / U) g + f
  const uint32_t e = ((64u >> lg) * g) + (lane >> lg), u = 16 * (lane & ((1u << lg) - 1));
  const uint8_t *gfrom = txm_shfl_ptr(from, e);
  const uint32_t gw = (uint32_t)__shfl((int)w, (int)e);
  TxmUnit r;
  r.on = e < left;
  r.v = make_uint4(0, 0, 0, 0);  // an entry nothing is read through, and the bytes past w
  if (r.on && u < gw) r.v = *(const uint4 *)(gfrom + u);
  return r;
}

template <uint32_t U>
__device__ __forceinline__ void txm_sub(const TxmArgs &a, uint64_t k0, uint32_t lane,
                                        const uint8_t *from, uint32_t w, uint32_t left) {
  uint8_t *to = a.oframes + k0 * a.oslot + 16 * lane;  // (k0 is 64 bits)
  if constexpr (U == 4) {  // 64-byte slots: the four loads of a turn in flight together
    TxmUnit r[4];
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) r[g] = txm_sub_load(2, g, lane, from, w, left);
#pragma unroll
    for (uint32_t g = 0; g < 4; g++)
      if (r[g].on) *(uint4 *)(to + 1024 * g) = r[g].v;
  } else {
    const uint32_t units = a.oslot / 16;  // 8, 16, 32 or 64
    const uint32_t lg = 31 - __clz((int)units);
    for (uint32_t g = 0; g < units && (64u >> lg) * g < left; g++) {
      const TxmUnit r = txm_sub_load(lg, g, lane, from, w, left);
      if (r.on) *(uint4 *)(to + (size_t)1024 * g) = r.v;
    }
  }
}

// The wave path, for every other slot: the whole wave moves one entry after
// another, 1 KiB an instruction
__device__ __forceinline__ void txm_wave(const TxmArgs &a, uint64_t k0, uint32_t lane,
                                         const uint8_t *from, uint32_t w, uint32_t left) {
  const uint64_t fv = (uint64_t)(uintptr_t)from;
  for (uint32_t e = 0; e < left; e++) {
    const uint32_t flo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fv, (int)e);
    const uint32_t fhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fv >> 32), (int)e);
    const uint32_t gw = (uint32_t)__builtin_amdgcn_readlane((int)w, (int)e);
    const uint8_t *gfrom = (const uint8_t *)(uintptr_t)(((uint64_t)fhi << 32) | flo);
    uint8_t *to = a.oframes + (k0 + e) * a.oslot;
    for (uint32_t u = 16 * lane; u < a.oslot; u += 16 * 64) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (u < gw) v = *(const uint4 *)(gfrom + u);
      *(uint4 *)(to + u) = v;
    }
  }
}

__global__ __launch_bounds__(kTxmThreads) void txm_gather(const TxmArgs a) {
  __shared__ TxmShared sh;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t total = txm_stage(a, sh, tid);
  const uint32_t m = total < a.ocap ? (uint32_t)total : a.ocap;
  const uint32_t first = blockIdx.x * kTxmBlockEntries;
  if (first >= m) return;
  const uint32_t units = a.oslot / 16;
  const bool sub = units <= 64 && 64 % units == 0;
  for (uint32_t it = 0; it < kTxmTurns; it++) {
    const uint64_t k0 = (uint64_t)first + wv * kTxmPerWave + it * 64;  // (may pass 2^32)
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
      at = S.now ? (uint64_t)S.now[i] : (uint64_t)S.now0 + (uint64_t)i * (uint64_t)S.now_step;
      from = S.frames + (size_t)i * S.slot;
      w = S.slot < a.oslot ? S.slot : a.oslot;
    }
    if (mine) {
      const size_t k = k0 + lane;
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
    }
    if (units == 4)
      txm_sub<4>(a, k0, lane, from, w, left);
    else if (sub)
      txm_sub<0>(a, k0, lane, from, w, left);
    else
      txm_wave(a, k0, lane, from, w, left);
  }
}

static uint32_t txm_devices(const vp_ctx *c) {
  switch (c->kind) {
    case KIND_NAT: return c->nat.n_devices;
    case KIND_BRIDGE: return c->brg.n_devices;
    case KIND_LB: return c->lb.n_devices;
    case KIND_FW: return c->fw.n_devices;
    case KIND_POL: return c->pol.n_devices;
    default: return 0;
  }
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_merge(vp_ctx *c, const vp_tx_source *srcs, uint32_t n_srcs,
                           const vp_tx_merged *o, void *stream) {
  if (!c || !srcs || !o || !o->count) return VP_EINVAL;
  if (n_srcs == 0 || n_srcs > VP_TX_MERGE_MAX) return VP_EINVAL;
  if (o->slot < 64 || o->slot % 16 || ((uintptr_t)o->frames & 15)) return VP_EINVAL;
  if ((!o->frames || !o->len || !o->src || !o->which) && o->cap) return VP_EINVAL;
  TxmArgs a = {};
  for (uint32_t j = 0; j < n_srcs; j++) {  // per source, what vp_tx_rebatch rejects
    const vp_tx_source &s = srcs[j];
    const vp_dev_batch *b = s.batch;
    const vp_tx_lists *l = s.lists;
    if (!s.ctx || !b || !l || !l->offset || s.in_port > 0xFFFF) return VP_EINVAL;
    if (!l->idx && l->cap) return VP_EINVAL;
    if (b->slot < 64 || b->slot % 16 || ((uintptr_t)b->frames & 15)) return VP_EINVAL;
    if (s.ctx->gpu != c->gpu) return VP_EINVAL;
    const uint32_t nd = txm_devices(s.ctx);
    if (nd > VP_MAX_DEVICES || s.port >= nd) return VP_EINVAL;
    if ((!b->frames || !b->len) && b->n && l->cap && o->cap) return VP_EINVAL;
    if (b->frames && o->frames && b->n && o->cap) {  // the two slot arrays may not overlap
      const uintptr_t s0 = (uintptr_t)b->frames, s1 = s0 + (uint64_t)b->n * b->slot;
      const uintptr_t d0 = (uintptr_t)o->frames, d1 = d0 + (uint64_t)o->cap * o->slot;
      if (s0 < d1 && d0 < s1) return VP_EINVAL;
    }
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
  const uint32_t full = o->cap ? (o->cap - 1) / kTxmBlockEntries + 1 : 0;
  txm_rank<<<full + n_srcs, kTxmThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  if (full) {
    txm_gather<<<full, kTxmThreads, 0, s>>>(a);
    VP_HIP(hipGetLastError());
  }
  return 0;
}
