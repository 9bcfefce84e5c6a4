// A port's transmit list as the next NF's device batch (vp_tx_rebatch,
// include/vigpath.h): the frames that one of vp_tx_build's lists names,
// gathered into consecutive slots with their len[], time and index of origin.
// One launch:
//
//   txr_gather  each block takes kTxrBlockEntries consecutive entries of the
//               port's list; a wave walks 64 of them per turn: idx[], len[]
//               and the time one entry per lane, stored coalesced, then the
//               slots in 16-byte units. Block 0 writes the list's true count.
//
// No block waits for another, nothing is kept between the turns, and there is
// no workspace: the list's bounds are read from offset[] by every block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"

namespace vp {

VP_PRELOAD_UNIT(txbatch)

constexpr uint32_t kTxrBlockEntries = 2048;
constexpr uint32_t kTxrThreads = 256, kTxrWaves = kTxrThreads / 64;
constexpr uint32_t kTxrPerWave = kTxrBlockEntries / kTxrWaves;
constexpr uint32_t kTxrTurns = kTxrPerWave / 64;  // 64 entries, one per lane, per turn
static_assert(kTxrBlockEntries % (64 * kTxrWaves) == 0, "whole waves");

struct TxrArgs {
  const uint8_t *frames;  // the source batch
  const uint16_t *len;
  const int64_t *now;
  int64_t now0, now_step;
  uint32_t n, slot;
  const uint32_t *idx;  // the lists
  const uint32_t *offset;
  uint32_t lcap, nd, port;
  uint8_t *oframes;  // the next batch
  uint32_t oslot, ocap;
  uint16_t *olen;
  int64_t *onow;
  uint32_t *osrc;
  uint32_t *count;
};

// The sub-wave path, for a destination slot of U 16-byte units where U divides
// 64: lanes U f .. U f + U - 1 move entry (64 / U) g + f of this turn, one
// unit each, so one instruction stores 1 KiB of consecutive output bytes (16
// frames for 64-byte slots). `i` is the lane's own entry's packet, `ok`
// whether anything may be read through it; entries at or beyond `left` do not
// exist.
struct TxrUnit {
  uint4 v;
  bool on;
};

__device__ __forceinline__ TxrUnit txr_sub_load(const TxrArgs &a, uint32_t lg, uint32_t g,
                                                uint32_t lane, uint32_t i, bool ok,
                                                uint32_t left, uint32_t w) {
  // U = 1 << lg
  const uint32_t e = ((64u >> lg) * g) + (lane >> lg), u = 16 * (lane & ((1u << lg) - 1));
  const uint32_t gi = __shfl(i, (int)e);
  const bool gok = __shfl((int)ok, (int)e) != 0;
  TxrUnit r;
  r.on = e < left;
  r.v = make_uint4(0, 0, 0, 0);  // an index outside the batch, and the bytes past w
  if (r.on && gok && u < w) r.v = *(const uint4 *)(a.frames + (size_t)gi * a.slot + u);
  return r;
}

template <uint32_t U>
__device__ __forceinline__ void txr_sub(const TxrArgs &a, uint64_t k0, uint32_t lane, uint32_t i,
                                        bool ok, uint32_t left, uint32_t w) {
  uint8_t *to = a.oframes + k0 * a.oslot + 16 * lane;  // (k0 is 64 bits)
  if constexpr (U == 4) {  // 64-byte slots: the four loads of a turn in flight together
    TxrUnit r[4];
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) r[g] = txr_sub_load(a, 2, g, lane, i, ok, left, w);
#pragma unroll
    for (uint32_t g = 0; g < 4; g++)
      if (r[g].on) *(uint4 *)(to + 1024 * g) = r[g].v;
  } else {
    const uint32_t units = a.oslot / 16;  // 8, 16, 32 or 64
    const uint32_t lg = 31 - __clz((int)units);
    for (uint32_t g = 0; g < units && (64u >> lg) * g < left; g++) {
      const TxrUnit r = txr_sub_load(a, lg, g, lane, i, ok, left, w);
      if (r.on) *(uint4 *)(to + (size_t)1024 * g) = r.v;
    }
  }
}

// The wave path, for every other slot: the whole wave moves one entry after
// another, 1 KiB an instruction
__device__ __forceinline__ void txr_wave(const TxrArgs &a, uint64_t k0, uint32_t lane, uint32_t i,
                                         bool ok, uint32_t left, uint32_t w) {
  for (uint32_t e = 0; e < left; e++) {
    const uint32_t gi = (uint32_t)__builtin_amdgcn_readlane((int)i, (int)e);
    const bool gok = __builtin_amdgcn_readlane((int)ok, (int)e) != 0;
    const uint8_t *from = a.frames + (size_t)gi * a.slot;
    uint8_t *to = a.oframes + (k0 + e) * a.oslot;
    for (uint32_t u = 16 * lane; u < a.oslot; u += 16 * 64) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (gok && u < w) v = *(const uint4 *)(from + u);
      *(uint4 *)(to + u) = v;
    }
  }
}

__global__ __launch_bounds__(kTxrThreads) void txr_gather(const TxrArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  // E = min(offset[n_devices], cap) entries are in idx[]; the port's are lo .. hi
  const uint32_t t = a.offset[a.nd], E = t < a.lcap ? t : a.lcap;
  const uint32_t o0 = a.offset[a.port], o1 = a.offset[a.port + 1];
  const uint32_t lo = o0 < E ? o0 : E, hi = o1 < E ? o1 : E;
  const uint32_t C =
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(hi > lo ? hi - lo : 0u));  // (bad bounds: 0)
  if (blockIdx.x == 0 && tid == 0) *a.count = C;
  const uint32_t m = C < a.ocap ? C : a.ocap;
  const uint32_t first = blockIdx.x * kTxrBlockEntries;
  if (first >= m) return;
  const uint32_t w = a.slot < a.oslot ? a.slot : a.oslot;
  const uint32_t units = a.oslot / 16;
  const bool sub = units <= 64 && 64 % units == 0;
  for (uint32_t it = 0; it < kTxrTurns; it++) {
    const uint64_t k0 = (uint64_t)first + wv * kTxrPerWave + it * 64;  // (may pass 2^32)
    if (k0 >= m) break;
    const uint32_t left = m - k0 < 64 ? (uint32_t)(m - k0) : 64;
    const bool mine = lane < left;
    uint32_t i = ~0u;
    if (mine) i = a.idx[(size_t)lo + k0 + lane];
    const bool ok = mine && i < a.n;  // nothing is read through an index outside the batch
    uint32_t l = 0;
    uint64_t at = 0;
    if (ok) {
      l = a.len[i];
      at = a.now ? (uint64_t)a.now[i] : (uint64_t)a.now0 + (uint64_t)i * (uint64_t)a.now_step;
    }
    if (mine) {
      const size_t k = k0 + lane;
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
      if (a.osrc) a.osrc[k] = i;
    }
    if (units == 4)
      txr_sub<4>(a, k0, lane, i, ok, left, w);
    else if (sub)
      txr_sub<0>(a, k0, lane, i, ok, left, w);
    else
      txr_wave(a, k0, lane, i, ok, left, w);
  }
}

static uint32_t txr_devices(const vp_ctx *c) {
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

extern "C" int vp_tx_rebatch(vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l,
                             uint32_t port, const vp_tx_next *o, void *stream) {
  if (!c || !b || !l || !o || !l->offset || !o->count) return VP_EINVAL;
  if (!l->idx && l->cap) return VP_EINVAL;
  const uint32_t nd = txr_devices(c);
  if (nd > VP_MAX_DEVICES || port >= nd) return VP_EINVAL;
  if (b->slot < 64 || b->slot % 16 || o->slot < 64 || o->slot % 16) return VP_EINVAL;
  if (((uintptr_t)b->frames | (uintptr_t)o->frames) & 15) return VP_EINVAL;
  if ((!o->frames || !o->len) && o->cap) return VP_EINVAL;
  if ((!b->frames || !b->len) && b->n && l->cap && o->cap) return VP_EINVAL;
  if (b->frames && o->frames && b->n && o->cap) {  // the two slot arrays may not overlap
    const uintptr_t s0 = (uintptr_t)b->frames, s1 = s0 + (uint64_t)b->n * b->slot;
    const uintptr_t d0 = (uintptr_t)o->frames, d1 = d0 + (uint64_t)o->cap * o->slot;
    if (s0 < d1 && d0 < s1) return VP_EINVAL;
  }
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  TxrArgs a;
  a.frames = b->frames;
  a.len = b->len;
  a.now = b->now;
  a.now0 = b->now0;
  a.now_step = b->now_step;
  a.n = b->frames && b->len ? b->n : 0;  // (allowed NULL only where nothing is gathered)
  a.slot = b->slot;
  a.idx = l->idx;
  a.offset = l->offset;
  a.lcap = l->cap;
  a.nd = nd;
  a.port = port;
  a.oframes = o->frames;
  a.oslot = o->slot;
  a.ocap = o->cap;
  a.olen = o->len;
  a.onow = o->now;
  a.osrc = o->src;
  a.count = o->count;
  // at least one block, so that count is written when cap == 0
  const uint32_t blocks = o->cap ? (o->cap - 1) / kTxrBlockEntries + 1 : 1;
  txr_gather<<<blocks, kTxrThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  return 0;
}
