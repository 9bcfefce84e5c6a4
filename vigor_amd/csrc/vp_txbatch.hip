// A port's transmit list as the next NF's device batch (vp_tx_rebatch,
// include/vigpath.h): the frames that one of vp_tx_build's lists names,
// gathered into consecutive slots with their len[], time and index of origin.
// One launch:
//
//   txr_gather  each block takes kSlotBlockEntries consecutive entries of the
//               port's list; a wave walks 64 of them per turn: idx[], len[]
//               and the time one entry per lane, stored coalesced, then the
//               slots through the slot mover (vp_slots_dev.h). Block 0 writes
//               the list's true count.
//
// No block waits for another, nothing is kept between the turns, and there is
// no workspace: the list's bounds are read from offset[] by every block.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(txbatch)

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

// What a lane holds of its entry for the slot mover: the packet's index in the
// source batch (32 bits: one shuffle per group) and whether anything may be
// read through it; the batch's base, its slot and the width taken are uniform.
struct TxrSrc {
  const uint8_t *frames;
  uint32_t slot, w, i;
  bool ok;
  __device__ __forceinline__ TxrSrc at(uint32_t e) const {
    return {frames, slot, w, (uint32_t)__shfl(i, (int)e), __shfl((int)ok, (int)e) != 0};
  }
  __device__ __forceinline__ TxrSrc at_uniform(uint32_t e) const {
    return {frames, slot, w, (uint32_t)__builtin_amdgcn_readlane((int)i, (int)e),
            __builtin_amdgcn_readlane((int)ok, (int)e) != 0};
  }
  __device__ __forceinline__ uint4 unit(uint32_t u, bool on) const {
    uint4 v = make_uint4(0, 0, 0, 0);  // an index outside the batch, and the bytes past w
    if (on && ok && u < w) v = *(const uint4 *)(frames + (size_t)i * slot + u);
    return v;
  }
};

__global__ __launch_bounds__(kSlotThreads) void txr_gather(const TxrArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  uint32_t lo;
  const uint32_t C = (uint32_t)__builtin_amdgcn_readfirstlane(
      (int)list_port(a.offset, a.port, list_entries(a.offset, a.nd, a.lcap), lo));
  if (blockIdx.x == 0 && tid == 0) *a.count = C;
  const uint32_t m = C < a.ocap ? C : a.ocap;
  const uint32_t first = blockIdx.x * kSlotBlockEntries;
  if (first >= m) return;
  const uint32_t w = a.slot < a.oslot ? a.slot : a.oslot;
  const SlotPath path = slot_path(a.oslot);
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k0 = (uint64_t)first + wv * kSlotPerWave + it * 64;  // (may pass 2^32)
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
      at = batch_time(a.now, a.now0, a.now_step, i);
    }
    if (mine) {
      const size_t k = k0 + lane;
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
      if (a.osrc) a.osrc[k] = i;
    }
    slot_move(path, TxrSrc{a.frames, a.slot, w, i, ok}, a.oframes, a.oslot, k0, lane, left);
  }
}

// What the call rejects of one source for the destination slots; vp_tx_merge
// asks the same of each of its sources
int tx_source_check(const vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l, uint32_t port,
                    const uint8_t *oframes, uint32_t oslot, uint32_t ocap, uint32_t *nd) {
  if (!b || !l || !l->offset || (!l->idx && l->cap)) return VP_EINVAL;
  *nd = ctx_devices(c);
  if (*nd > VP_MAX_DEVICES || port >= *nd || !slots_ok(b->frames, b->slot)) return VP_EINVAL;
  if ((!b->frames || !b->len) && b->n && l->cap && ocap) return VP_EINVAL;
  // the two slot arrays may not overlap: the gather is not in place
  const uint64_t sn = (uint64_t)b->n * b->slot, dn = (uint64_t)ocap * oslot;
  return bytes_overlap(b->frames, sn, oframes, dn) ? VP_EINVAL : 0;
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_rebatch(vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l,
                             uint32_t port, const vp_tx_next *o, void *stream) {
  if (!c || !o || !o->count || !slot_dest_ok(o)) return VP_EINVAL;
  uint32_t nd;
  VP_TRY(tx_source_check(c, b, l, port, o->frames, o->slot, o->cap, &nd));
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
  const uint32_t blocks = o->cap ? (o->cap - 1) / kSlotBlockEntries + 1 : 1;
  txr_gather<<<blocks, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  return 0;
}
