// A stage's packets back in the slots they started from (vp_tx_return,
// include/vigpath.h): the inverse of vp_tx_rebatch. Entry k of `from` goes to
// slot home[k] of `home`, and its out port, translated into a port of the
// composite box, to out_dev[home[k]]. One launch:
//
//   txt_scatter each block takes kSlotBlockEntries consecutive entries; a wave
//               walks 64 of them per turn: home[], out_dev[] and in_dev[] one
//               entry per lane, the first of a run of equal homes found with
//               one shuffle (a turn's lane 0 reads the entry before it), the
//               action chosen, out_dev stored, then the slots through this
//               unit's mover. A wave adds its counts to *stats once, at its
//               end.
//
// The mover is the family's (vp_slots_dev.h: the 64-byte path with four loads
// in flight, the sub-wave path, the wave path) with the index on the other
// side: it reads the consecutive slots k0 .. and writes slot home[k] of each
// entry that is written home. It is this unit's own: slot_move's destination is
// k0 * slot by construction, and a per-entry destination in it would change
// the five kernels that share it.
//
// No block waits for another, nothing is kept between the turns but the
// counts, and there is no workspace, no LDS and no private segment.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(txreturn)

struct TxtArgs {
  const uint8_t *frames;  // from
  uint32_t slot, n;
  const uint16_t *out, *in;
  uint32_t in_port;
  uint8_t *hframes;  // home
  uint32_t hslot, hn;
  const uint16_t *hin;
  uint32_t hin_port;
  uint16_t *hout;
  const uint32_t *home;
  uint32_t nd;
  uint32_t port[VP_MAX_DEVICES];
  uint32_t on_drop, on_flood, on_bad;
  uint32_t move;  // 0: the batch is its own home, no frame byte moves
  vp_tx_return_stats *stats;
};

// What a lane holds of its entry for the mover: its home slot and whether it
// is written there (0 for an entry that does not exist)
struct TxtDst {
  uint32_t h, wr;
};

// The 16 bytes at offset u of source slot k, zero past the width taken
__device__ __forceinline__ uint4 txt_unit(const TxtArgs &a, uint64_t k, uint32_t u, uint32_t w,
                                          bool on) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (on && u < w) v = *(const uint4 *)(a.frames + k * a.slot + u);
  return v;
}

// Sub-wave path, U = 1 << lg units a slot: lanes U f .. U f + U - 1 move entry
// (64 / U) g + f of the turn, one unit each
__device__ __forceinline__ SlotUnit txt_sub_load(const TxtArgs &a, const TxtDst d, uint32_t lg,
                                                 uint32_t g, uint64_t k0, uint32_t lane,
                                                 uint32_t w, uint8_t *&to) {
  const uint32_t e = ((64u >> lg) * g) + (lane >> lg), u = 16 * (lane & ((1u << lg) - 1));
  const uint32_t h = (uint32_t)__shfl((int)d.h, (int)e);
  SlotUnit r;
  r.on = __shfl((int)d.wr, (int)e) != 0;
  r.v = txt_unit(a, k0 + e, u, w, r.on);
  to = a.hframes + (uint64_t)h * a.hslot + u;  // (every byte address in 64 bits)
  return r;
}

template <uint32_t U>
__device__ __forceinline__ void txt_sub(const TxtArgs &a, const TxtDst d, uint64_t k0,
                                        uint32_t lane, uint32_t left, uint32_t w) {
  if constexpr (U == 4) {  // 64-byte slots: the four loads of a turn in flight together
    SlotUnit r[4];
    uint8_t *to[4];
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) r[g] = txt_sub_load(a, d, 2, g, k0, lane, w, to[g]);
#pragma unroll
    for (uint32_t g = 0; g < 4; g++)
      if (r[g].on) *(uint4 *)to[g] = r[g].v;
  } else {
    const uint32_t units = a.hslot / 16;  // 8, 16, 32 or 64
    const uint32_t lg = 31 - __clz((int)units);
    for (uint32_t g = 0; g < units && (64u >> lg) * g < left; g++) {
      uint8_t *to;
      const SlotUnit r = txt_sub_load(a, d, lg, g, k0, lane, w, to);
      if (r.on) *(uint4 *)to = r.v;
    }
  }
}

// Wave path: the whole wave moves one written entry after another
__device__ __forceinline__ void txt_wave(const TxtArgs &a, const TxtDst d, uint64_t k0,
                                         uint32_t lane, uint32_t left, uint32_t w) {
  for (uint32_t e = 0; e < left; e++) {
    if (!__builtin_amdgcn_readlane((int)d.wr, (int)e)) continue;
    const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)d.h, (int)e);
    uint8_t *to = a.hframes + (uint64_t)h * a.hslot;
    for (uint32_t u = 16 * lane; u < a.hslot; u += 16 * 64)
      *(uint4 *)(to + u) = txt_unit(a, k0 + e, u, w, true);
  }
}

__device__ __forceinline__ void txt_count(uint64_t *to, uint32_t v, uint32_t lane) {
  v = wave_sum(v);
  if (lane == 0 && v) atomicAdd((unsigned long long *)to, (unsigned long long)v);
}

__global__ __launch_bounds__(kSlotThreads) void txt_scatter(const TxtArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t w0 = (uint64_t)blockIdx.x * kSlotBlockEntries + wv * kSlotPerWave;
  if (w0 >= a.n) return;
  // port[] one value per lane (lane d and d + 32 hold port[d]), fetched by out
  // port with a shuffle: a table indexed per lane would live in scratch memory
  uint32_t tab = 0;
#pragma unroll
  for (uint32_t d = 0; d < VP_MAX_DEVICES; d++) tab = (lane & 31) == d ? a.port[d] : tab;
  const uint32_t w = a.slot < a.hslot ? a.slot : a.hslot;
  const SlotPath path = slot_path(a.hslot);
  uint32_t c_ret = 0, c_drop = 0, c_skip = 0, c_dup = 0, c_bad = 0;
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k0 = w0 + it * 64;  // (may pass 2^32)
    if (k0 >= a.n) break;
    const uint32_t left = a.n - k0 < 64 ? (uint32_t)(a.n - k0) : 64;
    const bool mine = lane < left;
    const uint64_t k = k0 + lane;
    uint32_t h = (uint32_t)k, out = 0, in = a.in_port;
    bool fst = mine;
    if (a.home) {
      if (mine) h = a.home[k];
      uint32_t hp = (uint32_t)__shfl_up((int)h, 1);
      if (lane == 0 && k0) hp = a.home[k0 - 1];
      fst = mine && (k == 0 || h != hp);
    }
    if (mine) {
      out = a.out[k];
      if (a.in) in = a.in[k];
    }
    // vp_tx_build's order: dropped, flooded, a port, anything else
    const uint32_t via = (uint32_t)__shfl((int)tab, (int)(out & 31));
    const uint32_t act = out == in                ? a.on_drop
                         : out == VP_FLOOD_FRAME ? a.on_flood
                         : out < a.nd            ? via
                                                 : a.on_bad;
    const bool inh = h < a.hn, skip = act == VP_RET_SKIP, drop = act == VP_RET_DROP;
    const bool wr = fst && inh && !skip;
    c_ret += wr;
    c_drop += wr && drop;
    c_skip += fst && skip;
    c_dup += mine && !fst;
    c_bad += fst && !inh;
    if (wr) {
      uint32_t val = act;
      if (drop) val = a.hin ? a.hin[h] : a.hin_port;  // the home packet's own in port
      a.hout[h] = (uint16_t)val;
    }
    if (a.move) {
      const TxtDst d{h, wr ? 1u : 0u};
      if (path.units == 4)
        txt_sub<4>(a, d, k0, lane, left, w);
      else if (path.sub)
        txt_sub<0>(a, d, k0, lane, left, w);
      else
        txt_wave(a, d, k0, lane, left, w);
    }
  }
  if (a.stats) {  // (zeroed on the stream before the launch)
    txt_count(&a.stats->returned, c_ret, lane);
    txt_count(&a.stats->dropped, c_drop, lane);
    txt_count(&a.stats->skipped, c_skip, lane);
    txt_count(&a.stats->dup, c_dup, lane);
    txt_count(&a.stats->bad_home, c_bad, lane);
  }
}

static bool ret_action_ok(uint32_t a) {
  return a <= 0xFFFFu || a == VP_RET_SKIP || a == VP_RET_DROP;
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_return(vp_ctx *c, const vp_dev_batch *from, const vp_dev_batch *home,
                            const vp_tx_way_home *way, void *stream) {
  if (!c || !from || !home || !way) return VP_EINVAL;
  if (from->n && (!from->frames || !from->out_dev)) return VP_EINVAL;
  if (from->n && home->n && (!home->frames || !home->out_dev)) return VP_EINVAL;
  if (!slots_ok(from->frames, from->slot) || !slots_ok(home->frames, home->slot))
    return VP_EINVAL;
  if ((!from->in_dev && from->in_port > 0xFFFFu) || (!home->in_dev && home->in_port > 0xFFFFu))
    return VP_EINVAL;
  if (!ret_action_ok(way->on_drop) || !ret_action_ok(way->on_flood) || !ret_action_ok(way->on_bad))
    return VP_EINVAL;
  // the batch is its own home (stage 0, rewritten in place): only out_dev is
  // translated; any other overlap of the two slot arrays is refused
  const bool in_place =
      from->frames && from->frames == home->frames && from->slot == home->slot && !way->home;
  if (!in_place && bytes_overlap(from->frames, (uint64_t)from->n * from->slot, home->frames,
                                 (uint64_t)home->n * home->slot))
    return VP_EINVAL;
  // (the context is read from here on)
  const uint32_t nd = ctx_devices(c);
  if (nd > VP_MAX_DEVICES) return VP_EINVAL;
  for (uint32_t d = 0; d < nd; d++)
    if (!ret_action_ok(way->port[d])) return VP_EINVAL;
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the waves add to *stats: it starts from zero on the same stream
  if (way->stats) VP_HIP(hipMemsetAsync(way->stats, 0, sizeof(vp_tx_return_stats), s));
  if (!from->n) return 0;
  TxtArgs a;
  a.frames = from->frames;
  a.slot = from->slot;
  a.n = from->n;
  a.out = from->out_dev;
  a.in = from->in_dev;
  a.in_port = from->in_port;
  a.hframes = home->frames;
  a.hslot = home->slot;
  a.hn = home->frames && home->out_dev ? home->n : 0;  // (NULL only where n == 0)
  a.hin = home->in_dev;
  a.hin_port = home->in_port;
  a.hout = home->out_dev;
  a.home = way->home;
  a.nd = nd;
  for (uint32_t d = 0; d < VP_MAX_DEVICES; d++) a.port[d] = d < nd ? way->port[d] : way->on_bad;
  a.on_drop = way->on_drop;
  a.on_flood = way->on_flood;
  a.on_bad = way->on_bad;
  a.move = in_place ? 0u : 1u;
  a.stats = way->stats;
  const uint32_t blocks = (from->n - 1) / kSlotBlockEntries + 1;
  txt_scatter<<<blocks, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  return 0;
}
