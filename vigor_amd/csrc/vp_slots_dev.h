// Device code shared by the transmit / receive family (vp_tx.hip,
// vp_txpack.hip, vp_txbatch.hip, vp_txmerge.hip, vp_rxunpack.hip,
// vp_rxmerge.hip): the block geometry, the small wave and list helpers, and the
// slot mover that writes a turn's 64 entries into consecutive slots.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace vp {

// A 256-thread block takes kSlotBlockEntries consecutive entries, a wave
// kSlotPerWave of them, 64 (one per lane) per turn.
constexpr uint32_t kSlotBlockEntries = 2048;
constexpr uint32_t kSlotThreads = 256, kSlotWaves = kSlotThreads / 64;
constexpr uint32_t kSlotPerWave = kSlotBlockEntries / kSlotWaves;
constexpr uint32_t kSlotTurns = kSlotPerWave / 64;
static_assert(kSlotBlockEntries % (64 * kSlotWaves) == 0, "whole waves");

__device__ __forceinline__ uint32_t pad16(uint32_t l) { return (l + 15u) & ~15u; }

// The bytes of a 16-byte unit at or beyond `keep` (>= 1) cleared
__device__ __forceinline__ uint4 unit_clear(uint4 v, uint32_t keep) {
  if (keep < 16) {
    const uint32_t w = keep >> 2, m = (1u << (8 * (keep & 3))) - 1u;
    v.x = w > 0 ? v.x : v.x & m;
    v.y = w > 1 ? v.y : w == 1 ? v.y & m : 0u;
    v.z = w > 2 ? v.z : w == 2 ? v.z & m : 0u;
    v.w = w == 3 ? v.w & m : 0u;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Inclusive scan over the wave's 64 lanes (uint32_t or uint64_t)
template <class T>
__device__ __forceinline__ T wave_scan(T x, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(x, o);
    if (lane >= o) x += u;
  }
  return x;
}

// Packet i's time in a batch: now[i], or now0 + i * now_step in 64 bits
__device__ __forceinline__ uint64_t batch_time(const int64_t *now, int64_t now0, int64_t now_step,
                                               uint32_t i) {
  return now ? (uint64_t)now[i] : (uint64_t)now0 + (uint64_t)i * (uint64_t)now_step;
}

// vp_tx_build's lists: E = min(offset[n_devices], cap) entries are in idx[];
// port's are lo .. lo + C - 1 (bad bounds: C = 0)
__device__ __forceinline__ uint32_t list_entries(const uint32_t *offset, uint32_t nd,
                                                 uint32_t cap) {
  const uint32_t t = offset[nd];
  return t < cap ? t : cap;
}
__device__ __forceinline__ uint32_t list_port(const uint32_t *offset, uint32_t port, uint32_t E,
                                              uint32_t &lo) {
  const uint32_t o0 = offset[port], o1 = offset[port + 1];
  lo = o0 < E ? o0 : E;
  const uint32_t hi = o1 < E ? o1 : E;
  return hi > lo ? hi - lo : 0u;
}

// The slot mover. A wave writes the `left` <= 64 entries of a turn into the
// consecutive `oslot`-byte slots k0 .. k0 + left - 1 of `oframes`, in aligned
// 16-byte units, whole slots (zero where the source gives nothing). What an
// entry is read from is a descriptor S that every lane holds of its own entry:
//   S at(e) const          entry e's descriptor, e per lane (__shfl)
//   S at_uniform(e) const  the same for a wave-uniform e (v_readlane)
//   uint4 unit(u, on) const  the 16 bytes at byte offset u of the slot image;
//                          zero, and nothing read, where nothing may be read
//                          or the entry does not exist (!on)
// A slot of U = oslot / 16 units with U dividing 64 takes the sub-wave path:
// lanes U f .. U f + U - 1 move entry (64 / U) g + f, one unit each, so one
// instruction stores 1 KiB of consecutive output bytes (16 frames for 64-byte
// slots, whose four loads of a turn are issued before the four stores). Any
// other slot takes the wave path: the whole wave moves one entry after
// another, 1 KiB an instruction. Entries at or beyond `left` do not exist.
struct SlotUnit {
  uint4 v;
  bool on;
};

template <class S>
__device__ __forceinline__ SlotUnit slot_sub_load(const S &src, uint32_t lg, uint32_t g,
                                                  uint32_t lane, uint32_t left) {
  // U = 1 << lg
  const uint32_t e = ((64u >> lg) * g) + (lane >> lg), u = 16 * (lane & ((1u << lg) - 1));
  const S d = src.at(e);
  SlotUnit r;
  r.on = e < left;
  r.v = d.unit(u, r.on);
  return r;
}

template <uint32_t U, class S>
__device__ __forceinline__ void slot_sub(const S &src, uint8_t *oframes, uint32_t oslot,
                                         uint64_t k0, uint32_t lane, uint32_t left) {
  uint8_t *to = oframes + k0 * oslot + 16 * lane;  // (k0 is 64 bits)
  if constexpr (U == 4) {  // 64-byte slots: the four loads of a turn in flight together
    SlotUnit r[4];
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) r[g] = slot_sub_load(src, 2, g, lane, left);
#pragma unroll
    for (uint32_t g = 0; g < 4; g++)
      if (r[g].on) *(uint4 *)(to + 1024 * g) = r[g].v;
  } else {
    const uint32_t units = oslot / 16;  // 8, 16, 32 or 64
    const uint32_t lg = 31 - __clz((int)units);
    for (uint32_t g = 0; g < units && (64u >> lg) * g < left; g++) {
      const SlotUnit r = slot_sub_load(src, lg, g, lane, left);
      if (r.on) *(uint4 *)(to + (size_t)1024 * g) = r.v;
    }
  }
}

template <class S>
__device__ __forceinline__ void slot_wave(const S &src, uint8_t *oframes, uint32_t oslot,
                                          uint64_t k0, uint32_t lane, uint32_t left) {
  for (uint32_t e = 0; e < left; e++) {
    const S d = src.at_uniform(e);
    uint8_t *to = oframes + (k0 + e) * oslot;
    for (uint32_t u = 16 * lane; u < oslot; u += 16 * 64) *(uint4 *)(to + u) = d.unit(u, true);
  }
}

// Which path a slot takes; a kernel works it out once, before its turns (the
// division is not hoisted out of them otherwise)
struct SlotPath {
  uint32_t units;
  bool sub;
};
__device__ __forceinline__ SlotPath slot_path(uint32_t oslot) {
  const uint32_t units = oslot / 16;
  return {units, units <= 64 && 64 % units == 0};
}

template <class S>
__device__ __forceinline__ void slot_move(const SlotPath path, const S &src, uint8_t *oframes,
                                          uint32_t oslot, uint64_t k0, uint32_t lane,
                                          uint32_t left) {
  if (path.units == 4)
    slot_sub<4>(src, oframes, oslot, k0, lane, left);
  else if (path.sub)
    slot_sub<0>(src, oframes, oslot, k0, lane, left);
  else
    slot_wave(src, oframes, oslot, k0, lane, left);
}

// A 64-bit lane value fetched as two 32-bit halves
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t e) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)e);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)e);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t e) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)e);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)e);
  return ((uint64_t)hi << 32) | lo;
}

// vp_rx_unpack's stream and destination as its kernels take them
// (vp_rxunpack.hip); vp_rx_merge (vp_rxmerge.hip) fills one per queue without
// pos[] for rxu_sizes, whose sums, scanned, are every wave's first position.
struct RxuArgs {
  const uint8_t *data;  // the stream
  uint64_t bytes;
  const uint64_t *pos;
  const uint32_t *sel;
  const uint16_t *len;
  const int64_t *now;
  int64_t now0, now_step;
  uint32_t meta_n;
  uint32_t m;            // min(n, cap): the entries that are written
  uint32_t n;
  const uint64_t *base;  // pos == NULL: every wave's first position (scanned sums)
  uint8_t *oframes;      // the batch
  uint32_t oslot;
  uint16_t *olen;
  int64_t *onow;
  uint32_t *osrc;
  uint32_t *count;
};

// Entry k's index into len[] / now[] and its length; the length is 0 where the
// index is outside them, and nothing is read through such an index
__device__ __forceinline__ void rxu_meta(const RxuArgs &a, uint64_t k, bool mine, uint32_t &mm,
                                         bool &in, uint32_t &l) {
  mm = (uint32_t)k;
  if (mine && a.sel) mm = a.sel[k];
  in = mine && mm < a.meta_n;
  l = in ? a.len[mm] : 0u;
}

// Every wave of every block sums the padded lengths of the kSlotPerWave entries
// below a.m it stands for into sums[block * kSlotWaves + wave]
__global__ void rxu_sizes(const RxuArgs a, uint64_t *sums);

}  // namespace vp
