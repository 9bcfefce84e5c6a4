// A packed frame stream as a device batch (vp_rx_unpack, include/vigpath.h):
// the inverse of vp_tx_pack. Frames that lie at 16-byte aligned positions in
// one run of bytes are scattered into consecutive slots, with their len[],
// time and index of origin.
//
// With pos[] one launch:
//
//   rxu_scatter each block takes kRxuBlockEntries consecutive entries; a wave
//               walks 64 of them per turn: sel[], len[], the time and pos[]
//               one entry per lane, validated, len / now / src stored
//               coalesced, then the slots in 16-byte units. Block 0 writes
//               the count.
//
// Without pos[] the positions are the running sum of the padded lengths, and
// two launches come first on the same stream:
//
//   rxu_sizes   every wave of every block sums the padded lengths of the
//               kRxuPerWave entries it will scatter into a workspace word;
//   txp_scan    vp_tx_pack's one-block exclusive scan of those words, in
//               place, with a 64-bit carry;
//
// and rxu_scatter starts each wave at its word and scans each turn's lengths
// with shuffles, the running position in a scalar. The sums are per wave, not
// per block, so the scatter needs neither a second pass over len[] nor LDS.
//
// No block waits for another: the order between the passes is the stream's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"

namespace vp {

VP_PRELOAD_UNIT(rxunpack)

constexpr uint32_t kRxuBlockEntries = 2048;
constexpr uint32_t kRxuThreads = 256, kRxuWaves = kRxuThreads / 64;
constexpr uint32_t kRxuPerWave = kRxuBlockEntries / kRxuWaves;
constexpr uint32_t kRxuTurns = kRxuPerWave / 64;  // 64 entries, one per lane, per turn
static_assert(kRxuBlockEntries % (64 * kRxuWaves) == 0, "whole waves");
// a frame's padded length is at most 65536 (len is 16 bits)
static_assert((uint64_t)kRxuPerWave * 65536u < (1ull << 32), "a wave's sum in 32 bits");

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

__device__ __forceinline__ uint32_t rxu_pad(uint32_t l) { return (l + 15u) & ~15u; }

// Entry k's index into len[] / now[] and its length; the length is 0 where the
// index is outside them, and nothing is read through such an index
__device__ __forceinline__ void rxu_meta(const RxuArgs &a, uint64_t k, bool mine, uint32_t &mm,
                                         bool &in, uint32_t &l) {
  mm = (uint32_t)k;
  if (mine && a.sel) mm = a.sel[k];
  in = mine && mm < a.meta_n;
  l = in ? a.len[mm] : 0u;
}

__global__ __launch_bounds__(kRxuThreads) void rxu_sizes(const RxuArgs a, uint64_t *sums) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t w0 = (uint64_t)blockIdx.x * kRxuBlockEntries + wv * kRxuPerWave;
  uint32_t sum = 0;
  for (uint32_t it = 0; it < kRxuTurns; it++) {
    const uint64_t k = w0 + it * 64 + lane;
    if (w0 + it * 64 >= a.m) break;
    uint32_t mm, l;
    bool in;
    rxu_meta(a, k, k < a.m, mm, in, l);
    sum += rxu_pad(l);
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
  if (lane == 0) sums[(size_t)blockIdx.x * kRxuWaves + wv] = sum;  // (0 past the end)
}

// The bytes of a 16-byte unit at or beyond `keep` (>= 1) cleared
__device__ __forceinline__ uint4 rxu_clear(uint4 v, uint32_t keep) {
  if (keep < 16) {
    const uint32_t w = keep >> 2, m = (1u << (8 * (keep & 3))) - 1u;
    v.x = w > 0 ? v.x : v.x & m;
    v.y = w > 1 ? v.y : w == 1 ? v.y & m : 0u;
    v.z = w > 2 ? v.z : w == 2 ? v.z & m : 0u;
    v.w = w == 3 ? v.w & m : 0u;
  }
  return v;
}

// Unit u (a byte offset) of a slot whose frame lies at p with r bytes to keep;
// r is 0 for an entry that is not readable, and then nothing is read
__device__ __forceinline__ uint4 rxu_unit(const uint8_t *data, uint64_t p, uint32_t r, uint32_t u) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (u < r) v = rxu_clear(*(const uint4 *)(data + p + u), r - u);
  return v;
}

// The sub-wave path, for a slot of U 16-byte units where U divides 64: lanes
// U f .. U f + U - 1 move entry (64 / U) g + f of this turn, one unit each, so
// one instruction stores 1 KiB of consecutive output bytes. `p` and `r` are
// the lane's own entry's; entries at or beyond `left` do not exist.
struct RxuUnit {
  uint4 v;
  bool on;
};

__device__ __forceinline__ RxuUnit rxu_sub_load(const RxuArgs &a, uint32_t lg, uint32_t g,
                                                uint32_t lane, uint64_t p, uint32_t r,
                                                uint32_t left) {
  // U = 1 << lg
  const uint32_t e = ((64u >> lg) * g) + (lane >> lg), u = 16 * (lane & ((1u << lg) - 1));
  const uint64_t gp = __shfl((unsigned long long)p, (int)e);
  const uint32_t gr = __shfl(r, (int)e);
  RxuUnit x;
  x.on = e < left;
  x.v = rxu_unit(a.data, gp, x.on ? gr : 0u, u);
  return x;
}

template <uint32_t U>
__device__ __forceinline__ void rxu_sub(const RxuArgs &a, uint64_t k0, uint32_t lane, uint64_t p,
                                        uint32_t r, uint32_t left) {
  uint8_t *to = a.oframes + k0 * a.oslot + 16 * lane;  // (k0 is 64 bits)
  if constexpr (U == 4) {  // 64-byte slots: the four loads of a turn in flight together
    RxuUnit x[4];
#pragma unroll
    for (uint32_t g = 0; g < 4; g++) x[g] = rxu_sub_load(a, 2, g, lane, p, r, left);
#pragma unroll
    for (uint32_t g = 0; g < 4; g++)
      if (x[g].on) *(uint4 *)(to + 1024 * g) = x[g].v;
  } else {
    const uint32_t units = a.oslot / 16;  // 8, 16, 32 or 64
    const uint32_t lg = 31 - __clz((int)units);
    for (uint32_t g = 0; g < units && (64u >> lg) * g < left; g++) {
      const RxuUnit x = rxu_sub_load(a, lg, g, lane, p, r, left);
      if (x.on) *(uint4 *)(to + (size_t)1024 * g) = x.v;
    }
  }
}

// The wave path, for every other slot: the whole wave moves one entry after
// another, 1 KiB an instruction
__device__ __forceinline__ void rxu_wave(const RxuArgs &a, uint64_t k0, uint32_t lane, uint64_t p,
                                         uint32_t r, uint32_t left) {
  for (uint32_t e = 0; e < left; e++) {
    const uint32_t plo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, (int)e);
    const uint32_t phi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(p >> 32), (int)e);
    const uint32_t gr = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)e);
    const uint64_t gp = ((uint64_t)phi << 32) | plo;
    uint8_t *to = a.oframes + (k0 + e) * a.oslot;
    for (uint32_t u = 16 * lane; u < a.oslot; u += 16 * 64)
      *(uint4 *)(to + u) = rxu_unit(a.data, gp, gr, u);
  }
}

__global__ __launch_bounds__(kRxuThreads) void rxu_scatter(const RxuArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (blockIdx.x == 0 && tid == 0) *a.count = a.n;
  const uint64_t w0 = (uint64_t)blockIdx.x * kRxuBlockEntries + wv * kRxuPerWave;
  if (w0 >= a.m) return;
  const uint32_t units = a.oslot / 16;
  const bool sub = units <= 64 && 64 % units == 0;
  uint64_t run = 0;  // pos == NULL: this turn's first position
  if (!a.pos) run = a.base[(size_t)blockIdx.x * kRxuWaves + wv];
  for (uint32_t it = 0; it < kRxuTurns; it++) {
    const uint64_t k0 = w0 + it * 64;  // (may pass 2^32)
    if (k0 >= a.m) break;
    const uint32_t left = a.m - k0 < 64 ? (uint32_t)(a.m - k0) : 64;
    const bool mine = lane < left;
    const uint64_t k = k0 + lane;
    uint32_t mm, l;
    bool in;
    rxu_meta(a, k, mine, mm, in, l);
    uint64_t p = 0;
    if (a.pos) {
      if (mine) p = a.pos[k];
    } else {
      const uint32_t ext = rxu_pad(l);
      uint32_t x = ext;  // inclusive scan over the wave
#pragma unroll
      for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(x, o);
        if (lane >= o) x += u;
      }
      p = run + (x - ext);
      run += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    // readable: inside len[], aligned, and its kept bytes' units inside the
    // stream; compared without a sum that could wrap
    uint32_t r = l < a.oslot ? l : a.oslot;
    const bool ok = in && (p & 15) == 0 && p <= a.bytes && rxu_pad(r) <= a.bytes - p;
    uint64_t at = 0;
    if (ok)
      at = a.now ? (uint64_t)a.now[mm] : (uint64_t)a.now0 + (uint64_t)mm * (uint64_t)a.now_step;
    else
      l = r = 0;
    if (mine) {
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
      if (a.osrc) a.osrc[k] = mm;
    }
    if (units == 4)
      rxu_sub<4>(a, k0, lane, p, r, left);
    else if (sub)
      rxu_sub<0>(a, k0, lane, p, r, left);
    else
      rxu_wave(a, k0, lane, p, r, left);
  }
}

// The waves' sums, for the largest call so far. One workspace per context: a
// call on another stream than the last one's waits for that one's launches
// first (as txp_reserve does for vp_tx_pack's sums).
static int rxu_reserve(vp_ctx *c, size_t m, hipStream_t s) {
  Workspace &w = c->ws;
  if (!w.rxu_ev) VP_HIP(hipEventCreateWithFlags(&w.rxu_ev, hipEventDisableTiming));
  if (m > w.rxu_sum_n) {
    if (w.rxu_used) VP_HIP(hipEventSynchronize(w.rxu_ev));
    hipFree(w.rxu_sum);
    w.rxu_sum = nullptr;
    w.rxu_sum_n = 0;
    VP_HIP(hipMalloc((void **)&w.rxu_sum, 8 * m));
    w.rxu_sum_n = m;
  } else if (w.rxu_used && w.rxu_last != s) {
    VP_HIP(hipStreamWaitEvent(s, w.rxu_ev, 0));
  }
  return 0;
}

}  // namespace vp

using namespace vp;

extern "C" int vp_rx_unpack(vp_ctx *c, const vp_rx_stream *in, const vp_tx_next *o, void *stream) {
  if (!c || !in || !o || !o->count) return VP_EINVAL;
  if (!in->data && in->bytes) return VP_EINVAL;
  if (((uintptr_t)in->data | (uintptr_t)o->frames) & 15) return VP_EINVAL;
  if (!in->len && in->meta_n) return VP_EINVAL;
  if (o->slot < 64 || o->slot % 16) return VP_EINVAL;
  if ((!o->frames || !o->len) && o->cap) return VP_EINVAL;
  if (in->bytes && o->cap) {  // the stream and the slot array may not overlap
    const uintptr_t s0 = (uintptr_t)in->data, s1 = s0 + in->bytes;
    const uintptr_t d0 = (uintptr_t)o->frames, d1 = d0 + (uint64_t)o->cap * o->slot;
    if (s0 < d1 && d0 < s1) return VP_EINVAL;
  }
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  RxuArgs a;
  a.data = in->data;
  a.bytes = in->bytes;
  a.pos = in->pos;
  a.sel = in->sel;
  a.len = in->len;
  a.now = in->now;
  a.now0 = in->now0;
  a.now_step = in->now_step;
  a.meta_n = in->meta_n;
  a.n = in->n;
  a.m = in->n < o->cap ? in->n : o->cap;
  a.base = nullptr;
  a.oframes = o->frames;
  a.oslot = o->slot;
  a.olen = o->len;
  a.onow = o->now;
  a.osrc = o->src;
  a.count = o->count;
  // at least one block, so that count is written when nothing else is
  const uint32_t blocks = a.m ? (a.m - 1) / kRxuBlockEntries + 1 : 1;
  const bool sums = !in->pos && a.m;
  if (sums) {
    Workspace &w = c->ws;
    const uint32_t words = blocks * kRxuWaves;
    VP_TRY(rxu_reserve(c, words, s));
    rxu_sizes<<<blocks, kRxuThreads, 0, s>>>(a, w.rxu_sum);
    VP_HIP(hipGetLastError());
    txp_scan<<<1, kTxpScanThreads, 0, s>>>(w.rxu_sum, words);
    VP_HIP(hipGetLastError());
    a.base = w.rxu_sum;
  }
  rxu_scatter<<<blocks, kRxuThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  if (sums) {
    Workspace &w = c->ws;
    VP_HIP(hipEventRecord(w.rxu_ev, s));
    w.rxu_used = true;
    w.rxu_last = s;
  }
  return 0;
}
