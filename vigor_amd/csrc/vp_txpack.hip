// Transmit streams for a device-resident batch (vp_tx_pack,
// include/vigpath.h): the frames that vp_tx_build's lists name, gathered into
// one contiguous run of bytes per port, each at its own length rounded up to
// 16 bytes. Three launches on one stream:
//
//   txp_sizes  each block takes kTxpBlockEntries consecutive list entries,
//              reads idx[e] and len[idx[e]] and writes the sum of the padded
//              lengths into a workspace word;
//   txp_scan   one block: the exclusive scan of those sums in place, tiled
//              with a 64-bit carry;
//   txp_copy   each block computes its entries' padded lengths again, scans
//              them (shuffles inside a wave, LDS across the waves), adds the
//              block's base, writes pos[] and the port_off[] words whose
//              boundary entry it owns, and copies the frames in 16-byte units.
//
// No block waits for another: the order between the passes is the stream's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "vp_internal.h"

namespace vp {

VP_PRELOAD_UNIT(txpack)

constexpr uint32_t kTxpBlockEntries = 2048;
constexpr uint32_t kTxpThreads = 256, kTxpWaves = kTxpThreads / 64;
constexpr uint32_t kTxpPerWave = kTxpBlockEntries / kTxpWaves;
constexpr uint32_t kTxpTurns = kTxpPerWave / 64;  // 64 entries, one per lane, per turn
// a frame's copy is at most 65535 bytes (len is 16 bits) rounded up to 16
static_assert((uint64_t)kTxpBlockEntries * 65536u < (1ull << 32), "a block's sum in 32 bits");
static_assert(kTxpBlockEntries % (64 * kTxpWaves) == 0, "whole waves");
// txp_scan: one block (kTxpScanThreads, vp_internal.h), kTxpScanItems
// consecutive sums per thread and tile
constexpr uint32_t kTxpScanItems = 8;
constexpr uint32_t kTxpScanTile = kTxpScanThreads * kTxpScanItems;
constexpr uint32_t kTxpLean = 64;  // the widest padded frame of the four-lane path

__device__ __forceinline__ uint32_t txp_pad(uint32_t clen) { return (clen + 15u) & ~15u; }

// E = min(offset[n_devices], cap): the entries idx[] really holds
__device__ __forceinline__ uint32_t txp_entries(const uint32_t *offset, uint32_t nd,
                                                uint32_t cap) {
  const uint32_t t = offset[nd];
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(t < cap ? t : cap));
}

// Entry first + local's packet index and copied length; (0, 0) past the
// lists' end and for an index outside the batch, through which nothing is read
__device__ __forceinline__ void txp_entry(const uint32_t *__restrict__ idx,
                                          const uint16_t *__restrict__ len, uint32_t first,
                                          uint32_t local, uint32_t rem, uint32_t n, uint32_t slot,
                                          uint32_t &i, uint32_t &clen) {
  i = 0;
  clen = 0;
  if (local < rem) {
    i = idx[(size_t)first + local];
    if (i < n) {
      const uint32_t l = len[i];
      clen = l < slot ? l : slot;
    } else {
      i = 0;
    }
  }
}

__device__ __forceinline__ uint32_t txp_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kTxpThreads) void txp_sizes(
    const uint32_t *__restrict__ idx, const uint32_t *__restrict__ offset, uint32_t cap,
    uint32_t nd, const uint16_t *__restrict__ len, uint32_t n, uint32_t slot,
    uint64_t *__restrict__ sums) {
  __shared__ uint32_t wtot[kTxpWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t total = txp_entries(offset, nd, cap);
  const uint32_t first = blockIdx.x * kTxpBlockEntries;
  if (first >= total) {  // (also the block that owns entry E itself)
    if (tid == 0) sums[blockIdx.x] = 0;
    return;
  }
  const uint32_t rem = total - first;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t it = 0; it < kTxpTurns; it++) {
    uint32_t i, clen;
    txp_entry(idx, len, first, wv * kTxpPerWave + it * 64 + lane, rem, n, slot, i, clen);
    sum += txp_pad(clen);
  }
  sum = txp_wave_sum(sum);
  if (lane == 0) wtot[wv] = sum;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxpWaves; k++) t += wtot[k];
    sums[blockIdx.x] = t;
  }
}

// One block scans the m block sums in place, tile after tile with a running
// 64-bit carry: m is 8193 for 2^24 entries, two tiles.
__global__ __launch_bounds__(kTxpScanThreads) void txp_scan(uint64_t *sums, uint32_t m) {
  __shared__ uint64_t wsum[kTxpScanThreads / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint64_t carry = 0;
  for (uint32_t tile = 0; tile < m; tile += kTxpScanTile) {
    const uint32_t j0 = tile + tid * kTxpScanItems;
    uint64_t v[kTxpScanItems], t = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxpScanItems; k++) {
      v[k] = j0 + k < m ? sums[j0 + k] : 0ull;
      t += v[k];
    }
    uint64_t x = t;  // inclusive scan of the threads' sums over the wave
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint64_t u = __shfl_up((unsigned long long)x, o);
      if (lane >= o) x += u;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint64_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxpScanThreads / 64; k++) {
      const uint64_t s = wsum[k];
      if (k < wv) before += s;
      total += s;
    }
    uint64_t run = carry + before + x - t;
#pragma unroll
    for (uint32_t k = 0; k < kTxpScanItems; k++) {
      if (j0 + k < m) sums[j0 + k] = run;
      run += v[k];
    }
    carry += total;
    __syncthreads();  // (wsum is written again by the next tile)
  }
}

// The bytes of a 16-byte unit at or beyond `keep` (>= 1) cleared
__device__ __forceinline__ uint4 txp_clear(uint4 v, uint32_t keep) {
  if (keep < 16) {
    const uint32_t w = keep >> 2, m = (1u << (8 * (keep & 3))) - 1u;
    v.x = w > 0 ? v.x : v.x & m;
    v.y = w > 1 ? v.y : w == 1 ? v.y & m : 0u;
    v.z = w > 2 ? v.z : w == 2 ? v.z & m : 0u;
    v.w = w == 3 ? v.w & m : 0u;
  }
  return v;
}

// The four-lane path: lanes 4k .. 4k + 3 move entry 16 g + k of this turn,
// one 16-byte unit each, so the wave moves 16 frames of at most 64 bytes.
struct TxpLean {
  uint4 v;
  uint64_t at;
  bool on;
};

__device__ __forceinline__ TxpLean txp_lean_load(const uint8_t *__restrict__ frames,
                                                 uint32_t slot, uint32_t g, uint32_t lane,
                                                 uint32_t i, uint32_t clen, uint32_t excl,
                                                 uint64_t base, uint64_t cap_bytes) {
  const int src = (int)(16 * g + (lane >> 2));
  const uint32_t u = 16 * (lane & 3);
  const uint32_t gi = __shfl(i, src), gc = __shfl(clen, src), ge = __shfl(excl, src);
  const uint32_t gp = txp_pad(gc);
  TxpLean r;
  r.at = base + ge;
  r.on = u < gp && r.at + gp <= cap_bytes;  // written whole or not at all
  r.at += u;
  r.v = make_uint4(0, 0, 0, 0);
  if (r.on)
    r.v = txp_clear(*(const uint4 *)(frames + (size_t)gi * slot + u), gc - u);
  return r;
}

__device__ __forceinline__ void txp_lean_store(uint8_t *__restrict__ data, const TxpLean &r) {
  if (r.on) *(uint4 *)(data + r.at) = r.v;
}

// The wide path: the whole wave moves one entry after another, 1 KiB a turn
__device__ __forceinline__ void txp_wide(const uint8_t *__restrict__ frames, uint32_t slot,
                                         uint8_t *__restrict__ data, uint32_t g, uint32_t lane,
                                         uint32_t i, uint32_t clen, uint32_t excl, uint64_t base,
                                         uint64_t cap_bytes) {
  for (uint32_t k = 0; k < 16; k++) {
    const int src = (int)(16 * g + k);
    const uint32_t gi = (uint32_t)__builtin_amdgcn_readlane((int)i, src);
    const uint32_t gc = (uint32_t)__builtin_amdgcn_readlane((int)clen, src);
    const uint32_t ge = (uint32_t)__builtin_amdgcn_readlane((int)excl, src);
    const uint32_t gp = txp_pad(gc);
    const uint64_t at = base + ge;
    if (gp == 0 || at + gp > cap_bytes) continue;
    const uint8_t *from = frames + (size_t)gi * slot;
    for (uint32_t u = 16 * lane; u < gp; u += 16 * 64)
      *(uint4 *)(data + at + u) = txp_clear(*(const uint4 *)(from + u), gc - u);
  }
}

__global__ __launch_bounds__(kTxpThreads) void txp_copy(
    const uint8_t *__restrict__ frames, uint32_t slot, const uint16_t *__restrict__ len,
    uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ offset,
    uint32_t cap, uint32_t nd, const uint64_t *__restrict__ sums, uint8_t *__restrict__ data,
    uint64_t cap_bytes, uint64_t *__restrict__ port_off, uint64_t *__restrict__ pos) {
  __shared__ uint32_t idx_s[kTxpBlockEntries];   // the entries' packets and copied
  __shared__ uint16_t clen_s[kTxpBlockEntries];  // lengths, kept for the second pass
  __shared__ uint32_t wtot[kTxpWaves];
  // the ports whose boundary entry min(offset[d], E) is in this block: its
  // place in the block, and per wave and turn the lanes that hold one
  __shared__ uint32_t bnd_s[VP_MAX_DEVICES + 1];
  __shared__ unsigned long long bflag_s[kTxpWaves * kTxpTurns];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t total = txp_entries(offset, nd, cap);
  const uint32_t first = blockIdx.x * kTxpBlockEntries;
  if (first > total) return;  // (first == total: the block that owns entry E)
  const uint32_t rem = total - first;
  if (tid < kTxpWaves * kTxpTurns) bflag_s[tid] = 0;
  __syncthreads();
  if (tid <= nd) {
    const uint32_t o = offset[tid], e = o < total ? o : total;
    const uint32_t bd = e >= first && e - first < kTxpBlockEntries ? e - first : ~0u;
    bnd_s[tid] = bd;
    if (bd != ~0u) atomicOr(&bflag_s[bd >> 6], 1ull << (bd & 63));
  }
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t it = 0; it < kTxpTurns; it++) {
    const uint32_t local = wv * kTxpPerWave + it * 64 + lane;
    uint32_t i, clen;
    txp_entry(idx, len, first, local, rem, n, slot, i, clen);
    idx_s[local] = i;
    clen_s[local] = (uint16_t)clen;
    sum += txp_pad(clen);
  }
  sum = txp_wave_sum(sum);
  if (lane == 0) wtot[wv] = sum;
  __syncthreads();
  const uint64_t base = sums[blockIdx.x];
  uint32_t run = 0;  // this turn's first byte, from the block's base
  for (uint32_t k = 0; k < wv; k++) run += wtot[k];
  for (uint32_t it = 0; it < kTxpTurns; it++) {
    const uint32_t local = wv * kTxpPerWave + it * 64 + lane;
    const uint32_t i = idx_s[local], clen = clen_s[local], pad = txp_pad(clen);
    uint32_t x = pad;  // inclusive scan over the wave
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(x, o);
      if (lane >= o) x += u;
    }
    const uint32_t excl = run + x - pad;
    run += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    if (pos && local < rem) pos[(size_t)first + local] = base + excl;
    const unsigned long long flag = bflag_s[wv * kTxpTurns + it];
    if ((flag >> lane) & 1ull) {
      for (uint32_t d = 0; d <= nd; d++)
        if (bnd_s[d] == local) port_off[d] = base + excl;
    }
    const unsigned long long wide = __ballot(pad > kTxpLean);
    if (wide == 0) {
      if (__ballot(pad != 0) == 0) continue;
      TxpLean r[4];
#pragma unroll
      for (uint32_t g = 0; g < 4; g++)
        r[g] = txp_lean_load(frames, slot, g, lane, i, clen, excl, base, cap_bytes);
#pragma unroll
      for (uint32_t g = 0; g < 4; g++) txp_lean_store(data, r[g]);
    } else {
      for (uint32_t g = 0; g < 4; g++) {
        if (((wide >> (16 * g)) & 0xFFFFull) == 0)
          txp_lean_store(data,
                         txp_lean_load(frames, slot, g, lane, i, clen, excl, base, cap_bytes));
        else
          txp_wide(frames, slot, data, g, lane, i, clen, excl, base, cap_bytes);
      }
    }
  }
}

static uint32_t txp_devices(const vp_ctx *c) {
  switch (c->kind) {
    case KIND_NAT: return c->nat.n_devices;
    case KIND_BRIDGE: return c->brg.n_devices;
    case KIND_LB: return c->lb.n_devices;
    case KIND_FW: return c->fw.n_devices;
    case KIND_POL: return c->pol.n_devices;
    default: return 0;
  }
}

// The block sums, for the largest call so far. One workspace per context: a
// call on another stream than the last one's waits for that one's launches
// first (as tx_reserve does for vp_tx_build's counts).
static int txp_reserve(vp_ctx *c, size_t m, hipStream_t s) {
  Workspace &w = c->ws;
  if (!w.txp_ev) VP_HIP(hipEventCreateWithFlags(&w.txp_ev, hipEventDisableTiming));
  if (m > w.txp_sum_n) {
    if (w.txp_used) VP_HIP(hipEventSynchronize(w.txp_ev));
    hipFree(w.txp_sum);
    w.txp_sum = nullptr;
    w.txp_sum_n = 0;
    VP_HIP(hipMalloc((void **)&w.txp_sum, 8 * m));
    w.txp_sum_n = m;
  } else if (w.txp_used && w.txp_last != s) {
    VP_HIP(hipStreamWaitEvent(s, w.txp_ev, 0));
  }
  return 0;
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_pack(vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l,
                          const vp_tx_frames *o, void *stream) {
  if (!c || !b || !l || !o || !o->port_off || !l->offset) return VP_EINVAL;
  if (!l->idx && l->cap) return VP_EINVAL;
  if ((!b->frames || !b->len) && b->n && l->cap) return VP_EINVAL;
  if (b->slot < 64 || b->slot % 16) return VP_EINVAL;
  if (((uintptr_t)b->frames | (uintptr_t)o->data) & 15) return VP_EINVAL;
  if (!o->data && o->cap_bytes) return VP_EINVAL;
  const uint32_t nd = txp_devices(c);
  if (nd > VP_MAX_DEVICES) return VP_EINVAL;
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the block after the last full one owns entry E when E == cap is a
  // multiple of the block's entries
  const uint32_t blocks = l->cap / kTxpBlockEntries + 1;
  Workspace &w = c->ws;
  VP_TRY(txp_reserve(c, blocks, s));
  txp_sizes<<<blocks, kTxpThreads, 0, s>>>(l->idx, l->offset, l->cap, nd, b->len, b->n, b->slot,
                                           w.txp_sum);
  VP_HIP(hipGetLastError());
  txp_scan<<<1, kTxpScanThreads, 0, s>>>(w.txp_sum, blocks);
  VP_HIP(hipGetLastError());
  txp_copy<<<blocks, kTxpThreads, 0, s>>>(b->frames, b->slot, b->len, b->n, l->idx, l->offset,
                                          l->cap, nd, w.txp_sum, o->data, o->cap_bytes,
                                          o->port_off, o->pos);
  VP_HIP(hipGetLastError());
  VP_HIP(hipEventRecord(w.txp_ev, s));
  w.txp_used = true;
  w.txp_last = s;
  return 0;
}
