// Transmit streams for a device-resident batch (vp_tx_pack,
// include/vigpath.h): the frames that vp_tx_build's lists name, gathered into
// one contiguous run of bytes per port, each at its own length rounded up to
// 16 bytes. Three launches on one stream:
//
//   txp_sizes  each block takes kSlotBlockEntries consecutive list entries,
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
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(txpack)

// a frame's copy is at most 65535 bytes (len is 16 bits) rounded up to 16
static_assert((uint64_t)kSlotBlockEntries * 65536u < (1ull << 32), "a block's sum in 32 bits");
// txp_scan: one block (kTxpScanThreads, vp_internal.h), kTxpScanItems
// consecutive sums per thread and tile
constexpr uint32_t kTxpScanItems = 8;
constexpr uint32_t kTxpScanTile = kTxpScanThreads * kTxpScanItems;
constexpr uint32_t kTxpLean = 64;  // the widest padded frame of the four-lane path

// E, the entries idx[] really holds, in a scalar
__device__ __forceinline__ uint32_t txp_entries(const uint32_t *offset, uint32_t nd,
                                                uint32_t cap) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)list_entries(offset, nd, cap));
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

__global__ __launch_bounds__(kSlotThreads) void txp_sizes(
    const uint32_t *__restrict__ idx, const uint32_t *__restrict__ offset, uint32_t cap,
    uint32_t nd, const uint16_t *__restrict__ len, uint32_t n, uint32_t slot,
    uint64_t *__restrict__ sums) {
  __shared__ uint32_t wtot[kSlotWaves];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t total = txp_entries(offset, nd, cap);
  const uint32_t first = blockIdx.x * kSlotBlockEntries;
  if (first >= total) {  // (also the block that owns entry E itself)
    if (tid == 0) sums[blockIdx.x] = 0;
    return;
  }
  const uint32_t rem = total - first;
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    uint32_t i, clen;
    txp_entry(idx, len, first, wv * kSlotPerWave + it * 64 + lane, rem, n, slot, i, clen);
    sum += pad16(clen);
  }
  sum = wave_sum(sum);
  if (lane == 0) wtot[wv] = sum;
  __syncthreads();
  if (tid == 0) {
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSlotWaves; k++) t += wtot[k];
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
    const uint64_t x = wave_scan(t, lane);  // of the threads' sums
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
  const uint32_t gp = pad16(gc);
  TxpLean r;
  r.at = base + ge;
  r.on = u < gp && r.at + gp <= cap_bytes;  // written whole or not at all
  r.at += u;
  r.v = make_uint4(0, 0, 0, 0);
  if (r.on)
    r.v = unit_clear(*(const uint4 *)(frames + (size_t)gi * slot + u), gc - u);
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
    const uint32_t gp = pad16(gc);
    const uint64_t at = base + ge;
    if (gp == 0 || at + gp > cap_bytes) continue;
    const uint8_t *from = frames + (size_t)gi * slot;
    for (uint32_t u = 16 * lane; u < gp; u += 16 * 64)
      *(uint4 *)(data + at + u) = unit_clear(*(const uint4 *)(from + u), gc - u);
  }
}

__global__ __launch_bounds__(kSlotThreads) void txp_copy(
    const uint8_t *__restrict__ frames, uint32_t slot, const uint16_t *__restrict__ len,
    uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ offset,
    uint32_t cap, uint32_t nd, const uint64_t *__restrict__ sums, uint8_t *__restrict__ data,
    uint64_t cap_bytes, uint64_t *__restrict__ port_off, uint64_t *__restrict__ pos) {
  __shared__ uint32_t idx_s[kSlotBlockEntries];   // the entries' packets and copied
  __shared__ uint16_t clen_s[kSlotBlockEntries];  // lengths, kept for the second pass
  __shared__ uint32_t wtot[kSlotWaves];
  // the ports whose boundary entry min(offset[d], E) is in this block: its
  // place in the block, and per wave and turn the lanes that hold one
  __shared__ uint32_t bnd_s[VP_MAX_DEVICES + 1];
  __shared__ unsigned long long bflag_s[kSlotWaves * kSlotTurns];
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t total = txp_entries(offset, nd, cap);
  const uint32_t first = blockIdx.x * kSlotBlockEntries;
  if (first > total) return;  // (first == total: the block that owns entry E)
  const uint32_t rem = total - first;
  if (tid < kSlotWaves * kSlotTurns) bflag_s[tid] = 0;
  __syncthreads();
  if (tid <= nd) {
    const uint32_t o = offset[tid], e = o < total ? o : total;
    const uint32_t bd = e >= first && e - first < kSlotBlockEntries ? e - first : ~0u;
    bnd_s[tid] = bd;
    if (bd != ~0u) atomicOr(&bflag_s[bd >> 6], 1ull << (bd & 63));
  }
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint32_t local = wv * kSlotPerWave + it * 64 + lane;
    uint32_t i, clen;
    txp_entry(idx, len, first, local, rem, n, slot, i, clen);
    idx_s[local] = i;
    clen_s[local] = (uint16_t)clen;
    sum += pad16(clen);
  }
  sum = wave_sum(sum);
  if (lane == 0) wtot[wv] = sum;
  __syncthreads();
  const uint64_t base = sums[blockIdx.x];
  uint32_t run = 0;  // this turn's first byte, from the block's base
  for (uint32_t k = 0; k < wv; k++) run += wtot[k];
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint32_t local = wv * kSlotPerWave + it * 64 + lane;
    const uint32_t i = idx_s[local], clen = clen_s[local], pad = pad16(clen);
    const uint32_t x = wave_scan(pad, lane);
    const uint32_t excl = run + x - pad;
    run += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    if (pos && local < rem) pos[(size_t)first + local] = base + excl;
    const unsigned long long flag = bflag_s[wv * kSlotTurns + it];
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

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_pack(vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l,
                          const vp_tx_frames *o, void *stream) {
  if (!c || !b || !l || !o || !o->port_off || !l->offset) return VP_EINVAL;
  if (!l->idx && l->cap) return VP_EINVAL;
  if ((!b->frames || !b->len) && b->n && l->cap) return VP_EINVAL;
  if (!slots_ok(b->frames, b->slot) || ((uintptr_t)o->data & 15)) return VP_EINVAL;
  if (!o->data && o->cap_bytes) return VP_EINVAL;
  const uint32_t nd = ctx_devices(c);
  if (nd > VP_MAX_DEVICES) return VP_EINVAL;
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the block after the last full one owns entry E when E == cap is a
  // multiple of the block's entries
  const uint32_t blocks = l->cap / kSlotBlockEntries + 1;
  CallBuf &w = c->ws.txp_sum;  // the blocks' sums
  VP_TRY(callbuf_reserve(w, 8 * (size_t)blocks, s));
  uint64_t *sums = (uint64_t *)w.p;
  txp_sizes<<<blocks, kSlotThreads, 0, s>>>(l->idx, l->offset, l->cap, nd, b->len, b->n, b->slot,
                                            sums);
  VP_HIP(hipGetLastError());
  txp_scan<<<1, kTxpScanThreads, 0, s>>>(sums, blocks);
  VP_HIP(hipGetLastError());
  txp_copy<<<blocks, kSlotThreads, 0, s>>>(b->frames, b->slot, b->len, b->n, l->idx, l->offset,
                                           l->cap, nd, sums, o->data, o->cap_bytes, o->port_off,
                                           o->pos);
  VP_HIP(hipGetLastError());
  return callbuf_done(w, s);
}
