// Transmit dispatch for a device-resident batch (vp_tx_build,
// include/vigpath.h): what nf.c does with nf_process's return value
// (nf.c:159-174: drop, flood(), rte_eth_tx_burst) as a stable multi-way
// partition of the packet indices by output port. Three launches on one
// stream:
//
//   tx_count    each block classifies a chunk of kTxBlockPackets packets and
//               writes its entries per port into a workspace row (port-major:
//               cnt[d * blocks + block]); the byte sums and the drop / flood /
//               bad-port counts are reduced in the block, then one atomic per
//               port and block;
//   tx_scan     one block: the exclusive scan of those blocks x n_devices
//               counts in place (port-major order is list order), offset[]
//               and stats->packets[] from it;
//   tx_scatter  each block classifies its chunk again and writes every entry
//               at its stable rank: the block's base, the waves before it (LDS),
//               and inside a wave a ballot of the lanes that feed the port and
//               a popcount of the lanes below.
//
// No block waits for another: the order between the passes is the stream's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(tx)

constexpr uint32_t kTxBlockPackets = kSlotBlockEntries;  // vigor_amd.TX_BLOCK_PACKETS
constexpr uint32_t kTxThreads = kSlotThreads, kTxWaves = kSlotWaves, kTxPerWave = kSlotPerWave;
constexpr uint32_t kTxPerThread = kTxBlockPackets / kTxThreads;
// tx_count packs a thread's entries for one port as count << 20 | bytes
static_assert(kTxPerThread * 65535u < (1u << 20) && kTxPerThread < (1u << 12), "packed sums");
static_assert((uint64_t)kTxBlockPackets * 65535u < (1ull << 32), "a block's byte sum in 32 bits");
// tx_scan: one block, kTxScanItems consecutive counts per thread and tile
constexpr uint32_t kTxScanThreads = 1024, kTxScanItems = 8;
constexpr uint32_t kTxScanTile = kTxScanThreads * kTxScanItems;

// A packet's class as kind << 16 | value: a unicast entry's port (< n_devices),
// a flood's input port (the one port it skips; any value >= n_devices skips
// none), or nothing (dropped, bad port, past the batch's end).
constexpr uint32_t kTxNone = 0, kTxUni = 1, kTxFlood = 2;

__device__ __forceinline__ uint32_t tx_class(uint32_t out, uint32_t in, uint32_t nd) {
  if (out == in) return kTxNone << 16;
  if (out == VP_FLOOD_FRAME) return kTxFlood << 16 | in;
  if (out < nd) return kTxUni << 16 | out;
  return kTxNone << 16;
}

__global__ __launch_bounds__(kTxThreads) void tx_count(
    const uint16_t *__restrict__ out, const uint16_t *__restrict__ in_dev, uint32_t in_port,
    const uint16_t *__restrict__ len, uint32_t n, uint32_t nd, uint32_t blocks,
    uint32_t *__restrict__ cnt, vp_tx_stats *stats) {
  // [nd][kTxThreads]: a thread adds only to its own column, count << 20 |
  // bytes per port. The adds are LDS atomics whose result is not used: no
  // lane ever shares an address, but a plain read-add-write of one port's
  // cell would chain the iterations through LDS round trips
  extern __shared__ uint32_t acc[];
  __shared__ uint32_t misc[3];  // dropped, flooded, bad_port
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (uint32_t d = 0; d < nd; d++) acc[d * kTxThreads + tid] = 0;
  if (tid < 3) misc[tid] = 0;
  uint32_t dropped = 0, flooded = 0, bad = 0;
  const uint32_t first = blockIdx.x * kTxBlockPackets;
#pragma unroll
  for (uint32_t it = 0; it < kTxPerThread; it++) {
    const uint32_t i = first + it * kTxThreads + tid;
    if (i >= n) continue;
    const uint32_t o = out[i], in = in_dev ? in_dev[i] : in_port;
    const uint32_t add = (1u << 20) | (stats ? (uint32_t)len[i] : 0u);
    if (o == in) {
      dropped++;
    } else if (o == VP_FLOOD_FRAME) {
      flooded++;
      for (uint32_t d = 0; d < nd; d++)
        if (d != in) atomicAdd(&acc[d * kTxThreads + tid], add);
    } else if (o < nd) {
      atomicAdd(&acc[o * kTxThreads + tid], add);
    } else {
      bad++;
    }
  }
  __syncthreads();
  for (uint32_t d = wv; d < nd; d += kTxWaves) {
    uint32_t c = 0, b = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxWaves; k++) {
      const uint32_t v = acc[d * kTxThreads + 64 * k + lane];
      c += v >> 20;
      b += v & 0xFFFFFu;
    }
    c = wave_sum(c);
    b = wave_sum(b);
    if (lane == 0) {
      cnt[(size_t)d * blocks + blockIdx.x] = c;
      if (stats && b) atomicAdd((unsigned long long *)&stats->bytes[d], (unsigned long long)b);
    }
  }
  if (!stats) return;
  dropped = wave_sum(dropped);
  flooded = wave_sum(flooded);
  bad = wave_sum(bad);
  if (lane == 0) {
    if (dropped) atomicAdd(&misc[0], dropped);
    if (flooded) atomicAdd(&misc[1], flooded);
    if (bad) atomicAdd(&misc[2], bad);
  }
  __syncthreads();
  if (tid < 3 && misc[tid]) {
    uint64_t *dst = tid == 0 ? &stats->dropped : tid == 1 ? &stats->flooded : &stats->bad_port;
    atomicAdd((unsigned long long *)dst, (unsigned long long)misc[tid]);
  }
}

// One block scans all m = n_devices x blocks counts (port-major) in place,
// tile after tile with a running carry: m is 2 x 8192 for two ports and 2^24
// packets, two tiles.
__global__ __launch_bounds__(kTxScanThreads) void tx_scan(uint32_t *cnt, uint32_t m,
                                                          uint32_t blocks, uint32_t nd,
                                                          uint32_t *__restrict__ offset,
                                                          vp_tx_stats *stats) {
  __shared__ uint32_t wsum[kTxScanThreads / 64];
  __shared__ uint32_t off_s[VP_MAX_DEVICES + 1];  // each port's first position
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t carry = 0;
  for (uint32_t tile = 0; tile < m; tile += kTxScanTile) {
    const uint32_t j0 = tile + tid * kTxScanItems;
    uint32_t v[kTxScanItems], t = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxScanItems; k++) {
      v[k] = j0 + k < m ? cnt[j0 + k] : 0u;
      t += v[k];
    }
    const uint32_t x = wave_scan(t, lane);  // of the threads' sums
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTxScanThreads / 64; k++) {
      const uint32_t s = wsum[k];
      if (k < wv) before += s;
      total += s;
    }
    uint32_t run = carry + before + x - t;
    uint32_t q = j0 / blocks, r = j0 - q * blocks;  // item j = port q's block r
#pragma unroll
    for (uint32_t k = 0; k < kTxScanItems; k++) {
      if (j0 + k < m) {
        cnt[j0 + k] = run;
        if (r == 0) off_s[q] = run;
      }
      run += v[k];
      if (++r == blocks) {
        r = 0;
        q++;
      }
    }
    carry += total;
    __syncthreads();  // (wsum is written again by the next tile)
  }
  __syncthreads();
  if (tid <= nd) {
    // (m == 0: an empty batch, nothing was scanned and every list is empty)
    const uint32_t lo = tid < nd && m ? off_s[tid] : carry;
    offset[tid] = lo;
    if (stats && tid < nd) {
      const uint32_t hi = tid + 1 < nd && m ? off_s[tid + 1] : carry;
      stats->packets[tid] = hi - lo;
    }
  }
}

// f(d, lanes) for every port d that packets of this wave feed, `lanes` the
// ballot of the lanes that do; all 64 lanes call it together. Without a flood
// in the wave that is one turn per distinct output port (1 or 2 in practice);
// a flood feeds every port.
template <class F>
__device__ __forceinline__ void tx_wave_ports(uint32_t code, uint32_t nd, F &&f) {
  const uint32_t kind = code >> 16, val = code & 0xFFFFu;
  if (__ballot(kind == kTxFlood) == 0) {
    unsigned long long pend = __ballot(kind == kTxUni);
    while (pend) {
      const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)val, __ffsll(pend) - 1);
      const unsigned long long lanes = __ballot(kind == kTxUni && val == d);
      f(d, lanes);
      pend &= ~lanes;
    }
  } else {
    for (uint32_t d = 0; d < nd; d++) {
      const unsigned long long lanes =
          __ballot((kind == kTxUni && val == d) || (kind == kTxFlood && val != d));
      if (lanes) f(d, lanes);
    }
  }
}

__global__ __launch_bounds__(kTxThreads) void tx_scatter(
    const uint16_t *__restrict__ out, const uint16_t *__restrict__ in_dev, uint32_t in_port,
    uint32_t n, uint32_t nd, uint32_t blocks, const uint32_t *__restrict__ base,
    uint32_t *__restrict__ idx, uint32_t cap) {
  __shared__ uint32_t code_s[kTxBlockPackets];  // a lane's own classes, kept for pass 2
  __shared__ uint32_t wtot[kTxWaves][VP_MAX_DEVICES];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // a wave takes kTxPerWave consecutive packets, so list order is block,
  // wave, iteration, lane
  const uint32_t first = blockIdx.x * kTxBlockPackets + wv * kTxPerWave;
  // lane d: port d's entries among this wave's packets, then its next position
  uint32_t run = 0;
  for (uint32_t it = 0; it < kTxPerWave / 64; it++) {
    const uint32_t i = first + it * 64 + lane;
    uint32_t code = kTxNone << 16;
    if (i < n) code = tx_class(out[i], in_dev ? in_dev[i] : in_port, nd);
    code_s[wv * kTxPerWave + it * 64 + lane] = code;
    tx_wave_ports(code, nd, [&](uint32_t d, unsigned long long lanes) {
      if (lane == d) run += (uint32_t)__popcll(lanes);
    });
  }
  if (lane < VP_MAX_DEVICES) wtot[wv][lane] = run;
  __syncthreads();
  run = 0;
  if (lane < nd) {
    run = base[(size_t)lane * blocks + blockIdx.x];
    for (uint32_t k = 0; k < wv; k++) run += wtot[k][lane];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t it = 0; it < kTxPerWave / 64; it++) {
    const uint32_t i = first + it * 64 + lane;
    const uint32_t code = code_s[wv * kTxPerWave + it * 64 + lane];
    tx_wave_ports(code, nd, [&](uint32_t d, unsigned long long lanes) {
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)run, (int)d);
      if ((lanes >> lane) & 1ull) {
        const uint32_t pos = at + (uint32_t)__popcll(lanes & below);
        if (pos < cap) idx[pos] = i;
      }
      if (lane == d) run += (uint32_t)__popcll(lanes);
    });
  }
}

}  // namespace vp

using namespace vp;

extern "C" int vp_tx_build(vp_ctx *c, const vp_dev_batch *b, const vp_tx_lists *l,
                           void *stream) {
  if (!c || !b || !l || !b->out_dev || !l->offset) return VP_EINVAL;
  if ((!l->idx && l->cap) || (l->stats && !b->len && b->n)) return VP_EINVAL;
  if (!b->in_dev && b->in_port > 0xFFFFu) return VP_EINVAL;
  const uint32_t nd = ctx_devices(c), n = b->n;
  if (nd > VP_MAX_DEVICES) return VP_EINVAL;
  // every list position is a 32-bit number
  if ((uint64_t)n * std::max(1u, nd > 0 ? nd - 1 : 0u) > 0xFFFFFFFFull) return VP_EINVAL;
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));  // (the resident kernel holds the context's stream)
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const uint32_t blocks = (uint32_t)(((uint64_t)n + kTxBlockPackets - 1) / kTxBlockPackets);
  const size_t m = (size_t)blocks * nd;
  CallBuf &w = c->ws.tx_cnt;  // the blocks x n_devices counts
  VP_TRY(callbuf_reserve(w, 4 * m, s));
  uint32_t *cnt = (uint32_t *)w.p;
  if (l->stats) VP_HIP(hipMemsetAsync(l->stats, 0, sizeof(vp_tx_stats), s));
  if (blocks) {
    tx_count<<<blocks, kTxThreads, 4 * kTxThreads * std::max(1u, nd), s>>>(
        b->out_dev, b->in_dev, b->in_port, b->len, n, nd, blocks, cnt, l->stats);
    VP_HIP(hipGetLastError());
  }
  tx_scan<<<1, kTxScanThreads, 0, s>>>(cnt, (uint32_t)m, blocks, nd, l->offset, l->stats);
  VP_HIP(hipGetLastError());
  if (m && l->cap) {
    tx_scatter<<<blocks, kTxThreads, 0, s>>>(b->out_dev, b->in_dev, b->in_port, n, nd, blocks,
                                             cnt, l->idx, l->cap);
    VP_HIP(hipGetLastError());
  }
  return callbuf_done(w, s);
}
