// A packed frame stream as a device batch (vp_rx_unpack, include/vigpath.h):
// the inverse of vp_tx_pack. Frames that lie at 16-byte aligned positions in
// one run of bytes are scattered into consecutive slots, with their len[],
// time and index of origin.
//
// With pos[] one launch:
//
//   rxu_scatter each block takes kSlotBlockEntries consecutive entries; a wave
//               walks 64 of them per turn: sel[], len[], the time and pos[]
//               one entry per lane, validated, len / now / src stored
//               coalesced, then the slots through the slot mover
//               (vp_slots_dev.h). Block 0 writes the count.
//
// Without pos[] the positions are the running sum of the padded lengths, and
// two launches come first on the same stream:
//
//   rxu_sizes   every wave of every block sums the padded lengths of the
//               kSlotPerWave entries it will scatter into a workspace word;
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
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(rxunpack)

// a frame's padded length is at most 65536 (len is 16 bits)
static_assert((uint64_t)kSlotPerWave * 65536u < (1ull << 32), "a wave's sum in 32 bits");

__global__ __launch_bounds__(kSlotThreads) void rxu_sizes(const RxuArgs a, uint64_t *sums) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t w0 = (uint64_t)blockIdx.x * kSlotBlockEntries + wv * kSlotPerWave;
  uint32_t sum = 0;
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k = w0 + it * 64 + lane;
    if (w0 + it * 64 >= a.m) break;
    uint32_t mm, l;
    bool in;
    rxu_meta(a, k, k < a.m, mm, in, l);
    sum += pad16(l);
  }
  sum = wave_sum(sum);
  if (lane == 0) sums[(size_t)blockIdx.x * kSlotWaves + wv] = sum;  // (0 past the end)
}

// What a lane holds of its entry for the slot mover: the frame lies at `p` in
// the stream with `r` bytes to keep; r is 0 for an entry that is not readable,
// and then nothing is read
struct RxuFrame {
  const uint8_t *data;
  uint64_t p;
  uint32_t r;
  __device__ __forceinline__ RxuFrame at(uint32_t e) const {
    return {data, shfl64(p, e), (uint32_t)__shfl(r, (int)e)};
  }
  __device__ __forceinline__ RxuFrame at_uniform(uint32_t e) const {
    return {data, readlane64(p, e), (uint32_t)__builtin_amdgcn_readlane((int)r, (int)e)};
  }
  __device__ __forceinline__ uint4 unit(uint32_t u, bool on) const {
    const uint32_t keep = on ? r : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (u < keep) v = unit_clear(*(const uint4 *)(data + p + u), keep - u);
    return v;
  }
};

__global__ __launch_bounds__(kSlotThreads) void rxu_scatter(const RxuArgs a) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (blockIdx.x == 0 && tid == 0) *a.count = a.n;
  const uint64_t w0 = (uint64_t)blockIdx.x * kSlotBlockEntries + wv * kSlotPerWave;
  if (w0 >= a.m) return;
  const SlotPath path = slot_path(a.oslot);
  uint64_t run = 0;  // pos == NULL: this turn's first position
  if (!a.pos) run = a.base[(size_t)blockIdx.x * kSlotWaves + wv];
  for (uint32_t it = 0; it < kSlotTurns; it++) {
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
      const uint32_t ext = pad16(l);
      const uint32_t x = wave_scan(ext, lane);
      p = run + (x - ext);
      run += (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    // readable: inside len[], aligned, and its kept bytes' units inside the
    // stream; compared without a sum that could wrap
    uint32_t r = l < a.oslot ? l : a.oslot;
    const bool ok = in && (p & 15) == 0 && p <= a.bytes && pad16(r) <= a.bytes - p;
    uint64_t at = 0;
    if (ok)
      at = batch_time(a.now, a.now0, a.now_step, mm);
    else
      l = r = 0;
    if (mine) {
      a.olen[k] = (uint16_t)l;
      if (a.onow) a.onow[k] = (int64_t)at;
      if (a.osrc) a.osrc[k] = mm;
    }
    slot_move(path, RxuFrame{a.data, p, r}, a.oframes, a.oslot, k0, lane, left);
  }
}

}  // namespace vp

using namespace vp;

extern "C" int vp_rx_unpack(vp_ctx *c, const vp_rx_stream *in, const vp_tx_next *o, void *stream) {
  if (!c || !in || !o || !o->count || !slot_dest_ok(o)) return VP_EINVAL;
  if ((!in->data && in->bytes) || ((uintptr_t)in->data & 15)) return VP_EINVAL;
  if (!in->len && in->meta_n) return VP_EINVAL;
  // the stream and the slot array may not overlap
  if (bytes_overlap(in->data, in->bytes, o->frames, (uint64_t)o->cap * o->slot)) return VP_EINVAL;
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
  const uint32_t blocks = a.m ? (a.m - 1) / kSlotBlockEntries + 1 : 1;
  const bool sums = !in->pos && a.m;
  CallBuf &w = c->ws.rxu_sum;  // the waves' sums
  if (sums) {
    const uint32_t words = blocks * kSlotWaves;
    VP_TRY(callbuf_reserve(w, 8 * (size_t)words, s));
    rxu_sizes<<<blocks, kSlotThreads, 0, s>>>(a, (uint64_t *)w.p);
    VP_HIP(hipGetLastError());
    txp_scan<<<1, kTxpScanThreads, 0, s>>>((uint64_t *)w.p, words);
    VP_HIP(hipGetLastError());
    a.base = (const uint64_t *)w.p;
  }
  rxu_scatter<<<blocks, kSlotThreads, 0, s>>>(a);
  VP_HIP(hipGetLastError());
  return sums ? callbuf_done(w, s) : 0;
}
