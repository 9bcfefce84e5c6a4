// vp_table_erase / vp_table_free (include/vigpath.h): a batch
// of entries taken out of a context's table by key or by index, on the
// device, as the loop
//
//   for q = 0 .. n-1: if query q names a live entry, map_erase its key and
//                     dchain_free_index its index
//
// would leave it: the erased indices on the front of the free list, the last
// erasing query's first, nothing else moved. The work follows n.
//
//   er_by_key     one query per lane, grid-stride, the lookups' resolve (the
//   er_by_index   16-byte load, key_mask, key_hash, tbl_probe_masked; the
//                 index test): the index a query names into hit[q], and
//                 atomicMin(claim[index], q), so of the queries that name an
//                 index the first one holds it whatever the scheduling;
//   er_rank       each wave takes kSlotPerWave consecutive queries (the tx/rx
//                 units' geometry, vp_slots_dev.h): a query wins iff it holds
//                 its index's claim; the wave's winners into a workspace word;
//   txp_scan      vp_tx_pack's one-block exclusive scan of those words, one
//                 word more than there are waves: the last one is the total;
//   er_apply      the same geometry: a winner's position r is its wave's word
//                 plus the winners before it in the wave (ballots); it writes
//                 the entry out, pushes its index at stack[stack_top + r],
//                 leaves a tombstone and resets the claim word; every other
//                 query writes a miss;
//   er_commit     one thread moves the control block, as exp_commit does.
//
// No block waits for another: the order between the launches is the stream's.
#include <hip/hip_runtime.h>

#include "vp_slots_dev.h"
#include "vp_state_dev.h"

namespace vp {

VP_PRELOAD_UNIT(erase)

using namespace stimg;

namespace {

__global__ __launch_bounds__(256) void er_by_key(TableDev t, uint32_t tt, const uint4 *keys,
                                                 uint32_t n, uint32_t *hit, uint32_t *claim) {
  const uint4 mask = key_mask(tt);
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const uint4 k = keys[q];
    uint4 raw;
    uint32_t i = kNone;
    // (a set pad byte: no entry holds these 16 bytes)
    if (!any4(make_uint4(k.x & ~mask.x, k.y & ~mask.y, k.z & ~mask.z, k.w & ~mask.w)))
      i = tbl_probe_masked(t, key_hash(tt, k), k, mask, &raw);
    hit[q] = i;
    if (i != kNone) atomicMin(&claim[i], q);  // (i < cap: an entry's index)
  }
}

__global__ __launch_bounds__(256) void er_by_index(TableDev t, const uint32_t *idx, uint32_t n,
                                                   uint32_t *hit, uint32_t *claim) {
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    uint32_t i = idx[q];
    if (!(i < t.cap && t.slot_of[i] != kNone)) i = kNone;
    hit[q] = i;
    if (i != kNone) atomicMin(&claim[i], q);
  }
}

// The wave's first query; its turns take 64 consecutive ones each.
__device__ __forceinline__ uint64_t er_wave_first(uint32_t wave) {
  return (uint64_t)blockIdx.x * kSlotBlockEntries + (uint64_t)wave * kSlotPerWave;
}

// A query that lost its index to an earlier one names nothing live when its
// turn comes: hit[q] becomes a miss, so er_apply reads the winners from hit[]
// alone and may reset the claim words while other waves still run.
__global__ __launch_bounds__(kSlotThreads) void er_rank(uint32_t n, uint32_t *hit,
                                                        const uint32_t *claim, uint64_t *sums) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t q0 = er_wave_first(wave);
  uint32_t cnt = 0;
  for (uint32_t turn = 0; turn < kSlotTurns; turn++) {
    const uint64_t q = q0 + 64 * turn + lane;
    bool win = false;
    if (q < n) {
      const uint32_t i = hit[q];
      if (i != kNone) {
        win = claim[i] == (uint32_t)q;
        if (!win) hit[q] = kNone;
      }
    }
    cnt += (uint32_t)__popcll(__ballot(win));
  }
  if (lane == 0) sums[blockIdx.x * kSlotWaves + wave] = cnt;
}

// base[]: the scanned sums. Free in query order: the first winner is pushed
// first, so the last one ends on top (double-chain-impl.c:1968-1981), as
// exp_apply pushes an expiry's indices.
__global__ __launch_bounds__(kSlotThreads) void er_apply(TableDev t, uint32_t tt, SideVals sv,
                                                         uint32_t n, const uint32_t *hit,
                                                         uint32_t *claim, const uint64_t *base,
                                                         LkOut o) {
  __shared__ uint32_t tombs;
  if (threadIdx.x == 0) tombs = 0;
  __syncthreads();
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t q0 = er_wave_first(wave);
  const uint32_t top = t.ctl->stack_top;
  uint32_t r0 = (uint32_t)base[blockIdx.x * kSlotWaves + wave];
  for (uint32_t turn = 0; turn < kSlotTurns; turn++) {
    const uint64_t q = q0 + 64 * turn + lane;
    const uint32_t i = q < n ? hit[q] : kNone;
    const bool win = i != kNone;
    const uint64_t wins = __ballot(win);
    if (q < n) {
      uint4 raw = make_uint4(0u, 0u, 0u, 0u);
      uint32_t e = 0;
      if (win) {
        e = t.slot_of[i];
        raw = reinterpret_cast<const uint4 *>(t.bk + (e >> 2))[e & 3];
      }
      lk_put(t, tt, sv, o, (uint32_t)q, i, raw);  // (the entry as it was)
      if (win) {
        // (r < the winners <= n_live, and stack_top + n_live <= cap)
        t.stack[top + r0 + (uint32_t)__popcll(wins & ((1ull << lane) - 1ull))] = i;
        t.bk[e >> 2].idx[e & 3] = kTomb;
        t.slot_of[i] = kNone;
        claim[i] = ~0u;
      }
    }
    wave_append(&tombs, win);  // (counted per block, one global atomic)
    r0 += (uint32_t)__popcll(wins);
  }
  __syncthreads();
  if (threadIdx.x == 0 && tombs) atomicAdd(&t.ctl->n_tomb, tombs);
}

// total: the scan's last word. Every erased entry was in this rank's buckets
// (no communicator: st_enter), so sh_live follows n_live. exp_count carries
// the number to the host's read-back of the control block.
__global__ void er_commit(Ctl *ctl, const uint64_t *total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const uint32_t k = (uint32_t)*total;
    ctl->stack_top += k;
    ctl->n_live -= k;
    ctl->sh_live -= k;
    ctl->exp_count = k;
  }
}

int erase_run(vp_ctx *c, FlowTable &ft, uint32_t tt, uint32_t n, const void *in, bool by_key,
              const vp_lookup_out *out, hipStream_t s, uint32_t *k_out) {
  if (!ft.claim || ft.claim_dirty) {
    if (!ft.claim) VP_TRY(dalloc(&ft.claim, ft.cap));
    VP_HIP(hipMemsetAsync(ft.claim, 0xFF, 4ull * std::max(ft.cap, 1u), s));
    ft.claim_dirty = false;
  }
  const uint32_t blocks = (uint32_t)(((uint64_t)n + kSlotBlockEntries - 1) / kSlotBlockEntries);
  const uint32_t words = blocks * kSlotWaves;  // (n < 2^32: below 2^23 + 4)
  CallBuf &w = c->ws.erase_ws;
  const size_t sums_bytes = 8 * ((size_t)words + 1);
  VP_TRY(callbuf_reserve(w, sums_bytes + 4 * (size_t)n, s));
  uint64_t *sums = (uint64_t *)w.p;
  uint32_t *hit = (uint32_t *)((uint8_t *)w.p + sums_bytes);
  ft.claim_dirty = true;  // (until the call has reset every word it claimed)
  const TableDev t = tbl_dev(ft);
  if (by_key)
    er_by_key<<<grid_for(n), 256, 0, s>>>(t, tt, (const uint4 *)in, n, hit, ft.claim);
  else
    er_by_index<<<grid_for(n), 256, 0, s>>>(t, (const uint32_t *)in, n, hit, ft.claim);
  VP_HIP(hipGetLastError());
  VP_HIP(hipMemsetAsync(sums + words, 0, 8, s));
  er_rank<<<blocks, kSlotThreads, 0, s>>>(n, hit, ft.claim, sums);
  VP_HIP(hipGetLastError());
  txp_scan<<<1, kTxpScanThreads, 0, s>>>(sums, words + 1);
  VP_HIP(hipGetLastError());
  er_apply<<<blocks, kSlotThreads, 0, s>>>(t, tt, SideVals{c->be_rec, c->pol_size, c->pol_time}, n,
                                           hit, ft.claim, sums, lk_out(out, tt));
  VP_HIP(hipGetLastError());
  er_commit<<<1, 64, 0, s>>>(ft.ctl, sums + words);
  VP_HIP(hipGetLastError());
  VP_TRY(callbuf_done(w, s));
  if (s != c->stream) VP_HIP(hipStreamSynchronize(s));
  // one read-back: the counters' mirror, the number erased, the purge rule
  const uint64_t rebuilds = ft.rebuilds;
  VP_TRY(tbl_check_tombs(c, ft));
  ft.claim_dirty = false;
  *k_out = ft.h_ctl.exp_count;
  if (ft.rebuilds != rebuilds) VP_TRY(read_ctl(c, ft));  // (the purge moved n_tomb)
  return 0;
}

int table_erase(const char *fn, vp_ctx *c, int table, uint32_t n, const void *in, bool by_key,
                const vp_lookup_out *out, uint32_t *n_erased, void *stream) {
  StTable tb;
  VP_TRY(lk_enter(fn, c, table, n, in, by_key, out, false, &tb));
  if (n_erased) *n_erased = 0;
  if (n == 0) return 0;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  FlowTable &ft = *tb.t;
  uint32_t k = 0;
  VP_TRY(erase_run(c, ft, tb.tt, n, in, by_key, out, s, &k));
  if (n_erased) *n_erased = k;
  if (k == 0) return 0;  // (nothing changed: marks and a following stay)
  // The table changed outside the packet sequence: a moment of its own, which
  // ends a following as a packet does; the touch journal of this table says
  // nothing of the entries that left (seeded again by the next launch of the
  // resident kernel, if it was on). ts_floor stays a lower bound: an erase
  // only raises the least stamp. What run_batch keeps per table beside that
  // (fs_hint, runs_seen, ctl_clean) describes the traffic and the segment
  // counters, which an erase does not touch.
  c->seq += 1;
  c->st_following = false;
  if (ft.jr_on) {
    ft.jr_on = false;
    c->jr_want = true;
  }
  return 0;
}

}  // namespace
}  // namespace vp

int vp_table_erase(vp_ctx *c, int table, uint32_t n, const uint8_t *keys, const vp_lookup_out *out,
                   uint32_t *n_erased, void *stream) {
  return vp::table_erase("vp_table_erase", c, table, n, keys, true, out, n_erased, stream);
}

int vp_table_free(vp_ctx *c, int table, uint32_t n, const uint32_t *idx, const vp_lookup_out *out,
                  uint32_t *n_erased, void *stream) {
  return vp::table_erase("vp_table_free", c, table, n, idx, false, out, n_erased, stream);
}
