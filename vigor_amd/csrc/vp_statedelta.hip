// vp_state_mark / vp_state_delta_size / vp_state_delta_save / vp_state_follow /
// vp_state_delta_apply (include/vigpath.h): what changed in a
// context's table state since a mark, and its application to a context that
// holds the state of that mark.
//
// Save, per table: one pass over tseq[] that keeps the live indices touched
// since the mark (sd_collect: a ballot and one atomic per wave), the free
// list as the full image writes it (st_freed), one read-back for the sizes,
// the sort of the kept pairs into LRU order (tbl_live_sort), the image's
// gather over them (st_gather), one copy to the host. No bucket is read for
// an entry that was not touched.
// Apply: the host checks the header, the sizes and the follow condition, the
// delta is uploaded, sd_check reads the delta alone (indices into two
// bitmaps, stamps, pads, values, new[]'s keys into a scratch set), sd_check2
// reads it against the table (the partition of the indices, the kept
// entries' stamps and count, every new key looked up); nothing of the
// context is written before both have passed. Then sd_erase gives up the
// bucket entries of the indices that leave or change their key (the expiry's
// erase), sd_upsert puts the new keys in with tbl_insert's claim protocol, in
// place, and scatters stamps and values, and sd_commit writes the stack and
// the control block.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "vp_state_dev.h"

namespace vp {

VP_PRELOAD_UNIT(statedelta)

using namespace stimg;

namespace {

// ---------------------------------------------------------------- save --

// Every live index whose last touch has a sequence number of base or later,
// with that number, in any order: the live test of exp_collect over one
// streaming pass of tseq[] (slot_of[] is read only where tseq passes: a freed
// index keeps its last stamp). A wave's 64 indices are compacted by ballot
// and prefix count behind one atomicAdd (wave_append); every iteration is
// taken by whole waves.
__global__ __launch_bounds__(256) void sd_collect(TableDev t, uint64_t base, uint64_t *ekey,
                                                  uint32_t *eidx, uint32_t *count) {
  for (uint32_t i0 = blockIdx.x * blockDim.x; i0 < t.cap; i0 += gridDim.x * blockDim.x) {
    const uint32_t i = i0 + threadIdx.x;
    uint64_t q = 0;
    bool take = false;
    if (i < t.cap) {
      q = t.tseq[i];
      take = q >= base && t.slot_of[i] != kNone;
    }
    const uint32_t k = wave_append(count, take);
    if (take) {  // (k < cap: an index is taken once)
      eidx[k] = i;
      ekey[k] = q;
    }
  }
}

// --------------------------------------------------------------- apply --

__device__ __forceinline__ bool bit_of(const uint32_t *bm, uint32_t i) {
  return (bm[i >> 5] >> (i & 31)) & 1u;
}

// One table's scratch of an apply: the error word, the bitmap of the delta's
// free indices and of new[]'s (one bit per index, zero on entry), the set of
// new[]'s keys (entry numbers, kNone on entry; hmask + 1 >= 2 n_new slots),
// the reduction over the kept entries {largest stamp + 1, ~least stamp, their
// number} and the counters of the write {erased, inserted, tombstones
// reused}, all zero on entry.
struct SdScratch {
  unsigned long long *err;
  uint32_t *bm_free, *bm_new, *hset;
  uint32_t hmask;
  unsigned long long *red;
  uint32_t *cnt;
};

// Reads the delta only (im: new[] as an image's arrays, n_live = n_new). A
// key goes into the set: an entry on its path with the same key is a twin.
struct SdCheck {
  uint32_t *bm_idx, *bm_freed;
  const ImgDev &im;
  uint32_t tt;
  const SdScratch &s;
  __device__ __forceinline__ void key(uint32_t j, uint4 k, unsigned long long *err) const {
    uint32_t b = key_hash(tt, k) & s.hmask;
    for (uint32_t step = 0; step <= s.hmask; step++) {
      const uint32_t old = atomicCAS(&s.hset[b], kNone, j);
      if (old == kNone) break;
      if (eq4(im.key[old], k)) {
        img_fail(err, E_KEY_TWICE, max(j, old));
        break;
      }
      b = (b + 1) & s.hmask;
    }
  }
};
__global__ __launch_bounds__(256) void sd_check(ImgDev im, uint32_t tt, uint32_t cap,
                                                int64_t last_now, uint32_t vmax, SdScratch s) {
  img_check(im, tt, cap, last_now, vmax, s.err, SdCheck{s.bm_new, s.bm_free, im, tt, s},
            blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// map_get of a masked key in the table as it stands: the index that holds it,
// or kNone (an erased entry's key words are stale and skipped).
__device__ __forceinline__ uint32_t sd_find(const TableDev &t, uint4 mask, uint32_t h, uint4 key) {
  uint32_t b = home_bucket(h, t.bmask, t.mix, t.lin);
  for (uint32_t s = 0; s <= t.bmask; s++) {
    const uint4 *q = reinterpret_cast<const uint4 *>(t.bk + b);
    const uint4 ix = q[3];
    const uint32_t id[3] = {ix.x, ix.y, ix.z};
#pragma unroll
    for (uint32_t e = 0; e < kBucketEntries; e++) {
      if (id[e] == kEmpty) return kNone;
      if (id[e] != kTomb && eq4(and4(q[e], mask), key)) return id[e];
    }
    b = (b + 1) & t.bmask;
  }
  return kNone;
}

// The delta against the table (both bitmaps complete, every index of the
// delta below cap: launched only after sd_check passed). By index: in both
// lists; below fresh_next, in neither, and not live here (the kept entries
// plus n_new would not be n_live); the kept entries' stamps and number. By
// entry of new[]: its key held by a kept entry at another index.
__global__ __launch_bounds__(256) void sd_check2(ImgDev im, TableDev t, uint32_t tt, SdScratch s) {
  const uint4 mask = key_mask(tt);
  const uint32_t n = max(t.cap, im.n_live);
  unsigned long long hi = 0, lo = 0;  // largest stamp + 1, ~least stamp
  uint32_t kept = 0;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    if (j < t.cap) {
      const bool f = bit_of(s.bm_free, j), w = bit_of(s.bm_new, j);
      if (f && w) img_fail(s.err, E_BOTH, j);
      if (!f && !w && j < im.fresh) {
        if (t.slot_of[j] == kNone) {
          img_fail(s.err, E_NOT_KEPT, j);
        } else {
          const unsigned long long ts = t.ts[j];
          hi = max(hi, ts + 1);
          lo = max(lo, ~ts);
          kept++;
        }
      }
    }
    if (j < im.n_live) {
      const uint4 k = im.key[j];
      const uint32_t at = sd_find(t, mask, key_hash(tt, k), k);
      if (at != kNone && at != im.lru[j] && at < im.fresh && !bit_of(s.bm_free, at) &&
          !bit_of(s.bm_new, at))
        img_fail(s.err, E_KEY_KEPT, j);
    }
  }
  for (uint32_t o = 32; o > 0; o >>= 1) {
    hi = max(hi, (unsigned long long)__shfl_xor(hi, o));
    lo = max(lo, (unsigned long long)__shfl_xor(lo, o));
    kept += __shfl_xor(kept, o);
  }
  if (__lane_id() == 0 && kept) {
    atomicMax(&s.red[0], hi);
    atomicMax(&s.red[1], lo);
    atomicAdd(&s.red[2], (unsigned long long)kept);
  }
}

// The first write. An index that is live here and free in the delta (in
// freed[] or in its tail), or that new[] gives another key, gives up its
// bucket entry as exp_apply does: a tombstone, slot_of = kNone.
__global__ __launch_bounds__(256) void sd_erase(ImgDev im, TableDev t, uint32_t tt, SdScratch s) {
  const uint4 mask = key_mask(tt);
  const uint32_t n = max(t.cap, im.n_live);
  for (uint32_t j0 = blockIdx.x * blockDim.x; j0 < n; j0 += gridDim.x * blockDim.x) {
    const uint32_t j = j0 + threadIdx.x;
    // (an index of new[] is neither in freed[] nor in the tail: the two
    // clauses never meet on one index)
    uint32_t gone[2] = {kNone, kNone};
    if (j < t.cap && t.slot_of[j] != kNone && (j >= im.fresh || bit_of(s.bm_free, j))) gone[0] = j;
    if (j < im.n_live) {
      const uint32_t i = im.lru[j];
      if (t.slot_of[i] != kNone && !eq4(and4(tbl_key_of(t, i), mask), im.key[j])) gone[1] = i;
    }
#pragma unroll
    for (uint32_t g = 0; g < 2; g++) {
      if (gone[g] != kNone) {
        const uint32_t e = t.slot_of[gone[g]];
        t.bk[e >> 2].idx[e & 3] = kTomb;
        t.slot_of[gone[g]] = kNone;
      }
      wave_append(&s.cnt[0], gone[g] != kNone);
    }
  }
}

// new[] into the table: an index that still has its entry holds the same key
// and gets its key words again (the value some tables keep in them), any
// other is inserted; stamps, LRU ranks seq + j and values by index.
__global__ __launch_bounds__(256) void sd_upsert(ImgDev im, TableDev t, uint32_t tt, SideVals sv,
                                                 uint64_t seq, SdScratch s) {
  uint32_t disp = 0;
  for (uint32_t j0 = blockIdx.x * blockDim.x; j0 < im.n_live; j0 += gridDim.x * blockDim.x) {
    const uint32_t j = j0 + threadIdx.x;
    bool put = false, tomb = false;
    if (j < im.n_live) {
      const uint32_t i = im.lru[j];
      const uint4 k = raw_key(tt, im, j);
      const uint32_t e = t.slot_of[i];
      if (e != kNone) {
        reinterpret_cast<uint4 *>(t.bk + (e >> 2))[e & 3] = k;
      } else {
        const uint32_t h = key_hash(tt, im.key[j]);
        const uint32_t kw[4] = {k.x, k.y, k.z, k.w};
        t.hash_of[i] = h;
        t.slot_of[i] = tbl_insert(t, h, kw, i, &tomb, &disp);
        put = true;
      }
      t.ts[i] = (uint64_t)im.ts[j];
      t.tseq[i] = seq + j;
      t.birth[i] = 0;
      side_put(tt, sv, i, im, j);
    }
    wave_append(&s.cnt[1], put);
    wave_append(&s.cnt[2], tomb);
  }
  for (uint32_t o = 32; o > 0; o >>= 1) disp += __shfl_xor(disp, o);
  if ((threadIdx.x & 63) == 0 && disp) atomicAdd(&t.ctl->disp_count, disp);
}

// The stack (its top = the first index handed out) and the control block.
__global__ __launch_bounds__(256) void sd_commit(ImgDev im, TableDev t, uint32_t n_live,
                                                 SdScratch s) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < im.n_freed;
       j += gridDim.x * blockDim.x)
    t.stack[im.n_freed - 1u - j] = im.freed[j];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    t.ctl->stack_top = im.n_freed;
    t.ctl->fresh_next = im.fresh;
    t.ctl->n_live = n_live;
    t.ctl->sh_live = n_live;
    t.ctl->n_tomb += s.cnt[0] - s.cnt[2];
    t.ctl->new_count = s.cnt[1];
  }
}

// ---------------------------------------------------------------- host --

bool mark_eq(const vp_state_mark_t &a, const vp_state_mark_t &b) {
  return a.seq == b.seq && a.epoch == b.epoch;
}

int base_check(const vp_ctx *c, const vp_state_mark_t *base, const char *who) {
  if (base->epoch != c->st_epoch)
    return ST_BAD("%s: the base's epoch %llu is not this context's %llu", who,
                  (unsigned long long)base->epoch, (unsigned long long)c->st_epoch);
  if (base->seq > c->seq)
    return ST_BAD("%s: the base's seq %llu lies ahead of this context's %llu", who,
                  (unsigned long long)base->seq, (unsigned long long)c->seq);
  return 0;
}

int delta_save(vp_ctx *c, const vp_state_mark_t *base, uint8_t *buf, uint64_t cap,
               uint64_t *bytes, vp_state_mark_t *mark, bool size_only) {
  StTable tabs[2];
  int nt = 0;
  VP_TRY(st_enter(c, tabs, &nt));
  VP_TRY(base_check(c, base, size_only ? "state delta size" : "state delta save"));
  if (size_only) return st_size_bound(c, tabs, nt, kDelta.hdr, bytes);
  Section sec[2];
  // the touched indices and the free list of every table, one read-back
  DevBuf res;
  VP_TRY(dalloc((uint32_t **)&res.p, 6));
  uint32_t *d_res = (uint32_t *)res.p, h_res[6] = {};
  VP_HIP(hipMemsetAsync(d_res, 0, sizeof h_res, c->stream));
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    sd_collect<<<grid_for(t.cap, 256, 512), 256, 0, c->stream>>>(tbl_dev(t), base->seq, t.ekey,
                                                                  t.eidx, d_res + 4 + k);
    VP_HIP(hipGetLastError());
    VP_TRY(st_launch_freed(c, t, t.eidx2, d_res + 2 * k));
  }
  VP_HIP(hipMemcpyAsync(h_res, d_res, sizeof h_res, hipMemcpyDeviceToHost, c->stream));
  uint64_t at = kDelta.hdr;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    VP_TRY(read_ctl(c, t));  // (waits for the stream: h_res is there)
    const Ctl &h = t.h_ctl;
    const uint32_t n_freed = h_res[2 * k], fresh = h_res[2 * k + 1], n_new = h_res[4 + k];
    if (n_new > h.n_live || h.n_live > t.cap || n_freed > h.stack_top || fresh > t.cap ||
        (uint64_t)h.n_live + n_freed + (t.cap - fresh) != t.cap)
      return state_fail("state delta save: table %d holds %u touched of %u live, %u freed, tail "
                        "from %u of %u", k, n_new, h.n_live, n_freed, fresh, t.cap);
    sec[k] = section_at(at, t.cap, n_new, fresh, tabs[k].tt, n_freed, h.n_live);
    at = sec[k].end;
  }
  const uint64_t total = at;
  *bytes = total;
  if (cap < total)
    return ST_BAD("state delta save: the delta takes %llu bytes, the buffer holds %llu",
                  (unsigned long long)total, (unsigned long long)cap);
  DevBuf img;
  VP_TRY(dalloc((uint8_t **)&img.p, total));
  uint8_t *d = (uint8_t *)img.p;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    const Section &s = sec[k];
    // (the free list leaves the expiry workspace before the sort writes there)
    if (s.n_freed)
      VP_HIP(hipMemcpyAsync(d + s.freed, t.eidx2, 4ull * s.n_freed, hipMemcpyDeviceToDevice,
                            c->stream));
    const uint64_t *seq = nullptr;
    const uint32_t *idx = nullptr;
    VP_TRY(tbl_live_sort(c, t, s.n_live, &seq, &idx));
    VP_TRY(st_launch_gather(c, t, tabs[k].tt, idx, section_dev(s, d), section_pads(s, d)));
  }
  VP_HIP(hipMemcpyAsync(buf, d, total, hipMemcpyDeviceToHost, c->stream));
  VP_HIP(hipStreamSynchronize(c->stream));
  // the headers
  put_header(kDelta, buf, c->kind, nt, total, c->last_now);
  put64(buf + 32, base->seq);
  put64(buf + 40, base->epoch);
  put64(buf + 48, c->seq);
  put64(buf + 56, c->st_epoch);
  for (int k = 0; k < nt; k++) put_table_header(kDelta, buf, sec[k]);
  *mark = vp_state_mark_t{c->seq, c->st_epoch};
  return 0;
}

#define SD_BAD(...) ST_BAD("state delta apply: " __VA_ARGS__)

int delta_apply(vp_ctx *c, const uint8_t *buf, uint64_t bytes) {
  StTable tabs[2];
  int nt = 0;
  VP_TRY(st_enter(c, tabs, &nt));
  // ---- the host's checks: nothing is uploaded before they pass
  if (!c->st_following) return SD_BAD("the context follows no mark");
  if (c->seq != c->st_follow_seq)
    return SD_BAD("the context changed since it followed (sequence %llu, then %llu)",
                  (unsigned long long)c->seq, (unsigned long long)c->st_follow_seq);
  const Expect want = st_expect(c, tabs, nt);
  char msg[256];
  int64_t last_now;
  if (!read_header(kDelta, want, buf, bytes, &last_now, msg, sizeof msg)) return ST_BAD("%s", msg);
  if (last_now < c->last_now)
    return SD_BAD("last_now %lld is below the context's %lld", (long long)last_now,
                  (long long)c->last_now);
  const vp_state_mark_t base{get64(buf + 32), get64(buf + 40)};
  const vp_state_mark_t mark{get64(buf + 48), get64(buf + 56)};
  if (!mark_eq(base, c->st_mark))
    return SD_BAD("base mark (%llu, %llu), the context follows (%llu, %llu)",
                  (unsigned long long)base.seq, (unsigned long long)base.epoch,
                  (unsigned long long)c->st_mark.seq, (unsigned long long)c->st_mark.epoch);
  if (mark.epoch != base.epoch || mark.seq < base.seq)
    return SD_BAD("mark (%llu, %llu) does not follow its base", (unsigned long long)mark.seq,
                  (unsigned long long)mark.epoch);
  Section sec[2];
  if (!read_sections(kDelta, want, buf, bytes, sec, msg, sizeof msg)) return ST_BAD("%s", msg);
  // ---- upload, then the device's checks
  DevBuf img, scratch;
  VP_TRY(dalloc((uint8_t **)&img.p, bytes));
  uint8_t *d = (uint8_t *)img.p;
  VP_HIP(hipMemcpyAsync(d, buf, bytes, hipMemcpyHostToDevice, c->stream));
  // scratch, in 32-bit words: per table the error word and the reduction (4 x
  // u64), the counters (4), then the two bitmaps; the key sets behind (kNone)
  constexpr uint64_t kFixed = 12;
  uint64_t woff = 0, fixed[2], bmw[2], hoff[2], hsz[2];
  for (int k = 0; k < nt; k++) {
    fixed[k] = woff;
    bmw[k] = (sec[k].cap + 31) / 32;
    woff += kFixed + 2 * bmw[k];
  }
  const uint64_t zero_words = woff;
  for (int k = 0; k < nt; k++) {
    hoff[k] = woff;
    hsz[k] = std::max<uint64_t>(next_pow2(2ull * sec[k].n_live), 2);
    woff += hsz[k];
  }
  VP_TRY(dalloc((uint32_t **)&scratch.p, woff));
  uint32_t *sw = (uint32_t *)scratch.p;
  VP_HIP(hipMemsetAsync(sw, 0, 4 * zero_words, c->stream));
  VP_HIP(hipMemsetAsync(sw + zero_words, 0xFF, 4 * (woff - zero_words), c->stream));
  SdScratch sc[2];
  unsigned long long h_fix[2][4];  // {err, red[0..2]}
  for (int k = 0; k < nt; k++) {
    uint32_t *f = sw + fixed[k];
    sc[k] = SdScratch{(unsigned long long *)f, f + kFixed, f + kFixed + bmw[k], sw + hoff[k],
                      (uint32_t)(hsz[k] - 1), (unsigned long long *)f + 1, f + 8};
    VP_HIP(hipMemsetAsync(sc[k].err, 0xFF, 8, c->stream));
  }
  auto read_fixed = [&]() -> int {
    for (int k = 0; k < nt; k++)
      VP_HIP(hipMemcpyAsync(h_fix[k], sc[k].err, 32, hipMemcpyDeviceToHost, c->stream));
    VP_HIP(hipStreamSynchronize(c->stream));
    return 0;
  };
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    sd_check<<<grid_for(std::max({s.n_live, s.n_freed, 1u})), 256, 0, c->stream>>>(
        section_dev(s, d), tabs[k].tt, s.cap, last_now, value_bound(c, tabs[k].tt), sc[k]);
    VP_HIP(hipGetLastError());
  }
  VP_TRY(read_fixed());
  for (int k = 0; k < nt; k++)
    if (h_fix[k][0] != ~0ull) return img_refuse(kDelta.who, "idx", k, tabs[k].tt, h_fix[k][0]);
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    sd_check2<<<grid_for(std::max(s.cap, s.n_live)), 256, 0, c->stream>>>(
        section_dev(s, d), tbl_dev(*tabs[k].t), tabs[k].tt, sc[k]);
    VP_HIP(hipGetLastError());
  }
  VP_TRY(read_fixed());
  uint64_t floor[2];
  for (int k = 0; k < nt; k++) {
    if (h_fix[k][0] != ~0ull) return img_refuse(kDelta.who, "idx", k, tabs[k].tt, h_fix[k][0]);
    const Section &s = sec[k];
    const uint64_t kept = h_fix[k][3];
    if (kept + s.n_live != s.n_table)
      return SD_BAD("table %d: %llu kept entries and n_new %u are not n_live %u", k,
                    (unsigned long long)kept, s.n_live, s.n_table);
    const int64_t ts0 = s.n_live ? (int64_t)get64(buf + s.ts) : 0;
    if (kept && s.n_live && (int64_t)(h_fix[k][1] - 1) > ts0)
      return SD_BAD("table %d: ts[0] %lld is below a kept entry's stamp %lld", k, (long long)ts0,
                    (long long)(h_fix[k][1] - 1));
    floor[k] = kept ? ~h_fix[k][2] : s.n_live ? (uint64_t)ts0 : UINT64_MAX;
  }
  // ---- the write: from here on the context's state is the delta's
  uint32_t most = 0;
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    const ImgDev im = section_dev(s, d);
    const TableDev t = tbl_dev(*tabs[k].t);
    sd_erase<<<grid_for(std::max(s.cap, s.n_live)), 256, 0, c->stream>>>(im, t, tabs[k].tt, sc[k]);
    if (s.n_live)
      sd_upsert<<<grid_for(s.n_live), 256, 0, c->stream>>>(
          im, t, tabs[k].tt, SideVals{c->be_rec, c->pol_size, c->pol_time}, c->seq, sc[k]);
    sd_commit<<<grid_for(std::max(s.n_freed, 1u)), 256, 0, c->stream>>>(im, t, s.n_table,
                                                                        sc[k]);
    VP_HIP(hipGetLastError());
    most = std::max(most, s.n_live);
  }
  VP_HIP(hipStreamSynchronize(c->stream));
  c->seq += most;  // (past every tseq handed out above)
  c->st_mark = mark;
  c->st_follow_seq = c->seq;
  VP_TRY(st_replaced(c, tabs, nt, floor, last_now));
  for (int k = 0; k < nt; k++) VP_TRY(tbl_check_tombs(c, *tabs[k].t));
  return 0;
}

}  // namespace
}  // namespace vp

int vp_state_mark(vp_ctx *c, vp_state_mark_t *mark) {
  if (!c || !mark) return VP_EINVAL;
  vp::StTable tabs[2];
  int nt = 0;
  VP_TRY(vp::st_enter(c, tabs, &nt));
  *mark = vp_state_mark_t{c->seq, c->st_epoch};
  return 0;
}

int vp_state_delta_size(vp_ctx *c, const vp_state_mark_t *base, uint64_t *bytes) {
  if (!c || !base || !bytes) return VP_EINVAL;
  return vp::delta_save(c, base, nullptr, 0, bytes, nullptr, true);
}

int vp_state_delta_save(vp_ctx *c, const vp_state_mark_t *base, void *buf, uint64_t cap,
                        uint64_t *bytes, vp_state_mark_t *mark) {
  if (!c || !base || !bytes || !mark || (!buf && cap)) return VP_EINVAL;
  return vp::delta_save(c, base, (uint8_t *)buf, cap, bytes, mark, false);
}

int vp_state_follow(vp_ctx *c, const vp_state_mark_t *mark) {
  if (!c || !mark) return VP_EINVAL;
  vp::StTable tabs[2];
  int nt = 0;
  VP_TRY(vp::st_enter(c, tabs, &nt));
  c->st_mark = *mark;
  c->st_follow_seq = c->seq;
  c->st_following = true;
  return 0;
}

int vp_state_delta_apply(vp_ctx *c, const void *buf, uint64_t bytes) {
  if (!c || !buf) return VP_EINVAL;
  return vp::delta_apply(c, (const uint8_t *)buf, bytes);
}
