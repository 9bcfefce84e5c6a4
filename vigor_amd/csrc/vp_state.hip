// vp_state_size / vp_state_save / vp_state_load (include/vigpath.h, DESIGN.md
// §5.14): the libVig-level state of a context's tables as a canonical,
// layout-independent image in host memory, and its way back into a context.
//
// Save, per table: every live index with its tseq (tbl_live_collect: the
// journal seed's and the expiry's scan), the free list in hand-out order
// with the never-used tail normalised (st_freed), one read-back, the sort
// into LRU order (tbl_live_sort), one gather kernel that writes the image's
// arrays coalesced (st_gather), one copy to the host.
// Load: the host checks sizes, counts and offsets against the byte count,
// the image is uploaded, st_check reads only the image and reports the first
// offending field; then the bucket array is built aside by insertion
// (st_insert) and every key looked up in it (st_dup: a key that occurs twice
// finds the other entry); only then st_commit writes the stamps, values,
// stack and control block, and the host swaps the pointers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "vp_state_dev.h"

namespace vp {

VP_PRELOAD_UNIT(state)

using namespace stimg;

namespace {

constexpr uint32_t kStMagic = VP_STATE_MAGIC;
constexpr uint32_t kStVersion = VP_STATE_VERSION;
constexpr uint32_t kStHdr = 32;

// ---------------------------------------------------------------- save --

// freed[] of the image: the stack from its top down to the first index that
// does not belong to the never-used tail. The tail is the longest run at the
// end of the hand-out order (stack top first, then fresh_next .. cap - 1)
// that is ascending and consecutive up to cap - 1: entries j = 0, 1, .. of
// the stack with stack[j] == fresh_next - 1 - j extend it downwards. Every
// block finds that j itself (the run is rarely longer than a few entries),
// then the grid copies. res = {n_freed, the normalised fresh_next}.
__global__ __launch_bounds__(256) void st_freed(TableDev t, uint32_t *freed, uint32_t *res) {
  __shared__ uint32_t first;
  const uint32_t top = t.ctl->stack_top, fresh = t.ctl->fresh_next;
  if (threadIdx.x == 0) first = top;
  __syncthreads();
  for (uint32_t base = 0; base < top; base += blockDim.x) {
    const uint32_t j = base + threadIdx.x;
    if (j < top && t.stack[j] != fresh - 1u - j) atomicMin(&first, j);
    __syncthreads();
    const uint32_t f = first;
    __syncthreads();
    if (f < top) break;
  }
  const uint32_t j0 = first, n = top - j0;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    freed[r] = t.stack[top - 1u - r];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    res[0] = n;
    res[1] = fresh - j0;
  }
}

// The image's arrays of one table, entry j = the j-th oldest live index.
// Thread 0 also zeroes the pad bytes behind each array (pad[]: from, to).
__global__ __launch_bounds__(256) void st_gather(TableDev t, uint32_t tt, SideVals sv,
                                                 const uint32_t *idx, ImgDev im, Pads pads) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < im.n_live;
       j += gridDim.x * blockDim.x) {
    const uint32_t i = idx[j];
    const Entry e = entry_of(t, tt, sv, i, tbl_key_of(t, i));
    im.lru[j] = i;
    im.ts[j] = e.ts;
    im.key[j] = e.key;
    value_put(tt, im.val, j, e.val);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (uint32_t a = 0; a < 5; a++)
      for (uint32_t b = 0; b < pads.n[a]; b++) pads.at[a][b] = 0;
}

// ---------------------------------------------------------------- load --

// What st_check / st_dup report: code << 32 | position, the least one wins.
enum StErr : uint32_t {
  E_LRU_RANGE = 1, E_FREED_RANGE, E_LRU_TAIL, E_FREED_TAIL, E_LRU_TWICE, E_FREED_TWICE,
  E_FREED_NORM, E_TS_NEG, E_TS_FUTURE, E_TS_ORDER, E_KEY_PAD, E_VAL_RANGE, E_KEY_TWICE
};
__device__ __forceinline__ void st_fail(unsigned long long *err, uint32_t code, uint32_t j) {
  atomicMin(err, ((unsigned long long)code << 32) | j);
}

// Reads the image only. bitmap: one bit per index, zero on entry; vmax: the
// first value out of range (0: any).
__global__ __launch_bounds__(256) void st_check(ImgDev im, uint32_t tt, uint32_t cap,
                                                int64_t last_now, uint32_t vmax,
                                                uint32_t *bitmap, unsigned long long *err) {
  const uint4 mask = key_mask(tt);
  const uint32_t n = max(im.n_live, im.n_freed);
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    if (j < im.n_live) {
      const uint32_t i = im.lru[j];
      if (i >= cap) {
        st_fail(err, E_LRU_RANGE, j);
      } else {
        if (i >= im.fresh) st_fail(err, E_LRU_TAIL, j);
        if (atomicOr(&bitmap[i >> 5], 1u << (i & 31)) & (1u << (i & 31)))
          st_fail(err, E_LRU_TWICE, j);
      }
      const int64_t ts = im.ts[j];
      if (ts < 0) st_fail(err, E_TS_NEG, j);
      if (ts > last_now) st_fail(err, E_TS_FUTURE, j);
      if (j > 0 && im.ts[j - 1] > ts) st_fail(err, E_TS_ORDER, j);
      const uint4 k = im.key[j];
      if (any4(make_uint4(k.x & ~mask.x, k.y & ~mask.y, k.z & ~mask.z, k.w & ~mask.w)))
        st_fail(err, E_KEY_PAD, j);
      if (vmax && reinterpret_cast<const uint32_t *>(im.val)[j] >= vmax)
        st_fail(err, E_VAL_RANGE, j);
    }
    if (j < im.n_freed) {
      const uint32_t i = im.freed[j];
      if (i >= cap) {
        st_fail(err, E_FREED_RANGE, j);
      } else {
        if (i >= im.fresh) st_fail(err, E_FREED_TAIL, j);
        if (atomicOr(&bitmap[i >> 5], 1u << (i & 31)) & (1u << (i & 31)))
          st_fail(err, E_FREED_TWICE, j);
      }
      if (j == im.n_freed - 1 && i + 1 == im.fresh) st_fail(err, E_FREED_NORM, j);
    }
  }
}

// The bucket array built aside (`t`: new buckets, slot_of, hash_of and
// control block; the checked image names every index once and below cap).
__global__ __launch_bounds__(256) void st_insert(TableDev t, uint32_t tt, ImgDev im) {
  uint32_t disp = 0;
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < im.n_live;
       j += gridDim.x * blockDim.x) {
    const uint32_t i = im.lru[j];
    const uint4 k = raw_key(tt, im, j);
    const uint32_t h = key_hash(tt, im.key[j]);
    const uint32_t kw[4] = {k.x, k.y, k.z, k.w};
    bool tomb = false;
    t.hash_of[i] = h;
    t.slot_of[i] = tbl_insert(t, h, kw, i, &tomb, &disp);
  }
  for (uint32_t o = 32; o > 0; o >>= 1) disp += __shfl_xor(disp, o);
  if ((threadIdx.x & 63) == 0 && disp) atomicAdd(&t.ctl->disp_count, disp);
}

// map_get of every image key in the array built aside: the first entry on
// its probe path that holds the key is its own unless the key occurs twice.
__global__ __launch_bounds__(256) void st_dup(TableDev t, uint32_t tt, ImgDev im,
                                              unsigned long long *err) {
  const uint4 mask = key_mask(tt);
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < im.n_live;
       j += gridDim.x * blockDim.x) {
    const uint32_t i = im.lru[j];
    const uint4 key = im.key[j];
    uint32_t b = home_bucket(t.hash_of[i], t.bmask, t.mix, t.lin), found = kNone;
    for (uint32_t s = 0; s <= t.bmask && found == kNone; s++) {
      const uint4 *q = reinterpret_cast<const uint4 *>(t.bk + b);
      const uint4 ix = q[3];
      const uint32_t id[3] = {ix.x, ix.y, ix.z};
      bool end = false;
#pragma unroll
      for (uint32_t e = 0; e < kBucketEntries; e++) {
        if (end || found != kNone) continue;
        if (id[e] == kEmpty) {
          end = true;
          continue;
        }
        const uint4 k = and4(q[e], mask);
        if (k.x == key.x && k.y == key.y && k.z == key.z && k.w == key.w) found = id[e];
      }
      if (end) break;
      b = (b + 1) & t.bmask;
    }
    if (found != i) st_fail(err, E_KEY_TWICE, j);
  }
}

// The point of no return: stamps, LRU ranks and values by index into the
// table's own arrays, the stack (its top = the first index handed out) and
// the new control block.
__global__ __launch_bounds__(256) void st_commit(TableDev t, uint32_t tt, SideVals sv,
                                                 ImgDev im) {
  const uint32_t n = max(im.n_live, im.n_freed);
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    if (j < im.n_live) {
      const uint32_t i = im.lru[j];
      t.ts[i] = (uint64_t)im.ts[j];
      t.tseq[i] = j;
      t.birth[i] = 0;
      if (tt == TT_LBBACK) {
        const uint2 v = reinterpret_cast<const uint2 *>(im.val)[j];
        sv.be_rec[i] = make_uint4(im.key[j].x, v.x, v.y, 0u);
      } else if (tt == TT_POL) {
        const uint4 v = reinterpret_cast<const uint4 *>(im.val)[j];
        sv.pol_size[i] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        sv.pol_time[i] = (int64_t)((uint64_t)v.z | ((uint64_t)v.w << 32));
      }
    }
    if (j < im.n_freed) t.stack[im.n_freed - 1u - j] = im.freed[j];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    t.ctl->stack_top = im.n_freed;
    t.ctl->fresh_next = im.fresh;
    t.ctl->n_live = im.n_live;
    t.ctl->sh_live = im.n_live;
  }
}

}  // namespace

// ---------------------------------------------------------------- host --

int st_tables(vp_ctx *c, StTable out[2]) {
  switch (c->kind) {
    case KIND_NAT: out[0] = {&c->ft, TT_NAT}; return 1;
    case KIND_BRIDGE: out[0] = {&c->ft, TT_BRIDGE}; return 1;
    case KIND_FW: out[0] = {&c->ft, TT_FW}; return 1;
    case KIND_POL: out[0] = {&c->ft, TT_POL}; return 1;
    case KIND_LB: out[0] = {&c->ft, TT_LBFLOW}; out[1] = {&c->ft2, TT_LBBACK}; return 2;
    default: return 0;
  }
}

int st_enter(vp_ctx *c, StTable tabs[2], int *ntabs) {
  if (!c) return VP_EINVAL;
  if (hipSetDevice(c->gpu) != hipSuccess) return VP_EIO;
  VP_TRY(serve_stop(c));
  VP_HIP(hipStreamSynchronize(c->stream));
  if (c->comm) return VP_ENOTSUP;
  *ntabs = st_tables(c, tabs);
  return *ntabs ? 0 : VP_EINVAL;
}

int st_launch_freed(vp_ctx *c, FlowTable &t, uint32_t *freed, uint32_t *res) {
  st_freed<<<grid_for(t.cap), 256, 0, c->stream>>>(tbl_dev(t), freed, res);
  VP_HIP(hipGetLastError());
  return 0;
}

int st_launch_gather(vp_ctx *c, FlowTable &t, uint32_t tt, const uint32_t *idx, const ImgDev &im,
                     const Pads &pads) {
  st_gather<<<grid_for(std::max(im.n_live, 1u)), 256, 0, c->stream>>>(
      tbl_dev(t), tt, SideVals{c->be_rec, c->pol_size, c->pol_time}, idx, im, pads);
  VP_HIP(hipGetLastError());
  return 0;
}

namespace {

int state_save(vp_ctx *c, uint8_t *buf, uint64_t cap, uint64_t *bytes, bool size_only) {
  StTable tabs[2];
  int nt = 0;
  VP_TRY(st_enter(c, tabs, &nt));
  Section sec[2];
  if (size_only) {  // an upper bound: every stacked index counted as freed
    uint64_t at = kStHdr;
    for (int k = 0; k < nt; k++) {
      FlowTable &t = *tabs[k].t;
      VP_TRY(read_ctl(c, t));
      sec[k] = Section{t.cap, t.h_ctl.n_live, 0, kValSize[tabs[k].tt], t.h_ctl.stack_top};
      section_layout(sec[k], at);
      at = sec[k].end;
    }
    *bytes = at;
    return 0;
  }
  // live indices and the free list of every table, one read-back each
  DevBuf res;
  VP_TRY(dalloc((uint32_t **)&res.p, 4));
  uint32_t h_res[4] = {};
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    VP_TRY(tbl_live_collect(c, t));
    VP_TRY(st_launch_freed(c, t, t.eidx2, (uint32_t *)res.p + 2 * k));
  }
  VP_HIP(hipMemcpyAsync(h_res, res.p, sizeof h_res, hipMemcpyDeviceToHost, c->stream));
  uint64_t at = kStHdr;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    VP_TRY(read_ctl(c, t));
    const Ctl &h = t.h_ctl;
    if (h.exp_count != h.n_live || h.n_live > t.cap || h_res[2 * k] > h.stack_top ||
        h_res[2 * k + 1] > t.cap ||
        (uint64_t)h.n_live + h_res[2 * k] + (t.cap - h_res[2 * k + 1]) != t.cap)
      return state_fail("state save: table %d holds %u live of %u counted, %u freed, tail from %u "
                        "of %u", k, h.exp_count, h.n_live, h_res[2 * k], h_res[2 * k + 1], t.cap);
    sec[k] = Section{t.cap, h.n_live, h_res[2 * k + 1], kValSize[tabs[k].tt], h_res[2 * k]};
    section_layout(sec[k], at);
    at = sec[k].end;
  }
  const uint64_t total = at;
  *bytes = total;
  if (cap < total) return ST_BAD("state save: the image takes %llu bytes, the buffer holds %llu",
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
    const uint64_t ends[5] = {s.lru + 4ull * s.n_live, s.freed + 4ull * s.n_freed,
                              s.ts + 8ull * s.n_live, s.val, s.val + (uint64_t)s.vsz * s.n_live};
    Pads pads{};
    for (int a = 0; a < 5; a++) {
      pads.at[a] = d + ends[a];
      pads.n[a] = (uint32_t)(pad16(ends[a]) - ends[a]);
    }
    VP_TRY(st_launch_gather(c, t, tabs[k].tt, idx, section_dev(s, d), pads));
  }
  VP_HIP(hipMemcpyAsync(buf, d, total, hipMemcpyDeviceToHost, c->stream));
  VP_HIP(hipStreamSynchronize(c->stream));
  // the headers
  memset(buf, 0, kStHdr);
  put32(buf, kStMagic);
  put32(buf + 4, kStVersion);
  put32(buf + 8, (uint32_t)c->kind);
  put32(buf + 12, (uint32_t)nt);
  put64(buf + 16, total);
  put64(buf + 24, (uint64_t)c->last_now);
  for (int k = 0; k < nt; k++) {
    uint8_t *h = buf + sec[k].lru - kStTblHdr;
    memset(h, 0, kStTblHdr);
    put32(h, sec[k].cap);
    put32(h + 4, sec[k].n_live);
    put32(h + 8, sec[k].fresh);
    put32(h + 12, sec[k].vsz);
    put32(h + 16, sec[k].n_freed);
  }
  return 0;
}

const char *err_text(uint32_t code) {
  switch (code) {
    case E_LRU_RANGE: return "lru[%u] is not below the capacity";
    case E_FREED_RANGE: return "freed[%u] is not below the capacity";
    case E_LRU_TAIL: return "lru[%u] lies in the never-used tail";
    case E_FREED_TAIL: return "freed[%u] lies in the never-used tail";
    case E_LRU_TWICE: return "lru[%u] names an index that is named twice";
    case E_FREED_TWICE: return "freed[%u] names an index that is named twice";
    case E_FREED_NORM: return "freed[%u] is fresh_next - 1: the tail is not normalised";
    case E_TS_NEG: return "ts[%u] is negative";
    case E_TS_FUTURE: return "ts[%u] is later than last_now";
    case E_TS_ORDER: return "ts[%u] is earlier than the entry before it";
    case E_KEY_PAD: return "key[%u] has a non-zero pad byte";
    case E_VAL_RANGE: return "value[%u] is out of range";
    case E_KEY_TWICE: return "key[%u] occurs twice";
    default: return "entry %u";
  }
}
int image_fail(int k, uint32_t tt, unsigned long long e) {
  char what[96];
  snprintf(what, sizeof what, err_text((uint32_t)(e >> 32)), (uint32_t)e);
  return ST_BAD("state load: table %d (%s): %s", k, kTblName[tt], what);
}

// The arrays of a table built aside, freed unless they were swapped in.
struct Aside {
  Bucket *bk = nullptr;
  uint32_t *slot_of = nullptr, *hash_of = nullptr;
  Ctl *ctl = nullptr;
  uint64_t nb = 0;
  ~Aside() {
    hipFree(bk);
    hipFree(slot_of);
    hipFree(hash_of);
    hipFree(ctl);
  }
};

int state_load(vp_ctx *c, const uint8_t *buf, uint64_t bytes) {
  StTable tabs[2];
  int nt = 0;
  VP_TRY(st_enter(c, tabs, &nt));
  // ---- the host's checks: nothing is uploaded before they pass
  if (bytes < kStHdr) return ST_BAD("state load: %llu bytes hold no header", (unsigned long long)bytes);
  if (get32(buf) != kStMagic) return ST_BAD("state load: magic 0x%08x", get32(buf));
  if (get32(buf + 4) != kStVersion) return ST_BAD("state load: version %u", get32(buf + 4));
  if (get32(buf + 8) != (uint32_t)c->kind)
    return ST_BAD("state load: kind %u into a context of kind %d", get32(buf + 8), c->kind);
  if (get32(buf + 12) != (uint32_t)nt)
    return ST_BAD("state load: n_tables %u, this NF has %d", get32(buf + 12), nt);
  if (get64(buf + 16) != bytes)
    return ST_BAD("state load: total_bytes %llu, %llu given", (unsigned long long)get64(buf + 16),
                  (unsigned long long)bytes);
  const int64_t last_now = (int64_t)get64(buf + 24);
  if (last_now < -1) return ST_BAD("state load: last_now %lld", (long long)last_now);
  Section sec[2];
  uint64_t at = kStHdr;
  for (int k = 0; k < nt; k++) {
    const FlowTable &t = *tabs[k].t;
    if (bytes - at < kStTblHdr) return ST_BAD("state load: table %d: header past the end", k);
    const uint8_t *h = buf + at;
    Section &s = sec[k];
    s = Section{get32(h), get32(h + 4), get32(h + 8), get32(h + 12), get32(h + 16)};
    if (s.cap != t.cap) return ST_BAD("state load: table %d: capacity %u, the context's is %u", k, s.cap, t.cap);
    if (s.n_live > s.cap) return ST_BAD("state load: table %d: n_live %u above the capacity", k, s.n_live);
    if (s.fresh > s.cap) return ST_BAD("state load: table %d: fresh_next %u above the capacity", k, s.fresh);
    if (s.vsz != kValSize[tabs[k].tt]) return ST_BAD("state load: table %d: value size %u", k, s.vsz);
    if (s.n_freed > s.cap || (uint64_t)s.n_live + s.n_freed + (s.cap - s.fresh) != s.cap)
      return ST_BAD("state load: table %d: n_live %u + n_freed %u + tail %u is not the capacity %u",
                    k, s.n_live, s.n_freed, s.cap - s.fresh, s.cap);
    if (get32(h + 20) | get32(h + 24) | get32(h + 28))
      return ST_BAD("state load: table %d: reserved header word not zero", k);
    section_layout(s, at);
    if (s.end > bytes) return ST_BAD("state load: table %d: arrays end at %llu of %llu bytes", k,
                                     (unsigned long long)s.end, (unsigned long long)bytes);
    const uint64_t ends[5] = {s.lru + 4ull * s.n_live, s.freed + 4ull * s.n_freed,
                              s.ts + 8ull * s.n_live, s.val, s.val + (uint64_t)s.vsz * s.n_live};
    for (uint64_t e : ends)
      for (uint64_t b = e; b < pad16(e); b++)
        if (buf[b]) return ST_BAD("state load: table %d: pad byte at %llu not zero", k, (unsigned long long)b);
    at = s.end;
  }
  if (at != bytes) return ST_BAD("state load: %llu bytes behind the last table",
                                 (unsigned long long)(bytes - at));
  // ---- upload, then the device's checks of the image's contents
  DevBuf img, scratch;
  VP_TRY(dalloc((uint8_t **)&img.p, bytes));
  uint8_t *d = (uint8_t *)img.p;
  VP_HIP(hipMemcpyAsync(d, buf, bytes, hipMemcpyHostToDevice, c->stream));
  uint64_t words[2], woff = 2 * 2;  // (err words first, 64 bits each)
  for (int k = 0; k < nt; k++) {
    words[k] = woff;
    woff += (sec[k].cap + 31) / 32;
  }
  VP_TRY(dalloc((uint32_t **)&scratch.p, woff));
  uint32_t *sw = (uint32_t *)scratch.p;
  unsigned long long *err = (unsigned long long *)scratch.p, h_err[2] = {~0ull, ~0ull};
  VP_HIP(hipMemsetAsync(sw, 0, 4 * woff, c->stream));
  VP_HIP(hipMemsetAsync(err, 0xFF, 16, c->stream));
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    const uint32_t tt = tabs[k].tt;
    const uint32_t vmax = value_bound(c, tt);
    st_check<<<grid_for(std::max({s.n_live, s.n_freed, 1u})), 256, 0, c->stream>>>(
        section_dev(s, d), tt, s.cap, last_now, vmax, sw + words[k], err + k);
    VP_HIP(hipGetLastError());
  }
  VP_HIP(hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, c->stream));
  VP_HIP(hipStreamSynchronize(c->stream));
  for (int k = 0; k < nt; k++)
    if (h_err[k] != ~0ull) return image_fail(k, tabs[k].tt, h_err[k]);
  // ---- the bucket arrays aside, and every key looked up in them
  Aside as[2];
  TableDev nd[2];
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    Aside &a = as[k];
    a.nb = t.nb_nominal;
    while (a.nb * kBucketEntries * 85 / 100 < sec[k].n_live) a.nb <<= 1;
    VP_TRY(dalloc(&a.bk, a.nb));
    VP_TRY(dalloc(&a.slot_of, t.cap));
    VP_TRY(dalloc(&a.hash_of, t.cap));
    VP_TRY(dalloc(&a.ctl, 1));
    VP_HIP(hipMemsetAsync(a.bk, 0xFF, sizeof(Bucket) * a.nb, c->stream));
    VP_HIP(hipMemsetAsync(a.slot_of, 0xFF, 4ull * t.cap, c->stream));
    VP_HIP(hipMemsetAsync(a.ctl, 0, sizeof(Ctl), c->stream));
    nd[k] = tbl_dev(t);
    nd[k].bk = a.bk;
    nd[k].bmask = (uint32_t)(a.nb - 1);
    nd[k].mix = tbl_initial_mix();
    nd[k].lin = nullptr;
    nd[k].slot_of = a.slot_of;
    nd[k].hash_of = a.hash_of;
    nd[k].ctl = a.ctl;
    const uint32_t g = grid_for(std::max(sec[k].n_live, 1u));
    st_insert<<<g, 256, 0, c->stream>>>(nd[k], tabs[k].tt, section_dev(sec[k], d));
    st_dup<<<g, 256, 0, c->stream>>>(nd[k], tabs[k].tt, section_dev(sec[k], d), err + k);
    VP_HIP(hipGetLastError());
  }
  VP_HIP(hipMemcpyAsync(h_err, err, 16, hipMemcpyDeviceToHost, c->stream));
  VP_HIP(hipStreamSynchronize(c->stream));
  for (int k = 0; k < nt; k++)
    if (h_err[k] != ~0ull) return image_fail(k, tabs[k].tt, h_err[k]);
  // ---- apply: from here on the context's state is the image's
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    st_commit<<<grid_for(std::max({s.n_live, s.n_freed, 1u})), 256, 0, c->stream>>>(
        nd[k], tabs[k].tt, SideVals{c->be_rec, c->pol_size, c->pol_time}, section_dev(s, d));
    VP_HIP(hipGetLastError());
  }
  VP_HIP(hipStreamSynchronize(c->stream));
  uint32_t most = 0;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    Aside &a = as[k];
    std::swap(t.bk, a.bk);  // (the old arrays go with `as`)
    std::swap(t.slot_of, a.slot_of);
    std::swap(t.hash_of, a.hash_of);
    std::swap(t.ctl, a.ctl);
    t.bmask = nd[k].bmask;
    t.mix = nd[k].mix;
    t.lin_tried = false;
    t.layout_tries = 0;
    t.ins_since = sec[k].n_live;
    t.rebuilds++;
    t.ts_floor = sec[k].n_live ? get64(buf + sec[k].ts) : UINT64_MAX;
    t.fs_hint = 0;
    t.runs_seen = true;
    t.last_run_tiles = 0;
    t.ctl_clean = false;
    t.jr_on = false;
    most = std::max(most, sec[k].n_live);
  }
  c->jr_want = false;
  c->last_now = last_now;
  c->seq = (uint64_t)most + 1;  // (past every tseq: the LRU ranks 0 .. n_live - 1)
  c->fold_pending = false;
  c->st_epoch++;  // (the sequence restarted: marks taken before name nothing now)
  c->st_following = false;
  for (int k = 0; k < nt; k++) VP_TRY(tbl_layout_check(c, *tabs[k].t));
  return 0;
}

}  // namespace
}  // namespace vp

int vp_state_size(vp_ctx *c, uint64_t *bytes) {
  if (!c || !bytes) return VP_EINVAL;
  return vp::state_save(c, nullptr, 0, bytes, true);
}

int vp_state_save(vp_ctx *c, void *buf, uint64_t cap, uint64_t *bytes) {
  if (!c || !bytes || (!buf && cap)) return VP_EINVAL;
  return vp::state_save(c, (uint8_t *)buf, cap, bytes, false);
}

int vp_state_load(vp_ctx *c, const void *buf, uint64_t bytes) {
  if (!c || !buf) return VP_EINVAL;
  return vp::state_load(c, (const uint8_t *)buf, bytes);
}
