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

// Reads the image only. bitmap: one bit per index, zero on entry; vmax: the
// first value out of range (0: any). A key is looked at by st_dup.
struct StCheck {
  uint32_t *bm_idx, *bm_freed;
  __device__ __forceinline__ void key(uint32_t, uint4, unsigned long long *) const {}
};
__global__ __launch_bounds__(256) void st_check(ImgDev im, uint32_t tt, uint32_t cap,
                                                int64_t last_now, uint32_t vmax,
                                                uint32_t *bitmap, unsigned long long *err) {
  img_check(im, tt, cap, last_now, vmax, err, StCheck{bitmap, bitmap},
            blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
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
    if (found != i) img_fail(err, E_KEY_TWICE, j);
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
      side_put(tt, sv, i, im, j);
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

int st_replaced(vp_ctx *c, StTable tabs[2], int nt, const uint64_t floor[2], int64_t last_now) {
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    t.ts_floor = floor[k];
    t.fs_hint = 0;
    t.runs_seen = true;
    t.last_run_tiles = 0;
    t.ctl_clean = false;
    t.jr_on = false;
  }
  c->jr_want = false;
  c->last_now = last_now;
  c->fold_pending = false;
  for (int k = 0; k < nt; k++) VP_TRY(tbl_layout_check(c, *tabs[k].t));
  return 0;
}

int st_size_bound(vp_ctx *c, StTable tabs[2], int nt, uint32_t hdr, uint64_t *bytes) {
  uint64_t at = hdr;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    VP_TRY(read_ctl(c, t));
    const uint32_t n = t.h_ctl.n_live;
    at = section_at(at, t.cap, n, 0, tabs[k].tt, t.h_ctl.stack_top, n).end;
  }
  *bytes = at;
  return 0;
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
  if (size_only) return st_size_bound(c, tabs, nt, kImage.hdr, bytes);
  Section sec[2];
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
  uint64_t at = kImage.hdr;
  for (int k = 0; k < nt; k++) {
    FlowTable &t = *tabs[k].t;
    VP_TRY(read_ctl(c, t));
    const Ctl &h = t.h_ctl;
    if (h.exp_count != h.n_live || h.n_live > t.cap || h_res[2 * k] > h.stack_top ||
        h_res[2 * k + 1] > t.cap ||
        (uint64_t)h.n_live + h_res[2 * k] + (t.cap - h_res[2 * k + 1]) != t.cap)
      return state_fail("state save: table %d holds %u live of %u counted, %u freed, tail from %u "
                        "of %u", k, h.exp_count, h.n_live, h_res[2 * k], h_res[2 * k + 1], t.cap);
    sec[k] = section_at(at, t.cap, h.n_live, h_res[2 * k + 1], tabs[k].tt, h_res[2 * k], h.n_live);
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
    VP_TRY(st_launch_gather(c, t, tabs[k].tt, idx, section_dev(s, d), section_pads(s, d)));
  }
  VP_HIP(hipMemcpyAsync(buf, d, total, hipMemcpyDeviceToHost, c->stream));
  VP_HIP(hipStreamSynchronize(c->stream));
  // the headers
  put_header(kImage, buf, c->kind, nt, total, c->last_now);
  for (int k = 0; k < nt; k++) put_table_header(kImage, buf, sec[k]);
  return 0;
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
  const Expect want = st_expect(c, tabs, nt);
  char msg[256];
  int64_t last_now;
  if (!read_header(kImage, want, buf, bytes, &last_now, msg, sizeof msg)) return ST_BAD("%s", msg);
  Section sec[2];
  if (!read_sections(kImage, want, buf, bytes, sec, msg, sizeof msg)) return ST_BAD("%s", msg);
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
    if (h_err[k] != ~0ull) return img_refuse(kImage.who, "lru", k, tabs[k].tt, h_err[k]);
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
    if (h_err[k] != ~0ull) return img_refuse(kImage.who, "lru", k, tabs[k].tt, h_err[k]);
  // ---- apply: from here on the context's state is the image's
  for (int k = 0; k < nt; k++) {
    const Section &s = sec[k];
    st_commit<<<grid_for(std::max({s.n_live, s.n_freed, 1u})), 256, 0, c->stream>>>(
        nd[k], tabs[k].tt, SideVals{c->be_rec, c->pol_size, c->pol_time}, section_dev(s, d));
    VP_HIP(hipGetLastError());
  }
  VP_HIP(hipStreamSynchronize(c->stream));
  uint32_t most = 0;
  uint64_t floor[2];
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
    floor[k] = sec[k].n_live ? get64(buf + sec[k].ts) : UINT64_MAX;
    most = std::max(most, sec[k].n_live);
  }
  c->seq = (uint64_t)most + 1;  // (past every tseq: the LRU ranks 0 .. n_live - 1)
  c->st_epoch++;  // (the sequence restarted: marks taken before name nothing now)
  c->st_following = false;
  return st_replaced(c, tabs, nt, floor, last_now);
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
