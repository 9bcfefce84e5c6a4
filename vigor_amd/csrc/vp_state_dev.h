// What the state images (vp_state.hip) and the incremental
// ones (vp_statedelta.hip, §5.15) share beside the bytes' layout and reader
// (vp_state_img.h): an image's arrays on the device, the key masks and
// hashes, the check of those arrays with its error table (§5.16.1), what a
// context forgets when its tables are replaced, and the launchers of the save
// path's free-list writer and gather, whose kernels stay in vp_state.hip.
// Also what the lookups and the erase (vp_lookup.hip, vp_erase.hip; §5.16,
// §5.17) share: a query's answer arrays and their writer, and the calls' start.
#pragma once

#include <hip/hip_runtime.h>

#include "vp_state_img.h"
#include "vp_table.h"

namespace vp {
namespace stimg {

inline constexpr const char *kTblName[6] = {"flows", "MACs", "flows", "flows", "backends",
                                            "destinations"};

// The per-index arrays outside the buckets (viglb backends[], vigpol dyn_vals).
struct SideVals {
  uint4 *be_rec;
  uint64_t *pol_size;
  int64_t *pol_time;
};

// One table's arrays inside an image on the device (a delta's new[]: lru =
// idx[], n_live = n_new).
struct ImgDev {
  uint32_t *lru, *freed;
  int64_t *ts;
  uint4 *key;
  uint8_t *val;
  uint32_t n_live, n_freed, fresh;
};

// The pad bytes behind each array (from, count), zeroed by the gather.
struct Pads {
  uint8_t *at[5];
  uint32_t n[5];
};

template <class T>
int dalloc(T **p, size_t count) {
  if (count == 0) count = 1;
  hipError_t e = hipMalloc((void **)p, sizeof(T) * count);
  return e == hipSuccess ? 0 : hip_fail(e, "hipMalloc", __FILE__, __LINE__);
}

// The bits of a bucket entry's key words that are the libVig key; the others
// carry the entry's value (vigbridge: word 2 the port; vigfw, viglb flows:
// word 3 above the protocol byte) or are zero.
__host__ __device__ __forceinline__ uint4 key_mask(uint32_t tt) {
  switch (tt) {
    case TT_NAT: return make_uint4(~0u, ~0u, ~0u, ~0u);
    case TT_BRIDGE: return make_uint4(~0u, 0xFFFFu, 0u, 0u);
    case TT_FW:
    case TT_LBFLOW: return make_uint4(~0u, ~0u, ~0u, 0xFFu);
    default: return make_uint4(~0u, 0u, 0u, 0u);
  }
}
__device__ __forceinline__ uint4 and4(uint4 a, uint4 m) {
  return make_uint4(a.x & m.x, a.y & m.y, a.z & m.z, a.w & m.w);
}
__device__ __forceinline__ bool any4(uint4 a) { return (a.x | a.y | a.z | a.w) != 0; }
__device__ __forceinline__ bool eq4(uint4 a, uint4 b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

// The NF's own key hash of an image key (the generated *_hash functions the
// classify kernels evaluate through position tables: vp_nat.hip flowid_hash,
// vp_fw.hip fw_hash, vp_lb.hip lbflow_hash / ip_hash, vp_bridge.hip eth_hash,
// vp_pol.hip pol_hash), as the chain of crc32c_u32 steps it is.
__device__ __forceinline__ uint32_t key_hash(uint32_t tt, uint4 k) {
  uint32_t h = 0;
  switch (tt) {
    case TT_NAT:  // src_port, dst_port, src_ip, dst_ip, internal_device, protocol
      h = crc32c_u32(h, k.x & 0xFFFFu);
      h = crc32c_u32(h, k.x >> 16);
      h = crc32c_u32(h, k.y);
      h = crc32c_u32(h, k.z);
      h = crc32c_u32(h, k.w & 0xFFFFu);
      h = crc32c_u32(h, (k.w >> 16) & 0xFFu);
      break;
    case TT_FW:  // src_port, dst_port, src_ip, dst_ip, protocol
      h = crc32c_u32(h, k.x & 0xFFFFu);
      h = crc32c_u32(h, k.x >> 16);
      h = crc32c_u32(h, k.y);
      h = crc32c_u32(h, k.z);
      h = crc32c_u32(h, k.w & 0xFFu);
      break;
    case TT_LBFLOW:  // src_ip, dst_ip, src_port, dst_port, protocol
      h = crc32c_u32(h, k.x);
      h = crc32c_u32(h, k.y);
      h = crc32c_u32(h, k.z & 0xFFFFu);
      h = crc32c_u32(h, k.z >> 16);
      h = crc32c_u32(h, k.w & 0xFFu);
      break;
    case TT_BRIDGE:  // rte_ether_addr_hash: one step per address byte
      for (uint32_t b = 0; b < 4; b++) h = crc32c_u32(h, (k.x >> (8 * b)) & 0xFFu);
      h = crc32c_u32(h, k.y & 0xFFu);
      h = crc32c_u32(h, (k.y >> 8) & 0xFFu);
      break;
    default:  // ip_addr_hash
      h = crc32c_u32(h, k.x);
      break;
  }
  return h;
}

// What the image says of one live index: its stamp, its key and its value
// (the first kValSize[tt] bytes of val, the rest zero). One reader for the
// save's gather and the lookups (vp_lookup.hip).
struct Entry {
  int64_t ts;
  uint4 key, val;
};
// raw: the key words of index i's bucket entry (tbl_key_of, or the entry a
// probe stopped at).
__device__ __forceinline__ Entry entry_of(const TableDev &t, uint32_t tt, const SideVals &sv,
                                          uint32_t i, uint4 raw) {
  Entry e{(int64_t)t.ts[i], and4(raw, key_mask(tt)), make_uint4(0u, 0u, 0u, 0u)};
  if (tt == TT_BRIDGE) {
    e.val.x = raw.z;
  } else if (tt == TT_FW || tt == TT_LBFLOW) {
    e.val.x = raw.w >> 8;
  } else if (tt == TT_LBBACK) {
    const uint4 r = sv.be_rec[i];  // {ip, mac 0-3, mac 4-5 | nic << 16, 0}
    e.val.x = r.y;
    e.val.y = r.z;
  } else if (tt == TT_POL) {
    const uint64_t s = sv.pol_size[i], b = (uint64_t)sv.pol_time[i];
    e.val = make_uint4((uint32_t)s, (uint32_t)(s >> 32), (uint32_t)b, (uint32_t)(b >> 32));
  }
  return e;
}
// Entry j of a value array: kValSize[tt] bytes of v (vignat: nothing).
__device__ __forceinline__ void value_put(uint32_t tt, uint8_t *val, uint32_t j, uint4 v) {
  if (tt == TT_BRIDGE || tt == TT_FW || tt == TT_LBFLOW) {
    reinterpret_cast<uint32_t *>(val)[j] = v.x;
  } else if (tt == TT_LBBACK) {
    reinterpret_cast<uint2 *>(val)[j] = make_uint2(v.x, v.y);
  } else if (tt == TT_POL) {
    reinterpret_cast<uint4 *>(val)[j] = v;
  }
}

// vp_lookup_out as the lookup and erase kernels take it (vp_lookup.hip,
// vp_erase.hip); any pointer may be null.
struct LkOut {
  uint32_t *index;
  int64_t *ts;
  uint4 *key;
  uint8_t *value;
};
// out as the kernels' argument (null: nothing is wanted; a table without a
// value never has its value pointer looked at).
inline LkOut lk_out(const vp_lookup_out *out, uint32_t tt) {
  if (!out) return LkOut{nullptr, nullptr, nullptr, nullptr};
  return LkOut{out->index, out->ts, reinterpret_cast<uint4 *>(out->key),
               kValSize[tt] ? out->value : nullptr};
}
// Query q's answer: index i with the entry words raw, or a miss (i == kNone).
__device__ __forceinline__ void lk_put(const TableDev &t, uint32_t tt, const SideVals &sv,
                                       const LkOut &o, uint32_t q, uint32_t i, uint4 raw) {
  Entry e{0, make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
  if (i != kNone) e = entry_of(t, tt, sv, i, raw);
  if (o.index) o.index[q] = i;
  if (o.ts) o.ts[q] = e.ts;
  if (o.key) o.key[q] = e.key;
  if (o.value) value_put(tt, o.value, q, e.val);
}

// The entry's key words from the image's key and value.
__device__ __forceinline__ uint4 raw_key(uint32_t tt, const ImgDev &im, uint32_t j) {
  uint4 k = im.key[j];
  if (tt == TT_BRIDGE) k.z = reinterpret_cast<const uint32_t *>(im.val)[j];
  if (tt == TT_FW || tt == TT_LBFLOW) k.w |= reinterpret_cast<const uint32_t *>(im.val)[j] << 8;
  return k;
}

// Index i's values in the arrays outside the buckets from entry j of an image.
__device__ __forceinline__ void side_put(uint32_t tt, const SideVals &sv, uint32_t i,
                                         const ImgDev &im, uint32_t j) {
  if (tt == TT_LBBACK) {
    const uint2 v = reinterpret_cast<const uint2 *>(im.val)[j];
    sv.be_rec[i] = make_uint4(im.key[j].x, v.x, v.y, 0u);
  } else if (tt == TT_POL) {
    const uint4 v = reinterpret_cast<const uint4 *>(im.val)[j];
    sv.pol_size[i] = (uint64_t)v.x | ((uint64_t)v.y << 32);
    sv.pol_time[i] = (int64_t)((uint64_t)v.z | ((uint64_t)v.w << 32));
  }
}

// The first value out of range of a table's u32 values (0: any; st_check).
inline uint32_t value_bound(const vp_ctx *c, uint32_t tt) {
  return tt == TT_BRIDGE || tt == TT_FW ? 0x10000u : tt == TT_LBFLOW ? c->ft2.cap : 0u;
}

struct StTable {
  FlowTable *t;
  uint32_t tt;
};

inline ImgDev section_dev(const Section &s, uint8_t *img) {
  return ImgDev{reinterpret_cast<uint32_t *>(img + s.lru), reinterpret_cast<uint32_t *>(img + s.freed),
                reinterpret_cast<int64_t *>(img + s.ts), reinterpret_cast<uint4 *>(img + s.key),
                img + s.val, s.n_live, s.n_freed, s.fresh};
}
struct DevBuf {  // freed on every way out
  void *p = nullptr;
  ~DevBuf() { hipFree(p); }
};

// The pads behind the arrays of a section of the device's image at d.
inline Pads section_pads(const Section &s, uint8_t *d) {
  uint64_t ends[5];
  section_ends(s, ends);
  Pads pads{};
  for (int a = 0; a < 5; a++) {
    pads.at[a] = d + ends[a];
    pads.n[a] = (uint32_t)(pad16(ends[a]) - ends[a]);
  }
  return pads;
}

// ------------------------------------------------ the check of the arrays --

// What the check kernels report: code << 32 | position through atomicMin, so
// of two faults the one with the lower code is reported, and of two of one
// code the first. The order is part of the interface (E_BOTH to E_NOT_KEPT:
// a delta's only).
enum ImgErr : uint32_t {
  E_IDX_RANGE = 1, E_FREED_RANGE, E_IDX_TAIL, E_FREED_TAIL, E_IDX_TWICE, E_FREED_TWICE,
  E_FREED_NORM, E_BOTH, E_TS_NEG, E_TS_FUTURE, E_TS_ORDER, E_KEY_PAD, E_VAL_RANGE, E_KEY_TWICE,
  E_KEY_KEPT, E_NOT_KEPT
};
__device__ __forceinline__ void img_fail(unsigned long long *err, uint32_t code, uint32_t j) {
  atomicMin(err, ((unsigned long long)code << 32) | j);
}
// Sets index i's bit; whether it was set.
__device__ __forceinline__ bool bit_claim(uint32_t *bm, uint32_t i) {
  return atomicOr(&bm[i >> 5], 1u << (i & 31)) & (1u << (i & 31));
}

// The body of st_check and sd_check: reads the arrays only (a delta: new[],
// n_live = n_new). Every index below cap, outside the never-used tail and
// named once in its bitmap (p.bm_idx for lru[] / idx[], p.bm_freed for
// freed[]: one bit per index, zero on entry; an image gives one bitmap for
// both), the tail normalised, the stamps in order and within 0 .. last_now,
// the key's pad bits zero, a u32 value below vmax (0: any); then p.key(j, k,
// err) for what the unit has to say of a key. j0, step: the thread's grid
// stride, which the kernel works out (there the compiler reads blockDim as
// the uniform block size; in a device function it did not, at two VGPRs).
template <class P>
__device__ __forceinline__ void img_check(const ImgDev &im, uint32_t tt, uint32_t cap,
                                          int64_t last_now, uint32_t vmax,
                                          unsigned long long *err, const P &p, uint32_t j0,
                                          uint32_t step) {
  const uint4 mask = key_mask(tt);
  const uint32_t n = max(im.n_live, im.n_freed);
  for (uint32_t j = j0; j < n; j += step) {
    if (j < im.n_live) {
      const uint32_t i = im.lru[j];
      if (i >= cap) {
        img_fail(err, E_IDX_RANGE, j);
      } else {
        if (i >= im.fresh) img_fail(err, E_IDX_TAIL, j);
        if (bit_claim(p.bm_idx, i)) img_fail(err, E_IDX_TWICE, j);
      }
      const int64_t ts = im.ts[j];
      if (ts < 0) img_fail(err, E_TS_NEG, j);
      if (ts > last_now) img_fail(err, E_TS_FUTURE, j);
      if (j > 0 && im.ts[j - 1] > ts) img_fail(err, E_TS_ORDER, j);
      const uint4 k = im.key[j];
      if (any4(make_uint4(k.x & ~mask.x, k.y & ~mask.y, k.z & ~mask.z, k.w & ~mask.w)))
        img_fail(err, E_KEY_PAD, j);
      if (vmax && reinterpret_cast<const uint32_t *>(im.val)[j] >= vmax)
        img_fail(err, E_VAL_RANGE, j);
      p.key(j, k, err);
    }
    if (j < im.n_freed) {
      const uint32_t i = im.freed[j];
      if (i >= cap) {
        img_fail(err, E_FREED_RANGE, j);
      } else {
        if (i >= im.fresh) img_fail(err, E_FREED_TAIL, j);
        if (bit_claim(p.bm_freed, i)) img_fail(err, E_FREED_TWICE, j);
      }
      if (j == im.n_freed - 1 && i + 1 == im.fresh) img_fail(err, E_FREED_NORM, j);
    }
  }
}

// A code's text as a format of (the position, what the unit calls the index
// array: "lru", "idx").
inline const char *err_format(uint32_t code) {
  static const char *const text[] = {
      "entry %1$u",
      "%2$s[%1$u] is not below the capacity", "freed[%1$u] is not below the capacity",
      "%2$s[%1$u] lies in the never-used tail", "freed[%1$u] lies in the never-used tail",
      "%2$s[%1$u] names an index that is named twice",
      "freed[%1$u] names an index that is named twice",
      "freed[%1$u] is fresh_next - 1: the tail is not normalised",
      "index %1$u is named in %2$s[] and in freed[]",
      "ts[%1$u] is negative", "ts[%1$u] is later than last_now",
      "ts[%1$u] is earlier than the entry before it",
      "key[%1$u] has a non-zero pad byte", "value[%1$u] is out of range",
      "key[%1$u] occurs twice", "key[%1$u] is held by a kept entry at another index",
      "index %1$u is neither free nor new nor live here: the kept entries and n_new are not "
      "n_live"};
  return text[code <= E_NOT_KEPT ? code : 0];
}

}  // namespace stimg

// VP_EINVAL with its reason in vp_last_error().
#define ST_BAD(...) (state_fail(__VA_ARGS__), VP_EINVAL)

// A check kernel's error word e for table k as who's refusal.
inline int img_refuse(const char *who, const char *idx, int k, uint32_t tt, unsigned long long e) {
  char what[128];
  snprintf(what, sizeof what, stimg::err_format((uint32_t)(e >> 32)), (uint32_t)e, idx);
  return ST_BAD("%s: table %d (%s): %s", who, k, stimg::kTblName[tt], what);
}
// What the context expects of an image or a delta (vp_state_img.h).
inline stimg::Expect st_expect(const vp_ctx *c, const stimg::StTable tabs[2], int nt) {
  stimg::Expect x{c->kind, nt, {}, {}};
  for (int k = 0; k < nt; k++) {
    x.cap[k] = tabs[k].t->cap;
    x.tt[k] = tabs[k].tt;
  }
  return x;
}

// vp_state.hip. Every state call's start: the resident kernel stopped, a
// pending timestamp fold waited for, no communicator attached; the NF's
// tables in image order.
int st_enter(vp_ctx *c, stimg::StTable tabs[2], int *ntabs);
// The NF's tables in image order and their number, nothing stopped or
// waited for (0: a context of no known kind).
int st_tables(vp_ctx *c, stimg::StTable out[2]);
// An upper bound of an image's or a delta's size (hdr: its common header's):
// every live index in the arrays, every stacked one freed.
int st_size_bound(vp_ctx *c, stimg::StTable tabs[2], int nt, uint32_t hdr, uint64_t *bytes);
// st_freed: the free list in hand-out order with the never-used tail
// normalised into freed[] (room for stack_top entries), res = {n_freed, the
// normalised fresh_next}. Queued on c->stream.
int st_launch_freed(vp_ctx *c, FlowTable &t, uint32_t *freed, uint32_t *res);
// st_gather: the image's arrays of the im.n_live indices idx[], which it
// writes coalesced, and the zero pads. Queued on c->stream.
int st_launch_gather(vp_ctx *c, FlowTable &t, uint32_t tt, const uint32_t *idx,
                     const stimg::ImgDev &im, const stimg::Pads &pads);
// The tables were replaced (a load) or rewritten (an apply): the context's
// clock, and everything the host remembers about the tables' contents, which
// now says nothing; then the layout's check. floor[k]: table k's least stamp
// (UINT64_MAX: no entry). A new per-table hint of FlowTable belongs here, so
// that neither caller can forget it. Moves no sequence number: each caller
// does that itself, before.
int st_replaced(vp_ctx *c, stimg::StTable tabs[2], int nt, const uint64_t floor[2],
                int64_t last_now);
// vp_lookup.hip. How a lookup or an erase call `fn` starts: the context, then
// st_enter, then the table, the input (keys: 16-byte aligned, idx: 4) and the
// output pointers' alignments; VP_EINVAL names the argument. need_out: a NULL
// out is refused. *tb: the table asked about.
int lk_enter(const char *fn, vp_ctx *c, int table, uint32_t n, const void *in, bool by_key,
             const vp_lookup_out *out, bool need_out, stimg::StTable *tb);

}  // namespace vp
