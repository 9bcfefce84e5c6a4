// What the state images (vp_state.hip) and the incremental
// ones (vp_statedelta.hip, §5.15) share: the table types and their values, an
// image's arrays on the device and their layout in the bytes, the key masks
// and hashes, and the launchers of the save path's free-list writer and
// gather, whose kernels stay in vp_state.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

#include "vp_table.h"

namespace vp {
namespace stimg {

// What a table keeps per index beside the stamps (the image's key and value).
enum TblType : uint32_t { TT_NAT, TT_BRIDGE, TT_FW, TT_LBFLOW, TT_LBBACK, TT_POL };
inline constexpr uint32_t kValSize[6] = {0, 4, 4, 4, 8, 16};
inline constexpr const char *kTblName[6] = {"flows", "MACs", "flows", "flows", "backends",
                                            "destinations"};
constexpr uint32_t kStTblHdr = 32;

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

// The entry's key words from the image's key and value.
__device__ __forceinline__ uint4 raw_key(uint32_t tt, const ImgDev &im, uint32_t j) {
  uint4 k = im.key[j];
  if (tt == TT_BRIDGE) k.z = reinterpret_cast<const uint32_t *>(im.val)[j];
  if (tt == TT_FW || tt == TT_LBFLOW) k.w |= reinterpret_cast<const uint32_t *>(im.val)[j] << 8;
  return k;
}

// The first value out of range of a table's u32 values (0: any; st_check).
inline uint32_t value_bound(const vp_ctx *c, uint32_t tt) {
  return tt == TT_BRIDGE || tt == TT_FW ? 0x10000u : tt == TT_LBFLOW ? c->ft2.cap : 0u;
}

struct StTable {
  FlowTable *t;
  uint32_t tt;
};

inline uint64_t pad16(uint64_t v) { return (v + 15) & ~15ull; }

// One table's arrays in an image: offsets from the image's first byte, the
// table header at lru - kStTblHdr (a delta: n_live = n_new).
struct Section {
  uint32_t cap, n_live, fresh, vsz, n_freed;
  uint64_t lru, freed, ts, key, val, end;
};
inline void section_layout(Section &s, uint64_t at) {
  s.lru = at + kStTblHdr;
  s.freed = s.lru + pad16(4ull * s.n_live);
  s.ts = s.freed + pad16(4ull * s.n_freed);
  s.key = s.ts + pad16(8ull * s.n_live);
  s.val = s.key + 16ull * s.n_live;
  s.end = s.val + pad16((uint64_t)s.vsz * s.n_live);
}
inline ImgDev section_dev(const Section &s, uint8_t *img) {
  return ImgDev{reinterpret_cast<uint32_t *>(img + s.lru), reinterpret_cast<uint32_t *>(img + s.freed),
                reinterpret_cast<int64_t *>(img + s.ts), reinterpret_cast<uint4 *>(img + s.key),
                img + s.val, s.n_live, s.n_freed, s.fresh};
}
// Where each array ends and its pad begins.
inline void section_ends(const Section &s, uint64_t ends[5]) {
  ends[0] = s.lru + 4ull * s.n_live;
  ends[1] = s.freed + 4ull * s.n_freed;
  ends[2] = s.ts + 8ull * s.n_live;
  ends[3] = s.val;
  ends[4] = s.val + (uint64_t)s.vsz * s.n_live;
}

struct DevBuf {  // freed on every way out
  void *p = nullptr;
  ~DevBuf() { hipFree(p); }
};

inline void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
inline uint32_t get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

}  // namespace stimg

// VP_EINVAL with its reason in vp_last_error().
#define ST_BAD(...) (state_fail(__VA_ARGS__), VP_EINVAL)

// vp_state.hip. Every state call's start: the resident kernel stopped, a
// pending timestamp fold waited for, no communicator attached; the NF's
// tables in image order.
int st_enter(vp_ctx *c, stimg::StTable tabs[2], int *ntabs);
// The NF's tables in image order and their number, nothing stopped or
// waited for (0: a context of no known kind).
int st_tables(vp_ctx *c, stimg::StTable out[2]);
// st_freed: the free list in hand-out order with the never-used tail
// normalised into freed[] (room for stack_top entries), res = {n_freed, the
// normalised fresh_next}. Queued on c->stream.
int st_launch_freed(vp_ctx *c, FlowTable &t, uint32_t *freed, uint32_t *res);
// st_gather: the image's arrays of the im.n_live indices idx[], which it
// writes coalesced, and the zero pads. Queued on c->stream.
int st_launch_gather(vp_ctx *c, FlowTable &t, uint32_t tt, const uint32_t *idx,
                     const stimg::ImgDev &im, const stimg::Pads &pads);

}  // namespace vp
