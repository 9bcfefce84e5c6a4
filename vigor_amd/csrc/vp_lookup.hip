// vp_table_lookup / vp_table_entries / vp_table_value_size (include/vigpath.h,
// DESIGN.md §5.16): a batch of read-only questions to a context's table --
// which index holds this key, what does this index hold -- answered on the
// device with the image's keys, stamps and values (§5.14) and nothing copied
// that was not asked for.
//
// One query per lane. lk_by_key hashes the 16-byte key as the NF does
// (key_hash) and walks the live bucket array with the table's own probe
// (tbl_probe_masked: tombstones passed over, any home-bucket layout);
// lk_by_index tests the index as the batch path does (below the capacity,
// slot_of[] set) and reads its entry through slot_of. Both take stamp, key
// and value from entry_of, the save's reader, and write each output array one
// entry per lane. The calls start as the state calls do (st_enter) and change
// nothing in the context or its tables. lk_enter, the checks of the arguments
// behind st_enter, is also how vp_table_erase / vp_table_free start
// (vp_erase.hip).
#include <hip/hip_runtime.h>

#include "vp_state_dev.h"

namespace vp {

VP_PRELOAD_UNIT(lookup)

using namespace stimg;

namespace {

static_assert(VP_LOOKUP_MISS == kNone, "a miss is the probe's kNone");

__global__ __launch_bounds__(256) void lk_by_key(TableDev t, uint32_t tt, SideVals sv,
                                                 const uint4 *keys, uint32_t n, LkOut o) {
  const uint4 mask = key_mask(tt);
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    const uint4 k = keys[q];
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    uint32_t i = kNone;
    // (a set pad byte: no entry holds these 16 bytes)
    if (!any4(make_uint4(k.x & ~mask.x, k.y & ~mask.y, k.z & ~mask.z, k.w & ~mask.w)))
      i = tbl_probe_masked(t, key_hash(tt, k), k, mask, &raw);
    lk_put(t, tt, sv, o, q, i, raw);
  }
}

__global__ __launch_bounds__(256) void lk_by_index(TableDev t, uint32_t tt, SideVals sv,
                                                   const uint32_t *idx, uint32_t n, LkOut o) {
  for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
    uint32_t i = idx[q];
    uint4 raw = make_uint4(0u, 0u, 0u, 0u);
    if (i < t.cap && t.slot_of[i] != kNone)
      raw = tbl_key_of(t, i);
    else
      i = kNone;
    lk_put(t, tt, sv, o, q, i, raw);
  }
}

bool aligned(const void *p, uint32_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Table `table` of the NF, or VP_EINVAL.
int lk_table(const char *fn, int table, const StTable tabs[2], int nt, StTable *out) {
  if (table < 0 || table >= nt)
    return ST_BAD("%s: table %d: this NF has table%s", fn, table, nt == 2 ? "s 0 and 1" : " 0 only");
  *out = tabs[table];
  return 0;
}

}  // namespace

int lk_enter(const char *fn, vp_ctx *c, int table, uint32_t n, const void *in, bool by_key,
             const vp_lookup_out *out, bool need_out, StTable *tb) {
  if (!c) return ST_BAD("%s: ctx is NULL", fn);
  if (need_out && !out) return ST_BAD("%s: out is NULL", fn);
  StTable tabs[2];
  int nt = 0;
  VP_TRY(st_enter(c, tabs, &nt));
  VP_TRY(lk_table(fn, table, tabs, nt, tb));
  const char *in_name = by_key ? "keys" : "idx";
  const uint32_t vsz = kValSize[tb->tt];
  if (n && !in) return ST_BAD("%s: %s is NULL with n = %u", fn, in_name, n);
  if (!aligned(in, by_key ? 16 : 4))
    return ST_BAD("%s: %s is not %d-byte aligned", fn, in_name, by_key ? 16 : 4);
  if (!out) return 0;
  if (!aligned(out->index, 4)) return ST_BAD("%s: out->index is not 4-byte aligned", fn);
  if (!aligned(out->ts, 8)) return ST_BAD("%s: out->ts is not 8-byte aligned", fn);
  if (!aligned(out->key, 16)) return ST_BAD("%s: out->key is not 16-byte aligned", fn);
  if (vsz && !aligned(out->value, vsz))  // (4, 8 or 16: the width of one entry's store)
    return ST_BAD("%s: out->value is not %u-byte aligned", fn, vsz);
  return 0;
}

namespace {

int table_query(const char *fn, vp_ctx *c, int table, uint32_t n, const void *in, bool by_key,
                const vp_lookup_out *out, void *stream) {
  StTable tb;
  VP_TRY(lk_enter(fn, c, table, n, in, by_key, out, true, &tb));
  if (n == 0) return 0;
  // A gather bound by latency: one dependent bucket read per lane, so as many
  // waves as the device holds at once and no more -- grid_for's 2048 blocks
  // are 8 blocks of 4 waves per CU, 8 waves per SIMD; more queries stride.
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const TableDev t = tbl_dev(*tb.t);
  const SideVals sv{c->be_rec, c->pol_size, c->pol_time};
  const LkOut o = lk_out(out, tb.tt);
  if (by_key)
    lk_by_key<<<grid_for(n), 256, 0, s>>>(t, tb.tt, sv, (const uint4 *)in, n, o);
  else
    lk_by_index<<<grid_for(n), 256, 0, s>>>(t, tb.tt, sv, (const uint32_t *)in, n, o);
  VP_HIP(hipGetLastError());
  VP_HIP(hipStreamSynchronize(s));
  return 0;
}

int table_value_size(vp_ctx *c, int table, uint32_t *bytes) {
  const char *fn = "vp_table_value_size";
  if (!c) return ST_BAD("%s: ctx is NULL", fn);
  if (!bytes) return ST_BAD("%s: bytes is NULL", fn);
  StTable tabs[2], tb;
  const int nt = st_tables(c, tabs);
  VP_TRY(lk_table(fn, table, tabs, nt, &tb));
  *bytes = kValSize[tb.tt];
  return 0;
}

}  // namespace
}  // namespace vp

int vp_table_lookup(vp_ctx *c, int table, uint32_t n, const uint8_t *keys, const vp_lookup_out *out,
                    void *stream) {
  return vp::table_query("vp_table_lookup", c, table, n, keys, true, out, stream);
}

int vp_table_entries(vp_ctx *c, int table, uint32_t n, const uint32_t *idx, const vp_lookup_out *out,
                     void *stream) {
  return vp::table_query("vp_table_entries", c, table, n, idx, false, out, stream);
}

int vp_table_value_size(vp_ctx *c, int table, uint32_t *bytes) {
  return vp::table_value_size(c, table, bytes);
}
