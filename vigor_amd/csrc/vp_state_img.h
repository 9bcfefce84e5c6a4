// The bytes of a state image and of an incremental one
// (§5.15) as the host reads and writes them: the two headers, a table's
// arrays and their pads, and the one reader of bytes that come from outside
// the process. Plain C++ over (buf, bytes): no HIP, nothing of a context, so
// that the reader also builds alone on a CPU (tests/state_reader_main.cc).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/vigpath.h"

namespace vp {
namespace stimg {

// What a table keeps per index beside the stamps (the image's key and value).
enum TblType : uint32_t { TT_NAT, TT_BRIDGE, TT_FW, TT_LBFLOW, TT_LBBACK, TT_POL };
inline constexpr uint32_t kValSize[6] = {0, 4, 4, 4, 8, 16};
constexpr uint32_t kStTblHdr = 32;

inline void put32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
inline uint32_t get32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline uint64_t get64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline uint64_t pad16(uint64_t v) { return (v + 15) & ~15ull; }

// One table's arrays: offsets from the first byte, the table header at
// lru - kStTblHdr. n_live counts the arrays' entries (a delta: n_new, lru =
// idx[]), n_table the table's live entries (an image: the same number).
struct Section {
  uint32_t cap, n_live, fresh, vsz, n_freed, n_table;
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
inline Section section_at(uint64_t at, uint32_t cap, uint32_t n_live, uint32_t fresh,
                          uint32_t tt, uint32_t n_freed, uint32_t n_table) {
  Section s{cap, n_live, fresh, kValSize[tt], n_freed, n_table};
  section_layout(s, at);
  return s;
}
// Where each array ends and its pad begins.
inline void section_ends(const Section &s, uint64_t ends[5]) {
  ends[0] = s.lru + 4ull * s.n_live;
  ends[1] = s.freed + 4ull * s.n_freed;
  ends[2] = s.ts + 8ull * s.n_live;
  ends[3] = s.val;
  ends[4] = s.val + (uint64_t)s.vsz * s.n_live;
}

// What tells an image from a delta: the common header's first words and size
// (both begin magic, version, kind, n_tables, total_bytes, last_now; a delta's
// marks follow), whether a table header carries n_new at +20 where an image
// has a reserved word, and the name every refusal begins with.
struct Format {
  uint32_t magic, version, hdr;
  bool n_new;
  const char *who;
};
inline constexpr Format kImage{VP_STATE_MAGIC, VP_STATE_VERSION, 32, false, "state load"};
inline constexpr Format kDelta{VP_STATE_DELTA_MAGIC, VP_STATE_DELTA_VERSION, 64, true,
                               "state delta apply"};
// What the context expects of the bytes it is given.
struct Expect {
  int kind, nt;
  uint32_t cap[2], tt[2];
};

inline void put_header(const Format &f, uint8_t *buf, int kind, int nt, uint64_t total,
                       int64_t last_now) {
  memset(buf, 0, f.hdr);
  put32(buf, f.magic);
  put32(buf + 4, f.version);
  put32(buf + 8, (uint32_t)kind);
  put32(buf + 12, (uint32_t)nt);
  put64(buf + 16, total);
  put64(buf + 24, (uint64_t)last_now);
}
inline void put_table_header(const Format &f, uint8_t *buf, const Section &s) {
  uint8_t *h = buf + s.lru - kStTblHdr;
  memset(h, 0, kStTblHdr);
  put32(h, s.cap);
  put32(h + 4, s.n_table);
  put32(h + 8, s.fresh);
  put32(h + 12, s.vsz);
  put32(h + 16, s.n_freed);
  if (f.n_new) put32(h + 20, s.n_live);
}

// The reader. Each returns false with the refusal in msg; the first failing
// test decides the text, so their order is part of the interface.
#define VP_IMG_BAD(...) (snprintf(msg, len, __VA_ARGS__), false)

// The common header against the byte count and the context.
inline bool read_header(const Format &f, const Expect &x, const uint8_t *buf, uint64_t bytes,
                        int64_t *last_now, char *msg, size_t len) {
  typedef unsigned long long ull;
  if (bytes < f.hdr) return VP_IMG_BAD("%s: %llu bytes hold no header", f.who, (ull)bytes);
  if (get32(buf) != f.magic) return VP_IMG_BAD("%s: magic 0x%08x", f.who, get32(buf));
  if (get32(buf + 4) != f.version) return VP_IMG_BAD("%s: version %u", f.who, get32(buf + 4));
  if (get32(buf + 8) != (uint32_t)x.kind)
    return VP_IMG_BAD("%s: kind %u into a context of kind %d", f.who, get32(buf + 8), x.kind);
  if (get32(buf + 12) != (uint32_t)x.nt)
    return VP_IMG_BAD("%s: n_tables %u, this NF has %d", f.who, get32(buf + 12), x.nt);
  if (get64(buf + 16) != bytes)
    return VP_IMG_BAD("%s: total_bytes %llu, %llu given", f.who, (ull)get64(buf + 16), (ull)bytes);
  *last_now = (int64_t)get64(buf + 24);
  if (*last_now < -1) return VP_IMG_BAD("%s: last_now %lld", f.who, (long long)*last_now);
  return true;
}

// Table k's header and arrays at `at` (f.hdr, or the end of the table before;
// at <= bytes): sizes and counts against the capacity and the byte count, the
// pads, and behind the last table the end of the bytes.
inline bool read_section(const Format &f, const Expect &x, int k, const uint8_t *buf,
                         uint64_t bytes, uint64_t at, Section *out, char *msg, size_t len) {
  typedef unsigned long long ull;
  if (bytes - at < kStTblHdr) return VP_IMG_BAD("%s: table %d: header past the end", f.who, k);
  const uint8_t *h = buf + at;
  const uint32_t n_table = get32(h + 4), n_live = f.n_new ? get32(h + 20) : n_table;
  Section &s = *out;
  s = Section{get32(h), n_live, get32(h + 8), get32(h + 12), get32(h + 16), n_table};
  if (s.cap != x.cap[k])
    return VP_IMG_BAD("%s: table %d: capacity %u, the context's is %u", f.who, k, s.cap, x.cap[k]);
  if (n_table > s.cap)
    return VP_IMG_BAD("%s: table %d: n_live %u above the capacity", f.who, k, n_table);
  if (s.fresh > s.cap)
    return VP_IMG_BAD("%s: table %d: fresh_next %u above the capacity", f.who, k, s.fresh);
  if (s.vsz != kValSize[x.tt[k]]) return VP_IMG_BAD("%s: table %d: value size %u", f.who, k, s.vsz);
  if (s.n_freed > s.cap || (uint64_t)n_table + s.n_freed + (s.cap - s.fresh) != s.cap)
    return VP_IMG_BAD("%s: table %d: n_live %u + n_freed %u + tail %u is not the capacity %u",
                      f.who, k, n_table, s.n_freed, s.cap - s.fresh, s.cap);
  if (n_live > n_table)
    return VP_IMG_BAD("%s: table %d: n_new %u above n_live %u", f.who, k, n_live, n_table);
  if ((f.n_new ? 0u : get32(h + 20)) | get32(h + 24) | get32(h + 28))
    return VP_IMG_BAD("%s: table %d: reserved header word not zero", f.who, k);
  section_layout(s, at);
  if (s.end > bytes)
    return VP_IMG_BAD("%s: table %d: arrays end at %llu of %llu bytes", f.who, k, (ull)s.end,
                      (ull)bytes);
  uint64_t ends[5];
  section_ends(s, ends);
  for (uint64_t e : ends)
    for (uint64_t b = e; b < pad16(e); b++)
      if (buf[b]) return VP_IMG_BAD("%s: table %d: pad byte at %llu not zero", f.who, k, (ull)b);
  if (k == x.nt - 1 && s.end != bytes)
    return VP_IMG_BAD("%s: %llu bytes behind the last table", f.who, (ull)(bytes - s.end));
  return true;
}

// Every table's section behind the header.
inline bool read_sections(const Format &f, const Expect &x, const uint8_t *buf, uint64_t bytes,
                          Section sec[2], char *msg, size_t len) {
  uint64_t at = f.hdr;
  for (int k = 0; k < x.nt; at = sec[k++].end)
    if (!read_section(f, x, k, buf, bytes, at, &sec[k], msg, len)) return false;
  return true;
}

#undef VP_IMG_BAD

}  // namespace stimg
}  // namespace vp
