// vp_process_one's mailbox, device side (ServeBox, vp_internal.h): what the
// resident kernels nat_serve (vp_nat.hip), fw_serve (vp_fw.hip),
// bridge_serve (vp_bridge.hip) and pol_serve (vp_pol.hip) share --
// the poll loop, the chunks of a one-packet request, a burst's load, header
// tests, settle loop, stamp winner and answer words, and the allocate-and-
// insert of a new LAN flow. What a flow's key is, how a WAN packet finds its
// flow and what of the frame is rewritten stay with the NF.
#pragma once
#include "vp_table.h"

namespace vp {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
constexpr int kSys = 17;  // sc0 | sc1: system-coherent (bypasses the GPU caches)

// ----------------------------------------------------------- the table --
// The allocate step of one LAN packet whose key `key` (hash hh) is looked up
// under probe mask M3, at global sequence seq: the flow's index, allocated
// when new (*fresh = 1; dchain_allocate_new_index: the freed stack first,
// then the never-used range) with `key` stored, its last word as k3 (vigfw
// keeps int_devices in the padding bytes); kNone with nothing written when no
// index is free. The caller stamps the index (serve_stamp).
//
// serve_lan_by: the same with the lookup as a parameter, for a table whose
// match is not tbl_probe's (vigbridge: words 0-1 identify the MAC, word 2 is
// the learned port, vp_bridge.hip mac_probe); probe() returns the key's index
// or kNone.
template <class Probe>
__device__ __forceinline__ uint32_t serve_lan_by(const TableDev &t, uint32_t hh,
                                                 const uint32_t key[4], uint32_t k3,
                                                 uint64_t seq, uint32_t *fresh, Probe probe) {
  uint32_t idx = probe();
  if (idx != kNone) return idx;
  Ctl *c = t.ctl;
  const uint32_t st = c->stack_top, fn = c->fresh_next;
  if (st) {
    idx = t.stack[st - 1];
    c->stack_top = st - 1;
  } else if (fn < t.cap) {
    idx = fn;
    c->fresh_next = fn + 1;
  } else {
    return kNone;
  }
  const uint32_t k[4] = {key[0], key[1], key[2], k3};
  bool tomb = false;
  uint32_t disp = 0;
  const uint32_t e = tbl_insert(t, hh, k, idx, &tomb, &disp);
  if (tomb) c->n_tomb -= 1;
  c->n_live += 1;
  c->sh_live += 1;
  c->disp_count += disp;
  t.slot_of[idx] = e;
  t.hash_of[idx] = hh;
  t.birth[idx] = seq;
  *fresh = 1;
  return idx;
}
template <uint32_t M3>
__device__ __forceinline__ uint32_t serve_lan(const TableDev &t, uint32_t hh,
                                              const uint32_t key[4], uint32_t k3, uint64_t seq,
                                              uint32_t *fresh) {
  return serve_lan_by(t, hh, key, k3, seq, fresh, [&] { return tbl_probe<M3>(t, hh, key); });
}

// The touch of index idx at (now, seq), right behind the lookup: stamped
// after the answer instead, the stores' acknowledgement held the wave from
// its next poll (4.6-4.8 against 4.3-4.4 us per packet,
// profiles/r06z_serve_stamp.txt).
__device__ __forceinline__ void serve_stamp(const TableDev &t, uint32_t idx, int64_t now,
                                            uint64_t seq) {
  t.ts[idx] = (uint64_t)now;
  t.tseq[idx] = seq;
}

// --------------------------------------------------- the touch journal --
// Expiry inside the resident kernel (JournalDev, vp_table.h; viglb keeps
// two, one per expiring table).
// The wave keeps the journal's control words in registers (wave-uniform) and
// stores them back after every request (journal_store), so a kernel launched
// again after an idle exit or a stop goes on from them (journal_load).
struct JournalSt {
  uint32_t tail, cnt;  // ring position of the oldest record; records from there
  int64_t floor;       // lower bound of the live stamps (kJournalNone: none live)
  uint32_t expired;    // entries this request's walk expired
  uint32_t flags;      // kOneTombs: the walk left the table past the purge bound
};
__device__ __forceinline__ JournalSt journal_load(const JournalDev &j) {
  JournalSt s{0u, 0u, kJournalNone, 0u, 0u};
  if (j.ctl) {
    s.tail = __builtin_amdgcn_readfirstlane(j.ctl->tail);
    s.cnt = __builtin_amdgcn_readfirstlane(j.ctl->cnt);
    const uint64_t f = (uint64_t)j.ctl->floor;
    s.floor = (int64_t)((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)f) |
                        ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(f >> 32)) << 32));
  }
  return s;
}
__device__ __forceinline__ void journal_store(const JournalDev &j, const JournalSt &s,
                                              uint32_t lane) {
  if (lane == 0) {
    j.ctl->tail = s.tail;
    j.ctl->cnt = s.cnt;
    j.ctl->floor = s.floor;
  }
}
// The cutoff of a packet at `now`: now - E in unsigned 64-bit arithmetic (E
// from the table's own cutoff, vignat's 32-bit wrap inside it), compared as
// the pipeline compares it, signed (exp_collect).
__device__ __forceinline__ int64_t journal_cutoff(const JournalDev &j, int64_t now) {
  return (int64_t)((uint64_t)now - j.expire);
}
__device__ __forceinline__ uint32_t journal_pos(const JournalDev &j, uint32_t p) {
  return p >= j.n ? p - j.n : p;  // (p < 2 n: tail < n and at most n records)
}
// Room for `need` more records (the caller's touches; need <= n - live holds
// right after a seed, so a request posted again after one always fits).
__device__ __forceinline__ bool journal_room(const JournalDev &j, const JournalSt &s,
                                             uint32_t need) {
  return j.n - s.cnt >= need;
}

// expire_items_single_map (expirator.c:110-218) at `cutoff`, by the whole
// wave, before a request's packets: every current record from the tail whose
// index is stamped below the cutoff frees its index, oldest first, exactly as
// exp_apply does -- stack[top + rank], the youngest expired index on top, the
// bucket entry a tombstone, slot_of = kNone. One compare when nothing is due.
// The loop consumes at least one record per iteration or ends at a stopper
// (a current record stamped >= cutoff, the new floor): at most `cnt` (head -
// tail) iterations, no other exit, nothing another agent writes is read.
__device__ __forceinline__ void serve_expire(const TableDev &t, const JournalDev &j,
                                             JournalSt &s, int64_t cutoff, uint32_t lane) {
  if (cutoff <= s.floor) return;
  Ctl *c = t.ctl;
  const uint32_t top = __builtin_amdgcn_readfirstlane(c->stack_top);
  uint32_t freed = 0;
  bool stopped = false;
  for (uint32_t left = s.cnt; left > 0 && !stopped;) {
    const uint32_t m = min(left, 64u);
    uint32_t idx = 0;
    bool cur = false;
    int64_t ts = 0;
    if (lane < m) {
      const uint4 r = j.rec[journal_pos(j, s.tail + lane)];
      idx = r.z;
      cur = idx < t.cap && t.slot_of[idx] != kNone &&
            t.tseq[idx] == ((uint64_t)r.x | ((uint64_t)r.y << 32));
      if (cur) ts = (int64_t)t.ts[idx];
    }
    const uint64_t sb = __ballot(cur && ts >= cutoff);
    const uint32_t first = sb ? (uint32_t)__ffsll((unsigned long long)sb) - 1 : m;
    const bool dead = cur && lane < first;  // (below the stopper: ts < cutoff)
    const uint64_t eb = __ballot(dead);
    if (dead) {
      const uint32_t rank = (uint32_t)__popcll(eb & ((1ull << lane) - 1));
      const uint32_t e = t.slot_of[idx];
      // (the stack holds an index at most once: top + freed + rank < cap)
      if (top + freed + rank < t.cap) t.stack[top + freed + rank] = idx;
      if ((e >> 2) <= t.bmask) t.bk[e >> 2].idx[e & 3] = kTomb;
      t.slot_of[idx] = kNone;
    }
    freed += (uint32_t)__popcll(eb);
    s.tail = journal_pos(j, s.tail + first);
    s.cnt -= first;
    left -= first;
    if (sb) {
      const uint64_t u = (uint64_t)ts;
      s.floor = (int64_t)((uint64_t)(uint32_t)__shfl((int)(uint32_t)u, (int)first) |
                          ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(u >> 32), (int)first) << 32));
      stopped = true;
    }
  }
  if (!stopped) s.floor = kJournalNone;  // (the tail reached the head)
  if (freed) {
    uint32_t over = 0;
    if (lane == 0) {
      c->stack_top = top + freed;
      const uint32_t nt = c->n_tomb + freed, sl = c->sh_live - freed;
      c->n_tomb = nt;
      c->n_live -= freed;
      c->sh_live = sl;
      over = nt + sl > j.purge;
    }
    if (__builtin_amdgcn_readfirstlane(over)) s.flags |= kOneTombs;
    s.expired += freed;
    // (the walk's table writes before the request's lookups: one wave)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

// One record per touch, in packet order: lane 0's after a one-packet request
// (idx == kNone: the packet touched nothing) ...
__device__ __forceinline__ void journal_touch(const JournalDev &j, JournalSt &s, uint32_t idx,
                                              uint64_t seq, int64_t now, uint32_t lane) {
  if (idx == kNone) return;
  if (lane == 0)
    j.rec[journal_pos(j, s.tail + s.cnt)] = make_uint4((uint32_t)seq, (uint32_t)(seq >> 32), idx, 0u);
  if (s.cnt == 0) s.floor = now;  // (the only live stamp there is)
  s.cnt += 1;
}
// ... and a burst's, the lanes whose stamp won (burst_last) in lane order:
// an index touched by several packets of the burst is stamped by the last
// one alone, and the earlier touches' records would be stale the moment they
// were written. now0: the burst's first time, a lower bound of its stamps.
__device__ __forceinline__ void journal_touch_burst(const JournalDev &j, JournalSt &s, bool won,
                                                    uint32_t idx, uint64_t seq, int64_t now0,
                                                    uint32_t lane) {
  const uint64_t wb = __ballot(won);
  if (!wb) return;
  if (won) {
    const uint32_t rank = (uint32_t)__popcll(wb & ((1ull << lane) - 1));
    j.rec[journal_pos(j, journal_pos(j, s.tail + s.cnt) + rank)] =
        make_uint4((uint32_t)seq, (uint32_t)(seq >> 32), idx, 0u);
  }
  if (s.cnt == 0) s.floor = now0;
  s.cnt += (uint32_t)__popcll(wb);
}

// A frame's first 64 bytes from its four 16-byte chunks chunk(0..3); bytes
// past len read as 0.
template <class Chunk>
__device__ __forceinline__ RFrame serve_rframe(Chunk chunk, uint32_t len) {
  RFrame f;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint4 v = chunk_keep(chunk(j), 0, (int)len - 16 * j);
    f.w[4 * j] = v.x;
    f.w[4 * j + 1] = v.y;
    f.w[4 * j + 2] = v.z;
    f.w[4 * j + 3] = v.w;
  }
  return f;
}

// ------------------------------------------------- a one-packet request --
// The tagged chunks as every poll reads them, lane k chunk k (lanes past the
// chunks read nothing: an offset past the resource).
struct ServeIo {
  __amdgpu_buffer_rsrc_t ms, as;  // ServeBox msg, amsg
  int moff;
};
__device__ __forceinline__ ServeIo serve_io(ServeBox *box, uint32_t lane) {
  return ServeIo{
      __builtin_amdgcn_make_buffer_rsrc(box->msg, 0, 16 * kServeChunks, 0x00020000),
      __builtin_amdgcn_make_buffer_rsrc(box->amsg, 0, 16 * kServeChunks, 0x00020000),
      lane < kServeChunks ? (int)(16 * lane) : (int)(16 * kServeChunks)};
}

// Chunk 0's time (message bytes 4-11).
__device__ __forceinline__ int64_t serve_now(const v4u &c) {
  return (int64_t)((uint64_t)__builtin_amdgcn_readfirstlane(c[1]) |
                   ((uint64_t)__builtin_amdgcn_readfirstlane(c[2]) << 32));
}

// Chunk k >= 1 of `need` holds frame bytes 12k - 12 .. 12k - 1: into the
// frame's LDS copy.
__device__ __forceinline__ void serve_chunks_in(uint32_t *fword, const v4u &c, uint32_t lane,
                                                uint32_t need) {
  if (lane >= 1 && lane < need) {
    fword[3 * lane - 3] = c[0];
    fword[3 * lane - 2] = c[1];
    fword[3 * lane - 1] = c[2];
  }
}

// ------------------------------------------------------ a burst request --
// A burst request (ServeBox: nf.c's VIGOR_BATCH_SIZE loop, nf.c:178-215)
// brings n frames as nf_process would take them one after another, lane i =
// packet i at sequence seq0 + i; the whole wave serves it. The host sends a
// burst only while no expiry is due anywhere in it (serve_process_burst), or
// with the journal on the wave serves it up to the packet at which one falls
// due (burst_split), so no flow leaves during the burst: a lookup that hits is final the moment it
// is made, and only the misses depend on the packets before them
// (burst_settle). A burst is served whole (kBurstServed) or declined before
// any table write (kBurstDeclined: a frame with IPv4 options, the
// byte-addressed path's), and the host then runs it through the batch
// pipeline.

// Lane `lane`'s packet of a burst of n: its slot in the body, length, device,
// time and first 64 bytes.
struct BurstIn {
  __amdgpu_buffer_rsrc_t fs, os;  // ServeBox bframe, bout
  bool act;                       // lane < n
  uint32_t slot0, len, in;
  int64_t now;
  RFrame f;
};
constexpr uint32_t kBurstBody = kServeBurst * kServeFrame;
__device__ __forceinline__ BurstIn burst_load(ServeBox *box, uint32_t n, uint32_t lane) {
  BurstIn b;
  b.fs = __builtin_amdgcn_make_buffer_rsrc(box->bframe, 0, (int)kBurstBody, 0x00020000);
  const auto ns = __builtin_amdgcn_make_buffer_rsrc(box->bnow, 0, 8 * kServeBurst, 0x00020000);
  const auto es = __builtin_amdgcn_make_buffer_rsrc(box->bmeta, 0, 4 * kServeBurst, 0x00020000);
  b.os = __builtin_amdgcn_make_buffer_rsrc(box->bout, 0, 4 * kServeBurst, 0x00020000);
  b.act = lane < n;
  // (lanes past the burst read zeros and store nothing: offsets past the resources)
  b.slot0 = b.act ? lane * kServeFrame : kBurstBody;
  v4u q[4];
#pragma unroll
  for (int j = 0; j < 4; j++)
    q[j] = __builtin_amdgcn_raw_buffer_load_b128(b.fs, (int)(b.slot0 + 16 * j), 0, kSys);
  const uint32_t meta = __builtin_amdgcn_raw_buffer_load_b32(
      es, b.act ? (int)(4 * lane) : (int)(4 * kServeBurst), 0, kSys);
  const v2u nw = __builtin_amdgcn_raw_buffer_load_b64(
      ns, b.act ? (int)(8 * lane) : (int)(8 * kServeBurst), 0, kSys);
  b.len = min(meta & 0xFFFFu, kServeFrame), b.in = meta >> 16;
  b.now = (int64_t)((uint64_t)nw[0] | ((uint64_t)nw[1] << 32));
  b.f = serve_rframe([&](int j) { return make_uint4(q[j][0], q[j][1], q[j][2], q[j][3]); },
                     b.len);
  return b;
}

// The register path's tests on a frame (nat_main.c:30-38, fw_main.c:26-40) and
// the fields a FlowId is made of. go: TCP/UDP over a 20-byte IPv4 header;
// decline (wave-wide): some frame of the burst has a longer IPv4 header,
// which parse_l34 would follow -- the byte-addressed path's.
struct BurstHdr {
  uint32_t tl, proto, sp, dp, sip, dip;
  bool go, decline;
};
__device__ __forceinline__ BurstHdr burst_hdr(const BurstIn &b) {
  const RFrame &f = b.f;
  BurstHdr h;
  const uint32_t et = f.w[3] & 0xFFFF, ihl = (f.w[3] >> 16) & 0x0F;
  h.tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
  const uint16_t unread = (uint16_t)(b.len - 14);
  h.proto = f.w[5] >> 24;
  const bool ip = b.act && et == 0x0008 && unread >= 20 && unread >= h.tl;
  h.decline = __ballot(ip && ihl > 5) != 0;
  h.go = ip && ihl == 5 && ((h.proto == 6) | (h.proto == 17)) && (uint32_t)(b.len - 34) >= 4u;
  h.sp = f.w[8] >> 16, h.dp = f.w[9] & 0xFFFF;
  h.sip = f.u32at2(26), h.dip = f.u32at2(30);
  return h;
}

// A burst with the journal on, behind the decline test and before any other
// table write: the expiries due at its first packet (serve_expire), then the
// packets it serves -- with floor F after the walk, the lanes below the first
// lane k whose cutoff passes min(F, now_0): flows born or touched inside the
// burst are stamped at or after now_0, so no expiry is due at any of them
// (run_batch's test). k >= 1: lane 0's cutoff is at most F after its own walk
// and at most now_0. Returns k, or 0 when the journal has no room for the
// burst's touches (at most one record per index, journal_touch_burst):
// nothing was done. burst_now0: the burst's first time, wave-uniform.
__device__ __forceinline__ int64_t burst_now0(const BurstIn &b) {
  const uint64_t u = (uint64_t)b.now;
  return (int64_t)((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)u) |
                   ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(u >> 32)) << 32));
}
// One table's share of it: the walk at n0, then the lanes above 0 at which
// this table's next expiry falls due.
__device__ __forceinline__ uint64_t burst_walk(const TableDev &t, const JournalDev &j,
                                               JournalSt &s, const BurstIn &b, int64_t n0,
                                               uint32_t lane) {
  serve_expire(t, j, s, journal_cutoff(j, n0), lane);
  const int64_t lim = s.floor < n0 ? s.floor : n0;
  return __ballot(b.act && lane > 0 && journal_cutoff(j, b.now) > lim);
}
__device__ __forceinline__ uint32_t burst_split(const TableDev &t, const JournalDev &j,
                                                JournalSt &s, const BurstIn &b, uint32_t n,
                                                uint32_t lane, int64_t *now0) {
  if (!journal_room(j, s, min(n, t.cap))) return 0;
  const int64_t n0 = burst_now0(b);
  *now0 = n0;
  const uint64_t due = burst_walk(t, j, s, b, n0, lane);
  return due ? (uint32_t)__ffsll((unsigned long long)due) - 1 : n;
}

// The same for an NF with two expiring tables whose expiries both precede the
// parse (viglb: lb_main.c:21-22, flows then backends, each on its own lifetime
// and journal): room on both journals or nothing is done, both walks at now_0,
// and k is the first lane above 0 at which either table's next expiry falls
// due -- every active lane counts, parsed or not. A lane's touches go to one
// journal or the other, so each needs room for min(n, its cap) records.
__device__ __forceinline__ uint32_t burst_split2(const TableDev &t1, const JournalDev &j1,
                                                 JournalSt &s1, const TableDev &t2,
                                                 const JournalDev &j2, JournalSt &s2,
                                                 const BurstIn &b, uint32_t n, uint32_t lane,
                                                 int64_t *now0) {
  if (!journal_room(j1, s1, min(n, t1.cap)) || !journal_room(j2, s2, min(n, t2.cap))) return 0;
  const int64_t n0 = burst_now0(b);
  *now0 = n0;
  uint64_t due = burst_walk(t1, j1, s1, b, n0, lane);
  due |= burst_walk(t2, j2, s2, b, n0, lane);
  return due ? (uint32_t)__ffsll((unsigned long long)due) - 1 : n;
}

// The same for an NF whose expiry runs only at some packets (vigpol: behind
// the IPv4 parse, policer_main.c:113-123; `runs` is the lane's predicate, and
// only such lanes stamp). With v the lowest active lane that runs it, the walk
// is v's, at its time now_v, and k is the first running lane above v whose
// cutoff passes min(F, now_v): the stamps of the burst are at or after now_v,
// and a lane that does not run the expiry never cuts the burst. No running
// lane: no walk, and all n are served (they touch nothing). *now0 = now_v, the
// lower bound of the burst's stamps.
__device__ __forceinline__ uint32_t burst_split_if(const TableDev &t, const JournalDev &j,
                                                   JournalSt &s, const BurstIn &b, bool runs,
                                                   uint32_t n, uint32_t lane, int64_t *now0) {
  if (!journal_room(j, s, min(n, t.cap))) return 0;
  const uint64_t rb = __ballot(b.act && runs);
  if (!rb) return n;
  const int v = __ffsll((unsigned long long)rb) - 1;
  const uint64_t u = (uint64_t)b.now;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)(uint32_t)u, v));
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)(uint32_t)(u >> 32), v));
  const int64_t nv = (int64_t)((uint64_t)lo | ((uint64_t)hi << 32));
  *now0 = nv;
  serve_expire(t, j, s, journal_cutoff(j, nv), lane);
  const int64_t lim = s.floor < nv ? s.floor : nv;
  const uint64_t due =
      __ballot(b.act && runs && (int)lane > v && journal_cutoff(j, b.now) > lim);
  return due ? (uint32_t)__ffsll((unsigned long long)due) - 1 : n;
}

// After round 0 (every lane has looked its flow up in the table as the burst
// found it; hits are final) the misses settle in packet order: the lowest
// pending LAN lane m looks again (an earlier lane of this burst may have
// inserted its key) and allocates as a packet of its own would (lan_alloc:
// serve_lan, kNone when no index is free); a pending WAN lane below m has
// every flow born before it in the table and is final, hit or drop, once it
// has looked again (wan_again). At most one round per lane. A lane may be
// pending on both (vigbridge: every packet learns its src and looks its dst
// up): as lane m it allocates and stays a pending WAN lane, which looks again
// below the next m or behind the loop -- after its own insert and before any
// later lane's.
template <class WanAgain, class LanAlloc>
__device__ __forceinline__ void burst_settle(uint32_t lane, bool lpend, bool wpend,
                                             WanAgain wan_again, LanAlloc lan_alloc) {
  for (uint32_t r = 0; r < kServeBurst; r++) {
    const uint64_t lp = __ballot(lpend);
    if (!lp) break;
    const uint32_t m = (uint32_t)__ffsll((unsigned long long)lp) - 1;
    if (wpend && lane < m) {
      wan_again();
      wpend = false;
    }
    if (lane == m) {
      lan_alloc();
      lpend = false;
    }
    // (lane m's insert before the later lanes' lookups: one wave, workgroup
    // scope; an agent-scope release would write the XCD's L2 back)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  if (wpend) wan_again();  // (no LAN miss before them is left)
}

// Stamps: for every index the burst's last packet that touched it must win.
// True for the highest lane holding idx: it stores both words, the others
// store nothing (no order between lanes' stores is relied on).
__device__ __forceinline__ bool burst_last(uint32_t idx, uint32_t n, uint32_t lane) {
  bool last = idx != kNone;
  for (uint32_t j = 1; j < n; j++) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)idx, (int)j);
    if (j > lane && o == idx) last = false;
  }
  return last;
}

// The out words (out port | fresh << 16 | rewritten << 17), four lanes' in
// one store, and all of the burst's stores complete before the answer chunk
// that announces them.
__device__ __forceinline__ void burst_out(const BurstIn &b, uint32_t res, uint32_t n,
                                          uint32_t lane) {
  v4u o4;
#pragma unroll
  for (int k = 0; k < 4; k++) o4[k] = (uint32_t)__shfl((int)res, (int)((4 * lane + k) & 63));
  if (4 * lane < n) __builtin_amdgcn_raw_buffer_store_b128(o4, b.os, (int)(16 * lane), 0, kSys);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  __builtin_amdgcn_s_waitcnt(0);
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
}

// A burst's answer (lane 0): the status chunk and the answer word, where a
// relaunched server starts counting.
__device__ __forceinline__ void burst_answer(const ServeIo &io, ServeBox *box, uint32_t st,
                                             uint32_t bn, uint32_t want, uint32_t expired = 0) {
  __builtin_amdgcn_raw_buffer_store_b128((v4u){st, bn, expired, want}, io.as, 0, 0, kSys);
  __hip_atomic_store(&box->ans, (uint64_t)want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------- the poll loop --
// Every wave polls on its own, one poll in flight per wave: a wave's polls
// return in order, so polls queued behind a stale one would see a request
// late. serve(chunks): -1 nothing new (not yet whole, or another wave's), 0 a
// request served, 1 leave; last(): the last answer's wall clock, `idle` ticks
// after which the wave leaves.
//
// After an answer the next request cannot come before the answer has crossed
// to the host and the host's loop has turned round (about half a round trip
// plus its own time): a poll issued at once reads the mailbox too early and
// the request waits for the poll after it, a whole round trip later. The
// first poll after an answer waits `after` wall-clock ticks (flags bits
// 10-17; kServeAfter, vp_serve.hip) so that it reads about when the request lands.
// The delay adapts (flags bit 18): a request the first poll caught takes a
// tick off it, one that needed a later poll adds `up` (bits 19-23) -- a late
// poll costs a round trip, an early one only its excess -- so it settles just
// past where the caller's requests land, whatever the caller's loop.
template <class Serve, class Last>
__device__ __forceinline__ void serve_poll(const ServeIo &io, uint32_t flags, uint64_t idle,
                                           Serve serve, Last last) {
  uint32_t after = (flags >> 10) & 0xFFu;
  const uint32_t up = (flags >> 19) & 0x1Fu;
  const bool adapt = (flags >> 18) & 1u;
  uint32_t polls = 0;  // polls since the last answer
  for (;;) {
    const v4u q = __builtin_amdgcn_raw_buffer_load_b128(io.ms, io.moff, 0, kSys);
    const int st = serve(q);
    if (st == 1) break;
    polls++;
    if (st < 0) {
      if (wall_clock64() - last() > idle) break;
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    if (adapt && polls == 1 && after > 0) after--;
    if (adapt && polls > 1 && polls < 64) after = min(after + up, 200u);
    polls = 0;
    if (after) {
      const uint64_t w = wall_clock64();
      while (wall_clock64() - w < after) __builtin_amdgcn_s_sleep(1);
    }
  }
}

}  // namespace vp
