// viglb on MI355X: Maglev-style load balancing over a packet batch.
//
// Reference behaviour (paths relative to the reference repository):
//   nf_process              viglb/lb_main.c:20-68
//   lb_get_backend          viglb/lb_balancer.c:38-112
//   lb_process_heartbit     lb_balancer.c:114-143
//   lb_expire_flows/_backends  lb_balancer.c:145-167 (int64 x1000, no wrap)
//   cht_fill_cht            libvig/verified/cht.c:546-877
//   cht_find_preferred_available_backend  cht.c:969-1062
//
// Two expiring tables: flows (LoadBalancedFlow -> flow index, flow index ->
// backend index) and backends (ip -> backend index, backends[] records).
// Batches are cut where either may expire (run_batch). Inside a segment only
// two things change the state other packets observe: a heartbeat from an
// unknown IP allocates a backend (changes what the CHT scan finds), and a
// WAN packet whose flow points at a dead backend (the flow is erased, freed
// and looked up again). A segment is processed in rounds:
//   phase A (whole segment)  parse + hash + probe; WAN hits whose backend is
//            alive are rewritten at once; heartbeats of known IPs are logged
//            for rejuvenation; new flows (M), stale flows (S) and unknown
//            heartbeat IPs (H) are queued;
//   rounds   a round ends before the first queued WAN packet (M or S) that
//            follows a queued heartbeat, so every queued WAN packet of a
//            round precedes every backend allocation of that round and sees
//            the backend set of the round start. Per round:
//              S: if some backend is alive, free + re-allocate returns the
//                 same flow index (it is the free-list head), so a stale flow
//                 is re-pointed at its CHT choice and rejuvenated; with no
//                 backend alive it is freed (in packet order) and dropped;
//              M: de-duplicated, ranked and allocated in packet order (as
//                 vignat), each first sighting records its CHT choice; with
//                 no backend alive every M packet is dropped, nothing is
//                 allocated;
//              H: de-duplicated, ranked and allocated on the backend table;
//                 the first sighting writes the backend record;
//            later rounds first re-classify their queued packets against
//            the state earlier rounds left (lb_resolve).
// Flow table entry: key words {src_ip, dst_ip, src_port | dst_port << 16,
// protocol | backend_index << 8}; words 0-2 and the low byte of word 3 are
// the LoadBalancedFlow (lb_flow.h:6-12), the upper 24 bits carry
// flow_id_to_backend_id, so a hit resolves in one bucket read.
#include <hip/hip_runtime.h>
#include <cstddef>

#include <algorithm>
#include <cstring>
#include <vector>

#include "vp_serve_dev.h"
#include "vp_table.h"

namespace vp {

VP_PRELOAD_UNIT(lb)


// LoadBalancedFlow_hash (generated, 5 CRC steps: src_ip, dst_ip, src_port,
// dst_port, protocol): non-zero byte positions of the 20-byte CRC message.
static const int kLbFlowPos[13] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16};
constexpr int kLbFlowMsg = 20;
// ip_addr hash: one CRC step over the u32 address.
constexpr uint32_t kLbFlowTabs = 13;  // LoadBalancedFlow's CRC byte positions
constexpr int kLbTabs = 13 + 4;        // + ip_addr's four

__device__ __forceinline__ uint32_t lbflow_hash(const uint32_t *T, uint32_t sip,
                                                uint32_t dip, uint32_t sp,
                                                uint32_t dp, uint32_t proto) {
  return T[0 * 256 + (sip & 0xFF)] ^ T[1 * 256 + ((sip >> 8) & 0xFF)] ^
         T[2 * 256 + ((sip >> 16) & 0xFF)] ^ T[3 * 256 + (sip >> 24)] ^
         T[4 * 256 + (dip & 0xFF)] ^ T[5 * 256 + ((dip >> 8) & 0xFF)] ^
         T[6 * 256 + ((dip >> 16) & 0xFF)] ^ T[7 * 256 + (dip >> 24)] ^
         T[8 * 256 + (sp & 0xFF)] ^ T[9 * 256 + ((sp >> 8) & 0xFF)] ^
         T[10 * 256 + (dp & 0xFF)] ^ T[11 * 256 + ((dp >> 8) & 0xFF)] ^
         T[12 * 256 + (proto & 0xFF)];
}
// lbflow_hash for the 64-byte tile, its 13 table reads batched (crc13_lds).
__device__ __forceinline__ uint32_t lbflow_hash_batched(const uint32_t *T, uint32_t sip,
                                                        uint32_t dip, uint32_t sp,
                                                        uint32_t dp, uint32_t proto) {
  return crc13_lds(T, sip & 0xFF, (sip >> 8) & 0xFF, (sip >> 16) & 0xFF, sip >> 24, dip & 0xFF,
                   (dip >> 8) & 0xFF, (dip >> 16) & 0xFF, dip >> 24, sp & 0xFF,
                   (sp >> 8) & 0xFF, dp & 0xFF, (dp >> 8) & 0xFF, proto & 0xFF);
}

__device__ __forceinline__ uint32_t ip_hash(const uint32_t *I, uint32_t ip) {
  return I[0 * 256 + (ip & 0xFF)] ^ I[1 * 256 + ((ip >> 8) & 0xFF)] ^
         I[2 * 256 + ((ip >> 16) & 0xFF)] ^ I[3 * 256 + (ip >> 24)];
}

// map_get on the flow table; *w3 = the entry's word 3 (protocol | backend).
__device__ __forceinline__ uint32_t flow_probe(const TableDev &t, uint32_t h,
                                               uint32_t k0, uint32_t k1,
                                               uint32_t k2, uint32_t proto,
                                               uint32_t *w3) {
  uint32_t b = home_bucket(h, t.bmask, t.mix, t.lin);
  for (uint32_t i = 0; i <= t.bmask; i++) {
    const uint4 *q = reinterpret_cast<const uint4 *>(t.bk + b);
    const uint4 e0 = q[0], e1 = q[1], e2 = q[2], ix = q[3];
    if (ix.x == kEmpty) return kNone;
    if (ix.x != kTomb && e0.x == k0 && e0.y == k1 && e0.z == k2 &&
        (e0.w & 0xFF) == proto) {
      *w3 = e0.w;
      return ix.x;
    }
    if (ix.y == kEmpty) return kNone;
    if (ix.y != kTomb && e1.x == k0 && e1.y == k1 && e1.z == k2 &&
        (e1.w & 0xFF) == proto) {
      *w3 = e1.w;
      return ix.y;
    }
    if (ix.z == kEmpty) return kNone;
    if (ix.z != kTomb && e2.x == k0 && e2.y == k1 && e2.z == k2 &&
        (e2.w & 0xFF) == proto) {
      *w3 = e2.w;
      return ix.z;
    }
    b = (b + 1) & t.bmask;
  }
  return kNone;
}

struct LbArgs {
  uint8_t *frames;
  const uint16_t *len;
  const uint16_t *in_dev;  // null: every packet on port in0 (vp_dev_batch.in_port)
  uint32_t in0;
  uint16_t *out;
  uint32_t *log, *log2;  // flow / backend touch logs
  uint32_t slot, p0, p1;
  TableDev ft, bt;
  uint4 *be_rec;
  const uint32_t *cht;
  uint32_t height, bcap;
  const uint32_t *crc_tab;
  const uint32_t *dmacw;
  uint32_t *miss, *stale, *hb;  // queues M, S, H
  uint32_t *hbl;  // phase A: every heartbeat's position (its backend touch)
  uint16_t wan, n_dev;
  // phase A with touch bins (lb_classify64): a hit's touch goes to the bins
  // only and a dropped packet logs nothing; the packets the rounds finish
  // log their touches themselves and are applied after the fold as late
  // touches (lb_segment)
  bool binned;
};

// cht_find_preferred_available_backend: bucket = (u64)hash % height, the
// first allocated backend in its priority list; kNone if none is.
__device__ __forceinline__ uint32_t cht_choose(const LbArgs &a, uint32_t h) {
  const uint32_t *row = a.cht + (size_t)((uint64_t)h % a.height) * a.bcap;
  for (uint32_t p = 0; p < a.bcap; p++) {
    const uint32_t cand = row[p];
    if (a.bt.slot_of[cand] != kNone) return cand;
  }
  return kNone;
}

__device__ __forceinline__ void backend_macs(const LbArgs &a, uint4 rec,
                                             uint32_t nic, uint32_t mw[3]) {
  uint32_t s1 = 0, s2 = 0;  // config.device_macs[nic] (zero if no such NIC)
  if (nic < a.n_dev) {
    s1 = a.dmacw[2 * nic];
    s2 = a.dmacw[2 * nic + 1];
  }
  mw[0] = rec.y;                   // d_addr = backend.mac
  mw[1] = (rec.z & 0xFFFF) | s1;   // d_addr[4..5] | s_addr[0..1]
  mw[2] = s2;                      // s_addr[2..5]
}

// lb_main.c:56-65 on a register frame (IHL 5, total_length <= 50).
__device__ __forceinline__ bool lb_rewrite_fast(const LbArgs &a, RFrame &f,
                                                uint4 rec, uint32_t proto,
                                                uint32_t tl, uint32_t p) {
  const uint32_t nic = rec.z >> 16;
  a.out[p] = (uint16_t)nic;
  if (nic == a.wan) return false;
  f.set32at2(30, rec.x);  // dst_addr = backend.ip
  uint32_t mw[3];
  backend_macs(a, rec, nic, mw);
  f.w[0] = mw[0];
  f.w[1] = mw[1];
  f.w[2] = mw[2];
  fast_checksums(f, proto, tl);
  return true;
}

__device__ __forceinline__ void lb_rewrite_generic(const LbArgs &a, const GFrame &f,
                                                   const L34 &h, uint4 rec,
                                                   uint32_t p) {
  const uint32_t nic = rec.z >> 16;
  a.out[p] = (uint16_t)nic;
  if (nic == a.wan) return;
  f.w32(h.ip + 16, rec.x);
  uint32_t mw[3];
  backend_macs(a, rec, nic, mw);
  set_macs(f, mw);
  set_checksums(f, h.ip, h.l4);
}

// Decision for a parsed packet (phase A / re-classification). Heartbeats are
// logged or queued (H); WAN packets hitting a flow with a live backend are
// handed to `rw` with the backend record; the rest are queued (M / S).
// The backend touch log (log2) is written only for heartbeats: phase A lists
// them (hbl) and the segment applies them as late touches.
// lb_process_heartbit for a packet from a backend; the packet itself is
// dropped. I = the ip_addr hash tables.
__device__ __forceinline__ void lb_heartbeat(const LbArgs &a, const uint32_t *I, uint32_t p,
                                             uint32_t in, uint32_t sip) {
  const uint32_t key[4] = {sip, 0, 0, 0};
  const uint32_t bi = tbl_probe(a.bt, ip_hash(I, sip), key);
  a.out[p] = (uint16_t)in;
  if (!a.binned) a.log[p] = kNone;
  a.log2[p] = bi;  // kNone: queued, the round writes the real entry
  const uint32_t k = wave_append(&a.bt.ctl->defer_count, true);  // heartbeats seen
  if (a.hbl) a.hbl[k] = p;
  if (bi == kNone) a.hb[wave_append(&a.bt.ctl->miss_count, true)] = p;
}

// A WAN packet after its flow lookup (fi, and the entry's word 3): a flow
// with a live backend is handed to `rw` with the backend record; the rest
// are queued (M: no flow, S: its backend is gone).
template <class Rw>
__device__ __forceinline__ bool lb_flow_found(const LbArgs &a, uint32_t p, uint32_t fi,
                                              uint32_t w3, Rw rw, uint32_t *touch) {
  if (fi == kNone) {
    if (!a.binned) a.log[p] = kNone;
    a.miss[wave_append(&a.ft.ctl->miss_count, true)] = p;
    return false;
  }
  const uint32_t bi = w3 >> 8;
  // (both depend on bi only; the record of a dead backend is read and ignored)
  const bool live = a.bt.slot_of[bi] != kNone;
  const uint4 rec = a.be_rec[bi];
  if (!live) {  // backend gone: erase + re-lookup
    if (!a.binned) a.log[p] = kNone;
    a.stale[wave_append(&a.ft.ctl->defer_count, true)] = p;
    return false;
  }
  if (!a.binned) a.log[p] = fi;
  if (touch) *touch = fi;
  return rw(rec);
}

// Decision for a parsed packet (phase A / re-classification). Heartbeats are
// logged or queued (H); WAN packets hitting a flow with a live backend are
// handed to `rw` with the backend record; the rest are queued (M / S).
// The backend touch log (log2) is written only for heartbeats: phase A lists
// them (hbl) and the segment applies them as late touches. T = the flow hash
// tables, I = the ip_addr hash tables.
template <class Rw>
__device__ __forceinline__ bool lb_decide(const LbArgs &a, const uint32_t *T,
                                          const uint32_t *I, uint32_t p, uint32_t in,
                                          uint32_t sip, uint32_t dip, uint32_t sp,
                                          uint32_t dp, uint32_t proto, Rw rw,
                                          uint32_t *touch = nullptr) {
  if (in != a.wan) {
    lb_heartbeat(a, I, p, in, sip);
    return false;
  }
  uint32_t w3 = 0;
  const uint32_t fi =
      flow_probe(a.ft, lbflow_hash(T, sip, dip, sp, dp, proto), sip, dip,
                 sp | (dp << 16), proto, &w3);
  return lb_flow_found(a, p, fi, w3, rw, touch);
}

__device__ __forceinline__ void lb_generic_a(const LbArgs &a, const uint32_t *T,
                                             const uint32_t *I,
                                             uint32_t p) {
  const GFrame f{a.frames + (size_t)p * a.slot, a.slot};
  const uint32_t in = port_of(a.in_dev, a.in0, p);
  const L34 h = parse_l34(f, a.len[p]);
  if (!h.ok) {
    a.out[p] = (uint16_t)in;
    if (!a.binned) a.log[p] = kNone;
    return;
  }
  const uint32_t proto = f.r8(h.ip + 9);
  const uint32_t sp = f.r16(h.l4), dp = f.r16(h.l4 + 2);
  const uint32_t sip = f.r32(h.ip + 12), dip = f.r32(h.ip + 16);
  lb_decide(a, T, I, p, in, sip, dip, sp, dp, proto, [&](uint4 rec) {
    lb_rewrite_generic(a, f, h, rec, p);
    return false;
  });
}

__device__ __forceinline__ void lb_load_tables(uint32_t *T, const uint32_t *g) {
  for (uint32_t i = threadIdx.x; i < kLbTabs * 256; i += blockDim.x) T[i] = g[i];
  __syncthreads();
}

// Phase A for 64-byte slots (frames64_tiles, vp_device.h): frames 1 KiB
// contiguous per load through the wave's LDS tile, and a WAN packet's flow
// bucket gathered cooperatively (four lanes per 64-byte row) between the
// issue and finish halves, as vignat's tiles do. LDS holds the 13 flow-hash
// position tables and the allocation-order layout's four byte tables; the
// backend-address tables (heartbeats only) are read from global memory.
struct LbPend {
  uint32_t row;   // the flow's home bucket (kind 2), or kNone
  uint32_t kind;  // 0: done; 1: byte path; 2: WAN flow; 3: heartbeat
};
// The backends (up to 256: the BASELINE config's 256) are staged in LDS
// beside the tables, record and liveness in one 16-byte entry (the backend
// table does not change during phase A: heartbeats wait for the rounds), so a
// hit's backend costs one LDS read instead of a dependent global round trip.
// To make room, the tile loop keeps only the cursors of 256 touch bins and
// the overflow queue's (lb_segment keeps the flow table's bins at 256).
// Each staged backend is what a hit's rewrite needs, ready: bhdr[b] = {ip,
// the three MAC header words (backend_macs, the NIC's source MAC folded
// in)}, bnic[b] = its NIC | live << 16. The NIC's MAC was a global load that
// depended on the backend the row named (row -> backend -> NIC -> MAC): one
// more dependent round trip per packet.
constexpr uint32_t kLbLdsBackends = 256;
constexpr uint32_t kLbCurs = 257;  // bins 0..255, the overflow queue at 256
template <uint32_t W>  // waves per block
__device__ __forceinline__ void lb_tiles(LbArgs a, uint32_t n_all, TouchBins bins) {
  __shared__ uint32_t T[kLbFlowTabs * 256 + 1024];  // + the layout's byte tables
  __shared__ uint4 stage[W][256];
  __shared__ uint32_t cur[kLbCurs];
  __shared__ uint4 bhdr[kLbLdsBackends];
  __shared__ uint32_t bnic[kLbLdsBackends];
  for (uint32_t i = threadIdx.x; i < kLbCurs; i += blockDim.x) cur[i] = 0;
  for (uint32_t i = threadIdx.x; i < kLbFlowTabs * 256; i += blockDim.x) T[i] = a.crc_tab[i];
  const uint32_t *lin = T + kLbFlowTabs * 256;
  if (a.ft.mix == kMixLin)
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) T[kLbFlowTabs * 256 + i] = a.ft.lin[i];
  const bool lds_be = a.bcap <= kLbLdsBackends;
  if (lds_be)
    for (uint32_t b = threadIdx.x; b < a.bcap; b += blockDim.x) {
      const uint4 r = a.be_rec[b];
      const uint32_t nic = r.z >> 16;
      uint32_t mw[3];
      backend_macs(a, r, nic, mw);
      bhdr[b] = make_uint4(r.x, mw[0], mw[1], mw[2]);
      bnic[b] = nic | (a.bt.slot_of[b] != kNone ? 1u << 16 : 0u);
    }
  __syncthreads();
  const uint32_t *I = a.crc_tab + kLbFlowTabs * 256;  // ip_addr tables (global)
  frames64_tiles<kLbCurs - 1, true, W>(
      a.frames, a.len, a.in_dev, a.p0, a.p1, n_all, stage[threadIdx.x >> 6],
      reinterpret_cast<const uint4 *>(a.ft.bk),
      [&](uint32_t p, const RFrame &f, uint32_t in, uint32_t len, bool mine) {
        LbPend P{kNone, 0};
        if (!mine) return P;
        const uint32_t et = f.w[3] & 0xFFFF;
        const uint32_t ihl = (f.w[3] >> 16) & 0x0F;
        const uint32_t tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
        if (!(et == 0x0008 && ihl == 5 && tl <= 50)) {
          P.kind = 1;  // byte-addressed path (lb_generic_a)
          return P;
        }
        const uint16_t unread = (uint16_t)(len - 14);
        const uint32_t proto = f.w[5] >> 24;
        const bool ok = (unread >= 20) & (unread >= tl) &
                        ((proto == 6) | (proto == 17)) & ((uint32_t)(len - 34) >= 4u);
        if (!ok) {
          a.out[p] = (uint16_t)in;
          if (!a.binned) a.log[p] = kNone;
          return P;
        }
        if (in != a.wan) {
          P.kind = 3;
          return P;
        }
        const uint32_t sp = f.w[8] >> 16, dp = f.w[9] & 0xFFFF;
        P.kind = 2;
        P.row = home_bucket(lbflow_hash_batched(T, f.u32at2(26), f.u32at2(30), sp, dp, proto),
                            a.ft.bmask, a.ft.mix, lin);
        return P;
      },
      [&](const LbPend &P, const uint4 *row, uint32_t p, RFrame &f, uint32_t in,
          uint32_t len, uint32_t &touch) -> uint32_t {
        if (P.kind == 0) return 0u;
        if (P.kind == 1) {
          lb_generic_a(a, T, I, p);
          return 0u;
        }
        const uint32_t proto = f.w[5] >> 24;
        const uint32_t tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
        const uint32_t sp = f.w[8] >> 16, dp = f.w[9] & 0xFFFF;
        const uint32_t sip = f.u32at2(26), dip = f.u32at2(30);
        if (P.kind == 3) {
          lb_heartbeat(a, I, p, in, sip);
          return 0u;
        }
        // map_get on the flow table from the gathered home bucket (word 3:
        // protocol byte | backend << 8)
        const uint32_t key[4] = {sip, dip, sp | (dp << 16), proto};
        uint32_t w3 = 0;
        bool done;
        uint32_t fi = bucket_match<0xFFu>(row[0], row[1], row[2], row[3], key, &done, &w3);
        if (!done)
          fi = tbl_probe_from<0xFFu>(a.ft, (P.row + 1) & a.ft.bmask, key, a.ft.bmask, &w3);
        if (lds_be && fi != kNone) {  // a flow: its backend from LDS
          const uint32_t bi = w3 >> 8;
          const uint32_t meta = bnic[bi];
          const uint4 h = bhdr[bi];
          if (meta >> 16) {  // live: lb_main.c:56-65
            if (!a.binned) a.log[p] = fi;
            touch = fi;
            const uint32_t nic = meta & 0xFFFF;
            a.out[p] = (uint16_t)nic;
            if (nic == a.wan) return 0u;
            f.set32at2(30, h.x);  // dst_addr = backend.ip
            f.w[0] = h.y;
            f.w[1] = h.z;
            f.w[2] = h.w;
            fast_checksums(f, proto, tl);
            return 0xFu;
          }
        }
        // (no flow, a backend gone, or backends not staged: the queues)
        const bool rw = lb_flow_found(a, p, fi, w3, [&](uint4 rec) {
          return lb_rewrite_fast(a, f, rec, proto, tl, p);
        }, &touch);
        // dst address, MACs and checksums change bytes 0-47 (and the TCP
        // checksum 50-51): the whole 64-byte slot is stored back, since a
        // partial-line write costs more than a whole one
        return rw ? 0xFu : 0u;
      },
      bins, TileQueue{}, cur, 0, 0, a.in0);
}
__global__ __launch_bounds__(256, 4) void lb_classify64(LbArgs a, uint32_t n_all,
                                                       TouchBins bins) {
  lb_tiles<4>(a, n_all, bins);
}
// one 1024-thread block per CU (as vignat's nat_classify64w; VIGPATH_LB_WAVES)
__global__ __launch_bounds__(1024, 1) void lb_classify64w(LbArgs a, uint32_t n_all,
                                                         TouchBins bins) {
  lb_tiles<16>(a, n_all, bins);
}

__global__ __launch_bounds__(256) void lb_classify(LbArgs a) {
  __shared__ uint32_t T[kLbTabs * 256];
  lb_load_tables(T, a.crc_tab);
  for (uint32_t p = a.p0 + blockIdx.x * blockDim.x + threadIdx.x; p < a.p1;
       p += gridDim.x * blockDim.x)
    lb_generic_a(a, T, T + kLbFlowTabs * 256, p);
}

// Re-classify queued packets (unmodified frames) against the current state.
__global__ void lb_resolve(LbArgs a, const uint32_t *list, uint32_t n) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x)
    lb_generic_a(a, a.crc_tab, a.crc_tab + kLbFlowTabs * 256, list[j]);
}

struct Parsed {
  GFrame f;
  L34 h;
  uint32_t sip, dip, sp, dp, proto;
};
__device__ __forceinline__ Parsed lb_parse(const LbArgs &a, uint32_t p) {
  Parsed r;
  r.f = GFrame{a.frames + (size_t)p * a.slot, a.slot};
  r.h = parse_l34(r.f, a.len[p]);
  r.proto = r.f.r8(r.h.ip + 9);
  r.sp = r.f.r16(r.h.l4);
  r.dp = r.f.r16(r.h.l4 + 2);
  r.sip = r.f.r32(r.h.ip + 12);
  r.dip = r.f.r32(r.h.ip + 16);
  return r;
}

// Stale flows with some backend alive: free + allocate hands back the same
// index, so the flow keeps it, points at its CHT choice (every packet of the
// flow computes the same choice) and is rejuvenated.
__global__ void lb_stale_reassign(LbArgs a, const uint32_t *list, uint32_t n) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const Parsed q = lb_parse(a, p);
    const uint32_t h = lbflow_hash(a.crc_tab, q.sip, q.dip, q.sp, q.dp, q.proto);
    uint32_t w3 = 0;
    const uint32_t fi =
        flow_probe(a.ft, h, q.sip, q.dip, q.sp | (q.dp << 16), q.proto, &w3);
    const uint32_t c = cht_choose(a, h);
    const uint32_t e = a.ft.slot_of[fi];
    a.ft.bk[e >> 2].k[e & 3][3] = q.proto | (c << 8);
    a.log[p] = fi;
    lb_rewrite_generic(a, q.f, q.h, a.be_rec[c], p);
  }
}

// Stale flows with no backend alive (single thread, packet order): the first
// packet of each erases the key and frees the index onto the free-list front
// (double-chain-impl.c:1968-1981); every such packet is dropped.
__global__ void lb_stale_free_seq(LbArgs a, const uint32_t *list, uint32_t n) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Ctl *ctl = a.ft.ctl;
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t p = list[j];
    const Parsed q = lb_parse(a, p);
    const uint32_t h = lbflow_hash(a.crc_tab, q.sip, q.dip, q.sp, q.dp, q.proto);
    uint32_t w3 = 0;
    const uint32_t fi =
        flow_probe(a.ft, h, q.sip, q.dip, q.sp | (q.dp << 16), q.proto, &w3);
    a.out[p] = port_of(a.in_dev, a.in0, p);  // backend.nic = wan device = in
    a.log[p] = kNone;
    if (fi == kNone) continue;  // freed by an earlier packet of the flow
    const uint32_t e = a.ft.slot_of[fi];
    a.ft.bk[e >> 2].idx[e & 3] = kTomb;
    a.ft.slot_of[fi] = kNone;
    a.ft.stack[ctl->stack_top++] = fi;
    ctl->n_live--;
    ctl->sh_live--;  // (the layout and rebuild checks count this rank's entries)
    ctl->n_tomb++;
  }
}

__global__ void lb_miss_keys(LbArgs a, const uint32_t *list, uint32_t n,
                             uint32_t *mkey, uint32_t *mhash) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const Parsed q = lb_parse(a, list[j]);
    uint32_t *k = mkey + 4 * (size_t)j;
    k[0] = q.sip;
    k[1] = q.dip;
    k[2] = q.sp | (q.dp << 16);
    k[3] = q.proto;
    mhash[j] = lbflow_hash(a.crc_tab, q.sip, q.dip, q.sp, q.dp, q.proto);
  }
}

// New flows (some backend alive): every packet goes to its CHT choice (also
// when the flow table is full, lb_balancer.c:66 "doesn't matter if we can't
// insert"); the first sighting records the choice as the flow's backend.
__global__ void lb_miss_finish(LbArgs a, const uint32_t *list, uint32_t n,
                               const uint32_t *mkey, const uint32_t *mhash,
                               const uint32_t *scratch, const uint32_t *rep,
                               const uint32_t *assign) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const uint32_t j0 = scratch[rep[j]];
    const uint32_t idx = assign[j0];
    const uint32_t c = cht_choose(a, mhash[j]);
    if (idx != kNone && j0 == j) {
      const uint32_t e = a.ft.slot_of[idx];
      a.ft.bk[e >> 2].k[e & 3][3] = mkey[4 * (size_t)j + 3] | (c << 8);
    }
    a.log[p] = idx;
    const Parsed q = lb_parse(a, p);
    lb_rewrite_generic(a, q.f, q.h, a.be_rec[c], p);
  }
}

__global__ void lb_drop_list(LbArgs a, const uint32_t *list, uint32_t n) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    a.out[p] = port_of(a.in_dev, a.in0, p);
    a.log[p] = kNone;
  }
}

__global__ void lb_hb_keys(LbArgs a, const uint32_t *list, uint32_t n,
                           uint32_t *mkey, uint32_t *mhash) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const Parsed q = lb_parse(a, list[j]);
    uint32_t *k = mkey + 4 * (size_t)j;
    k[0] = q.sip;
    k[1] = k[2] = k[3] = 0;
    mhash[j] = ip_hash(a.crc_tab + kLbFlowTabs * 256, q.sip);
  }
}

// New backends: the first sighting of an IP writes backends[idx] = {ip,
// s_addr, in device} (lb_balancer.c:119-133).
__global__ void lb_hb_finish(LbArgs a, const uint32_t *list, uint32_t n,
                             const uint32_t *scratch, const uint32_t *rep,
                             const uint32_t *assign) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const uint32_t j0 = scratch[rep[j]];
    const uint32_t idx = assign[j0];
    a.log2[p] = idx;
    if (idx == kNone || j0 != j) continue;
    const GFrame f{a.frames + (size_t)p * a.slot, a.slot};
    const L34 h = parse_l34(f, a.len[p]);
    const uint32_t m0 = f.r32(6), m1 = f.r16(10);
    a.be_rec[idx] = make_uint4(f.r32(h.ip + 12), m0, m1 | (port_of(a.in_dev, a.in0, p) << 16), 0);
  }
}

// ========================================================= one packet ==
// nf.c calls nf_process once per packet (nf.c:150-176) or once per small
// burst (its VIGOR_BATCH_SIZE loop, nf.c:178-215). vp_process_one and small
// vp_process_mbufs calls go to lb_serve, one wave that stays resident and
// polls the host-coherent mailbox (ServeBox, vp_internal.h), as nat_serve,
// fw_serve, bridge_serve and pol_serve do for their NFs: no launch and no
// copy call per packet. The kernel restates lb_main.c:20-68 and
// lb_balancer.c:38-143. Until the context has met a due expiry the host sends
// requests only while none is due on the flow table or on the backend table
// (serve_process_one / serve_process_burst) and the instance without the
// journal runs; from then on the instance with it runs lb_expire_flows and
// lb_expire_backends itself, from one touch journal per table (serve_expire,
// vp_serve_dev.h), at the top of every packet as lb_main.c:21-22 does -- before
// the parse, so a frame that is no TCP or UDP packet over IPv4 expires too.
// A backend the walk has freed is gone for the lookups behind it: they test
// slot_of, which the walk sets to kNone (cht_choose, lb_one, lb_burst).
//
// One case is left to the batch pipeline: a WAN packet whose flow points at a
// dead backend while no backend is alive erases the flow and frees its index
// (lb_stale_free_seq). lb_serve never erases: it declines such a request
// before the packet itself has written anything. The walk in front of it may
// have expired entries (it can be what took the last backend), which the
// answer still reports; the pipeline's own expiry at that packet then finds
// nothing left due.

// lb_one's answers that are no backend index.
constexpr uint32_t kLbPass = 0xFFFFFFFEu;     // out = in, the frame as it came
constexpr uint32_t kLbDecline = 0xFFFFFFFDu;  // the erasure: the batch pipeline's

// lb_main.c:56-65 on a register frame (IHL 5), the L4 bytes past byte 64
// summed in `tail`: the out port, *rew = 1 when the frame changed.
__device__ __forceinline__ uint32_t lb_serve_rewrite(const LbArgs &a, RFrame &f, uint4 rec,
                                                     uint32_t proto, uint32_t tl, uint32_t tail,
                                                     uint32_t *rew) {
  const uint32_t nic = rec.z >> 16;
  if (nic == a.wan) return nic;
  f.set32at2(30, rec.x);  // dst_addr = backend.ip
  uint32_t mw[3];
  backend_macs(a, rec, nic, mw);
  f.w[0] = mw[0];
  f.w[1] = mw[1];
  f.w[2] = mw[2];
  fast_checksums(f, proto, tl, tail);
  *rew = 1;
  return nic;
}

// A new flow's index for key (sip, dip, sp | dp << 16, proto) that the caller
// has just looked up in vain, its backend c in word 3 (serve_lan without the
// second lookup); kNone when no index is free.
__device__ __forceinline__ uint32_t lb_flow_new(const LbArgs &a, uint32_t h, uint32_t sip,
                                                uint32_t dip, uint32_t ports, uint32_t proto,
                                                uint32_t c, uint64_t seq, uint32_t *fresh) {
  const uint32_t key[4] = {sip, dip, ports, proto};
  return serve_lan_by(a.ft, h, key, proto | (c << 8), seq, fresh, [] { return kNone; });
}

// lb_process_heartbit (lb_balancer.c:114-143) for source address sip, source
// MAC (m0: bytes 6-9, m1: 10-11) on device `in`: the backend's index, allocated
// and its record written when the address is new (*fresh = 1), kNone when the
// backend table is full. The caller stamps it.
__device__ __forceinline__ uint32_t lb_backend_seen(const LbArgs &a, uint32_t hh, uint32_t sip,
                                                    uint32_t m0, uint32_t m1, uint32_t in,
                                                    uint64_t seq, uint32_t *fresh) {
  const uint32_t key[4] = {sip, 0, 0, 0};
  uint32_t born = 0;
  const uint32_t bi = serve_lan<0xFFFFFFFFu>(a.bt, hh, key, 0u, seq, &born);
  if (born) {
    a.be_rec[bi] = make_uint4(sip, m0, m1 | (in << 16), 0);
    *fresh = 1;
  }
  return bi;
}

// A stale flow fi (its backend is gone) re-pointed at backend c, as
// lb_stale_reassign does: free + allocate hands the same index back.
__device__ __forceinline__ void lb_flow_repoint(const LbArgs &a, uint32_t fi, uint32_t proto,
                                                uint32_t c) {
  const uint32_t e = a.ft.slot_of[fi];
  a.ft.bk[e >> 2].k[e & 3][3] = proto | (c << 8);
}

// lb_process in packet order for one parsed TCP/UDP packet: the backend whose
// record rewrites it, kLbPass or kLbDecline. *fresh: bit 0 a flow was
// allocated, bit 1 a backend. *tf, *tb: the flow and the backend index it
// stamped (the journals' touches; a packet stamps one of them or neither).
// T: the 17 CRC tables.
__device__ __forceinline__ uint32_t lb_one(const LbArgs &a, const uint32_t *T, uint32_t in,
                                           uint32_t sip, uint32_t dip, uint32_t sp, uint32_t dp,
                                           uint32_t proto, uint32_t m0, uint32_t m1, int64_t now,
                                           uint64_t seq, uint32_t *fresh, uint32_t *tf,
                                           uint32_t *tb) {
  if (in != a.wan) {  // a heartbeat
    uint32_t born = 0;
    const uint32_t bi =
        lb_backend_seen(a, ip_hash(T + kLbFlowTabs * 256, sip), sip, m0, m1, in, seq, &born);
    if (bi != kNone) serve_stamp(a.bt, bi, now, seq);
    *tb = bi;
    *fresh |= born << 1;
    return kLbPass;
  }
  const uint32_t h = lbflow_hash(T, sip, dip, sp, dp, proto);
  uint32_t w3 = 0;
  const uint32_t fi = flow_probe(a.ft, h, sip, dip, sp | (dp << 16), proto, &w3);
  if (fi != kNone) {
    uint32_t bi = w3 >> 8;
    if (a.bt.slot_of[bi] == kNone) {  // its backend is gone
      bi = cht_choose(a, h);
      if (bi == kNone) return kLbDecline;  // (the packet has written nothing so far)
      lb_flow_repoint(a, fi, proto, bi);
    }
    serve_stamp(a.ft, fi, now, seq);
    *tf = fi;
    return bi;
  }
  const uint32_t c = cht_choose(a, h);
  if (c == kNone) return kLbPass;  // no backend alive: nothing written
  uint32_t born = 0;
  const uint32_t idx = lb_flow_new(a, h, sip, dip, sp | (dp << 16), proto, c, seq, &born);
  if (idx != kNone) serve_stamp(a.ft, idx, now, seq);
  *tf = idx;
  *fresh |= born;
  return c;  // (also when no index was free, lb_balancer.c:66)
}

// A burst request (vp_serve_dev.h) for viglb. Round 0: every lane looks
// itself up in the state as the burst found it. Final there: a WAN hit on a
// live backend (nothing inside a burst changes that flow's backend or kills
// it), a heartbeat from a known address, and every frame that is no TCP or UDP
// packet over IPv4. Pending, all as burst_settle's lpend (the lowest pending
// lane runs per round, so they settle in packet order):
//   H  a heartbeat from an unknown address: allocates on the backend table,
//      and changes what cht_choose finds for every later lane;
//   M  a WAN miss: its choice depends on every H before it, its index on every
//      M before it, and a later lane with its key must take its backend;
//   S  a WAN hit on a dead backend: its choice depends on every H before it.
// Each looks again before it acts: H may find its address brought by an
// earlier lane (a plain stamp), M its key stored (a plain hit on the stored
// backend), S its backend index handed to an earlier H (which the reference
// then takes for the flow's live backend: a plain hit) or the flow re-pointed
// by an earlier S. As many rounds as pending lanes; steady traffic has none.
// The erasure (S with no backend alive) declines the burst: when round 0
// finds an S lane and the backend table's n_live is 0 behind the walks.
// Conservative (an earlier H of the burst might have revived a backend) but
// exact, since the pipeline then gets the burst whole; with n_live above 0
// there it stays so (nothing expires among the served lanes), and no S lane
// can find cht_choose empty later.
// With the journals on (J; jf / fs the flows', jb / bs the backends'), behind
// the IPv4-options decline, which still writes nothing: both journals need
// room or the answer is kBurstFull with nothing done; then both walks at the
// first packet's time and the cut (burst_split2) -- *k <= n packets are served,
// round 0, the settle loop, the stamps and the rewrite run over those lanes
// only, and the winners of the two stamp passes are the journals' touches. A
// backend the walk has freed is dead for round 0 (slot_of), so its flows are
// S lanes; the erasure's decline comes behind the walk, which may be what
// took n_live to 0, and the caller reports what the walk did with it.
template <bool J>
__device__ __forceinline__ uint32_t lb_burst(const LbArgs &a, const uint32_t *T, ServeBox *box,
                                             uint32_t n, uint64_t seq0, uint32_t lane,
                                             const JournalDev &jf, JournalSt &fs,
                                             const JournalDev &jb, JournalSt &bs, uint32_t *k) {
  BurstIn b = burst_load(box, n, lane);
  const BurstHdr h = burst_hdr(b);
  if (h.decline) return kBurstDeclined;
  int64_t now0 = 0;
  bool go = h.go;
  if (J) {
    n = burst_split2(a.ft, jf, fs, a.bt, jb, bs, b, n, lane, &now0);
    if (!n) return kBurstFull;
    go = go && lane < n;
  }
  *k = n;
  RFrame &f = b.f;
  const uint32_t in = b.in;
  // the L4 checksum's bytes past 64, [64, min(14 + total_length, len)), summed
  // straight from the mailbox (as nat_serve's burst)
  uint32_t tail = 0;
  {
    const uint32_t end = go && in == a.wan ? min(14 + h.tl, b.len) : 0u;
    for (uint32_t base = 64; __ballot(base < end); base += 128) {
      v4u x[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        const uint32_t cc = base + 16 * u;
        x[u] = __builtin_amdgcn_raw_buffer_load_b128(
            b.fs, (int)(cc < end ? b.slot0 + cc : kBurstBody), 0, kSys);
      }
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        const uint32_t cc = base + 16 * u;
        tail = sum16x4(
            chunk_keep(make_uint4(x[u][0], x[u][1], x[u][2], x[u][3]), 0, (int)end - (int)cc),
            tail);
      }
    }
  }
  const bool hbp = go && in != a.wan, wanp = go && in == a.wan;
  const uint32_t ports = h.sp | (h.dp << 16);
  const uint32_t hf = lbflow_hash_batched(T, h.sip, h.dip, h.sp, h.dp, h.proto);
  const uint32_t hi = ip_hash(T + kLbFlowTabs * 256, h.sip);
  const uint32_t m0 = f.u32at2(6), m1 = f.w[2] >> 16;  // a heartbeat's source MAC
  // round 0. fi: the flow to stamp, bi: the backend to stamp, be: the backend
  // whose record rewrites the frame
  uint32_t fi = kNone, bi = kNone, be = kNone, w3 = 0, fresh = 0;
  auto flow_look = [&] {  // a flow whose backend is alive: final
    fi = flow_probe(a.ft, hf, h.sip, h.dip, ports, h.proto, &w3);
    if (fi != kNone && a.bt.slot_of[w3 >> 8] != kNone) be = w3 >> 8;
  };
  if (hbp) {
    const uint32_t key[4] = {h.sip, 0, 0, 0};
    bi = tbl_probe(a.bt, hi, key);
  }
  if (wanp) flow_look();
  const bool stale = wanp && fi != kNone && be == kNone;
  if (a.bt.ctl->n_live == 0 && __ballot(stale)) return kBurstDeclined;
  burst_settle(
      lane, hbp ? bi == kNone : wanp && be == kNone, false, [] {},
      [&] {
        if (hbp) {
          uint32_t born = 0;
          bi = lb_backend_seen(a, hi, h.sip, m0, m1, in, seq0 + lane, &born);
          fresh |= born << 1;
          return;
        }
        flow_look();
        if (be != kNone) return;  // stored, re-pointed or revived by an earlier lane
        const uint32_t c = cht_choose(a, hf);
        if (c == kNone) {  // a miss with no backend alive: nothing written
          fi = kNone;
          return;
        }
        if (fi != kNone) {
          lb_flow_repoint(a, fi, h.proto, c);
        } else {
          uint32_t born = 0;
          fi = lb_flow_new(a, hf, h.sip, h.dip, ports, h.proto, c, seq0 + lane, &born);
          fresh |= born;
        }
        be = c;
      });
  // Stamps, once over the flow indices and once over the backend indices: a
  // packet that went to a backend stamps its flow if it has one (a miss that
  // found no index free has none), a heartbeat its backend.
  if (be == kNone) fi = kNone;
  const bool fwon = burst_last(fi, n, lane), bwon = burst_last(bi, n, lane);
  if (fwon) serve_stamp(a.ft, fi, b.now, seq0 + lane);
  if (bwon) serve_stamp(a.bt, bi, b.now, seq0 + lane);
  if (J) {
    journal_touch_burst(jf, fs, fwon, fi, seq0 + lane, now0, lane);
    journal_touch_burst(jb, bs, bwon, bi, seq0 + lane, now0, lane);
  }
  // the rewrite, each lane its own frame; back go a rewritten frame's first 64
  // bytes (a rewrite touches nothing past byte 51)
  uint32_t out = in, rew = 0;
  if (be != kNone) out = lb_serve_rewrite(a, f, a.be_rec[be], h.proto, h.tl, tail, &rew);
  if (rew) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      __builtin_amdgcn_raw_buffer_store_b128(
          (v4u){f.w[4 * j], f.w[4 * j + 1], f.w[4 * j + 2], f.w[4 * j + 3]}, b.fs,
          (int)(b.slot0 + 16 * j), 0, kSys);
  }
  burst_out(b, (out & 0xFFFFu) | ((fresh & 1u) << 16) | (rew << 17) | ((fresh >> 1) << 18), n,
            lane);
  return kBurstServed;
}

// The server: one wave (<<<1, 64>>>). Every poll reads the request chunks
// whole; a one-packet request brings a frame of up to kServeInline bytes in
// them, a longer one whole through `frame`. The frame goes into LDS, the wave
// sums the L4 bytes past byte 64, lane 0 runs the packet (in registers when
// IHL = 5, byte-addressed over the LDS copy otherwise), the frame goes back
// and the answer follows: out | flow allocated << 16 | backend allocated << 18,
// or kOneDeclined when the packet is the erasure and has written nothing.
// Packets take global sequence numbers seq0, seq0 + 1, ...; a burst request
// (lb_burst) takes as many as it serves, a declined request none. The kernel
// leaves on the leave request or after `idle` wall-clock ticks without a
// request; the host launches it again (serve_wait). flags: serve_poll's.
// J: the kernel expires from the touch journals jf (flows, a.ft) and jb
// (backends, a.bt), whose control words it keeps in registers (fs, bs) and
// stores back after every request; the whole wave walks both before lane 0
// parses, and the answer carries the two walks' count (their sum) and
// kOneTombs / kBurstTombs when either table passed its purge bound -- also
// beside kOneDeclined / kBurstDeclined, whose walk is done all the same. A
// context whose journals are off runs the instance without any of it.
template <bool J>
__global__ __launch_bounds__(64) void lb_serve(LbArgs a, ServeBox *box, uint64_t seq0,
                                               uint64_t idle, uint32_t flags, JournalDev jf,
                                               JournalDev jb) {
  __shared__ uint32_t T[kLbTabs * 256];
  __shared__ uint4 fr[kServeFrame / 16];
  const uint32_t lane = threadIdx.x;
  lb_load_tables(T, a.crc_tab);
  const ServeIo io = serve_io(box, lane);
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(box->frame, 0, kServeFrame, 0x00020000);
  uint32_t *fw = reinterpret_cast<uint32_t *>(fr);
  // the last answered request (a relaunched server goes on from the answer
  // word), the next packet's sequence, the last answer's wall clock
  uint32_t done = __builtin_amdgcn_readfirstlane((uint32_t)__hip_atomic_load(
      &box->ans, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
  uint64_t seq = seq0;
  uint64_t t0 = wall_clock64();
  // the touch journals' control words
  JournalSt fs = journal_load(J ? jf : JournalDev{});
  JournalSt bs = journal_load(J ? jb : JournalDev{});
  auto serve = [&](const v4u &c) -> int {
    const uint32_t want = done + 1;
    if (__builtin_amdgcn_readfirstlane(c[3]) != want) return -1;
    const uint32_t hi = __builtin_amdgcn_readfirstlane(c[0]);
    if (hi == kServeLeave) return 1;
    const uint32_t in = hi >> 16;
    fs.expired = 0, fs.flags = 0;
    bs.expired = 0, bs.flags = 0;
    if ((hi & 0xFFFFu) == kServeBurstOp) {  // chunk 0 alone, the frames in the burst body
      uint32_t bn = min(max(in, 1u), kServeBurst);
      uint32_t st = lb_burst<J>(a, T, box, bn, seq, lane, jf, fs, jb, bs, &bn);
      if (J && st != kBurstFull) {  // (a declined burst's walk counts too)
        if (fs.flags | bs.flags) st |= kBurstTombs;
        journal_store(jf, fs, lane);
        journal_store(jb, bs, lane);
      }
      if (lane == 0) burst_answer(io, box, st, bn, want, fs.expired + bs.expired);
      if ((st & 0xFFu) == kBurstServed) seq += bn;
      t0 = wall_clock64();
      done = want;
      // (every lane's table writes before the next request reads them)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      return 0;
    }
    const uint32_t len = min(hi & 0xFFFFu, kServeFrame);
    const bool inl = len <= kServeInline;
    const uint32_t need = inl ? (12 + len + 11) / 12 : 1u;  // chunks carrying it
    if (__ballot(lane < need && c[3] != want)) return -1;  // not whole yet: poll again
    // chunk 0's time (message bytes 4-11), its words widened unsigned (as
    // pol_serve: serve_now sign-extends a low word whose bit 31 is set)
    const int64_t now =
        (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(c[1]) |
                  ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(c[2]) << 32));
    const uint32_t nch = (len + 15) / 16;
    if (inl) {
      serve_chunks_in(fw, c, lane, need);
    } else {  // the whole frame from `frame` (the host wrote it before the chunks)
      for (uint32_t i = lane; i < nch; i += 64) {
        const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(16 * i), 0, kSys);
        fr[i] = make_uint4(v[0], v[1], v[2], v[3]);
      }
    }
    wave_lds_sync();
    // the L4 checksum's bytes past 64: [64, min(14 + total_length, len))
    uint32_t tail = 0;
    if (len > 64) {
      const uint8_t *fb = reinterpret_cast<const uint8_t *>(fr);
      const uint32_t tl = ((uint32_t)fb[16] << 8) | fb[17];
      const uint32_t end = min(14 + tl, len);
      for (uint32_t cc = 64 + 16 * lane; cc < end; cc += 1024)
        tail = sum16x4(chunk_keep(fr[cc / 16], 0, (int)end - (int)cc), tail);
      for (int o = 32; o > 0; o >>= 1) tail += __shfl_xor(tail, o);
    }
    // lb_main.c:21-22: both expiries before the parse, whatever the frame is
    const bool full = J && !(journal_room(jf, fs, 1) && journal_room(jb, bs, 1));
    if (J && !full) {
      serve_expire(a.ft, jf, fs, journal_cutoff(jf, now), lane);
      serve_expire(a.bt, jb, bs, journal_cutoff(jb, now), lane);
    }
    uint32_t res = 0, tf = kNone, tb = kNone;
    if (full) res = kOneFull;  // (nothing is done: seeded again)
    if (lane == 0 && !full) {
      uint32_t fresh = 0, out = in, be = kLbPass;
      RFrame f = serve_rframe([&](int j) { return fr[j]; }, len);
      const uint32_t et = f.w[3] & 0xFFFF, ihl = (f.w[3] >> 16) & 0x0F;
      if (et == 0x0008 && ihl == 5) {  // in registers (lb_main.c:27-38's tests)
        const uint32_t tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
        const uint16_t unread = (uint16_t)(len - 14);
        const uint32_t proto = f.w[5] >> 24;
        if ((unread >= 20) & (unread >= tl) & ((proto == 6) | (proto == 17)) &
            ((uint32_t)(len - 34) >= 4u)) {
          be = lb_one(a, T, in, f.u32at2(26), f.u32at2(30), f.w[8] >> 16, f.w[9] & 0xFFFF, proto,
                      f.u32at2(6), f.w[2] >> 16, now, seq, &fresh, &tf, &tb);
          if (be < kLbDecline) {
            uint32_t rew = 0;
            out = lb_serve_rewrite(a, f, a.be_rec[be], proto, tl, tail, &rew);
            if (rew) {
#pragma unroll
              for (int j = 0; j < 4; j++)
                fr[j] = make_uint4(f.w[4 * j], f.w[4 * j + 1], f.w[4 * j + 2], f.w[4 * j + 3]);
            }
          }
        }
      } else {  // byte-addressed over the LDS copy (IPv4 options)
        const GFrame g{reinterpret_cast<uint8_t *>(fr), len};
        const L34 l = parse_l34(g, len);
        if (l.ok) {
          be = lb_one(a, T, in, g.r32(l.ip + 12), g.r32(l.ip + 16), g.r16(l.l4), g.r16(l.l4 + 2),
                      g.r8(l.ip + 9), g.r32(6), g.r16(10), now, seq, &fresh, &tf, &tb);
          if (be < kLbDecline) {
            const uint4 rec = a.be_rec[be];
            out = rec.z >> 16;
            if (out != a.wan) {
              g.w32(l.ip + 16, rec.x);
              uint32_t mw[3];
              backend_macs(a, rec, out, mw);
              set_macs(g, mw);
              set_checksums(g, l.ip, l.l4);  // (the whole frame is in g)
            }
          }
        }
      }
      res = (out & 0xFFFFu) | ((fresh & 1u) << 16) | ((fresh >> 1) << 18) |
            (be == kLbDecline ? kOneDeclined : 0u);
    }
    wave_lds_sync();
    res = __builtin_amdgcn_readfirstlane(res);
    uint32_t expired = 0;
    if (J && !full) {
      res |= fs.flags | bs.flags;
      expired = fs.expired + bs.expired;
      journal_touch(jf, fs, __builtin_amdgcn_readfirstlane(tf), seq, now, lane);
      journal_touch(jb, bs, __builtin_amdgcn_readfirstlane(tb), seq, now, lane);
      journal_store(jf, fs, lane);
      journal_store(jb, bs, lane);
    }
    if (inl) {  // the answer chunks: the result and the frame in one store
      if (lane < need) {
        const v4u v = lane == 0 ? (v4u){res, expired, 0u, want}
                                : (v4u){fw[3 * lane - 3], fw[3 * lane - 2], fw[3 * lane - 1], want};
        __builtin_amdgcn_raw_buffer_store_b128(v, io.as, (int)(16 * lane), 0, kSys);
      }
    } else {
      for (uint32_t i = lane; i < nch; i += 64) {
        const uint4 v = fr[i];
        __builtin_amdgcn_raw_buffer_store_b128((v4u){v.x, v.y, v.z, v.w}, rs, (int)(16 * i), 0,
                                               kSys);
      }
      // (the frame complete before the answer chunk that announces it)
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      __builtin_amdgcn_s_waitcnt(0);
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      if (lane == 0)
        __builtin_amdgcn_raw_buffer_store_b128((v4u){res, expired, 0u, want}, io.as, 0, 0, kSys);
    }
    if (lane == 0) {
      // (the answer word: where a relaunched server starts counting; the host
      // reads the answer chunks. No release fence at system scope, which would
      // write back the whole L2)
      __hip_atomic_store(&box->ans, (uint64_t)want | ((uint64_t)res << 32), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!(res & (kOneDeclined | kOneFull))) seq += 1;
    t0 = wall_clock64();
    done = want;
    // (lane 0's table writes before the next request's lanes read them)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    wave_lds_sync();
    return 0;
  };
  serve_poll(io, flags, idle, serve, [&] { return t0; });
}

// =============================================================== host ==

static inline int64_t lb_flow_cutoff(const vp_ctx *c, int64_t t) {
  return (int64_t)((uint64_t)t - (uint64_t)((int64_t)c->lb.flow_expiration_time * 1000));
}
static inline int64_t lb_backend_cutoff(const vp_ctx *c, int64_t t) {
  return (int64_t)((uint64_t)t -
                   (uint64_t)((int64_t)c->lb.backend_expiration_time * 1000));
}

struct Queues {
  const uint32_t *m, *s, *h;
  uint32_t nm, ns, nh;
};

// One round (see the header): stale flows, new flows, then new backends.
static int lb_round(vp_ctx *c, LbArgs &a, const Queues &q, uint32_t *allocated) {
  Workspace &w = c->ws;
  VP_TRY(read_ctl(c, c->ft2));
  const bool alive = c->ft2.h_ctl.n_live > 0;
  if (q.ns) {
    if (alive) {
      lb_stale_reassign<<<grid_for(q.ns), 256, 0, c->stream>>>(a, q.s, q.ns);
    } else {
      lb_stale_free_seq<<<1, 64, 0, c->stream>>>(a, q.s, q.ns);
      VP_HIP(hipGetLastError());
      VP_TRY(tbl_check_tombs(c, c->ft));
      a.ft = tbl_dev(c->ft);
    }
    VP_HIP(hipGetLastError());
  }
  if (q.nm) {
    if (alive) {
      lb_miss_keys<<<grid_for(q.nm), 256, 0, c->stream>>>(a, q.m, q.nm, w.mkey,
                                                          w.mhash);
      VP_HIP(hipGetLastError());
      VP_TRY(tbl_new_keys(c, c->ft, NewKeys{q.nm, q.m}, c->seq, nullptr));
      a.ft = tbl_dev(c->ft);
      lb_miss_finish<<<grid_for(q.nm), 256, 0, c->stream>>>(
          a, q.m, q.nm, w.mkey, w.mhash, w.scratch, w.rep, w.assign);
      *allocated |= 1u;
    } else {
      lb_drop_list<<<grid_for(q.nm), 256, 0, c->stream>>>(a, q.m, q.nm);
    }
    VP_HIP(hipGetLastError());
  }
  if (q.nh) {
    lb_hb_keys<<<grid_for(q.nh), 256, 0, c->stream>>>(a, q.h, q.nh, w.mkey, w.mhash);
    VP_HIP(hipGetLastError());
    VP_TRY(tbl_new_keys(c, c->ft2, NewKeys{q.nh, q.h}, c->seq, nullptr));
    a.bt = tbl_dev(c->ft2);
    lb_hb_finish<<<grid_for(q.nh), 256, 0, c->stream>>>(a, q.h, q.nh, w.scratch,
                                                        w.rep, w.assign);
    VP_HIP(hipGetLastError());
    *allocated |= 2u;
  }
  return 0;
}

static int zero_queues(vp_ctx *c) {
  VP_HIP(hipMemsetAsync(&c->ft.ctl->miss_count, 0, 8, c->stream));  // M, S
  VP_HIP(hipMemsetAsync(&c->ft2.ctl->miss_count, 0, 4, c->stream));  // H
  return 0;
}

static int lb_segment(vp_ctx *c, const vp_dev_batch *b, const NowSpec &now,
                      uint32_t p0, uint32_t p1, float *ms, int *launches,
                      uint32_t *allocated) {
  Workspace &w = c->ws;
  LbArgs a{};
  a.frames = b->frames;
  a.len = b->len;
  a.in_dev = b->in_dev;
  a.in0 = b->in_dev ? 0u : b->in_port;  // (port_of: exactly one is live)
  a.out = b->out_dev;
  a.log = w.log;
  a.log2 = w.log2;
  a.slot = b->slot;
  a.p0 = p0;
  a.p1 = p1;
  a.ft = tbl_dev(c->ft);
  a.bt = tbl_dev(c->ft2);
  a.be_rec = c->be_rec;
  a.cht = c->cht;
  a.height = c->lb.cht_height;
  a.bcap = c->lb.backend_capacity;
  a.crc_tab = c->crc_tab;
  a.dmacw = c->dmacw;
  a.miss = w.miss;
  a.stale = w.defer;
  a.hb = w.aux;
  a.hbl = w.hbl;
  a.wan = c->lb.wan_device;
  a.n_dev = c->lb.n_devices;

  // the counters are still zero after a segment that queued nothing (no
  // misses, stale flows, heartbeats or bin overflows): no reset launches
  if (!c->ft.ctl_clean) {
    VP_TRY(zero_queues(c));
    VP_HIP(hipMemsetAsync(&c->ft2.ctl->defer_count, 0, 4, c->stream));  // heartbeats
    VP_HIP(hipMemsetAsync(&c->ft.ctl->touch_ovf, 0, 4, c->stream));
  }
  c->ft.ctl_clean = false;
  BinsPlan bp{};
  const bool tiles64 = b->slot == 64;
  VP_HIP(ev_record(c->ktime, c->ev0, c->stream));
  if (tiles64) {
    // the flow touches go to the touch bins (256 of them: lb_classify64 keeps
    // 256 bin cursors; a larger table logs every touch and refolds the log)
    static const uint32_t lw = [] {  // waves per block (VIGPATH_LB_WAVES: 4 or 16)
      const char *e = getenv("VIGPATH_LB_WAVES");
      return e && atoi(e) == 16 ? 16u : 4u;
    }();
    const void *k = lw == 16 ? (const void *)lb_classify64w : (const void *)lb_classify64;
    VP_TRY(tbl_bins_plan(c, c->ft, k, p0, p1, &bp, lw));
    if (bp.on && bp.bins.bbits > 8) bp = BinsPlan{};
    const uint32_t tiles = (p1 - (p0 & ~63u) + 63) / 64;
    const uint32_t grid = bp.on ? bp.grid : resident_grid(k, (tiles + lw - 1) / lw, 64 * (int)lw);
    LbArgs a64 = a;
    a64.binned = bp.on;
    c->last_kernel = lw == 16 ? "lb_classify64w" : "lb_classify64";
    if (lw == 16)
      lb_classify64w<<<grid, 1024, 0, c->stream>>>(a64, b->n, bp.bins);
    else
      lb_classify64<<<grid, 256, 0, c->stream>>>(a64, b->n, bp.bins);
  } else {
    lb_classify<<<grid_for(p1 - p0), 256, 0, c->stream>>>(a);
  }
  VP_HIP(hipGetLastError());
  VP_HIP(ev_record(c->ktime, c->ev1, c->stream));
  a.hbl = nullptr;  // re-classification rounds list no heartbeat twice
  if (bp.on) {
    // optimistic fold; its first thread publishes phase A's counts (the flow
    // table's control block, and the backend table's H and heartbeat counts
    // as extra words), which the host waits for while the fold runs
    static_assert(offsetof(Ctl, defer_count) == offsetof(Ctl, miss_count) + 4, "H, heartbeats");
    const uint32_t epoch = ++c->ft.pub_epoch;
    VP_TRY(tbl_bins_reduce(c, c->ft, bp, p0, now, c->seq,
                           PubArgs{c->ft.d_pub, c->ft.ctl, epoch, &c->ft2.ctl->miss_count,
                                   nullptr, 2, 0}));
    VP_TRY(tbl_wait_pub(c, c->ft, epoch));
    c->ft2.h_ctl.miss_count = c->ft.h_pub->xtra[0];
    c->ft2.h_ctl.defer_count = c->ft.h_pub->xtra[1];
  } else {
    // phase A's counts are copied out before the fold and waited for alone
    VP_TRY(read_ctl2_post(c, c->ft2, c->ft));
    VP_TRY(tbl_touch_reduce(c, c->ft, w.log, p0, p1, now, c->seq));
    VP_TRY(read_ctl2_wait(c, c->ft2, c->ft));
  }
  VP_TRY(seg_classify_ms(c, ms, launches));
  const uint32_t nm = c->ft.h_ctl.miss_count, ns = c->ft.h_ctl.defer_count;
  const uint32_t nh = c->ft2.h_ctl.miss_count, nhb = c->ft2.h_ctl.defer_count;
  const bool ovf = bp.on && c->ft.h_ctl.touch_ovf != 0;

  std::vector<uint32_t> M_all, S_all;  // phase A's queues (multi-round segments)
  if (nm || ns || nh) {
    VP_TRY(sort_keys(c, w.miss, w.miss_sorted, nm));
    VP_TRY(sort_keys(c, w.defer, w.defer_sorted, ns));
    VP_TRY(sort_keys(c, w.aux, w.aux_sorted, nh));
    if (!nh) {
      VP_TRY(lb_round(c, a, Queues{w.miss_sorted, w.defer_sorted, nullptr, nm, ns, 0},
                      allocated));
    } else {
      std::vector<uint32_t> M(nm), S(ns), H(nh);
      VP_HIP(hipMemcpyAsync(M.data(), w.miss_sorted, 4ull * nm,
                            hipMemcpyDeviceToHost, c->stream));
      VP_HIP(hipMemcpyAsync(S.data(), w.defer_sorted, 4ull * ns,
                            hipMemcpyDeviceToHost, c->stream));
      VP_HIP(hipMemcpyAsync(H.data(), w.aux_sorted, 4ull * nh,
                            hipMemcpyDeviceToHost, c->stream));
      VP_HIP(hipStreamSynchronize(c->stream));
      M_all = M;
      S_all = S;
      uint32_t im = 0, is = 0, ih = 0;
      bool first = true;
      std::vector<uint32_t> rl;
      while (im < nm || is < ns || ih < nh) {
        uint32_t end = p1;
        if (ih < nh) {  // stop before the first WAN packet after H[ih]
          const uint32_t h = H[ih];
          const uint32_t wm = (uint32_t)(std::lower_bound(M.begin() + im, M.end(), h) - M.begin());
          const uint32_t ws_ = (uint32_t)(std::lower_bound(S.begin() + is, S.end(), h) - S.begin());
          end = std::min(wm < nm ? M[wm] : p1, ws_ < ns ? S[ws_] : p1);
        }
        const uint32_t jm = (uint32_t)(std::lower_bound(M.begin() + im, M.end(), end) - M.begin());
        const uint32_t js = (uint32_t)(std::lower_bound(S.begin() + is, S.end(), end) - S.begin());
        const uint32_t jh = (uint32_t)(std::lower_bound(H.begin() + ih, H.end(), end) - H.begin());
        if (first) {
          VP_TRY(lb_round(c, a,
                          Queues{w.miss_sorted + im, w.defer_sorted + is,
                                 w.aux_sorted + ih, jm - im, js - is, jh - ih},
                          allocated));
          first = false;
        } else {
          // re-classify against the state earlier rounds left
          rl.assign(M.begin() + im, M.begin() + jm);
          rl.insert(rl.end(), S.begin() + is, S.begin() + js);
          rl.insert(rl.end(), H.begin() + ih, H.begin() + jh);
          if (!rl.empty()) {
            VP_HIP(hipMemcpyAsync(w.rlist, rl.data(), 4 * rl.size(),
                                  hipMemcpyHostToDevice, c->stream));
            VP_TRY(zero_queues(c));
            a.ft = tbl_dev(c->ft);
            a.bt = tbl_dev(c->ft2);
            lb_resolve<<<grid_for(rl.size()), 256, 0, c->stream>>>(a, w.rlist,
                                                                  (uint32_t)rl.size());
            VP_HIP(hipGetLastError());
            VP_TRY(read_ctl2(c, c->ft2, c->ft));
            const uint32_t rm = c->ft.h_ctl.miss_count, rs = c->ft.h_ctl.defer_count;
            const uint32_t rh = c->ft2.h_ctl.miss_count;
            VP_TRY(sort_keys(c, w.miss, w.miss_sorted, rm));
            VP_TRY(sort_keys(c, w.defer, w.defer_sorted, rs));
            VP_TRY(sort_keys(c, w.aux, w.aux_sorted, rh));
            VP_TRY(lb_round(c, a, Queues{w.miss_sorted, w.defer_sorted, w.aux_sorted,
                                         rm, rs, rh},
                            allocated));
          }
        }
        a.ft = tbl_dev(c->ft);
        a.bt = tbl_dev(c->ft2);
        im = jm;
        is = js;
        ih = jh;
      }
    }
  }
  if (bp.on) {
    // the fold applied phase A's binned touches; the packets the rounds
    // finished (the M and S queues) and the touches a full bin slice queued
    // follow as late touches (last toucher in packet order still wins)
    if (ovf)
      VP_TRY(tbl_late_touches(c, c->ft, bp.bins.oent, bp.bins.ocnt, 0, bp.range, bp.grid,
                              w.log, now, c->seq));
    if (nm || ns) {
      const uint32_t *lm = w.miss_sorted, *ls = w.defer_sorted;
      if (nh) {  // (the rounds re-sorted the queues: the phase-A lists again)
        VP_HIP(hipMemcpyAsync(w.rlist, M_all.data(), 4ull * nm, hipMemcpyHostToDevice,
                              c->stream));
        VP_HIP(hipMemcpyAsync(w.rlist + nm, S_all.data(), 4ull * ns, hipMemcpyHostToDevice,
                              c->stream));
        lm = w.rlist;
        ls = w.rlist + nm;
      }
      if (nm) VP_TRY(tbl_late_list(c, c->ft, lm, nm, w.log, now, c->seq));
      if (ns) VP_TRY(tbl_late_list(c, c->ft, ls, ns, w.log, now, c->seq));
    }
  } else if (nm || ns || nh) {
    // the rounds completed the log: refold it
    VP_TRY(tbl_touch_reduce(c, c->ft, w.log, p0, p1, now, c->seq));
  }
  if (nhb)  // the heartbeats' backend touches (log2 holds only theirs)
    VP_TRY(tbl_late_list(c, c->ft2, w.hbl, nhb, w.log2, now, c->seq));
  // steady state: frames and ports complete, only the flow fold may still
  // run (not when it reads the caller's time array)
  c->fold_pending = !(nm || ns || nh || ovf || nhb) && !b->now;
  c->ft.ctl_clean = !(nm || ns || nh || ovf || nhb);
  return 0;
}

static int lb_process_device(vp_ctx *c, const vp_dev_batch *b) {
  ExpiringTable tabs[2] = {{&c->ft, lb_flow_cutoff}, {&c->ft2, lb_backend_cutoff}};
  return run_batch(c, b, tabs, 2, lb_segment);
}

// ---------------------------------------------------- vp_process_one --
// viglb's launcher of the resident kernel (serve_launch, vp_serve.hip): of
// LbArgs what lb_serve reads -- both tables, the backend records, the CHT, the
// CRC tables and the devices' MACs; the batch's fields stay empty. The
// instance with the journals runs once both tables' are seeded (serve_ready
// seeds them together).
static int lb_serve_launch(vp_ctx *c, ServeBox *dbox, uint32_t flags) {
  LbArgs a{};
  a.ft = tbl_dev(c->ft);
  a.bt = tbl_dev(c->ft2);
  a.be_rec = c->be_rec;
  a.cht = c->cht;
  a.height = c->lb.cht_height;
  a.bcap = c->lb.backend_capacity;
  a.crc_tab = c->crc_tab;
  a.dmacw = c->dmacw;
  a.wan = c->lb.wan_device;
  a.n_dev = c->lb.n_devices;
  const JournalDev jf = serve_journal_dev(c, lb_ops().serve),
                   jb = serve_journal_dev(c, lb_ops().serve, true);
  if (jf.ctl && jb.ctl)
    lb_serve<true><<<1, 64, 0, c->stream>>>(a, dbox, c->seq, c->srv_idle, flags, jf, jb);
  else
    lb_serve<false><<<1, 64, 0, c->stream>>>(a, dbox, c->seq, c->srv_idle, flags, JournalDev{},
                                             JournalDev{});
  VP_HIP(hipGetLastError());
  return 0;
}

// The largest host batch routed to the server as burst requests: the largest
// swept n at which the served path measured faster per packet than the batch
// pipeline on the MI355X (profiles/r12_lb_serve.txt: 0.30 against 1.07-1.10
// us at 64, 0.296-0.299 against 0.553-0.560 at 128; at 256 the pipeline wins,
// 0.284-0.289 against 0.296-0.298, and by more at 384 and 512); larger calls
// take the pipeline. Below the other servers' 256 to 512: a served viglb frame
// crosses whole and 64 bytes of it come back, which costs 0.30 us per packet
// whatever the burst, and steady traffic costs viglb's pipeline no sort.
// VIGPATH_SERVE_BURST overrides it; 0 routes nothing.
constexpr uint32_t kLbBurstRoute = 128;

// viglb through the mailbox (serve_process_one / serve_process_burst,
// vp_serve.hip). The transfer sizes are vignat's: a rewrite changes bytes 0-11
// and 24-25, 30-33, 40-41 or 50-51, and the L4 checksum is recomputed over
// [34, 14 + total_length), so the whole frame goes, one longer than
// kServeInline through `frame`, and a burst's frame comes back in its first 64
// bytes. Two expiring tables, each with its own lifetime and its own touch
// journal: the kernel expires both. No stage clock.
const NfOps &lb_ops() {
  static const NfOps ops = [] {
    NfOps o{};
    o.process_device = lb_process_device;  o.serve_launch = lb_serve_launch;
    o.n_devices = [](const vp_ctx *c) -> uint32_t { return c->lb.n_devices; };
    o.reads_in_port = true;  // (LbArgs::in0)
    ServeNf &s = o.serve;
    s.cutoff = lb_flow_cutoff;  s.table = &vp_ctx::ft;
    s.one_whole = true;  s.one_in = kServeInline;  s.one_back = kServeInline;
    s.burst_in = kServeFrame;  s.burst_back = 64;  s.burst_route = kLbBurstRoute;
    s.prof = false;  s.journal = true;
    s.cutoff2 = lb_backend_cutoff;  s.table2 = &vp_ctx::ft2;
    return o;
  }();
  return ops;
}

void build_lb_tables(std::vector<uint32_t> &tab) {
  tab.assign(kLbTabs * 256, 0);
  for (int j = 0; j < 13; j++)
    build_position_table(&tab[j * 256], kLbFlowPos[j], kLbFlowMsg);
  for (int j = 0; j < 4; j++) build_position_table(&tab[(13 + j) * 256], j, 4);
}

// cht_fill_cht (cht.c:546-877): backend i visits bucket
// (31 i mod h + ((i mod (h-1)) + 1) j) mod h in round j; each bucket's
// priority list is filled round by round, backends in index order.
void lb_fill_cht(uint32_t height, uint32_t bcap, std::vector<uint32_t> &cht) {
  cht.assign((size_t)height * bcap, 0);
  std::vector<uint32_t> fill(height, 0);
  for (uint32_t j = 0; j < height; j++)
    for (uint32_t i = 0; i < bcap; i++) {
      const uint64_t off = (uint64_t)(uint32_t)(i * 31u) % height;
      const uint64_t shift = (uint64_t)i % (height - 1) + 1;
      const uint32_t bucket = (uint32_t)((off + shift * j) % height);
      cht[(size_t)bucket * bcap + fill[bucket]++] = i;
    }
}

int lb_dump(vp_ctx *c, uint8_t *f_alloc, int64_t *f_ts, uint8_t *f_keys,
            uint32_t *f_backend, uint8_t *b_alloc, int64_t *b_ts, uint32_t *b_ip,
            uint8_t *b_mac, uint16_t *b_nic) {
  const uint32_t fc = c->ft.cap, bc = c->ft2.cap;
  std::vector<uint32_t> keys(4ull * std::max(fc, bc));
  VP_TRY(tbl_dump(c, c->ft, f_alloc, f_ts, keys.data()));
  for (uint32_t i = 0; i < fc; i++) {
    const uint32_t *k = &keys[4ull * i];
    uint8_t *o = f_keys + 16ull * i;
    memcpy(o, k, 12);
    o[12] = (uint8_t)k[3];
    o[13] = o[14] = o[15] = 0;
    f_backend[i] = k[3] >> 8;
  }
  VP_TRY(tbl_dump(c, c->ft2, b_alloc, b_ts, keys.data()));
  std::vector<uint4> rec(bc);
  VP_HIP(hipMemcpy(rec.data(), c->be_rec, sizeof(uint4) * bc, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < bc; i++) {
    b_ip[i] = rec[i].x;
    memcpy(b_mac + 6ull * i, &rec[i].y, 4);
    memcpy(b_mac + 6ull * i + 4, &rec[i].z, 2);
    b_nic[i] = (uint16_t)(rec[i].z >> 16);
  }
  return 0;
}

}  // namespace vp
