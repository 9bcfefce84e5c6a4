// vigbridge on MI355X: MAC learning + forwarding lookup over a packet batch.
//
// Reference behaviour (paths relative to the reference repository):
//   nf_process                 vigbridge/bridge_main.c:311-329
//   expiry                     bridge_expire_entries, bridge_main.c:29-36
//                              (u32 wrap of expiration_time * 1000 as vignat)
//   learn src -> in port       bridge_put_update_entry, bridge_main.c:63-89
//                              (a known MAC is only rejuvenated; its port is
//                              not updated)
//   lookup {dst, in} static,   bridge_get_device, bridge_main.c:38-61
//   then dst dynamic; miss -> FLOOD_FRAME; -2 -> drop (return in port)
//   rte_ether_addr_hash        libvig/verified/ether.c:61-90 (6 CRC steps)
//   static table               read_static_ft_from_file, bridge_main.c:130-230
//
// Same segment scheme as vignat (vp_nat.hip header):
//   phase A  hash + probe src and dst; a known src is logged for
//            rejuvenation, an unknown one queued; a dst known at segment
//            start (or in the static table) is forwarded at once, an unknown
//            one flooded provisionally;
//   phase B  queued src MACs are de-duplicated (earliest packet wins) and
//            given dchain indices in packet order; the first sighting's in
//            port becomes the entry's port;
//   phase C  (only when B learned something) provisionally flooded frames are
//            looked up again: a MAC learned by a packet at or before this one
//            (the packet's own src counts: learn precedes lookup) forwards
//            there.
//
// Dynamic table entry: key words {mac[0..3], mac[4..5], port, 0}. Only words
// 0-1 identify the MAC; word 2 carries the DynamicValue (dyn_vals vector in
// the reference) so one bucket read resolves a lookup.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "vp_serve_dev.h"
#include "vp_table.h"

namespace vp {

VP_PRELOAD_UNIT(bridge)


// rte_ether_addr_hash: crc32c_u32 of each byte in turn, so the non-zero byte
// positions of the 24-byte CRC message are 0, 4, 8, 12, 16, 20.
constexpr int kEthTabs = 6;
// StaticKey hash (generated; nested struct field hashed by its own hash):
// crc(crc(0, ether_hash(addr)), device), an 8-byte message with non-zero
// bytes 0-3 (the MAC hash) and 4-5 (the u16 device).
constexpr int kStatTabs = 6;
constexpr int kBridgeTabs = kEthTabs + kStatTabs;

__device__ __forceinline__ uint32_t eth_hash(const uint32_t *T, uint32_t m0,
                                             uint32_t m1) {
  return T[0 * 256 + (m0 & 0xFF)] ^ T[1 * 256 + ((m0 >> 8) & 0xFF)] ^
         T[2 * 256 + ((m0 >> 16) & 0xFF)] ^ T[3 * 256 + (m0 >> 24)] ^
         T[4 * 256 + (m1 & 0xFF)] ^ T[5 * 256 + ((m1 >> 8) & 0xFF)];
}
__device__ __forceinline__ uint32_t static_hash(const uint32_t *T, uint32_t eh,
                                                uint32_t dev) {
  const uint32_t *S = T + kEthTabs * 256;
  return S[0 * 256 + (eh & 0xFF)] ^ S[1 * 256 + ((eh >> 8) & 0xFF)] ^
         S[2 * 256 + ((eh >> 16) & 0xFF)] ^ S[3 * 256 + (eh >> 24)] ^
         S[4 * 256 + (dev & 0xFF)] ^ S[5 * 256 + ((dev >> 8) & 0xFF)];
}

// eth_hash of two MACs, the 12 table reads issued back to back and waited
// for once (as vignat's flowid_hash_batched; T must be the kernel's LDS
// tables): *hs of src {s0, s1}, *hd of dst {d0, d1}.
__device__ __forceinline__ uint32_t bridge_lds_addr(const void *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
#define VP_ETH_RD(t, a, off) \
  asm volatile("ds_read_b32 %0, %1 offset:" #off : "=v"(t) : "v"(a))
__device__ __forceinline__ void eth_hash2(const uint32_t *T, uint32_t s0, uint32_t s1,
                                          uint32_t d0, uint32_t d1, uint32_t *hs,
                                          uint32_t *hd) {
  const uint32_t base = bridge_lds_addr(T);
  auto at = [&](uint32_t byte) { return base + (byte << 2); };
  uint32_t a0, a1, a2, a3, a4, a5, b0, b1, b2, b3, b4, b5;
  VP_ETH_RD(a0, at(s0 & 0xFF), 0);
  VP_ETH_RD(a1, at((s0 >> 8) & 0xFF), 1024);
  VP_ETH_RD(a2, at((s0 >> 16) & 0xFF), 2048);
  VP_ETH_RD(a3, at(s0 >> 24), 3072);
  VP_ETH_RD(a4, at(s1 & 0xFF), 4096);
  VP_ETH_RD(a5, at((s1 >> 8) & 0xFF), 5120);
  VP_ETH_RD(b0, at(d0 & 0xFF), 0);
  VP_ETH_RD(b1, at((d0 >> 8) & 0xFF), 1024);
  VP_ETH_RD(b2, at((d0 >> 16) & 0xFF), 2048);
  VP_ETH_RD(b3, at(d0 >> 24), 3072);
  VP_ETH_RD(b4, at(d1 & 0xFF), 4096);
  VP_ETH_RD(b5, at((d1 >> 8) & 0xFF), 5120);
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(b0),
                 "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4), "+v"(b5));
  *hs = (a0 ^ a1 ^ a2) ^ (a3 ^ a4 ^ a5);
  *hd = (b0 ^ b1 ^ b2) ^ (b3 ^ b4 ^ b5);
}
#undef VP_ETH_RD

// map_get on the dynamic table keyed by words 0-1, from bucket b on;
// *port = entry word 2.
__device__ __forceinline__ uint32_t mac_probe_from(const TableDev &t, uint32_t b,
                                                   uint32_t m0, uint32_t m1,
                                                   uint32_t *port) {
  for (uint32_t i = 0; i <= t.bmask; i++) {
    const uint4 *q = reinterpret_cast<const uint4 *>(t.bk + b);
    const uint4 k0 = q[0], k1 = q[1], k2 = q[2], ix = q[3];
    if (ix.x == kEmpty) return kNone;
    if (ix.x != kTomb && k0.x == m0 && k0.y == m1) {
      *port = k0.z;
      return ix.x;
    }
    if (ix.y == kEmpty) return kNone;
    if (ix.y != kTomb && k1.x == m0 && k1.y == m1) {
      *port = k1.z;
      return ix.y;
    }
    if (ix.z == kEmpty) return kNone;
    if (ix.z != kTomb && k2.x == m0 && k2.y == m1) {
      *port = k2.z;
      return ix.z;
    }
    b = (b + 1) & t.bmask;
  }
  return kNone;
}
__device__ __forceinline__ uint32_t mac_probe(const TableDev &t, uint32_t h,
                                              uint32_t m0, uint32_t m1,
                                              uint32_t *port) {
  return mac_probe_from(t, home_bucket(h, t.bmask, t.mix, t.lin), m0, m1, port);
}

struct BridgeArgs {
  const uint8_t *frames;
  const uint16_t *in_dev;
  uint16_t *out;
  uint32_t *log;
  uint64_t seq_base;
  uint32_t slot, p0, p1;
  TableDev t;
  TableDev st;  // static table: bk/bmask/mix only; idx = rule number
  const int32_t *st_val;
  uint32_t n_static;
  const uint32_t *crc_tab;
  uint32_t *miss;
  uint32_t *defer;
};

// nf_process's return value for a forwarding decision (bridge_main.c:322-328).
__device__ __forceinline__ uint16_t resolve(int32_t fwd, uint32_t in) {
  if (fwd == -1) return VP_FLOOD_FRAME;
  if (fwd == -2) return (uint16_t)in;
  return (uint16_t)fwd;
}

// Ethernet header words: dst = {w0, w1 & 0xFFFF}, src = {w1 >> 16 | w2 << 16,
// w2 >> 16} (bridge_main.c:312 borrows 14 bytes with no length check).
__device__ __forceinline__ uint4 eth_words(const BridgeArgs &a, uint32_t p) {
  return frame_ld16(a.frames + (size_t)p * a.slot);
}

// One dynamic-table bucket against a MAC (words 0-1): the index and *port
// (entry word 2) on a match; kNone with *done on an empty entry; kNone with
// !*done when the probe continues in the next bucket. Entries in order, the
// first match or empty entry decides; branch-free with static indices (an
// early return per entry made the entry number dynamic and put the whole
// row in scratch memory: 64 B per packet of stores, the bridge's write
// traffic in round 2).
__device__ __forceinline__ uint32_t mac_match(const uint4 *row, uint32_t m0, uint32_t m1,
                                              uint32_t *port, bool *done) {
  const uint4 ix = row[3];
  const bool e0 = ix.x == kEmpty, e1 = ix.y == kEmpty, e2 = ix.z == kEmpty;
  const bool h0 = !e0 & (ix.x != kTomb) & (row[0].x == m0) & (row[0].y == m1);
  const bool h1 = !e1 & (ix.y != kTomb) & (row[1].x == m0) & (row[1].y == m1);
  const bool h2 = !e2 & (ix.z != kTomb) & (row[2].x == m0) & (row[2].y == m1);
  const bool t0 = h0 | e0, t1 = h1 | e1;
  const bool s1 = !t0 & h1, s2 = !t0 & !t1 & h2;
  // (masks, not a select: a select of row[e].z became a load through a
  // selected address, with the row in scratch memory again)
  const uint32_t z = (row[0].z & (0u - (uint32_t)h0)) | (row[1].z & (0u - (uint32_t)s1)) |
                     (row[2].z & (0u - (uint32_t)s2));
  if (h0 | s1 | s2) *port = z;
  *done = t0 | t1 | h2 | e2;
  return h0 ? ix.x : e0 ? kNone : h1 ? ix.y : e1 ? kNone : h2 ? ix.z : kNone;
}

// Phase A. Blocks own contiguous ranges of 64-packet tiles, their four waves
// interleaved (the frames64_tiles layout, so the launch can bin its touches:
// tbl_bins_plan); a lane takes one packet of its wave's tile. The src and
// dst home buckets are fetched together, four lanes per 64-byte row
// (wave-cooperative, one request per row), then handed to their lanes
// through LDS; a probe that continues past its home bucket walks on alone.
// W: waves per block (4; 16, one 1024-thread block per CU sharing one copy
// of the tables, bridge_classify_w: VIGPATH_BRIDGE_WAVES=16).
template <uint32_t W>
__device__ __forceinline__ void bridge_tiles(BridgeArgs a, TouchBins bins) {
  __shared__ uint32_t T[kBridgeTabs * 256 + 1024];  // + the layout's tables
  __shared__ uint4 stage[W][256];
  __shared__ uint32_t cur[kCurs];
  for (uint32_t i = threadIdx.x; i < kCurs; i += blockDim.x) cur[i] = 0;
  for (uint32_t i = threadIdx.x; i < kBridgeTabs * 256; i += blockDim.x)
    T[i] = a.crc_tab[i];
  const uint32_t *lin = T + kBridgeTabs * 256;
  if (a.t.mix == kMixLin)
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) T[kBridgeTabs * 256 + i] = a.t.lin[i];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint4 *S = stage[wv];
  const uint32_t first = a.p0 & ~63u;
  const uint32_t tiles = (a.p1 - first + 63) / 64;
  const uint32_t rb = blockIdx.x;
  const uint32_t per_b = (tiles + gridDim.x - 1) / gridDim.x;
  const uint32_t tend = min(tiles, rb * per_b + per_b);
  const uint32_t range0 = first + rb * per_b * 64;
  const uint8_t *bk = reinterpret_cast<const uint8_t *>(a.t.bk);
  // the next tile's header chunk and port, requested behind this tile's rows
  // (prefetch: the header load's latency under this tile's work)
  uint4 hn = make_uint4(0, 0, 0, 0);
  uint32_t inn = 0;
  auto hfetch = [&](uint32_t tile) {
    const uint32_t p = first + tile * 64 + lane;
    if (p >= a.p0 && p < a.p1) {
      hn = eth_words(a, p);
      inn = a.in_dev[p];
    }
  };
  uint32_t tile = rb * per_b + wv;
  if (tile < tend) hfetch(tile);
  for (; tile < tend; tile += W) {  // wave-uniform
    const uint32_t p = first + tile * 64 + lane;
    const bool mine = p >= a.p0 && p < a.p1;
    const uint4 h = mine ? hn : make_uint4(0, 0, 0, 0);
    const uint32_t in = mine ? inn : 0u;
    const uint32_t d0 = h.x, d1 = h.y & 0xFFFF;
    const uint32_t s0 = (h.y >> 16) | (h.z << 16), s1 = h.z >> 16;
    uint32_t sh, dh;
    eth_hash2(T, s0, s1, d0, d1, &sh, &dh);
    // bridge_get_device: the static table first (bridge_main.c:38-61)
    int32_t st_fwd = 0;
    bool st_hit = false;
    if (a.n_static && mine) {
      const uint32_t key[4] = {d0, d1 | (in << 16), 0, 0};
      const uint32_t k = tbl_probe(a.st, static_hash(T, dh, in), key);
      if (k != kNone) {
        st_hit = true;
        st_fwd = a.st_val[k];
      }
    }
    // both home rows in flight at once: lane L fetches part L % 4 of the rows
    // of packet 16 j + L / 4, the row numbers by ds_bpermute issued together
    // and waited for once (as vignat's lean tile); kNone reads nothing
    const uint32_t sb = home_bucket(sh, a.t.bmask, a.t.mix, lin),
                   db = home_bucket(dh, a.t.bmask, a.t.mix, lin);
    const uint32_t vs = mine ? sb : kNone, vd = mine && !st_hit ? db : kNone;
    uint32_t r0, r1, r2, r3, r4, r5, r6, r7;
    const uint32_t src = lane & ~3u;  // byte address of lane L / 4
    asm volatile("ds_bpermute_b32 %0, %1, %2" : "=v"(r0) : "v"(src), "v"(vs));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:64" : "=v"(r1) : "v"(src), "v"(vs));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:128" : "=v"(r2) : "v"(src), "v"(vs));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:192" : "=v"(r3) : "v"(src), "v"(vs));
    asm volatile("ds_bpermute_b32 %0, %1, %2" : "=v"(r4) : "v"(src), "v"(vd));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:64" : "=v"(r5) : "v"(src), "v"(vd));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:128" : "=v"(r6) : "v"(src), "v"(vd));
    asm volatile("ds_bpermute_b32 %0, %1, %2 offset:192" : "=v"(r7) : "v"(src), "v"(vd));
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6),
                   "+v"(r7));
    const uint32_t part = lane & 3;
    auto rowq = [&](uint32_t r) {
      return r != kNone ? reinterpret_cast<const uint4 *>(bk + (size_t)r * 64)[part]
                        : make_uint4(0, 0, 0, 0);
    };
    uint4 q[8] = {rowq(r0), rowq(r1), rowq(r2), rowq(r3),
                  rowq(r4), rowq(r5), rowq(r6), rowq(r7)};
    if (tile + W < tend) hfetch(tile + W);
    uint4 srow[4], drow[4];
    wave_lds_sync();
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) S[chunk_swz(64 * j + lane)] = q[j];
    wave_lds_sync();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) srow[k] = S[chunk_swz(4 * lane + k)];
    wave_lds_sync();
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) S[chunk_swz(64 * j + lane)] = q[4 + j];
    wave_lds_sync();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) drow[k] = S[chunk_swz(4 * lane + k)];
    uint32_t touch = kNone;
    if (mine) {
      // bridge_put_update_entry: a known src is rejuvenated, an unknown one
      // queued for phase B
      uint32_t unused = 0;
      bool done;
      uint32_t si = mac_match(srow, s0, s1, &unused, &done);
      if (!done) {
        TableDev t = a.t;
        si = mac_probe_from(t, (sb + 1) & t.bmask, s0, s1, &unused);
      }
      touch = si;
      log_put(a.log, p, si);  // kNone: phase B writes the real entry
      if (si == kNone) a.miss[wave_append(&a.t.ctl->miss_count, true)] = p;
      if (st_hit) {
        a.out[p] = resolve(st_fwd, in);
      } else {
        uint32_t port = 0;
        uint32_t di = mac_match(drow, d0, d1, &port, &done);
        if (!done) di = mac_probe_from(a.t, (db + 1) & a.t.bmask, d0, d1, &port);
        // unknown: flooded unless learned earlier in this segment (phase C
        // re-examines flooded frames only when phase B learned something)
        a.out[p] = di != kNone ? (uint16_t)port : VP_FLOOD_FRAME;
      }
    }
    bins_put(bins, cur, rb, per_b * 64, range0, p, touch);
  }
  __syncthreads();
  bins_publish(bins, cur, rb);
}

__global__ __launch_bounds__(256) void bridge_classify(BridgeArgs a, TouchBins bins) {
  bridge_tiles<4>(a, bins);
}
__global__ __launch_bounds__(1024, 1) void bridge_classify_w(BridgeArgs a, TouchBins bins) {
  bridge_tiles<16>(a, bins);
}

// Keys + hashes of the queued src MACs (packet order).
__global__ void bridge_miss_keys(BridgeArgs a, const uint32_t *list, uint32_t n,
                                 uint32_t *mkey, uint32_t *mhash) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint4 h = eth_words(a, list[j]);
    const uint32_t s0 = (h.y >> 16) | (h.z << 16), s1 = h.z >> 16;
    uint32_t *k = mkey + 4 * (size_t)j;
    k[0] = s0;
    k[1] = s1;
    k[2] = 0;
    k[3] = 0;
    mhash[j] = eth_hash(a.crc_tab, s0, s1);
  }
}

// Touch log for every queued src; the first sighting stores its in port as
// the entry's DynamicValue (bridge_main.c:80-84).
__global__ void bridge_learn_finish(BridgeArgs a, const uint32_t *list,
                                    uint32_t n, const uint32_t *scratch,
                                    const uint32_t *rep, const uint32_t *assign) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const uint32_t j0 = scratch[rep[j]];
    const uint32_t idx = assign[j0];
    a.log[p] = idx;  // kNone: table full, nothing learned (bridge_main.c:73-76)
    if (j0 == j && idx != kNone) {
      const uint32_t e = a.t.slot_of[idx];
      a.t.bk[e >> 2].k[e & 3][2] = a.in_dev[p];
    }
  }
}

// Phase C over the segment's flooded frames: a static rule (e.g. one that
// floods explicitly) still wins; otherwise a MAC learned by a packet q' <= p
// (the packet's own src is learned before its dst is looked up) forwards.
__global__ void bridge_defer_finish(BridgeArgs a) {
  for (uint32_t p = a.p0 + blockIdx.x * blockDim.x + threadIdx.x; p < a.p1;
       p += gridDim.x * blockDim.x) {
    if (a.out[p] != VP_FLOOD_FRAME) continue;
    const uint4 h = eth_words(a, p);
    const uint32_t d0 = h.x, d1 = h.y & 0xFFFF;
    const uint32_t dh = eth_hash(a.crc_tab, d0, d1);
    if (a.n_static) {
      const uint32_t in = a.in_dev[p];
      const uint32_t key[4] = {d0, d1 | (in << 16), 0, 0};
      if (tbl_probe(a.st, static_hash(a.crc_tab, dh, in), key) != kNone) continue;
    }
    uint32_t port = 0;
    const uint32_t di = mac_probe(a.t, dh, d0, d1, &port);
    if (di != kNone && tbl_allocated_before(a.t, di, a.seq_base + p + 1))
      a.out[p] = (uint16_t)port;
  }
}

// ========================================================= one packet ==
// nf.c calls nf_process once per packet (nf.c:150-176) or once per small
// burst (its VIGOR_BATCH_SIZE loop, nf.c:178-215). vp_process_one and small
// vp_process_mbufs calls go to bridge_serve, one wave that stays resident and
// polls the host-coherent mailbox (ServeBox, vp_internal.h), as nat_serve and
// fw_serve do for vignat and vigfw: no launch and no copy call per packet.
// Until the context meets a due expiry the host sends requests only while
// none is due (serve_process_one / serve_process_burst) and the kernel
// restates bridge_main.c:311-329 without the expiry step; from then on it runs
// that step too, from the touch journal (serve_expire, vp_serve_dev.h). The
// bridge never rewrites a frame and reads only its 12 MAC bytes.

// T holds the CRC tables, then the layout's byte tables (kMixLin).
constexpr uint32_t kBridgeTabWords = kBridgeTabs * 256 + 1024;

// A frame's MACs from its first three words (eth_words' layout).
struct Macs {
  uint32_t d0, d1, s0, s1;
};
__device__ __forceinline__ Macs macs_of(uint32_t w0, uint32_t w1, uint32_t w2) {
  return Macs{w0, w1 & 0xFFFF, (w1 >> 16) | (w2 << 16), w2 >> 16};
}

// The static table's part of bridge_get_device (bridge_main.c:38-47): the
// rule keyed {dst, in}, dh = eth_hash(dst); *fwd = its device_to.
__device__ __forceinline__ bool bridge_static(const BridgeArgs &a, const uint32_t *T, uint32_t dh,
                                              uint32_t d0, uint32_t d1, uint32_t in,
                                              int32_t *fwd) {
  if (!a.n_static) return false;
  const uint32_t key[4] = {d0, d1 | (in << 16), 0, 0};
  const uint32_t k = tbl_probe(a.st, static_hash(T, dh, in), key);
  if (k == kNone) return false;
  *fwd = a.st_val[k];
  return true;
}

// bridge_put_update_entry (bridge_main.c:63-89) for src {s0, s1} (hash sh)
// from port `in` at global sequence seq, without the stamp: the MAC's index
// -- a known MAC keeps its port; an unknown one takes an index (serve_lan_by)
// and stores {s0, s1, in, 0} --, or kNone with nothing written when no index
// is free (bridge_main.c:73-76).
__device__ __forceinline__ uint32_t bridge_learn(const TableDev &t, uint32_t sh, uint32_t s0,
                                                 uint32_t s1, uint32_t in, uint64_t seq,
                                                 uint32_t *fresh) {
  const uint32_t key[4] = {s0, s1, in, 0};
  return serve_lan_by(t, sh, key, 0u, seq, fresh, [&] {
    uint32_t unused = 0;
    return mac_probe(t, sh, s0, s1, &unused);
  });
}

// A burst request (vp_serve_dev.h) for vigbridge. Every packet both learns
// its src and looks its dst up, so a lane may be pending on both: lpend = its
// src is unknown, wpend = its dst is unknown and no static rule decides. In
// burst_settle the lane learns in its own round (lane == m) and looks its dst
// up in a later one (lane < the next m, or behind the loop), so its lookup
// sees the learns of the lanes up to and including itself and of no later
// lane: a frame addressed to its own new src forwards, as learn precedes
// lookup in bridge_main.c:316-320. A hit of round 0 is final: nothing expires
// inside a burst and a known MAC's port never changes. Only the learn stamps
// (bridge_main.c:66-69, 86), so burst_last runs over the src index. Nothing
// of a frame comes back and no burst is declined. With the journal on (J) the
// expiries due at the first packet run first (bridge_main.c:311-315: before
// the learn, so a dst that has just expired is unknown and a src that has is
// learnt again, from the port it now comes from) and *k <= n packets are
// served (burst_split); the walk precedes round 0, whose hits stay final.
template <bool J>
__device__ __forceinline__ uint32_t bridge_burst(const BridgeArgs &a, const uint32_t *T,
                                                 ServeBox *box, uint32_t n, uint64_t seq0,
                                                 uint32_t lane, const JournalDev &j,
                                                 JournalSt &js, uint32_t *k) {
  const TableDev &t = a.t;
  const BurstIn b = burst_load(box, n, lane);
  bool act = b.act;
  int64_t now0 = 0;
  if (J) {
    n = burst_split(t, j, js, b, n, lane, &now0);
    if (!n) return kBurstFull;
    act = act && lane < n;
  }
  *k = n;
  const uint32_t in = b.in;
  const Macs m = macs_of(b.f.w[0], b.f.w[1], b.f.w[2]);
  uint32_t sh, dh;
  eth_hash2(T, m.s0, m.s1, m.d0, m.d1, &sh, &dh);
  // round 0, then the misses in packet order
  int32_t st_fwd = 0;
  const bool st_hit = act && bridge_static(a, T, dh, m.d0, m.d1, in, &st_fwd);
  uint32_t si = kNone, di = kNone, port = 0, fresh = 0;
  if (act) {
    uint32_t unused = 0;
    si = mac_probe(t, sh, m.s0, m.s1, &unused);
    if (!st_hit) di = mac_probe(t, dh, m.d0, m.d1, &port);
  }
  burst_settle(
      lane, act && si == kNone, act && !st_hit && di == kNone,
      [&] { di = mac_probe(t, dh, m.d0, m.d1, &port); },
      [&] { si = bridge_learn(t, sh, m.s0, m.s1, in, seq0 + lane, &fresh); });
  const bool won = burst_last(si, n, lane);
  if (won) serve_stamp(t, si, b.now, seq0 + lane);
  if (J) journal_touch_burst(j, js, won, si, seq0 + lane, now0, lane);
  const uint32_t out = st_hit ? resolve(st_fwd, in)
                       : di != kNone ? (port & 0xFFFFu)
                                     : (uint32_t)VP_FLOOD_FRAME;
  burst_out(b, (out & 0xFFFFu) | (fresh << 16), n, lane);
  return kBurstServed;
}

// The server: one wave (<<<1, 64>>>). Every poll reads the request chunks
// whole; a one-packet request is chunk 0 and, for a frame of at least one
// byte, chunk 1 with frame bytes 0-11 (bytes past len read as 0, the runt
// convention of DESIGN.md 7), which lane 0 takes from lane 1's registers: no
// LDS copy of the frame. Lane 0 runs the packet: learn the src, then look the
// dst up (static rules first; the lookup does not stamp). The answer is chunk
// 0 alone (out | fresh << 16). Packets take global sequence numbers seq0,
// seq0 + 1, ...; a burst request (bridge_burst) takes as many as it has
// frames. The kernel leaves on the leave request or after `idle` wall-clock
// ticks without a request; the host launches it again (serve_wait). flags:
// serve_poll's. J: the kernel expires from the touch journal j
// (vp_serve_dev.h), the whole wave's walk before lane 0's learn, and the answer
// chunk carries the walk's count; a context whose journal is off runs the
// instance without any of it.
template <bool J>
__global__ __launch_bounds__(64) void bridge_serve(BridgeArgs a, ServeBox *box, uint64_t seq0,
                                                   uint64_t idle, uint32_t flags, JournalDev j) {
  __shared__ uint32_t T[kBridgeTabWords];
  const uint32_t lane = threadIdx.x;
  for (uint32_t i = lane; i < kBridgeTabs * 256; i += 64) T[i] = a.crc_tab[i];
  if (a.t.mix == kMixLin) {  // (the layout's byte tables: their LDS copy)
    for (uint32_t i = lane; i < 1024; i += 64) T[kBridgeTabs * 256 + i] = a.t.lin[i];
    a.t.lin = T + kBridgeTabs * 256;
  }
  __syncthreads();
  const ServeIo io = serve_io(box, lane);
  // the last answered request (a relaunched server goes on from the answer
  // word), the next packet's sequence, the last answer's wall clock
  uint32_t done = __builtin_amdgcn_readfirstlane((uint32_t)__hip_atomic_load(
      &box->ans, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM));
  uint64_t seq = seq0;
  uint64_t t0 = wall_clock64();
  // the touch journal's control words
  JournalSt js = journal_load(J ? j : JournalDev{});
  auto serve = [&](const v4u &c) -> int {
    const uint32_t want = done + 1;
    if (__builtin_amdgcn_readfirstlane(c[3]) != want) return -1;
    const uint32_t hi = __builtin_amdgcn_readfirstlane(c[0]);
    if (hi == kServeLeave) return 1;
    const uint32_t in = hi >> 16;
    js.expired = 0, js.flags = 0;
    if ((hi & 0xFFFFu) == kServeBurstOp) {  // chunk 0 alone, the frames in the burst body
      uint32_t bn = min(max(in, 1u), kServeBurst);
      uint32_t st = bridge_burst<J>(a, T, box, bn, seq, lane, j, js, &bn);
      if (J && st == kBurstServed && js.flags) st |= kBurstTombs;
      if (J) journal_store(j, js, lane);
      if (lane == 0) burst_answer(io, box, st, bn, want, js.expired);
      if ((st & 0xFFu) == kBurstServed) seq += bn;
      t0 = wall_clock64();
      done = want;
      // (every lane's table writes before the next request reads them)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      return 0;
    }
    const uint32_t len = min(hi & 0xFFFFu, kServeFrame);
    const uint32_t got = min(len, 12u);          // frame bytes in chunk 1
    const uint32_t need = (12 + got + 11) / 12;  // chunks carrying the request
    if (__ballot(lane < need && c[3] != want)) return -1;  // not whole yet: poll again
    // (J: the cutoff compare needs the time exact -- both halves widened as
    // unsigned, as pol_serve reads it)
    const int64_t now =
        J ? (int64_t)((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(c[1]) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(c[2]) << 32))
          : serve_now(c);
    const uint4 h = chunk_keep(make_uint4((uint32_t)__builtin_amdgcn_readlane((int)c[0], 1),
                                          (uint32_t)__builtin_amdgcn_readlane((int)c[1], 1),
                                          (uint32_t)__builtin_amdgcn_readlane((int)c[2], 1), 0u),
                               0, (int)got);
    uint32_t res = 0, tix = kNone;
    const bool full = J && !journal_room(j, js, 1);  // (nothing is done: seeded again)
    // bridge_main.c:311-315: the expiry before the learn
    if (J && !full) serve_expire(a.t, j, js, journal_cutoff(j, now), lane);
    if (full) res = kOneFull;
    if (lane == 0 && !full) {
      const Macs m = macs_of(h.x, h.y, h.z);
      uint32_t sh, dh;
      eth_hash2(T, m.s0, m.s1, m.d0, m.d1, &sh, &dh);
      uint32_t fresh = 0;
      const uint32_t si = bridge_learn(a.t, sh, m.s0, m.s1, in, seq, &fresh);
      if (si != kNone) serve_stamp(a.t, si, now, seq);
      tix = si;  // (only the learn touches; the dst lookup does not stamp)
      int32_t fwd = 0;
      uint32_t out;
      if (bridge_static(a, T, dh, m.d0, m.d1, in, &fwd)) {
        out = resolve(fwd, in);
      } else {  // (after the learn: a frame to its own new src forwards)
        uint32_t port = 0;
        const uint32_t di = mac_probe(a.t, dh, m.d0, m.d1, &port);
        out = di != kNone ? (port & 0xFFFFu) : (uint32_t)VP_FLOOD_FRAME;
      }
      res = (out & 0xFFFFu) | (fresh << 16) | js.flags;
    }
    res = __builtin_amdgcn_readfirstlane(res);
    if (J) {
      journal_touch(j, js, __builtin_amdgcn_readfirstlane(tix), seq, now, lane);
      journal_store(j, js, lane);
    }
    if (lane == 0) {
      __builtin_amdgcn_raw_buffer_store_b128((v4u){res, js.expired, 0u, want}, io.as, 0, 0, kSys);
      // (the answer word: where a relaunched server starts counting; the host
      // reads the answer chunk. No release fence at system scope, which would
      // write back the whole L2)
      __hip_atomic_store(&box->ans, (uint64_t)want | ((uint64_t)res << 32), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (!full) seq += 1;
    t0 = wall_clock64();
    done = want;
    // (lane 0's table writes before the next request's lanes read them)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return 0;
  };
  serve_poll(io, flags, idle, serve, [&] { return t0; });
}

// =============================================================== host ==

// bridge_main.c:29-36: expiration_time * 1000 in 32 bits. The journal's E is
// 0 - bridge_cutoff(c, 0) (serve_expire_e): the wrapped product itself.
static inline int64_t bridge_cutoff(const vp_ctx *c, int64_t t) {
  const uint32_t e = c->brg.expiration_time * 1000u;  // u32, as vignat
  return (int64_t)((uint64_t)t - e);
}

// The tables every bridge kernel reads: the dynamic table as it is now, the
// static table and the CRC tables.
static void bridge_tables(vp_ctx *c, BridgeArgs *a) {
  a->t = tbl_dev(c->ft);
  a->st = TableDev{};
  a->st.bk = c->st_bk;
  a->st.bmask = c->st_bmask;
  a->st.mix = kMixMul;
  a->st_val = c->st_val;
  a->n_static = c->n_static;
  a->crc_tab = c->crc_tab;
}

static int bridge_segment(vp_ctx *c, const vp_dev_batch *b, const NowSpec &now,
                          uint32_t p0, uint32_t p1, float *ms, int *launches,
                          uint32_t *allocated) {
  FlowTable &t = c->ft;
  Workspace &w = c->ws;
  BridgeArgs a{};
  a.frames = b->frames;
  a.in_dev = b->in_dev;
  a.out = b->out_dev;
  a.log = w.log;
  a.seq_base = c->seq;
  a.slot = b->slot;
  a.p0 = p0;
  a.p1 = p1;
  bridge_tables(c, &a);
  a.miss = w.miss;
  a.defer = w.defer;

  // the classify launch bins its touches when it can (TouchBins; no touch
  // log then), else logs them and the log is folded
  BinsPlan bp{};
  static const uint32_t bw = [] {  // waves per block (VIGPATH_BRIDGE_WAVES: 4 or 16)
    const char *e = getenv("VIGPATH_BRIDGE_WAVES");
    return e && atoi(e) == 16 ? 16u : 4u;
  }();
  const void *bk = bw == 16 ? (const void *)bridge_classify_w : (const void *)bridge_classify;
  VP_TRY(tbl_bins_plan(c, t, bk, p0, p1, &bp, bw, 8));
  const uint32_t tiles = (p1 - (p0 & ~63u) + 63) / 64;
  const uint32_t grid = bp.on ? bp.grid : resident_grid(bk, (tiles + bw - 1) / bw, 64 * (int)bw);
  // (still zero after a segment that learned nothing: no reset launch)
  VP_TRY(seg_reset_counters(c, t));
  VP_HIP(ev_record(c->ktime, c->ev0, c->stream));
  BridgeArgs a1 = a;
  if (bp.on) a1.log = nullptr;
  c->last_kernel = bw == 16 ? "bridge_classify_w" : "bridge_classify";
  if (bw == 16)
    bridge_classify_w<<<grid, 1024, 0, c->stream>>>(a1, bp.bins);
  else
    bridge_classify<<<grid, 256, 0, c->stream>>>(a1, bp.bins);
  VP_HIP(hipGetLastError());
  VP_HIP(ev_record(c->ktime, c->ev1, c->stream));
  VP_TRY(tbl_fold_read_ctl(c, t, bp, w.log, p0, p1, now, c->seq));
  VP_TRY(seg_classify_ms(c, ms, launches));
  const bool ovf = bp.on && t.h_ctl.touch_ovf != 0;
  if (ovf)  // touches that found their bin slice full, logged alone
    VP_TRY(tbl_late_touches(c, t, bp.bins.oent, bp.bins.ocnt, 0, bp.range, bp.grid,
                            w.log, now, c->seq));
  const uint32_t nmiss = t.h_ctl.miss_count;
  // nothing learned: provisional floods stand; only the fold may still run
  // (not when it reads the caller's time array)
  c->fold_pending = !nmiss && !ovf && !b->now;
  t.ctl_clean = !nmiss && !ovf;
  if (!nmiss) return 0;

  VP_TRY(phase_b_round(c, t, nmiss, &a.t, [&] {
    bridge_miss_keys<<<grid_for(nmiss), 256, 0, c->stream>>>(a, w.miss_sorted, nmiss,
                                                             w.mkey, w.mhash);
  }, [&] {
    bridge_learn_finish<<<grid_for(nmiss), 256, 0, c->stream>>>(
        a, w.miss_sorted, nmiss, w.scratch, w.rep, w.assign);
  }));
  // (over the whole segment: the provisional floods addressed to a MAC learned here)
  bridge_defer_finish<<<grid_for(p1 - p0), 256, 0, c->stream>>>(a);
  VP_HIP(hipGetLastError());
  *allocated |= 1u;
  // the learning packets' touches on top of the fold (last toucher wins)
  VP_TRY(tbl_late_list(c, t, w.miss_sorted, nmiss, w.log, now, c->seq));
  VP_TRY(read_ctl(c, t));
  return 0;
}

static int bridge_process_device(vp_ctx *c, const vp_dev_batch *b) {
  ExpiringTable tabs[1] = {{&c->ft, bridge_cutoff}};
  return run_batch(c, b, tabs, 1, bridge_segment);
}

// ---------------------------------------------------- vp_process_one --
// vigbridge's launcher of the resident kernel (serve_launch, vp_serve.hip).
static int bridge_serve_launch(vp_ctx *c, ServeBox *dbox, uint32_t flags) {
  BridgeArgs a{};
  bridge_tables(c, &a);
  return serve_launch_one(c, bridge_serve<true>, bridge_serve<false>, a, dbox, flags,
                          serve_journal_dev(c, bridge_ops().serve));
}

// The largest host batch routed to the server as burst requests: the largest
// swept n at which the served path measured faster per packet than the batch
// pipeline on the MI355X (profiles/r10_bridge_serve.txt: 0.14 against 0.24 us
// at 256, 0.14 against 0.18 at 384, 0.139 against 0.137 at 512); larger calls
// take the pipeline. Above vignat's and vigfw's 256: a served vigbridge burst
// copies 16 bytes a frame in and none back. VIGPATH_SERVE_BURST overrides it;
// 0 routes nothing.
constexpr uint32_t kBridgeBurstRoute = 384;

// vigbridge through the mailbox (serve_process_one / serve_process_burst,
// vp_serve.hip): bridge_serve reads a frame's 12 MAC bytes and changes none,
// so one packet sends 12 bytes and takes none back; a burst copies a frame's
// first 16 bytes in and nothing back. No stage clock. The kernel expires from
// the touch journal.
const NfOps &bridge_ops() {
  static const NfOps ops = [] {
    NfOps o{};
    o.process_device = bridge_process_device;  o.serve_launch = bridge_serve_launch;
    o.n_devices = [](const vp_ctx *c) -> uint32_t { return c->brg.n_devices; };
    o.reads_in_port = false;
    ServeNf &s = o.serve;
    s.cutoff = bridge_cutoff;  s.table = &vp_ctx::ft;
    s.one_whole = false;  s.one_in = 12;  s.one_back = 0;
    s.burst_in = 16;  s.burst_back = 0;  s.burst_route = kBridgeBurstRoute;
    s.prof = false;  s.journal = true;
    s.cutoff2 = nullptr;  s.table2 = nullptr;
    return o;
  }();
  return ops;
}

void build_bridge_tables(std::vector<uint32_t> &tab) {
  tab.assign(kBridgeTabs * 256, 0);
  for (int j = 0; j < kEthTabs; j++)
    build_position_table(&tab[j * 256], 4 * j, 24);
  for (int j = 0; j < kStatTabs; j++)
    build_position_table(&tab[(kEthTabs + j) * 256], j, 8);
}

// Static table (read_static_ft_from_file): rule k keyed {mac, (u16)from},
// value `to`. Built on the host into the device bucket layout. A repeated key
// keeps the first rule: the reference's map_put appends the duplicate
// further along the same probe path, so map_get finds the first.
int bridge_static_build(const vp_bridge_config *cfg, std::vector<Bucket> &bk,
                        uint32_t *bmask) {
  uint32_t nb = 64;
  while ((uint64_t)nb * kBucketEntries < 2ull * cfg->n_static) nb <<= 1;
  bk.assign(nb, Bucket{});
  for (auto &x : bk)
    for (uint32_t e = 0; e < kBucketEntries; e++) x.idx[e] = kEmpty;
  *bmask = nb - 1;
  std::vector<uint32_t> tab;
  build_bridge_tables(tab);
  const uint32_t *E = tab.data(), *S = tab.data() + kEthTabs * 256;
  for (uint32_t r = 0; r < cfg->n_static; r++) {
    const vp_bridge_rule &R = cfg->static_rules[r];
    const uint32_t m0 = R.mac[0] | (R.mac[1] << 8) | (R.mac[2] << 16) |
                        ((uint32_t)R.mac[3] << 24);
    const uint32_t m1 = R.mac[4] | (R.mac[5] << 8);
    const uint32_t dev = (uint16_t)R.device_from;
    const uint32_t key[4] = {m0, m1 | (dev << 16), 0, 0};
    uint32_t eh = 0;
    for (int j = 0; j < 6; j++) eh ^= E[j * 256 + R.mac[j]];
    const uint32_t h = S[0 * 256 + (eh & 0xFF)] ^ S[1 * 256 + ((eh >> 8) & 0xFF)] ^
                       S[2 * 256 + ((eh >> 16) & 0xFF)] ^ S[3 * 256 + (eh >> 24)] ^
                       S[4 * 256 + (dev & 0xFF)] ^ S[5 * 256 + (dev >> 8)];
    uint32_t b = home_bucket(h, *bmask, kMixMul);
    bool placed = false;
    while (!placed) {
      for (uint32_t e = 0; e < kBucketEntries && !placed; e++) {
        Bucket &x = bk[b];
        if (x.idx[e] == kEmpty) {
          memcpy(x.k[e], key, 16);
          x.idx[e] = r;
          placed = true;
        } else if (!memcmp(x.k[e], key, 16)) {
          placed = true;  // duplicate: the first rule stays visible
        }
      }
      b = (b + 1) & *bmask;
    }
  }
  return 0;
}

}  // namespace vp
