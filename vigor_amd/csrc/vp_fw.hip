// vigfw on MI355X: batch classification + flow-state update + MAC rewrite.
//
// Reference behaviour (paths relative to the reference repository):
//   nf_process            vigfw/fw_main.c:21-80
//   flow manager          vigfw/fw_flowmanager.c:20-86
//   state                 vigfw/dataspec.ml:5-11 (fm, fv, int_devices, heap)
// Same segment / phase structure as vignat (vp_nat.hip header):
//   phase A  parse + hash; LAN packets whose FlowId exists at segment start
//            and WAN packets whose reversed FlowId exists are forwarded and
//            touch their flow; LAN misses and WAN misses are queued;
//   phase B  LAN misses: de-duplicated, ranked, given dchain indices in packet
//            order; the first sighting's input device is the flow's
//            int_devices entry; every LAN packet goes out on the WAN device,
//            table full or not (fw_flowmanager.c:49-53);
//   phase C  WAN misses look the reversed key up again: a flow allocated
//            earlier in packet order is a hit, anything else is dropped.
// The frame rewrite is the two MAC addresses only (fw_main.c:76-77).
//
// Table entry: key words {src_port | dst_port << 16, src_ip, dst_ip,
// protocol | int_device << 8}; the key is FlowId (vigfw/flow.h:3-9, 13 bytes
// + padding), the int_devices vector lives in the padding byte positions,
// and probes compare the protocol byte only (bucket_match<0xFF>).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "vp_serve_dev.h"
#include "vp_table.h"

namespace vp {

VP_PRELOAD_UNIT(fw)


// FlowId_hash for vigfw's FlowId (generated, codegen/main.ml:328-401): five
// CRC steps src_port, dst_port, src_ip, dst_ip, protocol; non-zero byte
// positions of the 20-byte CRC message.
static const int kFwPos[13] = {0, 1, 4, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16};
constexpr int kFwMsg = 20;
constexpr uint32_t kFwTabs = 13;

__device__ __forceinline__ uint32_t fw_hash(const uint32_t *T, uint32_t sp,
                                            uint32_t dp, uint32_t sip,
                                            uint32_t dip, uint32_t proto) {
  return T[0 * 256 + (sp & 0xFF)] ^ T[1 * 256 + ((sp >> 8) & 0xFF)] ^
         T[2 * 256 + (dp & 0xFF)] ^ T[3 * 256 + ((dp >> 8) & 0xFF)] ^
         T[4 * 256 + (sip & 0xFF)] ^ T[5 * 256 + ((sip >> 8) & 0xFF)] ^
         T[6 * 256 + ((sip >> 16) & 0xFF)] ^ T[7 * 256 + (sip >> 24)] ^
         T[8 * 256 + (dip & 0xFF)] ^ T[9 * 256 + ((dip >> 8) & 0xFF)] ^
         T[10 * 256 + ((dip >> 16) & 0xFF)] ^ T[11 * 256 + (dip >> 24)] ^
         T[12 * 256 + (proto & 0xFF)];
}

struct FwArgs {
  uint8_t *frames;
  const uint16_t *len;
  const uint16_t *in_dev;
  uint16_t *out;
  uint32_t *log;
  uint64_t seq_base;
  uint32_t slot, p0, p1;
  TableDev t;
  const uint32_t *crc_tab;
  const uint32_t *macw;  // per device: d_addr|s_addr header words
  uint32_t *miss;
  uint32_t *defer;
  uint32_t *reprobe;
  uint32_t tileq;  // 64-byte tiles: reprobes go to the block's TileQueue slice
  uint16_t wan, n_dev;
};

__device__ __forceinline__ void fw_macs(const FwArgs &a, uint32_t dst,
                                        uint32_t mw[3]) {
  if (dst < a.n_dev) {
    mw[0] = a.macw[3 * dst];
    mw[1] = a.macw[3 * dst + 1];
    mw[2] = a.macw[3 * dst + 2];
  } else {  // outside the configured devices (reference: out-of-range read)
    mw[0] = mw[1] = mw[2] = 0;
  }
}

// The FlowId a packet looks up: its own 5-tuple on a LAN device, the
// reversed one on the WAN device (fw_main.c:46-53 / 62-68).
__device__ __forceinline__ void fw_key(bool wan, uint32_t sp, uint32_t dp,
                                       uint32_t sip, uint32_t dip, uint32_t proto,
                                       uint32_t key[4]) {
  if (wan) {
    key[0] = dp | (sp << 16);
    key[1] = dip;
    key[2] = sip;
  } else {
    key[0] = sp | (dp << 16);
    key[1] = sip;
    key[2] = dip;
  }
  key[3] = proto;
}

// Generic (byte-addressed) phase A: IP options, any slot size.
__device__ uint32_t fw_generic_a(const FwArgs &a, const uint32_t *T, uint32_t p,
                                 uint32_t in, uint32_t len) {
  GFrame f{a.frames + (size_t)p * a.slot, a.slot};
  const L34 h = parse_l34(f, len);
  if (!h.ok) {  // not IPv4 / not TCP-UDP: drop (fw_main.c:29-40)
    a.out[p] = (uint16_t)in;
    log_put(a.log, p, kNone);
    return kNone;
  }
  const uint32_t proto = f.r8(h.ip + 9);
  const uint32_t sp = f.r16(h.l4), dp = f.r16(h.l4 + 2);
  const uint32_t sip = f.r32(h.ip + 12), dip = f.r32(h.ip + 16);
  const bool wan = in == a.wan;
  uint32_t key[4];
  fw_key(wan, sp, dp, sip, dip, proto, key);
  const uint32_t hh = wan ? fw_hash(T, dp, sp, dip, sip, proto)
                          : fw_hash(T, sp, dp, sip, dip, proto);
  uint32_t w3 = 0;
  const uint32_t idx = tbl_probe<0xFFu>(a.t, hh, key, &w3);
  if (idx == kNone) {
    if (wan)
      a.defer[wave_append(&a.t.ctl->defer_count, true)] = p;
    else
      a.miss[wave_append(&a.t.ctl->miss_count, true)] = p;
    log_put(a.log, p, kNone);  // phase B / C write the real entry
    return kNone;
  }
  log_put(a.log, p, idx);
  const uint32_t dst = wan ? (w3 >> 8) : a.wan;
  uint32_t mw[3];
  fw_macs(a, dst, mw);
  set_macs(f, mw);
  a.out[p] = (uint16_t)dst;
  return idx;
}

// Phase A, 64-byte slots in registers (frames64_tiles): fw_issue parses and
// hashes, fw_finish consumes the gathered home bucket.
enum : uint32_t { kFwDone = 0, kFwGeneric = 1, kFwProbe = 2 };
struct FwPend {
  uint32_t kind;
  uint32_t row;  // home bucket (gathered by frames64_tiles) or kNone
};

// T holds the CRC tables, then the layout's byte tables (fw_load_tables).
constexpr uint32_t kFwTabWords = kFwTabs * 256 + 1024;
__device__ __forceinline__ const uint32_t *fw_lin(const uint32_t *T) {
  return T + kFwTabs * 256;
}

__device__ __forceinline__ FwPend fw_issue(const FwArgs &a, const uint32_t *T,
                                           uint32_t p, const RFrame &f,
                                           uint32_t in, uint32_t len, bool mine) {
  FwPend P{kFwDone, kNone};
  if (!mine) return P;
  const uint32_t et = f.w[3] & 0xFFFF;
  const uint32_t ihl = (f.w[3] >> 16) & 0x0F;
  if (!(et == 0x0008 && ihl == 5)) {
    P.kind = kFwGeneric;
    return P;
  }
  // nf_then_get_rte_ipv4_header / nf_then_get_tcpudp_header with IHL = 5
  const uint32_t tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
  const uint16_t unread = (uint16_t)(len - 14);
  const uint32_t proto = f.w[5] >> 24;
  const bool ok = (unread >= 20) & (unread >= tl) &
                  ((proto == 6) | (proto == 17)) & ((uint32_t)(len - 34) >= 4u);
  if (!ok) {
    a.out[p] = (uint16_t)in;
    log_put(a.log, p, kNone);
    return P;
  }
  const uint32_t sp = f.w[8] >> 16, dp = f.w[9] & 0xFFFF;
  const uint32_t sip = f.u32at2(26), dip = f.u32at2(30);
  // (WAN packets hash the reversed FlowId; the 13 reads batched, crc13_lds)
  const bool w = in == a.wan;
  const uint32_t s0 = w ? dp : sp, d0 = w ? sp : dp, si = w ? dip : sip, di = w ? sip : dip;
  const uint32_t hh = crc13_lds(T, s0 & 0xFF, (s0 >> 8) & 0xFF, d0 & 0xFF, (d0 >> 8) & 0xFF,
                                si & 0xFF, (si >> 8) & 0xFF, (si >> 16) & 0xFF, si >> 24,
                                di & 0xFF, (di >> 8) & 0xFF, (di >> 16) & 0xFF, di >> 24,
                                proto & 0xFF);
  P.kind = kFwProbe;
  P.row = home_bucket(hh, a.t.bmask, a.t.mix, fw_lin(T));
  return P;
}

__device__ __forceinline__ bool fw_finish(const FwArgs &a, const uint32_t *T,
                                          const FwPend &P, const uint4 *row,
                                          uint32_t p, RFrame &f, uint32_t in,
                                          uint32_t len, uint32_t &touch) {
  if (P.kind == kFwDone) return false;
  if (P.kind == kFwGeneric) {
    touch = fw_generic_a(a, T, p, in, len);  // writes global memory itself
    return false;
  }
  const uint32_t proto = f.w[5] >> 24;
  const uint32_t sp = f.w[8] >> 16, dp = f.w[9] & 0xFFFF;
  const uint32_t sip = f.u32at2(26), dip = f.u32at2(30);
  const bool wan = in == a.wan;
  uint32_t key[4];
  fw_key(wan, sp, dp, sip, dip, proto, key);
  bool done;
  uint32_t w3 = 0;
  const uint32_t idx =
      bucket_match<0xFFu>(row[0], row[1], row[2], row[3], key, &done, &w3);
  if (!done) {  // the bucket is full of other keys: fw_reprobe walks on,
    log_put(a.log, p, kNone);  // so this wave does not wait for a dependent read
    if (a.tileq)
      touch = kReprobe;
    else
      a.reprobe[wave_append(&a.t.ctl->reprobe_count, true)] = p;
    return false;
  }
  if (idx == kNone) {
    if (wan)
      a.defer[wave_append(&a.t.ctl->defer_count, true)] = p;
    else
      a.miss[wave_append(&a.t.ctl->miss_count, true)] = p;
    log_put(a.log, p, kNone);
    return false;
  }
  log_put(a.log, p, idx);
  touch = idx;
  const uint32_t dst = wan ? (w3 >> 8) : a.wan;
  uint32_t mw[3];
  fw_macs(a, dst, mw);
  f.w[0] = mw[0];
  f.w[1] = mw[1];
  f.w[2] = mw[2];
  a.out[p] = (uint16_t)dst;
  return true;
}

// The CRC tables, and behind them the allocation-order layout's byte tables
// when the table uses it (fw_lin(T), vp_table.h kMixLin).
__device__ __forceinline__ void fw_load_tables(uint32_t *T, const FwArgs &a) {
  for (uint32_t i = threadIdx.x; i < kFwTabs * 256; i += blockDim.x) T[i] = a.crc_tab[i];
  if (a.t.mix == kMixLin)
    for (uint32_t i = threadIdx.x; i < 1024; i += blockDim.x) T[kFwTabs * 256 + i] = a.t.lin[i];
  __syncthreads();
}

// Phase A, any slot size: one packet per lane (byte path; no checksum work).
__global__ __launch_bounds__(256) void fw_classify(FwArgs a) {
  __shared__ uint32_t T[kFwTabWords];
  fw_load_tables(T, a);
  for (uint32_t p = a.p0 + blockIdx.x * blockDim.x + threadIdx.x; p < a.p1;
       p += gridDim.x * blockDim.x)
    fw_generic_a(a, T, p, a.in_dev[p], a.len[p]);
}

// Phase A for 64-byte slots: LDS-staged coalesced frame I/O.
__global__ __launch_bounds__(256, 4) void fw_classify64(FwArgs a, uint32_t n_all,
                                                       TouchBins bins, TileQueue rq) {
  __shared__ uint32_t T[kFwTabWords];
  __shared__ uint4 stage[4][256];
  __shared__ uint32_t cur[kCurs];
  for (uint32_t i = threadIdx.x; i < kCurs; i += blockDim.x) cur[i] = 0;
  fw_load_tables(T, a);  // (its barrier also covers cur)
  frames64_tiles<kCurOverflow, true>(
      a.frames, a.len, a.in_dev, a.p0, a.p1, n_all, stage[threadIdx.x >> 6],
      reinterpret_cast<const uint4 *>(a.t.bk),
      [&](uint32_t p, const RFrame &f, uint32_t in, uint32_t len, bool mine) {
        return fw_issue(a, T, p, f, in, len, mine);
      },
      [&](const FwPend &P, const uint4 *row, uint32_t p, RFrame &f, uint32_t in,
          uint32_t len, uint32_t &touch) -> uint32_t {
        // the MACs change (bytes 0-11); the whole slot is stored back, a
        // whole-line write
        return fw_finish(a, T, P, row, p, f, in, len, touch) ? 0xFu : 0u;
      },
      bins, rq, cur);
}

// Packets whose home bucket held three other keys finish here, queued per
// classify block (TileQueue): phase A's register path with the probe walked
// on bucket by bucket (reprobe_wave); their touches join the block's bins.
__global__ __launch_bounds__(256) void fw_reprobe(FwArgs a, const uint32_t *list,
                                                  const uint32_t *cnt, uint32_t n,
                                                  uint32_t range, uint32_t nblk,
                                                  uint64_t seq_base) {
  __shared__ uint32_t T[kFwTabWords];
  __shared__ uint4 stage[4][256];
  fw_load_tables(T, a);
  a.tileq = 1;  // a full bucket answers kReprobe: reprobe_wave walks on
  uint4 *S = stage[threadIdx.x >> 6];
  reprobe_slices(list, cnt, n, range, nblk, a.t.tseq, seq_base, [&](uint32_t p, bool act) {
    return reprobe_wave(
        a.frames, a.slot, a.len, a.in_dev, reinterpret_cast<const uint8_t *>(a.t.bk),
        a.t.bmask, p, act, S,
        [&](uint32_t q, const RFrame &f, uint32_t in, uint32_t len, bool mine) {
          return fw_issue(a, T, q, f, in, len, mine);
        },
        [&](const FwPend &P, const uint4 *row, uint32_t q, RFrame &f, uint32_t in,
            uint32_t len, uint32_t &touch) {
          return fw_finish(a, T, P, row, q, f, in, len, touch);
        });
  });
}

// ------------------------------------------------------------- phase B --

// FlowId keys and hashes of the queued LAN misses.
__global__ void fw_miss_keys(FwArgs a, const uint32_t *list, uint32_t n,
                             uint32_t *mkey, uint32_t *mhash) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    GFrame f{a.frames + (size_t)p * a.slot, a.slot};
    const L34 h = parse_l34(f, a.len[p]);
    const uint32_t proto = f.r8(h.ip + 9);
    const uint32_t sp = f.r16(h.l4), dp = f.r16(h.l4 + 2);
    const uint32_t sip = f.r32(h.ip + 12), dip = f.r32(h.ip + 16);
    uint32_t *k = mkey + 4 * (size_t)j;
    fw_key(false, sp, dp, sip, dip, proto, k);
    mhash[j] = fw_hash(a.crc_tab, sp, dp, sip, dip, proto);
  }
}

// Every LAN miss: forwarded to the WAN device whether or not an index was
// free (fw_flowmanager.c:49-53); the first sighting of a key records its
// input device as the flow's int_devices entry (fw_flowmanager.c:61-64).
__global__ void fw_miss_finish(FwArgs a, const uint32_t *list, uint32_t n,
                               const uint32_t *mkey, const uint32_t *scratch,
                               const uint32_t *rep, const uint32_t *assign) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const uint32_t j0 = scratch[rep[j]];
    const uint32_t idx = assign[j0];
    a.log[p] = idx;
    if (idx != kNone && j0 == j) {
      const uint32_t e = a.t.slot_of[idx];
      a.t.bk[e >> 2].k[e & 3][3] = mkey[4 * (size_t)j + 3] | ((uint32_t)a.in_dev[p] << 8);
    }
    GFrame f{a.frames + (size_t)p * a.slot, a.slot};
    uint32_t mw[3];
    fw_macs(a, a.wan, mw);
    set_macs(f, mw);
    a.out[p] = a.wan;
  }
}

// ------------------------------------------------------------- phase C --
// WAN packets whose reversed FlowId was not in the table at segment start:
// a hit iff a LAN packet before this one (packet order) allocated it.
__global__ void fw_defer_finish(FwArgs a, const uint32_t *list, uint32_t n) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n;
       j += gridDim.x * blockDim.x) {
    const uint32_t p = list[j];
    const uint64_t q = a.seq_base + p;
    const uint32_t in = a.in_dev[p];
    GFrame f{a.frames + (size_t)p * a.slot, a.slot};
    const L34 h = parse_l34(f, a.len[p]);
    const uint32_t proto = f.r8(h.ip + 9);
    const uint32_t sp = f.r16(h.l4), dp = f.r16(h.l4 + 2);
    const uint32_t sip = f.r32(h.ip + 12), dip = f.r32(h.ip + 16);
    uint32_t key[4];
    fw_key(true, sp, dp, sip, dip, proto, key);
    uint32_t w3 = 0;
    const uint32_t idx =
        tbl_probe<0xFFu>(a.t, fw_hash(a.crc_tab, dp, sp, dip, sip, proto), key, &w3);
    if (idx == kNone || !tbl_allocated_before(a.t, idx, q)) {
      a.out[p] = (uint16_t)in;  // unknown external flow (fw_main.c:56-59)
      a.log[p] = kNone;
      continue;
    }
    a.log[p] = idx;
    const uint32_t dst = w3 >> 8;
    uint32_t mw[3];
    fw_macs(a, dst, mw);
    set_macs(f, mw);
    a.out[p] = (uint16_t)dst;
  }
}

// ========================================================= one packet ==
// nf.c calls nf_process once per packet (nf.c:150-176) or once per small
// burst (its VIGOR_BATCH_SIZE loop, nf.c:178-215). Through the batch path
// each call costs a launch sequence and a host round trip; vp_process_one and
// small vp_process_mbufs calls instead go to fw_serve, one wave that stays
// resident and polls the host-coherent mailbox (ServeBox, vp_internal.h), as
// nat_serve does for vignat: no launch and no copy call per packet. Until the
// context meets a due expiry the host sends requests only while none is due
// (serve_process_one / serve_process_burst) and the kernel restates
// fw_main.c:21-80 without the expiry step; from then on it runs that step
// too, from the touch journal (serve_expire, vp_serve_dev.h).

// The FlowId a packet looks up (fw_key) and its hash from the LDS tables.
__device__ __forceinline__ uint32_t fw_key_hash(const uint32_t *T, bool wan, uint32_t sp,
                                                uint32_t dp, uint32_t sip, uint32_t dip,
                                                uint32_t proto, uint32_t key[4]) {
  fw_key(wan, sp, dp, sip, dip, proto, key);
  const uint32_t s0 = key[0] & 0xFFFF, d0 = key[0] >> 16, si = key[1], di = key[2];
  return crc13_lds(T, s0 & 0xFF, (s0 >> 8) & 0xFF, d0 & 0xFF, (d0 >> 8) & 0xFF, si & 0xFF,
                   (si >> 8) & 0xFF, (si >> 16) & 0xFF, si >> 24, di & 0xFF, (di >> 8) & 0xFF,
                   (di >> 16) & 0xFF, di >> 24, proto & 0xFF);
}

// flow_manager_allocate_or_refresh_flow (fw_flowmanager.c:38-62) for one LAN
// FlowId from device `in` at global sequence seq: the flow's index, allocated
// when new (serve_lan; int_devices in the key's padding bytes, as
// fw_miss_finish stores it), or kNone when no index is free
// (fw_flowmanager.c:47-51).
__device__ __forceinline__ uint32_t fw_one_lan(const TableDev &t, uint32_t hh,
                                               const uint32_t key[4], uint32_t in, uint64_t seq,
                                               uint32_t *fresh) {
  return serve_lan<0xFFu>(t, hh, key, key[3] | (in << 8), seq, fresh);
}

// fw_main.c:44-72 for one TCP/UDP packet: the device it goes out on, or kNone
// for a WAN packet of no known flow (a drop). A LAN packet goes out on the
// WAN device whether or not its flow found an index.
__device__ __forceinline__ uint32_t fw_one_flow(const FwArgs &a, const uint32_t *T, uint32_t in,
                                                uint32_t sp, uint32_t dp, uint32_t sip,
                                                uint32_t dip, uint32_t proto, int64_t now,
                                                uint64_t seq, uint32_t *fresh, uint32_t *tix) {
  const bool wan = in == a.wan;
  uint32_t key[4];
  const uint32_t hh = fw_key_hash(T, wan, sp, dp, sip, dip, proto, key);
  uint32_t idx, dst = a.wan;
  if (wan) {
    uint32_t w3 = 0;
    idx = tbl_probe<0xFFu>(a.t, hh, key, &w3);
    if (idx == kNone) return kNone;
    dst = w3 >> 8;
  } else {
    idx = fw_one_lan(a.t, hh, key, in, seq, fresh);
  }
  if (idx != kNone) serve_stamp(a.t, idx, now, seq);
  *tix = idx;  // (the index the packet touched, for the journal)
  return dst;
}

// A burst request (vp_serve_dev.h) for vigfw: a WAN lane that looks again
// probes the table. Only the first 64 bytes of a frame are read and only its
// first 16 can change. With the journal on (J) the expiries due at the first
// packet run first and *k <= n packets are served (burst_split).
template <bool J>
__device__ __forceinline__ uint32_t fw_burst(const FwArgs &a, const uint32_t *T, ServeBox *box,
                                             uint32_t n, uint64_t seq0, uint32_t lane,
                                             const JournalDev &j, JournalSt &js, uint32_t *k) {
  const TableDev &t = a.t;
  const BurstIn b = burst_load(box, n, lane);
  BurstHdr h = burst_hdr(b);  // fw_issue's tests (fw_main.c:26-40)
  if (h.decline) return kBurstDeclined;
  int64_t now0 = 0;
  if (J) {
    n = burst_split(t, j, js, b, n, lane, &now0);
    if (!n) return kBurstFull;
    h.go = h.go && lane < n;
  }
  *k = n;
  const uint32_t in = b.in;
  const bool wan = in == a.wan;
  const bool lanp = h.go && !wan, wanp = h.go && wan;
  uint32_t key[4];
  const uint32_t hh = fw_key_hash(T, wan, h.sp, h.dp, h.sip, h.dip, h.proto, key);
  // round 0, then the misses in packet order
  uint32_t idx = kNone, fresh = 0, w3 = 0;
  if (h.go) idx = tbl_probe<0xFFu>(t, hh, key, &w3);
  burst_settle(
      lane, lanp && idx == kNone, wanp && idx == kNone,
      [&] { idx = tbl_probe<0xFFu>(t, hh, key, &w3); },
      [&] { idx = fw_one_lan(t, hh, key, in, seq0 + lane, &fresh); });
  const bool won = burst_last(idx, n, lane);
  if (won) serve_stamp(t, idx, b.now, seq0 + lane);
  if (J) journal_touch_burst(j, js, won, idx, seq0 + lane, now0, lane);
  // the rewrite: a LAN packet goes out on the WAN device with or without a
  // flow (fw_flowmanager.c:49-53), a WAN packet to its flow's internal device
  uint32_t out = in, rew = 0;
  if (lanp || (wanp && idx != kNone)) {
    out = lanp ? (uint32_t)a.wan : (w3 >> 8);
    uint32_t mw[3];
    fw_macs(a, out, mw);
    // back: the frame's first 16 bytes (the MACs are bytes 0-11)
    __builtin_amdgcn_raw_buffer_store_b128((v4u){mw[0], mw[1], mw[2], b.f.w[3]}, b.fs,
                                           (int)b.slot0, 0, kSys);
    rew = 1;
  }
  burst_out(b, (out & 0xFFFFu) | (fresh << 16) | (rew << 17), n, lane);
  return kBurstServed;
}

// The server: one wave (<<<1, 64>>>). Every poll reads the request chunks
// whole (ServeBox: one PCIe read brings the doorbell, the time and the frame's
// first kServeInline bytes -- vigfw reads nothing past byte 14 + 60 + 4 = 78,
// so `frame` is never used). Lane 0 runs the packet: a frame with a 20-byte
// IPv4 header in registers (fw_issue's tests), any other byte-addressed over
// its LDS copy (parse_l34, as fw_generic_a). Only the MACs can change, so the
// answer is chunk 0 (out | fresh << 16) and chunk 1 (frame bytes 0-11) in one
// store instruction. Packets take global sequence numbers seq0, seq0 + 1, ...;
// a burst request (fw_burst) takes as many as it has frames. The kernel
// leaves on the leave request or after `idle` wall-clock ticks without a
// request; the host launches it again (serve_wait). flags: serve_poll's.
// J: the kernel expires from the touch journal j (vp_serve_dev.h); a context
// whose journal is off runs the instance without any of it.
template <bool J>
__global__ __launch_bounds__(64) void fw_serve(FwArgs a, ServeBox *box, uint64_t seq0,
                                               uint64_t idle, uint32_t flags, JournalDev j) {
  __shared__ uint32_t T[kFwTabWords];
  __shared__ uint4 fr[(kServeInline + 15) / 16];
  const uint32_t lane = threadIdx.x;
  fw_load_tables(T, a);
  if (a.t.mix == kMixLin) a.t.lin = fw_lin(T);  // (the layout's byte tables: their LDS copy)
  const ServeIo io = serve_io(box, lane);
  uint32_t *fword = reinterpret_cast<uint32_t *>(fr);
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
      uint32_t st = fw_burst<J>(a, T, box, bn, seq, lane, j, js, &bn);
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
    const uint32_t got = min(len, kServeInline);    // frame bytes in the chunks
    const uint32_t need = (12 + got + 11) / 12;      // chunks carrying the request
    if (__ballot(lane < need && c[3] != want)) return -1;  // not whole yet: poll again
    const int64_t now = serve_now(c);
    serve_chunks_in(fword, c, lane, need);
    wave_lds_sync();
    uint32_t res = 0, m0 = 0, m1 = 0, m2 = 0, tix = kNone;
    const bool full = J && !journal_room(j, js, 1);  // (nothing is done: seeded again)
    if (J && !full) serve_expire(a.t, j, js, journal_cutoff(j, now), lane);
    if (full) res = kOneFull;
    if (lane == 0 && !full) {
      const RFrame f = serve_rframe([&](int j) { return fr[j]; }, len);
      const uint32_t et = f.w[3] & 0xFFFF, ihl = (f.w[3] >> 16) & 0x0F;
      uint32_t sp = 0, dp = 0, sip = 0, dip = 0, proto = 0;
      bool ok;
      if (et == 0x0008 && ihl == 5) {
        // nf_then_get_rte_ipv4_header / nf_then_get_tcpudp_header with IHL = 5
        const uint32_t tl = bswap16((uint16_t)(f.w[4] & 0xFFFF));
        const uint16_t unread = (uint16_t)(len - 14);
        proto = f.w[5] >> 24;
        ok = (unread >= 20) & (unread >= tl) & ((proto == 6) | (proto == 17)) &
             ((uint32_t)(len - 34) >= 4u);
        sp = f.w[8] >> 16, dp = f.w[9] & 0xFFFF;
        sip = f.u32at2(26), dip = f.u32at2(30);
      } else {  // byte-addressed over the LDS copy (bytes past it read as 0)
        const GFrame g{reinterpret_cast<uint8_t *>(fr), got};
        const L34 h = parse_l34(g, len);
        ok = h.ok;
        if (ok) {
          proto = g.r8(h.ip + 9);
          sp = g.r16(h.l4), dp = g.r16(h.l4 + 2);
          sip = g.r32(h.ip + 12), dip = g.r32(h.ip + 16);
        }
      }
      uint32_t fresh = 0;
      const uint32_t dst =
          ok ? fw_one_flow(a, T, in, sp, dp, sip, dip, proto, now, seq, &fresh, &tix) : kNone;
      m0 = f.w[0], m1 = f.w[1], m2 = f.w[2];
      uint32_t out = in;
      if (dst != kNone) {  // fw_main.c:76-77
        uint32_t mw[3];
        fw_macs(a, dst, mw);
        m0 = mw[0], m1 = mw[1], m2 = mw[2];
        out = dst;
      }
      res = (out & 0xFFFFu) | (fresh << 16) | js.flags;
    }
    res = __builtin_amdgcn_readfirstlane(res);
    if (J) {
      journal_touch(j, js, __builtin_amdgcn_readfirstlane(tix), seq, now, lane);
      journal_store(j, js, lane);
    }
    m0 = __builtin_amdgcn_readfirstlane(m0);
    m1 = __builtin_amdgcn_readfirstlane(m1);
    m2 = __builtin_amdgcn_readfirstlane(m2);
    // the answer chunks: the result and frame bytes 0-11, one store
    if (lane < min(need, 2u)) {
      const v4u v = lane == 0 ? (v4u){res, js.expired, 0u, want} : (v4u){m0, m1, m2, want};
      __builtin_amdgcn_raw_buffer_store_b128(v, io.as, (int)(16 * lane), 0, kSys);
    }
    // (the answer word: where a relaunched server starts counting; the host
    // reads the answer chunks. No release fence at system scope, which would
    // write back the whole L2)
    if (lane == 0)
      __hip_atomic_store(&box->ans, (uint64_t)want | ((uint64_t)res << 32), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    if (!full) seq += 1;
    t0 = wall_clock64();
    done = want;
    // (lane 0's table writes before the next request's lanes read them)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    wave_lds_sync();  // (lane 0's reads of fr before the next request's writes)
    return 0;
  };
  serve_poll(io, flags, idle, serve, [&] { return t0; });
}

// =============================================================== host ==

// fw_flowmanager.c:66-73: FlowManager.expiration_time is a vigor_time_t, so
// expiration_time * 1000 is computed in 64 bits (no wrap, unlike vignat).
static inline int64_t fw_cutoff(const vp_ctx *c, int64_t t) {
  return (int64_t)((uint64_t)t - (uint64_t)((int64_t)c->fw.expiration_time * 1000));
}

static int fw_segment(vp_ctx *c, const vp_dev_batch *b, const NowSpec &now,
                      uint32_t p0, uint32_t p1, float *ms, int *launches,
                      uint32_t *allocated) {
  FlowTable &t = c->ft;
  Workspace &w = c->ws;
  FwArgs a{};
  a.frames = b->frames;
  a.len = b->len;
  a.in_dev = b->in_dev;
  a.out = b->out_dev;
  a.log = w.log;
  const uint64_t seq0 = c->seq;
  a.seq_base = seq0;
  a.slot = b->slot;
  a.p0 = p0;
  a.p1 = p1;
  a.t = tbl_dev(t);
  a.crc_tab = c->crc_tab;
  a.macw = c->macw;
  a.miss = w.miss;
  a.defer = w.defer;
  a.reprobe = w.reprobe;
  a.wan = c->fw.wan_device;
  a.n_dev = c->fw.n_devices;

  // 64-byte slots: the classify launch also bins its touches (TouchBins)
  const bool tiles64 = p1 > p0 && b->slot == 64;
  BinsPlan bp{};
  uint32_t grid64 = 0, range64 = 0;
  TileQueue rq{};
  if (tiles64) {
    VP_TRY(tbl_bins_plan(c, t, (const void *)fw_classify64, p0, p1, &bp));
    const uint32_t tiles = (p1 - (p0 & ~63u) + 63) / 64;
    grid64 = resident_grid((const void *)fw_classify64, (tiles + 3) / 4);
    range64 = (tiles + grid64 - 1) / grid64 * 64;
    rq = TileQueue{w.reprobe, w.reprobe_cnt, &t.ctl->reprobe_count};
    a.tileq = 1;
  }
  // (still zero after a segment that queued nothing: no reset launch)
  VP_TRY(seg_reset_counters(c, t));
  VP_HIP(ev_record(c->ktime, c->ev0, c->stream));
  if (p1 > p0) {
    c->last_kernel = tiles64 ? "fw_classify64" : "fw_classify";
    if (tiles64) {
      FwArgs a64 = a;
      if (bp.on) a64.log = nullptr;  // touches go to the bins only
      fw_classify64<<<grid64, 256, 0, c->stream>>>(a64, b->n, bp.bins, rq);
    } else {
      fw_classify<<<grid_for(p1 - p0), 256, 0, c->stream>>>(a);
    }
    VP_HIP(hipGetLastError());
  }
  VP_HIP(ev_record(c->ktime, c->ev1, c->stream));
  // phase A's counts, and the fold of its touches behind them; queued
  // packets follow as late touches
  VP_TRY(tbl_fold_read_ctl(c, t, bp, w.log, p0, p1, now, seq0));
  // reprobes come only from the 64-byte tiles (fw_generic_a walks in place)
  const uint32_t nre = t.h_ctl.reprobe_count;
  if (nre) {  // probes past a full home bucket: finish them, patch the fold
    fw_reprobe<<<std::min<uint32_t>(grid64, 2048), 256, 0, c->stream>>>(
        a, w.reprobe, w.reprobe_cnt, nre, range64, grid64, seq0);
    VP_HIP(hipGetLastError());
    VP_TRY(tbl_reprobe_stamp(c, t, w.reprobe, w.reprobe_cnt, nre, range64, grid64,
                             w.log, now, seq0));
    VP_TRY(read_ctl(c, t));  // the walk may have found new flows
  }
  const bool ovf = bp.on && t.h_ctl.touch_ovf != 0;
  if (ovf)  // touches that found their bin slice full, logged alone
    VP_TRY(tbl_late_touches(c, t, bp.bins.oent, bp.bins.ocnt, 0, range64, grid64,
                            w.log, now, seq0));
  VP_TRY(seg_classify_ms(c, ms, launches));
  const uint32_t nmiss = t.h_ctl.miss_count, ndefer = t.h_ctl.defer_count;
  if (nmiss) {
    VP_TRY(phase_b_round(c, t, nmiss, &a.t, [&] {
      fw_miss_keys<<<grid_for(nmiss), 256, 0, c->stream>>>(a, w.miss_sorted, nmiss, w.mkey,
                                                           w.mhash);
    }, [&] {
      fw_miss_finish<<<grid_for(nmiss), 256, 0, c->stream>>>(
          a, w.miss_sorted, nmiss, w.mkey, w.scratch, w.rep, w.assign);
    }));
    VP_TRY(tbl_late_list(c, t, w.miss_sorted, nmiss, w.log, now, seq0));
    *allocated |= 1u;
  }
  if (ndefer) {  // (a.t: phase B's round refreshed it)
    fw_defer_finish<<<grid_for(ndefer), 256, 0, c->stream>>>(a, w.defer, ndefer);
    VP_HIP(hipGetLastError());
    VP_TRY(tbl_late_list(c, t, w.defer, ndefer, w.log, now, seq0));
  }
  if (nmiss || ndefer) VP_TRY(read_ctl(c, t));
  // steady state: frames and ports complete, only the stamp fold may run
  // (not when it reads the caller's time array)
  c->fold_pending = !b->now && !nre && !nmiss && !ndefer && !ovf;
  t.ctl_clean = !nre && !nmiss && !ndefer && !ovf;
  return 0;
}

static int fw_process_device(vp_ctx *c, const vp_dev_batch *b) {
  ExpiringTable tabs[1] = {{&c->ft, fw_cutoff}};
  return run_batch(c, b, tabs, 1, fw_segment);
}

// ---------------------------------------------------- vp_process_one --
// vigfw's launcher of the resident kernel (serve_launch, vp_serve.hip).
static int fw_serve_launch(vp_ctx *c, ServeBox *dbox, uint32_t flags) {
  FwArgs a{};
  a.t = tbl_dev(c->ft);
  a.crc_tab = c->crc_tab;
  a.macw = c->macw;
  a.wan = c->fw.wan_device;
  a.n_dev = c->fw.n_devices;
  return serve_launch_one(c, fw_serve<true>, fw_serve<false>, a, dbox, flags,
                          serve_journal_dev(c, fw_ops().serve));
}

// The largest host batch routed to the server as burst requests: the largest
// swept n at which the served path measured faster per packet than the batch
// pipeline on the MI355X (profiles/r08_fw_serve.txt: 0.19 against 0.25 us at
// 256, a tie at 384, 0.19 against 0.14 at 512); larger calls take the
// pipeline. The same value as vignat's kServeBurstRoute (vp_nat.hip), from
// vigfw's own sweep. VIGPATH_SERVE_BURST overrides it; 0 routes nothing.
constexpr uint32_t kFwBurstRoute = 256;

// vigfw through the mailbox (serve_process_one / serve_process_burst,
// vp_serve.hip): fw_serve reads nothing past a frame's first kServeInline
// bytes and only the MACs change, so one packet sends at most that much and
// takes back bytes 0-11; fw_burst reads a frame's first 64 bytes and 16 come
// back.
const NfOps &fw_ops() {
  static const NfOps ops = [] {
    NfOps o{};
    o.process_device = fw_process_device;  o.serve_launch = fw_serve_launch;
    o.n_devices = [](const vp_ctx *c) -> uint32_t { return c->fw.n_devices; };
    o.reads_in_port = false;
    ServeNf &s = o.serve;
    s.cutoff = fw_cutoff;  s.table = &vp_ctx::ft;
    s.one_whole = false;  s.one_in = kServeInline;  s.one_back = 12;
    s.burst_in = 64;  s.burst_back = 16;  s.burst_route = kFwBurstRoute;
    s.prof = false;  s.journal = true;
    s.cutoff2 = nullptr;  s.table2 = nullptr;
    return o;
  }();
  return ops;
}

// State by flow index: alloc, ts, FlowId bytes (vigfw/flow.h layout, padding
// zero) and int_devices.
int fw_dump(vp_ctx *c, uint8_t *alloc, int64_t *ts, uint8_t *keys,
            uint32_t *int_dev) {
  const uint32_t cap = c->ft.cap;
  std::vector<uint32_t> k(4ull * cap);
  VP_TRY(tbl_dump(c, c->ft, alloc, ts, k.data()));
  for (uint32_t i = 0; i < cap; i++) {
    const uint32_t *e = &k[4ull * i];
    uint8_t *o = keys + 16ull * i;
    memcpy(o, e, 12);
    o[12] = (uint8_t)e[3];
    o[13] = o[14] = o[15] = 0;
    int_dev[i] = alloc[i] ? e[3] >> 8 : 0;
  }
  return 0;
}

void build_fw_tables(std::vector<uint32_t> &tab) {
  tab.assign(kFwTabs * 256, 0);
  for (uint32_t j = 0; j < kFwTabs; j++)
    build_position_table(&tab[j * 256], kFwPos[j], kFwMsg);
}

}  // namespace vp
