/*
 * vigpath — MI355X-native implementation of Vigor's per-packet receive path
 * (parse -> CRC32C flow hash -> libVig map probe -> state update -> header
 * rewrite + IPv4/L4 checksum) for vignat, vigbridge, viglb, vigfw and vigpol.
 *
 * C ABI only: plain pointers and sizes, no HIP or torch types. Two layers:
 *
 *  1. The reference's own operator surface, nf.h (reference nf.h:8-18):
 *       bool nf_init(void);
 *       int  nf_process(uint16_t device, uint8_t *buffer,
 *                       uint16_t packet_length, vigor_time_t now);
 *       void nf_config_init(int argc, char **argv); nf_config_usage();
 *       nf_config_print(); FLOOD_FRAME
 *     exported by the per-NF shim libraries libvignat_nf.so /
 *     libvigbridge_nf.so / libviglb_nf.so / libvigfw_nf.so /
 *     libvigpol_nf.so (one NF per binary, as the
 *     reference builds one NF per binary, Makefile.dpdk). They link unchanged
 *     against the reference's nf.c (nf.c:143-216). See INTEGRATION.md.
 *
 *  2. The batch interface those shims sit on (libvigpath.so), which is what a
 *     batching caller (nf.c's VIGOR_BATCH_SIZE path, nf.c:178-215, or a GPU
 *     host loop) binds. It replaces the per-packet loop
 *     `for each mbuf: nf_process(...)` (nf.c:150-176) with one call per
 *     batch whose results are identical to calling nf_process on every
 *     packet in order.
 *
 * Error convention: 0 on success, a negative errno-style code on failure;
 * never aborts. "Drop" keeps the reference encoding: out_dev == in_dev.
 */
#ifndef VIGPATH_H
#define VIGPATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VP_FLOOD_FRAME ((uint16_t)-1) /* nf.h:8 FLOOD_FRAME */
#define VP_MAX_DEVICES 32

/* error codes (negated errno values) */
#define VP_OK 0
#define VP_EINVAL (-22)
#define VP_ENOMEM (-12)
#define VP_EIO (-5)       /* HIP runtime failure */
#define VP_ENOTSUP (-95)  /* outside the supported domain */
#define VP_ESTATE (-71)   /* EPROTO: a device-side protocol of the library broke
                           * (e.g. the fold kernel ended without publishing its
                           * control block); distinct from a HIP failure */

typedef struct vp_ctx vp_ctx;

/* ------------------------------------------------------------ configs --
 * Field meanings and units are exactly the reference's struct nf_config. */

/* vignat/nat_config.h:5-31 (+ the device MACs nf_config_init reads through
 * rte_eth_macaddr_get, nat_config.c:34-37). */
typedef struct vp_nat_config {
  uint16_t wan_device;
  uint16_t lan_main_device;
  uint16_t start_port;
  uint32_t external_addr;   /* host-order value, as nf_parse_ipv4addr makes */
  uint32_t expiration_time; /* microseconds */
  uint32_t max_flows;       /* power of two (map.c:73, -DCAPACITY_POW2) */
  uint16_t n_devices;       /* rte_eth_dev_count_avail() */
  uint8_t device_macs[VP_MAX_DEVICES][6];
  uint8_t endpoint_macs[VP_MAX_DEVICES][6];
} vp_nat_config;

/* vigbridge/bridge_config.h:8-18; the --config static table is passed as
 * rules instead of a file name (bridge_main.c:130-230 parses the file into
 * exactly these triples). */
typedef struct vp_bridge_rule {
  uint8_t mac[6];
  int32_t device_from;
  int32_t device_to; /* -2 filters (bridge_main.c:322-325) */
} vp_bridge_rule;
typedef struct vp_bridge_config {
  uint32_t expiration_time; /* microseconds */
  uint32_t dyn_capacity;    /* power of two */
  uint16_t n_devices;
  uint32_t n_static;
  const vp_bridge_rule *static_rules;
} vp_bridge_config;

/* viglb/lb_config.h:8-38 */
typedef struct vp_lb_config {
  uint32_t flow_capacity;           /* power of two */
  uint32_t flow_expiration_time;    /* microseconds */
  uint32_t backend_capacity;        /* power of two, < cht_height */
  uint32_t cht_height;              /* prime */
  uint32_t backend_expiration_time; /* microseconds */
  uint16_t wan_device;
  uint16_t n_devices;
  uint8_t device_macs[VP_MAX_DEVICES][6];
} vp_lb_config;

/* vigfw/fw_config.h:9-24 (+ device MACs, as for vignat). */
typedef struct vp_fw_config {
  uint16_t wan_device;
  uint32_t expiration_time; /* microseconds */
  uint32_t max_flows;       /* power of two (map.c:73, -DCAPACITY_POW2) */
  uint16_t n_devices;       /* rte_eth_dev_count_avail() */
  uint8_t device_macs[VP_MAX_DEVICES][6];
  uint8_t endpoint_macs[VP_MAX_DEVICES][6];
} vp_fw_config;

/* vigpol/policer_config.h:8-24 (policer_config.c:17-93 parses it). */
typedef struct vp_pol_config {
  uint16_t lan_device;
  uint16_t wan_device;
  uint64_t rate;         /* B/s, > 0 */
  uint64_t burst;        /* B, > 0 */
  uint32_t dyn_capacity; /* power of two (map.c:73, -DCAPACITY_POW2) */
  uint16_t n_devices;    /* rte_eth_dev_count_avail() */
} vp_pol_config;

/* Create an NF instance whose state lives in HBM of HIP device `gpu`.
 * Returns 0 and *out, or VP_EINVAL for a configuration the reference's
 * nf_init would reject (non power-of-two capacities, ...). */
int vp_nat_create(const vp_nat_config *cfg, int gpu, vp_ctx **out);
int vp_bridge_create(const vp_bridge_config *cfg, int gpu, vp_ctx **out);
int vp_lb_create(const vp_lb_config *cfg, int gpu, vp_ctx **out);
int vp_fw_create(const vp_fw_config *cfg, int gpu, vp_ctx **out);
int vp_pol_create(const vp_pol_config *cfg, int gpu, vp_ctx **out);
void vp_destroy(vp_ctx *ctx);

/* ------------------------------------------------------------ batches -- */

/* A batch already resident in device memory (all pointers are device
 * pointers). Frames sit `slot` bytes apart from a 16-byte aligned start and
 * are rewritten in place, like the mbuf data nf_process mutates
 * (nf.c:154-156). `slot` must be a multiple of 16 and >= 64 (wider slots:
 * frames up to the slot, e.g. 1518 B in 1536 or mbuf-sized 2048). Bytes past a frame's slot read as 0.
 * Time: if `now` is NULL, packet i has now0 + i * now_step (ns); otherwise
 * now[i]. Times must be non-decreasing (nf.c takes them from
 * CLOCK_MONOTONIC, vigor-time.c:56-66) and >= 0 (nat_flowmanager.c:58). */
typedef struct vp_dev_batch {
  uint8_t *frames;
  uint32_t slot;
  uint32_t n;
  const uint16_t *len;
  const uint16_t *in_dev;
  const int64_t *now;
  int64_t now0;
  int64_t now_step;
  uint16_t *out_dev; /* nf_process's return value, stored as u16 (nf.c:156) */
  /* in_dev == NULL: every packet arrived on port in_port (nf.c receives each
   * burst from one device, nf.c:150-153 / 186-190), and no per-packet port
   * array is read. vp_process_device only; the host entry points need
   * in_dev. A port above 0xFFFF (nf_process's uint16_t device, nf.h:14) is
   * VP_EINVAL. */
  uint32_t in_port;
} vp_dev_batch;

/* Process one device-resident batch on HIP stream `stream` (a hipStream_t,
 * or NULL for the context's own stream). Returns after the results (frames,
 * out_dev) are in device memory; from then on no work of the library reads
 * the caller's buffers, so all of them (the per-packet time array included)
 * may be refilled or freed at once. With affine time (now == NULL) the fold
 * of the flow timestamps, which reads only library workspace, may still be
 * running on the context's stream when it returns; it is ordered before
 * every later call on this context (dumps, counts, the next batch) and
 * before work enqueued on `stream` afterwards. A batch with a time array
 * completes entirely before the call returns. */
int vp_process_device(vp_ctx *ctx, const vp_dev_batch *batch, void *stream);

/* ----------------------------------------------------------- transmit --
 * What nf.c does with nf_process's return value (nf.c:159-174; 201-209 in
 * the batched loop), for a batch that stays in device memory: per-port lists
 * of packet indices, built on the GPU from out_dev. The frames stay where
 * they are and are never read. */

typedef struct vp_tx_stats {
  uint64_t packets[VP_MAX_DEVICES]; /* entries of port d's list, flood copies included */
  uint64_t bytes[VP_MAX_DEVICES];   /* sum of len[] over those entries */
  uint64_t dropped;                 /* out_dev == in port (nf.c:159) */
  uint64_t flooded;                 /* out_dev == VP_FLOOD_FRAME (packets, not copies) */
  uint64_t bad_port;                /* anything else >= n_devices: in no list */
} vp_tx_stats;

typedef struct vp_tx_lists {
  uint32_t *idx;      /* device, `cap` entries: packet indices, port 0's list first,
                         then port 1's, ...; inside a list ascending (packet order) */
  uint32_t cap;
  uint32_t *offset;   /* device, n_devices + 1 entries: list d = idx[offset[d] .. offset[d+1]) */
  vp_tx_stats *stats; /* device, or NULL */
} vp_tx_lists;

/* Build the transmit lists of a device-resident batch (after
 * vp_process_device filled its out_dev). Reads batch->n, out_dev, in_dev (or
 * in_port when in_dev is NULL) and len (only with stats; may then not be
 * NULL), and nothing else of the batch. n_devices is the context's own
 * (its vp_*_config). Per packet i, in = its input port, out = out_dev[i], in
 * this order:
 *   out == in               dropped                              (nf.c:159)
 *   out == VP_FLOOD_FRAME   i joins the list of every port d < n_devices,
 *                           d != in (flood(), nf.c:82-96; an in >= n_devices
 *                           skips no port); counted once in `flooded`
 *   out < n_devices         i joins list `out`       (rte_eth_tx_burst(out))
 *   otherwise               counted in bad_port, in no list
 * Every list is in ascending packet order -- the order of nf.c's tx_burst
 * calls for that port -- and the result is deterministic: the same input
 * gives the same bytes. offset[] and *stats are written whole by every call
 * (never accumulated) and always hold the true counts. When the total
 * offset[n_devices] exceeds cap, positions at or beyond cap are not written,
 * positions below it hold what they would with enough room, and the call
 * still returns 0: the caller sees offset[n_devices] > cap.
 * The work (three kernel launches) is enqueued on `stream` (a hipStream_t,
 * or NULL for the context's own stream), ordered after the work already on
 * that stream, and the call MAY RETURN BEFORE THE LISTS ARE WRITTEN: wait for
 * the stream before reading them on the host. It makes no host round trip.
 * Like every call that launches device work on the context, it ends the NF's
 * resident kernel (vp_process_one): the kernel leaves, and the next small
 * call launches it again. After a multi-GPU attach the call is local to the
 * rank: not a collective, and it covers only this rank's slice.
 * VP_EINVAL: a NULL ctx, batch, lists, out_dev or offset; a NULL idx with
 * cap > 0; a NULL len with stats; in_dev NULL and in_port > 0xFFFF; n *
 * max(1, n_devices - 1) beyond 32 bits; a context with more than
 * VP_MAX_DEVICES devices. n == 0: all offsets 0, stats zero. */
int vp_tx_build(vp_ctx *ctx, const vp_dev_batch *batch, const vp_tx_lists *lists, void *stream);

typedef struct vp_tx_frames {
  uint8_t *data;      /* device, 16-byte aligned, cap_bytes bytes; may be NULL iff cap_bytes == 0 */
  uint64_t cap_bytes;
  uint64_t *port_off; /* device, n_devices + 1: port d's bytes are data[port_off[d] .. port_off[d+1]) */
  uint64_t *pos;      /* device, lists->cap entries, or NULL: pos[e] = byte offset in data of
                         entry e's frame */
} vp_tx_frames;

/* Pack the frames that the lists of vp_tx_build name into one contiguous
 * byte stream per port, in transmit order: what flood()'s reference counts
 * and rte_eth_tx_burst's mbuf pointers (nf.c:82-96, 159-174) amount to for a
 * batch in device memory. Reads batch->frames, slot, n and len, and the lists'
 * idx, cap and offset (device memory); writes nothing but out's buffers, and
 * never the frames. With
 *   E       = min(offset[n_devices], cap)   the entries idx really holds
 *   i       = idx[e]
 *   clen(e) = min(len[i], slot), pad(e) = (clen(e) + 15) & ~15     when i < n
 *   clen(e) = pad(e) = 0, and nothing is read through i            when i >= n
 *             (vp_tx_build writes no such entry; a garbage list cannot make
 *             the call read outside the batch)
 *   pos(e)  = sum of pad(k) over k < e, k < E   (64 bits)
 * the lists being port-major, one running sum lays port 0's frames first,
 * then port 1's, each port in packet order:
 *   data[pos(e) .. pos(e) + clen(e))            frame i's first clen bytes
 *   data[pos(e) + clen(e) .. pos(e) + pad(e))   zero
 *   port_off[d] = pos(min(offset[d], cap)) for d <= n_devices; port_off[n_devices]
 *                                               is the total
 *   pos[e] = pos(e) for e < E, when pos is not NULL; nothing at or beyond pos[E]
 * A flooded frame is copied once per list it stands in. An entry is written
 * whole or not at all: iff pos(e) + pad(e) <= cap_bytes. port_off[] and pos[]
 * always hold the true values, and the call still returns 0 when frames did
 * not fit: the caller sees port_off[n_devices] > cap_bytes (as vp_tx_build
 * does with cap). No byte of data at or beyond min(total, cap_bytes) is
 * written. The result is deterministic: the same inputs give the same bytes
 * everywhere the call writes. With cap == 0 every port_off is 0.
 * The work (three kernel launches, the grid sized from lists->cap) is enqueued
 * on `stream` (NULL: the context's own), after the work already there, and
 * the call MAY RETURN BEFORE IT RAN. It makes no host round trip: offset[] is
 * read on the device only. Ordering against the vp_tx_build that filled the
 * lists is the caller's (the same stream, or an event); the library orders its
 * own workspace. Like vp_tx_build it ends the NF's resident kernel, and after
 * a multi-GPU attach it is local to the rank.
 * VP_EINVAL: a NULL ctx, batch, lists, out, port_off or offset; a NULL idx
 * with cap > 0; a NULL frames or len with n > 0 and cap > 0; slot below 64 or
 * not a multiple of 16; frames or data not 16-byte aligned; a NULL data with
 * cap_bytes > 0; a context with more than VP_MAX_DEVICES devices. */
int vp_tx_pack(vp_ctx *ctx, const vp_dev_batch *batch, const vp_tx_lists *lists,
               const vp_tx_frames *out, void *stream);

typedef struct vp_tx_next {
  uint8_t  *frames; /* device, 16-byte aligned, cap * slot bytes; may be NULL iff cap == 0 */
  uint32_t  slot;   /* multiple of 16, >= 64; need not equal the source batch's slot */
  uint32_t  cap;    /* packets the buffers below hold */
  uint16_t *len;    /* device, cap entries */
  int64_t  *now;    /* device, cap entries, or NULL */
  uint32_t *src;    /* device, cap entries, or NULL: index in the source batch */
  uint32_t *count;  /* device, one word: entries of the port's list (may exceed cap) */
} vp_tx_next;

/* Hand one port's list to the next NF as a device batch: the frames that list
 * `port` of vp_tx_build names, gathered into consecutive slots with their
 * len[], their time and their index of origin -- the cable between two of the
 * reference's boxes (one NF per binary, nf.c:150-176 on each side), for two
 * contexts on one GPU. Reads batch->frames, slot, n, len and now (or now0 and
 * now_step), and the lists' idx, cap and offset (device memory); writes nothing
 * but out's buffers, and never the source batch or the lists. With
 *   E  = min(offset[n_devices], cap)          the entries idx really holds
 *   lo = min(offset[port], E), hi = min(offset[port + 1], E)
 *   C  = hi - lo                              what idx holds of that list
 *   i  = idx[lo + k] for k < C
 *   w  = min(batch->slot, out->slot)
 * the call writes *count = C, always the true count, also when C > out->cap,
 * and for k < min(C, out->cap) with i < n:
 *   frames[k*slot .. k*slot + w)         the first w bytes of source slot i,
 *                                        verbatim: the slot image, the bytes
 *                                        past len[i] included, as an mbuf
 *                                        passed on by pointer keeps them
 *   frames[k*slot + w .. (k+1)*slot)     zero (bytes past a frame's slot read
 *                                        as 0)
 *   len[k] = len[i]                      unchanged, not clipped to a slot
 *   now[k] = batch->now[i], or now0 + i * now_step (64 bits) when batch->now
 *                                        is NULL
 *   src[k] = i
 * and with i >= n (vp_tx_build writes no such entry; a garbage list cannot
 * make the call read outside the batch) nothing is read through i: the slot is
 * zero, len[k] = 0, now[k] = 0, src[k] = i. Nothing at or beyond entry
 * min(C, out->cap) of any buffer is written. The result is deterministic: the
 * same inputs give the same bytes. The order inside the output is the list's,
 * packet order, so a batch whose times do not go back gives times that do not
 * go back; the output is a valid vp_dev_batch for any context, with in_dev
 * NULL and an in_port of the caller's choosing.
 * The work (one kernel launch, the grid sized from out->cap, at least one
 * block so that count is written when cap == 0) is enqueued on `stream` (NULL:
 * the context's own), after the work already there, and the call MAY RETURN
 * BEFORE IT RAN. It makes no host round trip: offset[] is read on the device
 * only. Ordering against the vp_tx_build that filled the lists is the
 * caller's (the same stream, or an event). It needs no workspace. Like
 * vp_tx_build it ends the NF's resident kernel, and after a multi-GPU attach
 * it is local to the rank.
 * VP_EINVAL: a NULL ctx, batch, lists, out, offset or count; a NULL idx with
 * lists->cap > 0; port >= n_devices; a context with more than VP_MAX_DEVICES
 * devices; either slot below 64 or not a multiple of 16; either frames not
 * 16-byte aligned; a NULL out->frames or out->len with out->cap > 0; a NULL
 * batch->frames or batch->len with n > 0, lists->cap > 0 and out->cap > 0; the
 * byte ranges [batch->frames, + n * slot) and [out->frames, + cap * slot)
 * overlapping. */
int vp_tx_rebatch(vp_ctx *ctx, const vp_dev_batch *batch, const vp_tx_lists *lists,
                  uint32_t port, const vp_tx_next *out, void *stream);

#define VP_TX_MERGE_MAX 8

typedef struct vp_tx_source {
  vp_ctx *ctx;               /* the context whose n_devices shaped `lists` */
  const vp_dev_batch *batch; /* frames, slot, n, len, now | now0, now_step */
  const vp_tx_lists *lists;  /* as vp_tx_build wrote them */
  uint32_t port;             /* which list */
  uint32_t in_port;          /* port these packets arrive on (<= 0xFFFF) */
  const uint32_t *key;       /* device, batch->n entries, or NULL: key(i) = i */
} vp_tx_source;

typedef struct vp_tx_merged {
  uint8_t  *frames; /* device, 16-byte aligned, cap * slot bytes; may be NULL iff cap == 0 */
  uint32_t  slot;   /* multiple of 16, >= 64; need not equal any source's slot */
  uint32_t  cap;    /* packets the buffers below hold */
  uint16_t *len;    /* device, cap entries */
  int64_t  *now;    /* device, cap entries, or NULL */
  uint16_t *in_dev; /* device, cap entries, or NULL: srcs[j].in_port of each packet's source */
  uint32_t *key;    /* device, cap entries, or NULL: the packet's merge key */
  uint32_t *src;    /* device, cap entries, required with cap > 0: index in its source batch */
  uint8_t  *which;  /* device, cap entries, required with cap > 0: its source number j */
  uint32_t *count;  /* device, one word: total entries of all sources (may exceed cap) */
} vp_tx_merged;

/* Merge several lists into one NF's device batch: where the cables of several
 * boxes (or of several ports of one) lead into one box, that box sees their
 * packets interleaved by the time they entered the first box. What
 * vp_tx_rebatch does for one list, for n_srcs of them, ordered by a 32-bit key
 * per packet: the caller passes each packet's position in the chain's input.
 * Reads, of every source, batch->frames, slot, n, len and now (or now0 and
 * now_step), the lists' idx, cap and offset, and key (device memory); writes
 * nothing but out's buffers, and never a source batch, a list or a key array.
 * Per source j, with n_devices that of srcs[j].ctx,
 *   E_j  = min(offset[n_devices], cap)        the entries idx really holds
 *   lo_j = min(offset[port], E_j), hi_j = min(offset[port + 1], E_j)
 *   C_j  = hi_j - lo_j                        what idx holds of that list
 * and total = the sum of all C_j. Entry (j, m), m < C_j, is packet
 *   i = idx_j[lo_j + m]   with   key(j, m) = key_j[i], or i when key is NULL;
 *                                with i >= n_j the key is i, and nothing is
 *                                read through i
 * The output holds all entries ordered by key, ascending; among equal keys by
 * source number j, ascending; within one source in list order m. Equivalently
 * entry (j, m) with key x stands at position
 *   p = m + sum over j' < j of #{m' : key(j', m') <= x}
 *         + sum over j' > j of #{m' : key(j', m') <  x}
 * which is that stable merge provided every source's keys do not decrease
 * along its list -- true of key == NULL (vp_tx_build's lists ascend) and of the
 * composed origins of a batch in packet order. The precondition is the
 * caller's. Where keys do decrease the order is unspecified, but the call
 * still reads nothing outside the batches, lists and key arrays and writes
 * nothing at or beyond min(total, cap) of any output buffer.
 * The call writes *count = total, always the true value, also when total >
 * out->cap (0xFFFFFFFF where the sum passes 32 bits), and for every position
 * p < min(total, out->cap), with (j, m) the entry that stands there, i its
 * packet and w = min(srcs[j].batch->slot, out->slot):
 *   frames[p*slot .. p*slot + w)        the first w bytes of source j's slot
 *                                       i, verbatim, as vp_tx_rebatch; source
 *                                       slots may differ from each other
 *   frames[p*slot + w .. (p+1)*slot)    zero
 *   len[p] = len_j[i]                   unchanged, not clipped to a slot
 *   now[p] = now_j[i], or that source's now0 + i * now_step (64 bits)
 *   in_dev[p] = srcs[j].in_port
 *   key[p] = key(j, m),  src[p] = i,  which[p] = j
 * and with i >= n_j the slot is zero, len[p] = 0 and now[p] = 0. Nothing at or
 * beyond entry min(total, out->cap) of any buffer is written. The result is
 * deterministic. Times that do not go back inside every source and agree with
 * the key order give times that do not go back; the output is a valid
 * vp_dev_batch for `ctx` with in_dev = out->in_dev. With n_srcs == 1 and
 * key == NULL, frames, len, now and src hold exactly vp_tx_rebatch's bytes.
 * `ctx` is the receiving NF's context; it supplies the default stream. Every
 * source context must be on ctx's GPU (a source may be ctx itself). The work
 * (two kernel launches, the grids sized from out->cap, at least one block so
 * that count is written when cap == 0) is enqueued on `stream` (NULL: ctx's
 * own), after the work already there, and the call MAY RETURN BEFORE IT RAN. It
 * makes no host round trip: every offset[] is read on the device only.
 * Ordering against the vp_tx_build calls that filled the lists is the
 * caller's (the same stream, or events). It needs no workspace. It ends the
 * resident kernel of ctx and of every source context, and after a multi-GPU
 * attach it is local to the rank.
 * VP_EINVAL: a NULL ctx, srcs, out or count; n_srcs == 0 or above
 * VP_TX_MERGE_MAX; per source everything vp_tx_rebatch rejects (a NULL batch,
 * lists or offset; a NULL idx with lists->cap > 0; port >= n_devices; a
 * context with more than VP_MAX_DEVICES devices; a slot below 64 or not a
 * multiple of 16; frames not 16-byte aligned; a NULL batch->frames or
 * batch->len with n > 0, lists->cap > 0 and out->cap > 0; its slot array
 * overlapping out->frames); in_port > 0xFFFF; a source context that is NULL or
 * on another GPU; out->slot below 64 or not a multiple of 16; out->frames not
 * 16-byte aligned; a NULL out->frames, len, src or which with out->cap > 0. */
int vp_tx_merge(vp_ctx *ctx, const vp_tx_source *srcs, uint32_t n_srcs,
                const vp_tx_merged *out, void *stream);

/* ------------------------------------------------------------ receive --
 * The way back in: frames that arrive as one packed run of bytes -- a capture,
 * a buffer a NIC or another GPU wrote, the stream the pack call above made on
 * another device -- as a device batch in equal slots. */

typedef struct vp_rx_stream {
  const uint8_t  *data;    /* device, 16-byte aligned; may be NULL iff bytes == 0 */
  uint64_t        bytes;   /* bytes of data that may be read */
  uint32_t        n;       /* entries (frames) in the stream */
  const uint64_t *pos;     /* device, n entries, or NULL: byte offset of entry e's frame */
  const uint32_t *sel;     /* device, n entries, or NULL: m(e) = sel[e]; NULL: m(e) = e */
  uint32_t        meta_n;  /* entries of len[] and now[] */
  const uint16_t *len;     /* device, meta_n entries */
  const int64_t  *now;     /* device, meta_n entries, or NULL */
  int64_t         now0, now_step;
} vp_rx_stream;

/* Unpack a stream of frames into consecutive slots: the inverse of the pack
 * call above, filling the struct the rebatch call fills, so whatever consumes
 * a rebatched batch consumes an unpacked one. Reads data, pos, sel, len and
 * now (device memory); writes nothing but out's buffers. For entry e < n, with
 *   m      = sel[e], or e when sel is NULL     its index into len[] and now[]
 *   L      = len[m] when m < meta_n, else 0    (nothing is read through an
 *                                              m >= meta_n)
 *   ext(e) = (L + 15) & ~15
 *   p(e)   = pos[e], or, when pos is NULL, the sum of ext(k) over k < e (64
 *            bits): a self-describing stream, the frames back to back at
 *            their own padded lengths
 *   r      = min(L, out->slot)
 * entry e is readable iff m < meta_n, p(e) % 16 == 0 and
 * p(e) + ((r + 15) & ~15) <= bytes, the sum taken without wrapping (a p near
 * 2^64 is not readable). The call writes *count = n, also when n > out->cap,
 * and for k = e < min(n, out->cap), readable:
 *   frames[k*slot .. k*slot + r)         data[p .. p + r)
 *   frames[k*slot + r .. (k+1)*slot)     zero; the bytes of the last 16-byte
 *                                        unit past L are cleared, never
 *                                        trusted from the stream
 *   len[k] = L                           unchanged, not clipped to a slot
 *   now[k] = now[m], or now0 + m * now_step (64 bits) when now is NULL
 *   src[k] = m
 * and not readable: the slot is zero, len[k] = 0, now[k] = 0, src[k] = m, and
 * nothing is read from data for it. Nothing at or beyond entry min(n,
 * out->cap) of any buffer is written. The result is deterministic: the same
 * inputs give the same bytes. The output is a valid vp_dev_batch for any
 * context, with in_dev NULL and an in_port of the caller's choosing.
 * Port d of a packed batch comes back with, lo = offset[d], hi = offset[d + 1]
 * of its lists: pos = the packed pos + lo, sel = the lists' idx + lo, n = hi -
 * lo, meta_n = the batch's n, len and the time the batch's, data and bytes the
 * packed stream. Without pos the entries' lengths must be their own (sel, or
 * a len[] already in stream order) and data must start at the first frame
 * (the packed data + port_off[d]); that form matches a packed stream only
 * where every len is <= the source slot: pack pads min(len, slot), a
 * self-describing stream pads len. For the same reason, with pos, a len beyond
 * the source slot unpacked into a wider slot takes the bytes behind its frame
 * (the next frames') for its own up to min(len, out->slot): the stream does
 * not say where a clipped frame ends.
 * The work is enqueued on `stream` (NULL: the context's own), after the work
 * already there, and the call MAY RETURN BEFORE IT RAN: one kernel launch with
 * pos, three without (the padded lengths summed per wave, scanned by one
 * block, then the scatter), the grids sized from min(n, out->cap), at least
 * one block so that count is written. It makes no host round trip. The
 * library orders its own workspace (the sums) between streams. Like
 * vp_tx_build it ends the NF's resident kernel, and after a multi-GPU attach
 * it is local to the rank. The context supplies only the GPU and the default
 * stream: its n_devices plays no part.
 * VP_EINVAL: a NULL ctx, in, out or count; a NULL data with bytes > 0; data or
 * out->frames not 16-byte aligned; a NULL len with meta_n > 0; out->slot below
 * 64 or not a multiple of 16; a NULL out->frames or out->len with out->cap >
 * 0; the byte ranges [data, + bytes) and [out->frames, + cap * slot)
 * overlapping. n == 0: count 0, nothing else written. */
int vp_rx_unpack(vp_ctx *ctx, const vp_rx_stream *in, const vp_tx_next *out, void *stream);

#define VP_RX_MERGE_MAX 8

typedef struct vp_rx_queue {
  vp_rx_stream stream;  /* exactly vp_rx_unpack's input, every field with its meaning there */
  uint32_t     in_port; /* port these frames arrived on (<= 0xFFFF) */
} vp_rx_queue;

/* Merge several receive queues by time into one NF's device batch: a box with
 * several ports gets one packed stream per port, each with its own len[] and
 * times, and the NF's result depends on how their packets interleave. nf.c
 * polls its devices in turn and stamps each packet; this call gives the batch
 * that loop would have handed the NF, for streams already in device memory.
 * What vp_rx_unpack does for one stream, for n_queues of them, ordered by each
 * frame's 64-bit time, with the port of each packet beside it. Reads, of every
 * queue, data, pos, sel, len and now (device memory); writes nothing but out's
 * buffers. The output struct is vp_tx_merged as vp_tx_merge fills it, except
 * that out->key must be NULL: a time is 64 bits and comes out in out->now.
 * Entry (j, e), e < n_j, of queue j has m, L, p(e), r and "readable" exactly as
 * vp_rx_unpack defines them for queues[j].stream. Its key is the signed 64-bit
 * time
 *   t(j, e) = now_j[m], or now0_j + m * now_step_j (64 bits) when now_j is NULL
 *   t(j, e) = INT64_MAX when m >= meta_n_j (nothing is read through such an m)
 * and all 64 bits are compared, as signed values. The output holds every entry
 * of every queue ordered by time, ascending; among equal times by queue number
 * j, ascending (nf.c polls its devices in ascending order); within one queue in
 * entry order e. Equivalently entry (j, e) with time t stands at position
 *   p = e + sum over j' < j of #{e' : t(j', e') <= t}
 *         + sum over j' > j of #{e' : t(j', e') <  t}
 * which is that stable merge provided every queue's times do not decrease
 * along its entries. The precondition is the caller's. Where times do decrease
 * the order is unspecified, but the call still reads nothing outside the
 * queues' arrays and writes nothing at or beyond min(total, cap) of any output
 * buffer.
 * The call writes *count = total = the sum of all n_j, always the true sum,
 * also when it exceeds out->cap (0xFFFFFFFF where the sum passes 32 bits), and
 * for every position p < min(total, out->cap), with (j, e) the entry that
 * stands there:
 *   frames[p*slot .. (p+1)*slot)   the slot as vp_rx_unpack writes it: readable,
 *                                  data_j[p(e) .. p(e) + r) and zeros behind,
 *                                  the bytes of the last 16-byte unit past L
 *                                  cleared; not readable, a zero slot, and
 *                                  nothing is read from data_j for it
 *   len[p] = L                     unchanged, not clipped to a slot; 0 when not
 *                                  readable
 *   now[p] = t(j, e)               ALSO FOR AN ENTRY THAT IS NOT READABLE: the
 *                                  one deliberate difference from vp_rx_unpack,
 *                                  which stores 0 there. A broken frame must not
 *                                  make the batch's clock go back (the process
 *                                  call refuses such a batch); it is a packet of
 *                                  length 0 at its own time
 *   in_dev[p] = queues[j].in_port  when out->in_dev is not NULL
 *   src[p] = m,  which[p] = j
 * Nothing at or beyond entry min(total, out->cap) of any buffer is written. The
 * result is deterministic. Times that do not go back inside every queue give
 * times that do not go back; the output is a valid vp_dev_batch for `ctx` with
 * in_dev = out->in_dev. With one queue whose entries are all readable, frames,
 * len, now and src hold exactly vp_rx_unpack's bytes.
 * `ctx` is the receiving NF's context; it supplies the GPU, the default stream
 * and the workspace. The work is enqueued on `stream` (NULL: ctx's own), after
 * the work already there, and the call MAY RETURN BEFORE IT RAN: two kernel
 * launches (the ranks with the small records, then the frames), and before
 * them two per queue without pos (its padded lengths summed per wave and
 * scanned, as in vp_rx_unpack); the first grid is sized from the n_j, the second
 * from min(total, out->cap), at least one block so that count is written. It
 * makes no host round trip. The library orders its own workspace (each
 * position's place in its stream, 8 bytes, and the sums) between streams. Like
 * its neighbours it ends ctx's resident kernel, and after a multi-GPU attach it
 * is local to the rank.
 * VP_EINVAL (vp_last_error says which): a NULL ctx, queues, out or count;
 * n_queues == 0 or above VP_RX_MERGE_MAX; per queue everything vp_rx_unpack
 * rejects for its stream (a NULL data with bytes > 0; data not 16-byte aligned;
 * a NULL len with meta_n > 0; [data, + bytes) overlapping [out->frames, + cap *
 * slot)); in_port > 0xFFFF; out->key not NULL; out->slot below 64 or not a
 * multiple of 16; out->frames not 16-byte aligned; a NULL out->frames, len, src
 * or which with out->cap > 0. */
int vp_rx_merge(vp_ctx *ctx, const vp_rx_queue *queues, uint32_t n_queues,
                const vp_tx_merged *out, void *stream);

/* ----------------------------------------------------------- the way home --
 * A chain of NFs standing where one NF stands: the packets a later stage
 * received come back to the slots they started from in the caller's batch,
 * with their out ports renamed to the ports of the composite box. */

#define VP_RET_SKIP 0x10000u  /* leave the home packet alone (it travelled on over a link) */
#define VP_RET_DROP 0x10001u  /* home out_dev = the home packet's own in port (nf.c:159) */
/* any value <= 0xFFFF: written to home out_dev literally (VP_FLOOD_FRAME included) */

typedef struct vp_tx_return_stats {
  uint64_t returned;  /* entries written home (drops included) */
  uint64_t dropped;   /* of those, written as VP_RET_DROP */
  uint64_t skipped;   /* firsts whose action was VP_RET_SKIP */
  uint64_t dup;       /* entries that were not the first of their run of equal home indices */
  uint64_t bad_home;  /* firsts whose home index is >= home->n: nothing written */
} vp_tx_return_stats;

typedef struct vp_tx_way_home {
  const uint32_t *home;              /* device, from->n entries, or NULL: home(k) = k */
  uint32_t port[VP_MAX_DEVICES];     /* action for out == d, d < n_devices of ctx */
  uint32_t on_drop, on_flood, on_bad;/* out == the entry's in port; VP_FLOOD_FRAME; any other */
  vp_tx_return_stats *stats;         /* device, or NULL */
} vp_tx_way_home;

/* Return a stage's batch into the batch its packets came from: the inverse of
 * vp_tx_rebatch. Where that call gathers the slots a list names into
 * consecutive slots and records each one's index of origin, this one scatters
 * consecutive slots back to such indices, and translates each packet's out
 * port -- a port of the stage that produced `from` -- into a port of the box
 * that holds the whole chain. Reads from->frames, slot, n, out_dev and in_dev
 * (or in_port), home->slot, n and in_dev (or in_port), and way->home (device
 * memory); writes slots and out_dev entries of `home`, and nothing else.
 * `ctx` is the stage that produced `from`: it supplies n_devices, the GPU and
 * the default stream. For entry k < from->n, with
 *   h     = way->home[k], or k when way->home is NULL
 *   first = k == 0 or h differs from entry k - 1's h   (the first of a run of
 *           equal home indices: the copies one stage holds of one packet)
 *   out   = from->out_dev[k],  in = from->in_dev[k] or from->in_port
 * the action a is chosen in vp_tx_build's order:
 *   out == in               a = way->on_drop                         (nf.c:159)
 *   out == VP_FLOOD_FRAME   a = way->on_flood
 *   out < n_devices         a = way->port[out]
 *   otherwise               a = way->on_bad
 * Entry k is written home iff it is a first, h < home->n and a != VP_RET_SKIP,
 * and then, with slot_h = home->slot and w = min(from->slot, home->slot):
 *   home->frames[h*slot_h .. h*slot_h + w)        the first w bytes of from's
 *                                                 slot k, verbatim
 *   home->frames[h*slot_h + w .. (h+1)*slot_h)    zero
 *   home->out_dev[h] = a, or for a == VP_RET_DROP the home packet's own in
 *                      port: home->in_dev[h], or home->in_port
 * len is neither read nor written (no NF changes a length). Nothing else of
 * `home` is written: a slot of `home` that no written entry names keeps every
 * byte, and so does its out_dev entry.
 * from->frames == home->frames with equal slots and way->home == NULL is the
 * batch that is its own home: stage 0, which vp_process_device rewrote in
 * place. No frame byte moves, only out_dev is translated, and from->out_dev
 * and home->out_dev may then be the same array (only then). Any other overlap
 * of the two slot ranges [frames, + n * slot) is VP_EINVAL.
 * The result is deterministic whenever home[] does not decrease: the firsts
 * then have distinct homes, and no two lanes write one slot. That holds for
 * src[] of vp_tx_rebatch and vp_rx_unpack, key[] of vp_tx_merge, and origins
 * composed from them along a chain. Where home[] does decrease, which of two
 * firsts with one home wins is unspecified (bytes of both may mix in the
 * slot), but the call still reads and writes nothing outside the two batches.
 * *stats is written whole by every call (never accumulated) and always holds
 * the true counts, which are sums and so deterministic in every case. A first
 * whose action is VP_RET_SKIP and whose home index is >= home->n counts in
 * both skipped and bad_home; from->n = returned + dup + (the firsts not
 * written).
 * The work is enqueued on `stream` (NULL: the context's own), after the work
 * already there, and the call MAY RETURN BEFORE IT RAN: one kernel launch, the
 * grid sized from from->n, in front of it a 40-byte clear of *stats on the same
 * stream where stats is given (the waves add their counts to it); with
 * from->n == 0 that clear is all there is. It makes no host round trip and
 * needs no workspace. Like vp_tx_build it ends the NF's resident kernel, and
 * after a multi-GPU attach it is local to the rank.
 * VP_EINVAL: a NULL ctx, from, home or way; from->n > 0 with a NULL
 * from->frames or from->out_dev; a NULL home->frames or home->out_dev with
 * home->n > 0 and from->n > 0; either slot below 64 or not a multiple of 16;
 * either frames not 16-byte aligned; in_dev NULL with in_port > 0xFFFF, on
 * either batch; a port[d] with d < n_devices, or an on_* value, that is
 * neither <= 0xFFFF nor one of the two sentinels; a context with more than
 * VP_MAX_DEVICES devices; the overlap above. */
int vp_tx_return(vp_ctx *ctx, const vp_dev_batch *from, const vp_dev_batch *home,
                 const vp_tx_way_home *way, void *stream);

/* -------------------------------------------------------------- the chain --
 * The calls above joined into one object: several contexts on one GPU with
 * cables between them (firewall -> NAT, bridge -> policer, ...), what the
 * reference runs as one box per NF, standing where one NF stands. The chain
 * owns the lists, the batches between the stages and the origins; the stages'
 * contexts, and their table state, stay the caller's. */

#define VP_CHAIN_MAX_STAGES 16
#define VP_CABLE_SLOTS  0  /* a link hands a list over with vp_tx_rebatch */
#define VP_CABLE_STREAM 1  /* ... as a packed stream: vp_tx_pack, then vp_rx_unpack */

typedef struct vp_chain vp_chain;

/* What stage `from` sends to its port out_port arrives at stage `to` on port
 * in_port. */
typedef struct vp_chain_link {
  uint32_t from, out_port, to, in_port;
} vp_chain_link;

/* What stage `stage` sends to its unlinked port `port` leaves the composite
 * box on ext_port (vp_chain_process_device). */
typedef struct vp_chain_exit {
  uint32_t stage, port, ext_port;
} vp_chain_exit;

typedef struct vp_chain_config {
  vp_ctx *const *stages;      /* n_stages contexts on one GPU, in chain order */
  uint32_t n_stages;
  const vp_chain_link *links; /* n_links entries; may be NULL iff n_links == 0 */
  uint32_t n_links;
  const vp_chain_exit *exits; /* n_exits entries; may be NULL iff n_exits == 0 */
  uint32_t n_exits;
  uint32_t cable;             /* VP_CABLE_SLOTS or VP_CABLE_STREAM */
} vp_chain_config;

/* One stage's batch as the last run left it; every pointer a device pointer. */
typedef struct vp_chain_view {
  uint32_t n, slot;        /* packets the stage received (0: nothing reached it) */
  uint8_t *frames;         /* n * slot bytes, as the stage left them */
  const uint16_t *len;
  const uint16_t *out_dev; /* the stage's own out ports */
  const uint16_t *in_dev;  /* per-packet in port (stage 0 with a port array, a stage
                              with several inbound links), or NULL: every packet
                              arrived on in_port */
  uint32_t in_port;
  const int64_t *now;      /* per-packet time; NULL at stage 0 with affine time */
  const uint32_t *origin;  /* each packet's index in the caller's batch; NULL at
                              stage 0: origin(k) = k */
} vp_chain_view;

/* Make a chain of cfg->n_stages contexts. Nothing of cfg is kept: the arrays
 * may be freed when the call returns; the contexts must outlive the chain.
 * Every stage but 0 has one to VP_TX_MERGE_MAX inbound links. A stage with
 * several sees their packets merged by origin (each packet's index in the
 * chain's input), as cables into one box would deliver them; copies of one
 * input packet (floods, or a packet that arrives through two branches) arrive
 * in the order of the stage's inbound links in `links`. That is the order of
 * boxes that push each packet through all their cables before the next
 * whenever `links` is written in depth-first order, and only then. Packets a
 * stage sends to a port without a link have left the chain: they stay in that
 * stage's view with their out port.
 * With VP_CABLE_STREAM every stage that has one inbound link is fed through a
 * packed stream: the stream carries min(len, slot) bytes of a frame, so the
 * target sees zeros where the source slot held bytes past the frame's length.
 * Stages with several inbound links keep vp_tx_merge.
 * VP_EINVAL, in this order, the first five before any context is read: a NULL
 * cfg or out; n_stages == 0 or above VP_CHAIN_MAX_STAGES; a NULL stages, a
 * NULL links with n_links > 0 or a NULL exits with n_exits > 0; a NULL stage;
 * an unknown cable; stages on different GPUs, or one with more than
 * VP_MAX_DEVICES devices; a link that names a stage outside the chain, goes
 * backward (to <= from), leaves from a port its stage does not have, or
 * arrives on a port above 0xFFFF; a stage with more than VP_TX_MERGE_MAX
 * inbound links; a stage after 0 without one; an out port that feeds a stage
 * with several inbound links and is named by another link as well; an exit
 * that names a stage or a port the chain does not have, a linked port, or an
 * ext_port above 0xFFFF. From the GPU check on, vp_last_error() names the
 * offending stage, link or exit. VP_ENOTSUP: a stage attached to a multi-GPU
 * communicator (vp_attach_*). VP_ENOMEM: no host or device memory for the
 * chain's own bookkeeping. */
int vp_chain_create(const vp_chain_config *cfg, vp_chain **out);

/* Frees what the chain owns. The stages' contexts stay the caller's. A run
 * that succeeded ended drained, so the stream it was given plays no part
 * here and may be gone; only after a run that failed part-way, which may have
 * left work queued, is that run's stream waited for first: it must then still
 * exist at the next run and here. NULL: nothing. */
void vp_chain_destroy(vp_chain *ch);

/* One batch through the chain. Reads batch->frames, slot, n, len, in_dev (or
 * in_port) and the time; batch->out_dev is neither read nor written. Stage 0
 * processes the caller's batch in place (vp_process_device); its out ports go
 * into a buffer of the chain's own, cleared first. Then, for every stage in
 * order that has a link and received packets: vp_tx_build over its out ports;
 * one read of offset[] to the host, the one host synchronisation per stage (a
 * list that outgrew idx -- floods -- is built again with room); per linked
 * port vp_tx_rebatch into buffers the chain owns (VP_CABLE_STREAM: one
 * vp_tx_pack of all the lists with pos, then vp_rx_unpack per linked port);
 * vp_process_device of the target with every packet on the link's in_port and
 * the gathered per-packet times. A stage with several inbound links gets its
 * input when it is reached, after every earlier stage ran: one vp_tx_merge
 * over its links' lists in `links` order, each source keyed by its stage's
 * origins (stage 0: NULL), then vp_process_device with the merged per-packet
 * ports and times. Origins are 32 bits: behind stage 0 a link's src[], at a
 * merged stage the merge's key[], elsewhere origin_s[src[k]] composed by one
 * kernel (0xFFFFFFFF for a src outside the source batch, which vp_tx_return
 * counts as bad_home and never writes through).
 * Everything is enqueued on `stream` (NULL: stage 0's own), and the call
 * returns after the results are in device memory. State persists across calls
 * in the stages' contexts. The chain keeps its buffers from call to call and
 * replaces them by larger ones on demand; it waits for the stream before it
 * frees one, and a run that follows one that failed part-way first waits for
 * the failed run's stream. n == 0: returns 0, nothing is written, every view is empty.
 * VP_EINVAL: a NULL ch or batch; with n > 0 a NULL frames or len, a slot below
 * 64 or not a multiple of 16, frames not 16-byte aligned; in_dev NULL and
 * in_port > 0xFFFF. A failing stage's code is returned as it is; the views
 * are then undefined until the next run that succeeds. */
int vp_chain_run(vp_chain *ch, const vp_dev_batch *batch, void *stream);

/* Stage `stage`'s batch as the last vp_chain_run or vp_chain_process_device
 * left it. Stage 0's frames, len, in_dev and now are the caller's; everything
 * else is the chain's own memory: valid until the next run or until
 * vp_chain_destroy. n == 0 (and every pointer NULL) for a stage nothing
 * reached, and before the first run. VP_EINVAL: a NULL ch or out; a stage the
 * chain does not have. */
int vp_chain_view_get(vp_chain *ch, uint32_t stage, vp_chain_view *out);

/* The chain where one NF stands: vp_process_device's batch, and afterwards the
 * caller's batch as one box holding the whole chain would leave it -- frames
 * rewritten in place, out_dev[i] a port of the composite box (the exits) or,
 * for a drop, packet i's own in port. Does vp_chain_run, then one vp_tx_return
 * per stage that received packets, in ascending order, into the caller's
 * batch: home = the stage's origins (stage 0: the in-place form), the actions
 *   a linked port            VP_RET_SKIP (the packet travelled on; the stage
 *                            it reached has the later word)
 *   an exit                  its ext_port
 *   any other port, a drop,
 *   a port the stage lacks   VP_RET_DROP
 *   VP_FLOOD_FRAME           VP_FLOOD_FRAME where every port of the stage is
 *                            an exit; otherwise VP_RET_SKIP at stage 0 (a
 *                            stage that a copy reached decides) and
 *                            VP_RET_DROP later
 * A later stage's return overrides an earlier one's for the same packet; of
 * the copies one stage holds of a packet the first counts. Writes
 * batch->out_dev, which the caller owns. The known limit: a packet that stage
 * 0 flooded and no copy of which reached a later stage is not written: its
 * out_dev keeps the caller's value. *stats (host memory, or NULL) receives the
 * stages' vp_tx_return_stats summed: one device-to-host copy of all stages'
 * 40 bytes at the end, no kernel. Returns after the results are in device
 * memory. n == 0: returns 0, nothing is written, *stats zero.
 * VP_EINVAL: what vp_chain_run rejects; a NULL out_dev with n > 0. */
int vp_chain_process_device(vp_chain *ch, const vp_dev_batch *batch,
                            vp_tx_return_stats *stats, void *stream);

/* Host memory the GPU may read and write frames in directly: a DPDK mbuf
 * pool's memory (the hugepages rte_pktmbuf_pool_create, nf.c:235-242, lays
 * the mbufs out in), registered once after the pool is created. Page-locked
 * and mapped for the context's GPU (hipHostRegister; memory that is page-
 * locked already, e.g. hipHostMalloc'd, is only mapped). At most 16 ranges,
 * not overlapping. vp_unregister_host takes the base passed to
 * vp_register_host; vp_destroy unregisters what is left. */
int vp_register_host(vp_ctx *ctx, void *base, size_t bytes);
int vp_unregister_host(vp_ctx *ctx, void *base);

/* Host-resident batch shaped like DPDK rx bursts (nf.c:186-214): frames[i]
 * is the data of mbuf i (rte_pktmbuf_mtod, nf.c:154), len[i] its pkt_len,
 * in_dev[i] its port; every frame is rewritten in place and out_dev[i] gets
 * nf_process's return value, as calling nf_process on every packet in order
 * would (nf.c:150-176). Time: now[i], or now0 + i * now_step when now is
 * NULL (nf.c's per-packet loop stamps a polling sweep over the devices with
 * one current_time(), nf.c:56: now_step 0; its batched loop stamps every
 * packet, nf.c:197: a time array, or now_step > 0).
 * Frames inside memory registered with vp_register_host are read and written
 * by the GPU in place, in pipelined chunks: per frame the
 * first 64 bytes and, for vignat, the bytes its L4 checksum covers cross
 * PCIe inbound, and the bytes a rewrite can change (the first min(len, 64)
 * of a frame that is not dropped) outbound. Other frames are gathered and
 * scattered on the host through pinned staging. Bytes past a frame's length
 * read as 0 and are never written. Per-packet arrays in page-locked memory
 * are DMA'd in place. Frames and out_dev hold the results when the call
 * returns.
 * Every NF on one GPU serves a call of up to
 * VIGPATH_SERVE_BURST packets (default 256 for vignat and vigfw, 384 for
 * vigbridge, 512 for vigpol, 128 for viglb, each from its own measured crossover; 0:
 * none) from vp_process_one's resident kernel instead, as
 * burst requests of up to 64 frames, one lane of a wave per packet, while no
 * expiry is due anywhere in the call (viglb: on its flows or its backends), every frame is at most 2048 bytes
 * and the times do not go back: no launch, no copy call, and the kernel stays
 * for the next call (nf.c's VIGOR_BATCH_SIZE loop, nf.c:178-215). Every NF
 * hands over only the first call at which an expiry
 * is due: from the next one on its kernel expires the entries itself before
 * each request (vp_serve_expiry_stats_get; vigpol, as the reference, only at
 * packets whose IPv4 header parses; viglb its flows and then its backends,
 * each on its own lifetime, at every packet whatever its frame), and a burst
 * inside which an expiry falls
 * due is served up to that packet and the rest posted as the next request.
 * VIGPATH_SERVE_EXPIRE=0 turns that off (every due expiry takes the path
 * above); VIGPATH_SERVE_JOURNAL sets the journal's size in records per table
 * index (default 8, at least 2). A burst
 * holding a frame with IPv4 options is handed back and takes the path above
 * (vp_serve_stats_get counts both); vigbridge, which reads only the MACs,
 * and vigpol, which never parses L4, hand none back. vigpol's packets to one
 * destination address pass through its token bucket in packet order. viglb's
 * heartbeats from unknown addresses, new flows and flows whose backend died
 * settle in packet order inside the burst, and a backend that expires in the
 * kernel is dead for the packets behind it: its flows are re-pointed. The one
 * thing viglb's kernel leaves to the path above is the erasure of a flow whose
 * backend died while no backend is alive: that request is handed back too
 * (the expiries due at it are done by then, and counted). */
typedef struct vp_mbuf_batch {
  uint32_t n;
  uint8_t *const *frames;
  const uint16_t *len;
  const uint16_t *in_dev;
  const int64_t *now;
  int64_t now0;
  int64_t now_step;
  uint16_t *out_dev;
} vp_mbuf_batch;
int vp_process_mbufs(vp_ctx *ctx, const vp_mbuf_batch *batch);

/* The same with a per-packet time array (the batch form of nf_process the
 * nf.h shims call); a small burst is served by the NF's resident
 * kernel, which it does not end, exactly as through vp_process_mbufs. */
int vp_process_batch(vp_ctx *ctx, uint32_t n, const uint16_t *in_dev,
                     uint8_t *const *frames, const uint16_t *len,
                     const int64_t *now, uint16_t *out_dev);

/* One packet: nf_process (nf.h:14-15, called once per packet by nf.c:150-176;
 * the nf.h shims' nf_process calls this). The frame is rewritten in place and
 * the output port stored in *out_dev; same results as vp_process_batch with
 * n = 1. Every NF on one GPU serves it from a persistent
 * kernel that polls a host-coherent mailbox (no launch per packet) while no
 * expiry is due at `now`; otherwise, and for the one packet viglb's kernel
 * hands back (the erasure of a flow with no backend alive), it is
 * vp_process_batch with n = 1. Every NF takes that
 * path only for the first packet at which an expiry is due: afterwards the kernel expires the
 * entries itself, before the packet, and stays (vp_serve_expiry_stats_get;
 * VIGPATH_SERVE_EXPIRE=0: off).
 * The kernel leaves after VIGPATH_SERVE_IDLE_MS (default 20) without a
 * packet, at any other call on the context -- except a vp_process_batch /
 * vp_process_mbufs call small enough to be served by it as a burst -- and at
 * exit; VIGPATH_SERVE=0 turns it off. */
int vp_process_one(vp_ctx *ctx, uint16_t in_dev, uint8_t *frame, uint16_t len,
                   int64_t now, uint16_t *out_dev);

/* Host-resident contiguous batch (frames `slot` bytes apart). */
int vp_process_host(vp_ctx *ctx, uint32_t n, const uint16_t *in_dev,
                    uint8_t *frames, uint32_t slot, const uint16_t *len,
                    const int64_t *now, uint16_t *out_dev);

/* The same with every field of vp_dev_batch, as host pointers: time is
 * now[i], or now0 + i * now_step when now is NULL (nf.c stamps every packet
 * of one polling sweep with one current_time(), nf.c:56: now_step 0). Arrays
 * in page-locked memory (hipHostMalloc / hipHostRegister, e.g. a DPDK
 * hugepage pool) are DMA'd in place, others staged through pinned memory.
 * Frames and out_dev hold the results when the call returns. */
typedef vp_dev_batch vp_host_batch;
int vp_process_host_batch(vp_ctx *ctx, const vp_host_batch *batch);

/* -------------------------------------------------------- multi-GPU -- *
 * One vignat instance over N GPUs (one process and one context per GPU),
 * identical to a single nf.c processing the concatenation of the ranks'
 * slices (rank 0's packets first) of every global batch. The allocator
 * (dchain free list) is replicated; new flows are all-gathered and allocated
 * identically everywhere; timestamps are per-rank partial maxima merged
 * (all-reduce MAX) only where an expiry may happen. The flow dictionary is
 * either replicated (VP_SHARD_REPLICATED, the default: every rank probes
 * locally) or sharded by flow hash (VP_SHARD_OWNER: rank q's buckets hold
 * the keys with owner(FlowId_hash) = q; a LAN packet whose key another rank
 * owns is looked up there through an all-to-all of 16-byte keys and 4-byte
 * replies). After an attach, vp_process_device is a collective: every rank
 * calls it once per global batch with its own slice (n may be 0), in the
 * same order. See DESIGN.md §6. */

/* RCCL over xGMI: rank 0 creates the id, the host distributes it. */
#define VP_COMM_ID_BYTES 128
int vp_comm_unique_id(uint8_t id[VP_COMM_ID_BYTES]);
int vp_attach_rccl(vp_ctx *ctx, const uint8_t id[VP_COMM_ID_BYTES], int nranks,
                   int rank);

/* Host-memory collectives supplied by the caller (e.g. torch.distributed /
 * gloo, or several ranks sharing one GPU). Return 0 on success. */
typedef struct vp_comm_ops {
  void *user;
  /* every rank contributes `bytes`; recv receives nranks * bytes, rank order */
  int (*allgather)(void *user, const void *send, void *recv, size_t bytes);
  /* element-wise maximum over ranks of `count` u64 values (all < 2^63) */
  int (*allreduce_max_u64)(void *user, uint64_t *buf, size_t count);
  /* personalised exchange (VP_SHARD_OWNER only; may be NULL otherwise):
   * this rank sends send_bytes[q] bytes to rank q, the chunks consecutive in
   * `send` in rank order, and receives recv_bytes[q] bytes from rank q into
   * `recv`, laid out the same way */
  int (*alltoallv)(void *user, const void *send, const size_t *send_bytes,
                   void *recv, const size_t *recv_bytes);
} vp_comm_ops;
int vp_attach_comm(vp_ctx *ctx, const vp_comm_ops *ops, int nranks, int rank);

/* Dictionary placement over the attached ranks (collective; call on every
 * rank with the same mode after the attach and before the first batch). */
#define VP_SHARD_REPLICATED 0
#define VP_SHARD_OWNER 1
int vp_shard_mode(vp_ctx *ctx, int mode);

/* Collective: merge the ranks' timestamps so vp_nat_dump is exact on every
 * rank (the dictionary and allocator are identical everywhere already). */
int vp_sync_state(vp_ctx *ctx);

/* Abort this rank's collectives (not collective itself; any thread, also
 * while another thread is inside a vp_* call on the context): the RCCL
 * communicator is aborted (ncclCommAbort), so a rank waiting for a peer that
 * never comes returns instead of spinning; every later vp_* call on the
 * context that needs the ranks fails with VP_EIO. Host transports
 * (vp_attach_comm) have nothing to abort: returns 0. For watchdogs
 * (bench.py --gpus N); the context may only be destroyed afterwards. */
int vp_comm_abort(vp_ctx *ctx);

/* ------------------------------------------------------- observability -- */

/* vignat state by flow index i < max_flows: alloc[i] (dchain allocated?),
 * ts[i] (timestamp, only meaningful when allocated), key[16*i] (the FlowId
 * bytes, vignat/flow.h:3-10 layout, padding zero). */
int vp_nat_dump(vp_ctx *ctx, uint8_t *alloc, int64_t *ts, uint8_t *keys);

/* vigbridge dynamic table by index i < dyn_capacity: alloc[i], ts[i],
 * macs[6*i] (dyn_keys), port[i] (dyn_vals DynamicValue.device). */
int vp_bridge_dump(vp_ctx *ctx, uint8_t *alloc, int64_t *ts, uint8_t *macs,
                   uint16_t *port);

/* viglb state. Flows i < flow_capacity: f_alloc[i], f_ts[i], f_keys[16*i]
 * (LoadBalancedFlow bytes, lb_flow.h:6-12, padding zero), f_backend[i]
 * (flow_id_to_backend_id). Backends b < backend_capacity: b_alloc[b],
 * b_ts[b], and backends[b] (lb_backend.h:7-11) as b_ip[b], b_mac[6*b],
 * b_nic[b]. */
int vp_lb_dump(vp_ctx *ctx, uint8_t *f_alloc, int64_t *f_ts, uint8_t *f_keys,
               uint32_t *f_backend, uint8_t *b_alloc, int64_t *b_ts,
               uint32_t *b_ip, uint8_t *b_mac, uint16_t *b_nic);

/* vigfw state by flow index i < max_flows: alloc[i], ts[i], key[16*i] (the
 * FlowId bytes, vigfw/flow.h:3-9 layout, padding zero), int_dev[i] (the
 * int_devices vector, fw_flowmanager.c:61-64; 0 where not allocated). */
int vp_fw_dump(vp_ctx *ctx, uint8_t *alloc, int64_t *ts, uint8_t *keys,
               uint32_t *int_dev);

/* vigpol state by index i < dyn_capacity: alloc[i], ts[i], keys[i] (dyn_keys:
 * the destination address, raw network-order u32), bucket_size[i] and
 * bucket_time[i] (dyn_vals, vigpol/dynamic_value.h:7-10; meaningful where
 * allocated). */
int vp_pol_dump(vp_ctx *ctx, uint8_t *alloc, int64_t *ts, uint32_t *keys,
                uint64_t *bucket_size, int64_t *bucket_time);

/* ------------------------------------------------------- state images -- */

/* Save and restore a context's table state: failover, warm restart, moving
 * an NF to another GPU, warming a table without replaying its traffic.
 *
 * A dump (above) is an observation, not a state: it leaves out the order
 * among equal timestamps in the dchain's allocated list (which of two flows
 * with one stamp expires first) and the order of the free list (the index,
 * and for vignat the external port, of every later new flow). The image holds
 * both, and nothing that depends on how the device keeps the tables.
 *
 * The image, version 1. Little-endian; every array starts at a multiple of
 * 16 bytes from the image's first byte and is followed by zero bytes up to
 * the next multiple of 16; every reserved byte is zero. Its size follows the
 * live entries and the freed indices, not the capacity.
 *
 *   header, 32 bytes
 *     u32 magic        VP_STATE_MAGIC (the bytes "VPST")
 *     u32 version      VP_STATE_VERSION
 *     u32 kind         1 vignat, 2 vigbridge, 3 viglb, 4 vigfw, 5 vigpol
 *     u32 n_tables     1; viglb 2 (its flows, then its backends)
 *     u64 total_bytes  of the whole image
 *     i64 last_now     the time of the last packet processed (-1: none yet)
 *   then per table
 *     table header, 32 bytes
 *       u32 capacity
 *       u32 n_live
 *       u32 fresh_next   the never-used tail is fresh_next .. capacity - 1
 *       u32 value_size   bytes per entry in value[] (below)
 *       u32 n_freed
 *       u32 reserved[3]  zero
 *     u32 lru[n_live]    the allocated indices, oldest first: the dchain's
 *                        allocated list, the order in which they would expire
 *     u32 freed[n_freed] the free indices that precede the tail, in the order
 *                        the allocator will hand them out
 *     i64 ts[n_live]     entry j's timestamp; it never decreases along j
 *     u8  key[n_live][16]          entry j's key, zero-padded to 16 bytes
 *     u8  value[n_live][value_size] entry j's value
 *   Entry j of ts, key and value belongs to index lru[j].
 *
 *   table              key (as the dump gives it)       value (value_size)
 *   vignat flows       FlowId, 16 bytes                 none (0)
 *   vigbridge MACs     the address, 6 bytes             u32 port, <= 0xFFFF (4)
 *   vigfw flows        FlowId, 13 bytes                 u32 int_dev, <= 0xFFFF (4)
 *   viglb flows        LoadBalancedFlow, 13 bytes       u32 backend id, below
 *                                                       backend_capacity (4)
 *   viglb backends     the address, u32 as b_ip         mac[6], u16 nic (8)
 *   vigpol             the address, u32 as keys[]       u64 bucket_size,
 *                                                       i64 bucket_time (16)
 *
 * The image is canonical: two contexts in the same libVig state give the
 * same bytes, whatever their bucket layouts, batch splits or entry points
 * were. After the indices of freed[], the allocator hands out the tail in
 * ascending order; the tail is the longest run at the end of the hand-out
 * order that is ascending and consecutive up to capacity - 1, so freed[]
 * never ends with fresh_next - 1 (that index belongs to the tail).
 * n_live + n_freed + (capacity - fresh_next) == capacity, and lru, freed and
 * the tail name every index once.
 *
 * All three calls stop the NF's resident kernel and wait for the context's
 * stream first, and return VP_ENOTSUP on a context attached to a multi-GPU
 * communicator. buf is host memory.
 *
 * vp_state_size: *bytes = an upper bound of what a save would write now.
 * vp_state_save: writes the image and its size to *bytes. With cap too small
 * it writes *bytes only and returns VP_EINVAL.
 * vp_state_load: replaces the whole table state of ctx, the time of the last
 * packet and the packet sequence; afterwards every entry point behaves as on
 * the context that was saved. Configuration is not state: the NF kind and
 * the table capacities must match, while addresses, ports, expiry times,
 * static bridge rules and the CHT stay ctx's own. An image that is not
 * exactly as described above -- sizes, counts, an index out of range or
 * named twice, a time below 0, above last_now or decreasing along lru, a
 * value out of range, a key that occurs twice, a non-zero pad byte -- is
 * VP_EINVAL, vp_last_error() names the first offending field, and ctx still
 * holds the state it had before the call. */
#define VP_STATE_MAGIC 0x54535056u
#define VP_STATE_VERSION 1u
int vp_state_size(vp_ctx *ctx, uint64_t *bytes);
int vp_state_save(vp_ctx *ctx, void *buf, uint64_t cap, uint64_t *bytes);
int vp_state_load(vp_ctx *ctx, const void *buf, uint64_t bytes);

/* ------------------------------------------------ incremental state images -- */

/* What changed in a context's table state since a named earlier moment, and
 * its application to a context that holds that earlier state: a standby that
 * follows a live box without a full image every time.
 *
 * A mark names a moment of a context: seq is its packet sequence then, epoch
 * the number of vp_state_load calls it has had (a load restarts the
 * sequence, so marks of an earlier epoch name nothing any more). A full save
 * taken at a mark, with no packet in between, is the image of that mark.
 *
 * The delta from a mark B to now, version 1. Little-endian, arrays and pads
 * as in the image above.
 *
 *   header, 64 bytes
 *     u32 magic        VP_STATE_DELTA_MAGIC (the bytes "VPSD")
 *     u32 version      VP_STATE_DELTA_VERSION
 *     u32 kind, u32 n_tables            as in the image
 *     u64 total_bytes  of the whole delta
 *     i64 last_now     the time of the last packet processed (-1: none yet)
 *     u64 base_seq, u64 base_epoch      the mark B
 *     u64 mark_seq, u64 mark_epoch      the mark of now
 *                      (both as the saving context counts them)
 *   then per table
 *     table header, 32 bytes
 *       u32 capacity, n_live, fresh_next, value_size, n_freed   of the state
 *                        now, exactly as a full image taken now holds them
 *                        (after the same tail normalisation)
 *       u32 n_new
 *       u32 reserved[2]  zero
 *     u32 idx[n_new]     the indices that are live now and whose last touch
 *                        (allocation or rejuvenation) came after B, in LRU
 *                        order, oldest first
 *     u32 freed[n_freed] the whole free list before the tail, as in the image
 *     i64 ts[n_new]
 *     u8  key[n_new][16]
 *     u8  value[n_new][value_size]
 *   Entry j of ts, key and value belongs to index idx[j]; idx, ts, key and
 *   value together are called new[]. Nothing is said of an entry that was
 *   not touched since B.
 *
 * Applying it to a context that holds the state at B gives the state now:
 *   - every index outside freed[] and below fresh_next is live afterwards; an
 *     index that was live and is named free (in freed[] or in the tail)
 *     leaves, and its key is erased. Removals need no list of their own, and
 *     need not be the oldest entries (viglb erases a flow out of LRU order).
 *   - an index of new[] that holds the same key is updated in place (stamp,
 *     value); if it holds another key or is free, the old key (if any) is
 *     erased and the new one put in.
 *   - the entries that are neither free nor in new[] (the kept ones) keep
 *     their order, and new[] follows them in its own order.
 *   - the free list becomes freed[] and the tail from fresh_next.
 * freed[] travels whole, 4 bytes per freed index: a delta taken after a mass
 * expiry is not small.
 *
 * All five calls stop the NF's resident kernel and wait for the context's
 * stream first, and return VP_ENOTSUP on a context attached to a multi-GPU
 * communicator. buf is host memory.
 *
 * vp_state_mark: *mark names the present state.
 * vp_state_delta_size: *bytes = an upper bound of what a delta from base
 * would take now.
 * vp_state_delta_save: writes the delta from base to now, its size to *bytes
 * and the mark of now to *mark. base must carry this context's current epoch
 * and a seq not above the current one, else VP_EINVAL; any earlier mark of
 * the epoch will do, so deltas are cumulative and several standbys may
 * follow at their own pace. With cap too small it writes *bytes only and
 * returns VP_EINVAL. It changes nothing in ctx.
 * vp_state_follow: declares that ctx holds the state the primary named
 * *mark (call it after vp_state_load of the image taken at that mark).
 * vp_state_delta_apply: VP_EINVAL unless ctx is following, nothing has
 * changed it since (no packet, no load), and the delta's base is the
 * followed mark. On success the followed mark becomes the delta's mark. A
 * delta that is not exactly as described -- sizes and offsets against the
 * byte count, pad and reserved bytes, kind, table count, capacities, value
 * sizes; n_live + n_freed + (capacity - fresh_next) != capacity; freed[]
 * ending with fresh_next - 1; an index out of range, named twice in idx[] or
 * freed[], in both, or inside the tail; a stamp below 0, above last_now or
 * decreasing along new[]; new[0]'s stamp below the largest stamp of a kept
 * entry; last_now below ctx's; a value out of range; a non-zero key pad
 * byte; a key of new[] that a kept entry at another index holds, or that
 * occurs twice; the kept entries plus n_new differing from n_live -- is
 * VP_EINVAL as well. On every refusal vp_last_error() names the first
 * offending field, and ctx holds the state and the followed mark it had.
 * Processing packets on a following context promotes it: the following
 * ends. */
typedef struct vp_state_mark_t {
  uint64_t seq;
  uint64_t epoch;
} vp_state_mark_t;
#define VP_STATE_DELTA_MAGIC 0x44535056u
#define VP_STATE_DELTA_VERSION 1u
int vp_state_mark(vp_ctx *ctx, vp_state_mark_t *mark);
int vp_state_delta_size(vp_ctx *ctx, const vp_state_mark_t *base, uint64_t *bytes);
int vp_state_delta_save(vp_ctx *ctx, const vp_state_mark_t *base, void *buf, uint64_t cap,
                        uint64_t *bytes, vp_state_mark_t *mark);
int vp_state_follow(vp_ctx *ctx, const vp_state_mark_t *mark);
int vp_state_delta_apply(vp_ctx *ctx, const void *buf, uint64_t bytes);

/* ------------------------------------------------------ table lookups -- */

/* Ask a context's table about a batch of keys or of indices without copying
 * the table: is this flow tracked, when was it last seen, what is bound to
 * it. Read-only, answered on the device, n queries in one call.
 *
 * `table` is as in vp_table_stats_get: 0 the NF's flow table, 1 viglb's
 * backends. Keys, stamps and values are exactly those of the state image,
 * version 1 (above): the 16-byte zero-padded key, and per table the same
 * value_size and value encoding. A lookup of an image's key[j] returns
 * lru[j], ts[j] and value[j].
 *
 * vp_table_lookup, by key: query q hits iff a live entry holds exactly the
 * 16 bytes keys[q]. A key with a non-zero pad byte is therefore a miss, not
 * an error. A key may be given twice; both queries get the same answer.
 * vp_table_entries, by index: an index at or above the capacity, or one that
 * is not allocated, is a miss. For vignat the index is the flow's external
 * port minus start_port, so this is the reverse NAT lookup: which internal
 * 5-tuple holds external port P is entry P - start_port.
 * vp_table_value_size: *bytes = the table's value_size (0 for vignat); the
 * resident kernel stays.
 *
 * Every array of vp_lookup_out is device memory of n entries, written one
 * entry per query, and any of them may be NULL (not wanted). keys is [n][16]
 * and idx [n], device memory.
 *
 * The two queries change nothing in the context: no entry is rejuvenated,
 * the packet sequence does not advance, no mark is set and a vp_state_follow
 * stays in force, the vp_serve_* statistics and the touch journal's validity
 * are as before. Like the state calls they stop the NF's resident kernel and
 * wait for the context's stream first, so the timestamp fold a
 * vp_process_device call with affine time may leave running is visible.
 * They then run on `stream` (NULL: the context's own) and return once the
 * results are in device memory.
 *
 * VP_ENOTSUP on a context attached to a multi-GPU communicator. VP_EINVAL,
 * with the field named by vp_last_error(): a NULL ctx or out; a table the NF
 * does not have; n > 0 with NULL keys / idx; a pointer that is not 16-byte
 * aligned (keys, key), 8-byte aligned (ts), 4-byte aligned (index, idx) or,
 * for value, aligned to value_size (4, 8 or 16). A refused call writes
 * nothing. n == 0 is VP_OK and launches nothing. */
#define VP_LOOKUP_MISS 0xFFFFFFFFu

typedef struct vp_lookup_out {        /* all device pointers; any may be NULL */
  uint32_t *index;   /* [n]  by key: the entry's index, or VP_LOOKUP_MISS
                             by index: idx[q] if live, else VP_LOOKUP_MISS   */
  int64_t  *ts;      /* [n]  the entry's stamp; 0 for a miss                 */
  uint8_t  *key;     /* [n][16] the entry's key, zero-padded as in the image;
                             zero for a miss                                 */
  uint8_t  *value;   /* [n][value_size] as in the image; zero for a miss;
                             never touched when value_size is 0 (vignat)     */
} vp_lookup_out;

int vp_table_lookup (vp_ctx *ctx, int table, uint32_t n, const uint8_t  *keys /* [n][16] device */,
                     const vp_lookup_out *out, void *stream);
int vp_table_entries(vp_ctx *ctx, int table, uint32_t n, const uint32_t *idx  /* [n] device */,
                     const vp_lookup_out *out, void *stream);
int vp_table_value_size(vp_ctx *ctx, int table, uint32_t *bytes);

/* -------------------------------------------------------- table erase -- */

/* Take entries out of a context's table from the control plane: kill a
 * connection, evict a MAC that moved, take a backend out, reset a
 * subscriber's token bucket. On the device, n queries in one call; the work
 * follows n, not the capacity.
 *
 * `table`, keys, indices, value_size and the vp_lookup_out arrays are exactly
 * those of vp_table_lookup / vp_table_entries (above). vp_table_erase names
 * entries by key, vp_table_free by index. The call behaves like this loop:
 *
 *   for q = 0 .. n-1 in order: if the query names a live entry, map_erase its
 *   key and dchain_free_index its index.
 *
 * dchain_free_index pushes the index on the front of the free list, as expiry
 * does: the allocator hands out the index of the last erasing query first.
 * A query that names nothing live erases nothing and is not an error: a miss,
 * a key with a non-zero pad bit, an index at or above the capacity or not
 * allocated, and a key or index that an earlier query of the same call
 * already erased.
 *
 * For an erasing query out->index[q] is the freed index and ts / key / value
 * are the entry as it was before the erase. For every other query the outputs
 * are VP_LOOKUP_MISS and zeros, as for a lookup miss. *n_erased (host memory,
 * may be NULL) is the number of erasing queries. out may be NULL, and so may
 * any of its arrays.
 *
 * The state image after the call is the image before it with the erased
 * entries removed from lru[], the others keeping their order, and the erased
 * indices put before the old freed[] in reverse query order; the tail
 * normalisation of the image then applies. Nothing else changes: no stamp and
 * no other entry's value moves, last_now stays. viglb flows that point at an
 * erased backend stay as they are, and the data path finds the backend dead
 * as it does after a backend expiry.
 *
 * A call that erased at least one entry ends a vp_state_follow, as a packet
 * does, and advances the context's sequence by one, so a mark taken before
 * names an earlier moment: a delta saved afterwards from such a mark carries
 * the erasures in its freed[] and applies on a standby that holds that mark.
 * A call that erased nothing changes neither mark nor following.
 *
 * Like the lookups the calls stop the NF's resident kernel and wait for the
 * context's stream first, then run on `stream` (NULL: the context's own) and
 * return when done. VP_ENOTSUP on a context attached to a multi-GPU
 * communicator. VP_EINVAL, with the lookups' texts under these calls' names
 * in vp_last_error(): a NULL ctx; a table the NF does not have; n > 0 with
 * NULL keys / idx; a misaligned pointer. A refused call changes and writes
 * nothing. n == 0 is VP_OK, launches nothing and writes *n_erased = 0. */
int vp_table_erase(vp_ctx *ctx, int table, uint32_t n, const uint8_t  *keys /* [n][16] device */,
                   const vp_lookup_out *out /* may be NULL */, uint32_t *n_erased /* host, may be NULL */,
                   void *stream);
int vp_table_free (vp_ctx *ctx, int table, uint32_t n, const uint32_t *idx  /* [n] device */,
                   const vp_lookup_out *out, uint32_t *n_erased, void *stream);

/* Number of live flows / learned MACs / flows+backends. */
int64_t vp_live_count(vp_ctx *ctx);

/* Bookkeeping of one device table: table 0 = the NF's flow table (vignat /
 * vigfw flows, vigbridge dynamic MACs, viglb flows, vigpol destinations),
 * table 1 = viglb's backend table. */
typedef struct vp_table_stats {
  uint64_t live;        /* allocated indices (dchain) */
  uint64_t shard_live;  /* entries in this rank's buckets (= live unless
                         * VP_SHARD_OWNER) */
  uint64_t tombstones;  /* erased entries not yet rebuilt away */
  uint64_t buckets;     /* 64-byte buckets (3 entries each) */
  uint64_t rebuilds;    /* bucket-array rebuilds since creation */
  uint32_t layout;      /* home-bucket mode (vp_table.h kMix*) */
  uint32_t pad;
} vp_table_stats;
int vp_table_stats_get(vp_ctx *ctx, int table, vp_table_stats *out);

/* The NF's resident kernel (vp_process_one, and vp_process_batch /
 * vp_process_mbufs calls small enough to be served as burst requests) since
 * the context was created. A read of host-side counters: the kernel stays. */
typedef struct vp_serve_stats {
  uint64_t packets_one;   /* packets served by vp_process_one's kernel */
  uint64_t bursts;        /* burst requests served */
  uint64_t burst_packets; /* packets in them */
  uint64_t declined;      /* requests the kernel handed back (a burst with a byte-path
                             frame; viglb: a burst or a packet that erases a flow) */
  uint64_t launches;      /* launches of the resident kernel */
} vp_serve_stats;
int vp_serve_stats_get(vp_ctx *ctx, vp_serve_stats *out);

/* Expiry inside the resident kernel (every served NF), since the context
 * was created. The first request at which an expiry
 * is due takes the batch pipeline (`handed`); the next launch builds a touch
 * journal from the table (`seeds`) and from then on the kernel expires entries
 * itself, in the reference's LRU order, before every request. A pipeline call
 * that processes packets (a large batch, a declined burst) drops the journal:
 * the next due expiry is handed over once more and seeds it again. viglb has
 * two expiring tables and a journal for each: `handed` counts a request at
 * which either table was due, `seeds` counts tables, so one seeding of viglb
 * adds 2, and `expired` is the sum over both. A read of
 * host-side counters: the kernel stays. */
typedef struct vp_serve_expiry_stats {
  uint64_t seeds;    /* journal builds from a table (first and re-seeds; viglb: 2 a time) */
  uint64_t expired;  /* entries the resident kernel expired */
  uint64_t walks;    /* requests at which it expired at least one */
  uint64_t handed;   /* requests that took the pipeline because an expiry was due */
  uint64_t splits;   /* burst requests served in part (rest re-posted) */
} vp_serve_expiry_stats;
int vp_serve_expiry_stats_get(vp_ctx *ctx, vp_serve_expiry_stats *out);

/* Why the calling thread's last failing vp_* call failed: the HIP error and
 * the call site for VP_EIO / VP_ENOMEM, the broken invariant for VP_ESTATE,
 * the offending stage, link or exit for a configuration vp_chain_create
 * refused ("" if none was recorded). The text stays until the thread's next
 * failure that records one. */
const char *vp_last_error(void);

/* Per-context kernel timing (diagnostics, off by default): with on != 0,
 * every vp_process_device call brackets its classification kernel launches
 * with HIP events on the stream they run on (about 6 us of kernel-boundary
 * time per call). */
int vp_kernel_timing(vp_ctx *ctx, int on);

/* Kernel timing of the last vp_process_device call: time of the dominant
 * classification kernel in ms, summed over its launches (0 while
 * vp_kernel_timing is off), and the number of launches. */
int vp_last_kernel_ms(vp_ctx *ctx, float *ms, int *launches);

/* The name of the tile kernel the last vp_process_device call launched for
 * its 64-byte slots (vignat picks nat_classify64w or nat_classify64ws per
 * segment; viglb lb_classify64[w]); "" when none was.
 * vigpol names every segment, whatever the slot: its classify kernel plus the
 * phase-T path that produced the segment's results --
 * "pol_classify64+pol_runs" (run slots), "...+pol_scatter+pol_runs" (scan +
 * scatter) or "...+pol_buckets" (the sorting path, a grouping attempt that fell
 * back included), with pol_classify for slots other than 64 bytes. A call
 * that was cut into several segments reports its last segment's. The string
 * is static. */
const char *vp_last_kernel(vp_ctx *ctx);

/* Owner-sharded multi-GPU contexts (VP_SHARD_OWNER) with kernel timing on:
 * the last vp_process_device call's phase-A stage times in ms, summed over
 * its segments, from HIP events between the stages: ms[0] pass 1 (classify,
 * keys routed), ms[1] offsets (counts all-to-all, overflow all-reduce),
 * ms[2] keys all-to-all, ms[3] owner probe, ms[4] answers all-to-all,
 * ms[5] pass 2 (routed packets rewritten, touches binned), ms[6] fold;
 * the chunked pipeline records ms[7], its chunks' passes,
 * exchanges and probes together (they overlap), and ms[6] only.
 * vp_stage_ms writes at most `cap` floats and sets *stages to the number of
 * stages recorded (0..VP_STAGES, may exceed cap). vp_last_stage_ms is the
 * 0.2 entry point: exactly 7 floats (ms[0..6]), *stages at most 7. */
#define VP_STAGES 8
int vp_stage_ms(vp_ctx *ctx, float *ms, int cap, int *stages);
int vp_last_stage_ms(vp_ctx *ctx, float *ms, int *stages);

/* Diagnostics (bench.py): the memory-shape ceiling of the classify tile --
 * n slots of `slot` (64 or 128) bytes at `frames` (device memory, n a
 * multiple of 64) streamed with nat_classify64's grid and access shape, each
 * slot read and, store != 0, written back unchanged (write-through). *ms =
 * the mean duration of `reps` launches, each timed by its own dispatch's
 * timestamps. DESIGN.md §5.1. vp_probe_slots_w: the same with `waves` (4,
 * 8, 12 or 16) waves per block, as many blocks per CU as 16 waves make (16:
 * nat_classify64w's one 1024-thread block per CU, its tile order as
 * VIGPATH_SPLIT sets it); vp_probe_slots is waves = 4. */
int vp_probe_slots(void *frames, uint32_t n, uint32_t slot, int store, int reps, float *ms);
int vp_probe_slots_w(void *frames, uint32_t n, uint32_t slot, int store, int waves, int reps,
                     float *ms);
/* vp_probe_slots_p: the same pass with the cache policy of its loads and of
 * its stores given, each one of the VP_POLICY_* values below (the policy
 * bits of the gfx950 buffer instructions); vp_probe_slots_w is this call
 * with the tile kernels' own pair. Pairs other than that one run at 64-byte
 * slots and 4 or 16 waves; any other value or shape is VP_EINVAL. The table
 * this call measured is in DESIGN.md §5.1 and profiles/r07a_tile_policy.txt. */
#define VP_POLICY_PLAIN 0
#define VP_POLICY_NT 2       /* non-temporal */
#define VP_POLICY_SC1 16     /* loads: past the CU's L1; stores: write-through */
#define VP_POLICY_SC0_SC1 17 /* loads only */
#define VP_POLICY_SC1_NT 18  /* stores only */
int vp_probe_slots_p(void *frames, uint32_t n, uint32_t slot, int store, int waves,
                     int load_policy, int store_policy, int reps, float *ms);

/* Build identification (e.g. "vigpath gfx950"). */
const char *vp_version(void);

/* Exported by the nf.h shim libraries (libvig*_nf.so), not libvigpath.so:
 * the context nf_init() created, so a batching caller can pass it to
 * vp_process_batch / vp_process_device. NULL before nf_init(). */
vp_ctx *vp_nf_context(void);

#ifdef __cplusplus
}
#endif
#endif
