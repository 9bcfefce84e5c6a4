// The chain object (vp_chain_*, include/vigpath.h): several contexts on one GPU
// joined by the transmit / receive calls, standing where one NF stands
// (DESIGN.md §5.12). Host code over the C-ABI's own entry points, and one
// kernel:
//
//   chn_compose each block takes kSlotBlockEntries consecutive entries of a
//               stage's src[] (vp_tx_rebatch's or vp_rx_unpack's: indices into
//               the source stage's batch); a wave walks 64 of them per turn:
//               src[] one entry per lane, the source stage's origin gathered
//               through it, stored coalesced. An index outside the source
//               batch gives 0xFFFFFFFF, which vp_tx_return counts as bad_home
//               and never writes through.
//
// No block waits for another, nothing is kept between the turns, and there is
// no workspace, no LDS and no private segment.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <new>
#include <vector>

#include "vp_internal.h"
#include "vp_slots_dev.h"

namespace vp {

VP_PRELOAD_UNIT(chain)

constexpr uint32_t kChainNoOrigin = 0xFFFFFFFFu;

__global__ __launch_bounds__(kSlotThreads) void chn_compose(const uint32_t *__restrict__ src,
                                                           const uint32_t *__restrict__ origin_s,
                                                           uint32_t n_s, uint32_t cnt,
                                                           uint32_t *__restrict__ origin_t) {
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint64_t w0 = (uint64_t)blockIdx.x * kSlotBlockEntries + wv * kSlotPerWave;
  for (uint32_t it = 0; it < kSlotTurns; it++) {
    const uint64_t k = w0 + it * 64 + lane;  // (may pass 2^32)
    if (k >= cnt) break;  // (entries ascend with the lane and the turn)
    const uint32_t i = src[k];
    origin_t[k] = i < n_s ? origin_s[i] : kChainNoOrigin;
  }
}

// vp_last_error()'s text for a refused configuration
static int chain_refuse(const char *fmt, ...) {
  char text[200];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(text, sizeof text, fmt, ap);
  va_end(ap);
  state_fail("vp_chain_create: %s", text);  // (records the text)
  return VP_EINVAL;
}

// A device allocation the chain keeps from call to call
struct ChainMem {
  void *p = nullptr;
  size_t bytes = 0;
};

struct ChainInbound {
  uint32_t from, out_port, in_port;
};
struct ChainOutbound {
  uint32_t out_port, to;
};

// One stage: its place in the graph, what it owns, and its batch in the run
// that is under way (or was last)
struct ChainStage {
  vp_ctx *ctx = nullptr;
  uint32_t nd = 0;
  std::vector<ChainInbound> in;    // in `links` order
  std::vector<ChainOutbound> out;  // in `links` order
  // vp_tx_return's actions (way_home)
  uint32_t ret_port[VP_MAX_DEVICES] = {};
  uint32_t ret_flood = VP_RET_DROP;
  // the transmit lists over its out ports: idx (lcap entries) and offset
  ChainMem idx_m, off_m;
  uint32_t lcap = 0;
  bool built = false;  // offset[] of this run is in h_off
  uint32_t h_off[VP_MAX_DEVICES + 1] = {};
  // cable "stream": the packed lists -- data, pos (lcap entries), port_off
  ChainMem data_m, pos_m, poff_m;
  // its input batch (stages after 0): one allocation, carved below
  ChainMem buf_m;
  uint32_t cap = 0, bslot = 0;
  uint8_t *frames = nullptr;
  int64_t *now = nullptr;
  uint32_t *src = nullptr, *key = nullptr, *org = nullptr, *count = nullptr;
  uint16_t *len = nullptr, *outp = nullptr, *inp = nullptr;
  uint8_t *which = nullptr;
  vp_chain_view v{};  // the run's batch
  int64_t now0 = 0, now_step = 0;  // (stage 0 with affine time)
};

}  // namespace vp

using namespace vp;

struct vp_chain {
  std::vector<ChainStage> st;
  uint32_t cable = VP_CABLE_SLOTS;
  int gpu = 0;
  // the stream of the run under way, or of a run that failed part-way and may
  // have left work queued on it; null once a run has ended drained
  hipStream_t busy = nullptr;
  ChainMem out0_m;             // stage 0's out ports
  ChainMem stats_m;            // one vp_tx_return_stats per stage
  uint32_t *h_pin = nullptr;   // page-locked: an offset[] read, then the stages' stats
};

namespace vp {

static size_t chain_pin_bytes(size_t k) {
  const size_t a = sizeof(uint32_t) * (VP_MAX_DEVICES + 1), b = sizeof(vp_tx_return_stats) * k;
  return a > b ? a : b;
}

// m holds at least `bytes`: a larger request waits for the stream that may
// still use the old memory, frees it and allocates anew (contents are lost)
static int chain_reserve(vp_chain *ch, ChainMem &m, size_t bytes) {
  if (bytes <= m.bytes) return 0;
  if (m.p) {
    if (ch->busy) VP_HIP(stream_wait(ch->busy));
    hipFree(m.p);
    m.p = nullptr;
    m.bytes = 0;
  }
  VP_HIP(hipMalloc(&m.p, bytes));
  m.bytes = bytes;
  return 0;
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Stage t's input buffers for n packets of `slot` bytes: kept from call to
// call, replaced by larger ones on demand (at least doubled, at least 64)
static int chain_grow(vp_chain *ch, ChainStage &t, uint32_t n, uint32_t slot) {
  if (t.buf_m.p && t.cap >= n && t.bslot == slot) return 0;
  uint64_t cap = n;
  if (t.buf_m.p && t.bslot == slot && 2ull * t.cap > cap) cap = 2ull * t.cap;
  if (cap < 64) cap = 64;
  if (cap > 0xFFFFFFFFull) cap = 0xFFFFFFFFull;
  size_t at = 0;
  const size_t o_frames = at;
  at = up256(at + (size_t)cap * slot);
  const size_t o_now = at;
  at = up256(at + (size_t)cap * 8);
  const size_t o_src = at;
  at = up256(at + (size_t)cap * 4);
  const size_t o_key = at;
  at = up256(at + (size_t)cap * 4);
  const size_t o_org = at;
  at = up256(at + (size_t)cap * 4);
  const size_t o_len = at;
  at = up256(at + (size_t)cap * 2);
  const size_t o_out = at;
  at = up256(at + (size_t)cap * 2);
  const size_t o_in = at;
  at = up256(at + (size_t)cap * 2);
  const size_t o_which = at;
  at = up256(at + (size_t)cap);
  const size_t o_count = at;
  at += 256;
  // (another slot with room enough still lays the arrays out anew)
  if (at > t.buf_m.bytes) {
    VP_TRY(chain_reserve(ch, t.buf_m, at));
  } else if (ch->busy) {
    VP_HIP(stream_wait(ch->busy));
  }
  uint8_t *base = (uint8_t *)t.buf_m.p;
  t.frames = base + o_frames;
  t.now = (int64_t *)(base + o_now);
  t.src = (uint32_t *)(base + o_src);
  t.key = (uint32_t *)(base + o_key);
  t.org = (uint32_t *)(base + o_org);
  t.len = (uint16_t *)(base + o_len);
  t.outp = (uint16_t *)(base + o_out);
  t.inp = (uint16_t *)(base + o_in);
  t.which = base + o_which;
  t.count = (uint32_t *)(base + o_count);
  t.cap = (uint32_t)cap;
  t.bslot = slot;
  return 0;
}

// The run's batch of stage s as the calls take it
static vp_dev_batch chain_batch(const ChainStage &s) {
  vp_dev_batch b{};
  b.frames = s.v.frames;
  b.slot = s.v.slot;
  b.n = s.v.n;
  b.len = s.v.len;
  b.in_dev = s.v.in_dev;
  b.in_port = s.v.in_port;
  b.now = s.v.now;
  b.now0 = s.now0;
  b.now_step = s.now_step;
  b.out_dev = const_cast<uint16_t *>(s.v.out_dev);
  return b;
}

static vp_tx_lists chain_lists(const ChainStage &s) {
  vp_tx_lists l{};
  l.idx = (uint32_t *)s.idx_m.p;
  l.cap = s.lcap;
  l.offset = (uint32_t *)s.off_m.p;
  return l;
}

static void chain_view_empty(ChainStage &s) {
  s.v = vp_chain_view{};
  s.now0 = s.now_step = 0;
}

// Stage s's transmit lists over its result, offset[] read to the host (the
// one host synchronisation per stage). A list that outgrew idx (floods) is
// built again with room.
static int chain_build(vp_chain *ch, ChainStage &s, hipStream_t q) {
  const uint32_t n = s.v.n;
  VP_TRY(chain_reserve(ch, s.off_m, sizeof(uint32_t) * (VP_MAX_DEVICES + 1)));
  if (s.lcap < n) {
    VP_TRY(chain_reserve(ch, s.idx_m, sizeof(uint32_t) * (size_t)n));
    s.lcap = n;
  }
  const vp_dev_batch b = chain_batch(s);
  for (;;) {
    const vp_tx_lists l = chain_lists(s);
    VP_TRY(vp_tx_build(s.ctx, &b, &l, q));
    VP_HIP(hipMemcpyAsync(ch->h_pin, l.offset, sizeof(uint32_t) * (s.nd + 1),
                          hipMemcpyDeviceToHost, q));
    VP_HIP(stream_wait(q));
    for (uint32_t d = 0; d <= s.nd; d++) s.h_off[d] = ch->h_pin[d];
    const uint32_t total = s.h_off[s.nd];
    if (total <= s.lcap) break;
    VP_TRY(chain_reserve(ch, s.idx_m, sizeof(uint32_t) * (size_t)total));
    s.lcap = total;
  }
  s.built = true;
  return 0;
}

// Stage s's lists as one packed stream (cable "stream"): vp_tx_pack with pos
// into total * slot bytes, which hold every listed frame at its padded length
static int chain_pack(vp_chain *ch, ChainStage &s, hipStream_t q) {
  const uint64_t bytes = (uint64_t)s.h_off[s.nd] * s.v.slot;
  VP_TRY(chain_reserve(ch, s.data_m, (size_t)bytes));
  VP_TRY(chain_reserve(ch, s.pos_m, sizeof(uint64_t) * (size_t)s.lcap));
  VP_TRY(chain_reserve(ch, s.poff_m, sizeof(uint64_t) * (VP_MAX_DEVICES + 1)));
  const vp_dev_batch b = chain_batch(s);
  const vp_tx_lists l = chain_lists(s);
  vp_tx_frames f{};
  f.data = (uint8_t *)s.data_m.p;
  f.cap_bytes = bytes;
  f.port_off = (uint64_t *)s.poff_m.p;
  f.pos = (uint64_t *)s.pos_m.p;
  return vp_tx_pack(s.ctx, &b, &l, &f, q);
}

// Stage t's batch is its buffers' first cnt packets; `merged`: with the
// per-packet in ports and the merge's keys as origins
static void chain_view_own(ChainStage &t, uint32_t cnt, uint32_t slot, bool merged,
                           uint32_t in_port, const uint32_t *origin) {
  t.v.n = cnt;
  t.v.slot = slot;
  t.v.frames = t.frames;
  t.v.len = t.len;
  t.v.out_dev = t.outp;
  t.v.in_dev = merged ? t.inp : nullptr;
  t.v.in_port = merged ? 0 : in_port;
  t.v.now = t.now;
  t.v.origin = origin;
  t.now0 = t.now_step = 0;
}

// One link out of stage s into stage t, which has no other: the port's list as
// t's batch, its origins, and t's run
static int chain_hand_over(vp_chain *ch, uint32_t si, const ChainOutbound &o, bool &packed,
                           hipStream_t q) {
  ChainStage &s = ch->st[si], &t = ch->st[o.to];
  const uint32_t lo = s.h_off[o.out_port], cnt = s.h_off[o.out_port + 1] - lo;
  if (cnt == 0) {
    chain_view_empty(t);
    return 0;
  }
  const uint32_t slot = s.v.slot;
  VP_TRY(chain_grow(ch, t, cnt, slot));
  const vp_dev_batch b = chain_batch(s);
  const vp_tx_lists l = chain_lists(s);
  vp_tx_next nx{};
  nx.frames = t.frames;
  nx.slot = slot;
  nx.cap = cnt;
  nx.len = t.len;
  nx.now = t.now;
  nx.src = t.src;
  nx.count = t.count;
  if (ch->cable == VP_CABLE_STREAM) {
    if (!packed) VP_TRY(chain_pack(ch, s, q));
    packed = true;
    vp_rx_stream rx{};
    rx.data = (const uint8_t *)s.data_m.p;
    rx.bytes = (uint64_t)s.h_off[s.nd] * slot;
    rx.n = cnt;
    rx.pos = (const uint64_t *)s.pos_m.p + lo;
    rx.sel = l.idx + lo;
    rx.meta_n = b.n;
    rx.len = b.len;
    rx.now = b.now;
    rx.now0 = b.now0;
    rx.now_step = b.now_step;
    VP_TRY(vp_rx_unpack(s.ctx, &rx, &nx, q));
  } else {
    VP_TRY(vp_tx_rebatch(s.ctx, &b, &l, o.out_port, &nx, q));
  }
  // origins: behind stage 0 the indices themselves; else composed through the
  // source stage's
  const uint32_t *origin = t.src;
  if (si) {
    const uint32_t blocks = (cnt - 1) / kSlotBlockEntries + 1;
    chn_compose<<<blocks, kSlotThreads, 0, q>>>(t.src, s.v.origin, s.v.n, cnt, t.org);
    VP_HIP(hipGetLastError());
    origin = t.org;
  }
  chain_view_own(t, cnt, slot, false, t.in[0].in_port, origin);
  const vp_dev_batch tb = chain_batch(t);
  return vp_process_device(t.ctx, &tb, q);
}

// Stage t's input from its several inbound links, and its run: one vp_tx_merge
// over the links' lists in `links` order, each source keyed by its stage's
// origins (stage 0's are the packet indices: no key array)
static int chain_merge(vp_chain *ch, ChainStage &t, uint32_t slot, hipStream_t q) {
  vp_tx_source srcs[VP_TX_MERGE_MAX];
  vp_dev_batch bs[VP_TX_MERGE_MAX];
  vp_tx_lists ls[VP_TX_MERGE_MAX];
  uint32_t m = 0;
  uint64_t cnt = 0;
  for (const ChainInbound &in : t.in) {
    const ChainStage &s = ch->st[in.from];
    if (s.v.n == 0 || !s.built) continue;
    const uint32_t c = s.h_off[in.out_port + 1] - s.h_off[in.out_port];
    if (c == 0) continue;
    cnt += c;
    bs[m] = chain_batch(s);
    ls[m] = chain_lists(s);
    srcs[m].ctx = s.ctx;
    srcs[m].batch = &bs[m];
    srcs[m].lists = &ls[m];
    srcs[m].port = in.out_port;
    srcs[m].in_port = in.in_port;
    srcs[m].key = s.v.origin;  // (NULL at stage 0)
    m++;
  }
  if (cnt == 0) {
    chain_view_empty(t);
    return 0;
  }
  if (cnt > 0xFFFFFFFFull) return VP_EINVAL;
  VP_TRY(chain_grow(ch, t, (uint32_t)cnt, slot));
  vp_tx_merged o{};
  o.frames = t.frames;
  o.slot = slot;
  o.cap = (uint32_t)cnt;
  o.len = t.len;
  o.now = t.now;
  o.in_dev = t.inp;
  o.key = t.key;
  o.src = t.src;
  o.which = t.which;
  o.count = t.count;
  VP_TRY(vp_tx_merge(t.ctx, srcs, m, &o, q));
  chain_view_own(t, (uint32_t)cnt, slot, true, 0, t.key);
  const vp_dev_batch tb = chain_batch(t);
  return vp_process_device(t.ctx, &tb, q);
}

static int chain_batch_check(const vp_dev_batch *b, bool need_out) {
  if (!b->in_dev && b->in_port > 0xFFFFu) return VP_EINVAL;
  if (!b->n) return 0;
  if (!b->frames || !b->len || !slots_ok(b->frames, b->slot)) return VP_EINVAL;
  return need_out && !b->out_dev ? VP_EINVAL : 0;
}

// vp_chain_run without its last wait
static int chain_run(vp_chain *ch, const vp_dev_batch *batch, hipStream_t q) {
  const uint32_t k = (uint32_t)ch->st.size();
  for (ChainStage &s : ch->st) {
    chain_view_empty(s);
    s.built = false;
  }
  // (a run that failed part-way may have left work on its stream that still
  // uses the buffers)
  if (ch->busy && ch->busy != q) VP_HIP(stream_wait(ch->busy));
  ch->busy = q;
  if (!batch->n) return 0;
  ChainStage &s0 = ch->st[0];
  VP_TRY(chain_reserve(ch, ch->out0_m, sizeof(uint16_t) * (size_t)batch->n));
  VP_HIP(hipMemsetAsync(ch->out0_m.p, 0, sizeof(uint16_t) * (size_t)batch->n, q));
  s0.v.n = batch->n;
  s0.v.slot = batch->slot;
  s0.v.frames = batch->frames;
  s0.v.len = batch->len;
  s0.v.out_dev = (uint16_t *)ch->out0_m.p;
  s0.v.in_dev = batch->in_dev;
  s0.v.in_port = batch->in_port;
  s0.v.now = batch->now;
  s0.v.origin = nullptr;
  s0.now0 = batch->now0;
  s0.now_step = batch->now_step;
  const vp_dev_batch b0 = chain_batch(s0);
  VP_TRY(vp_process_device(s0.ctx, &b0, q));
  for (uint32_t si = 0; si < k; si++) {
    ChainStage &s = ch->st[si];
    if (s.in.size() > 1) VP_TRY(chain_merge(ch, s, batch->slot, q));
    if (s.out.empty() || s.v.n == 0) continue;  // (its targets' views are empty already)
    VP_TRY(chain_build(ch, s, q));
    bool packed = false;  // cable "stream": this stage's lists, packed once
    for (const ChainOutbound &o : s.out)
      if (ch->st[o.to].in.size() == 1)  // (a merging stage is assembled when it is reached)
        VP_TRY(chain_hand_over(ch, si, o, packed, q));
  }
  return 0;
}

// The wait that ends a run: nothing of the chain is in flight afterwards
static int chain_drained(vp_chain *ch, hipStream_t q) {
  VP_HIP(stream_wait(q));
  ch->busy = nullptr;
  return 0;
}

static void chain_free(vp_chain *ch) {
  if (!ch) return;
  hipSetDevice(ch->gpu);
  if (ch->busy) stream_wait(ch->busy);
  for (ChainStage &s : ch->st)
    for (ChainMem *m : {&s.idx_m, &s.off_m, &s.data_m, &s.pos_m, &s.poff_m, &s.buf_m}) hipFree(m->p);
  hipFree(ch->out0_m.p);
  hipFree(ch->stats_m.p);
  if (ch->h_pin) hipHostFree(ch->h_pin);
  delete ch;
}

}  // namespace vp

// vp_chain_create behind its NULL and count checks (may throw std::bad_alloc)
static int chain_create(const vp_chain_config *cfg, vp_chain **out) {
  const uint32_t k = cfg->n_stages;
  vp_chain *ch = new vp_chain;
  struct Guard {  // (frees the half-made chain on every refusal below)
    vp_chain *c;
    ~Guard() { chain_free(c); }
  } guard{ch};
  ch->cable = cfg->cable;
  ch->gpu = cfg->stages[0]->gpu;
  ch->st.resize(k);
  for (uint32_t s = 0; s < k; s++) {
    vp_ctx *c = cfg->stages[s];
    if (c->gpu != ch->gpu)
      return chain_refuse("stage %u is on GPU %d, stage 0 on GPU %d", s, c->gpu, ch->gpu);
    if (c->comm) {
      chain_refuse("stage %u is attached to a multi-GPU communicator", s);
      return VP_ENOTSUP;
    }
    ch->st[s].ctx = c;
    ch->st[s].nd = ctx_devices(c);
    if (ch->st[s].nd > VP_MAX_DEVICES)
      return chain_refuse("stage %u has more than %d devices", s, VP_MAX_DEVICES);
  }
  for (uint32_t j = 0; j < cfg->n_links; j++) {
    const vp_chain_link &l = cfg->links[j];
    char name[96];
    snprintf(name, sizeof name, "link %u (%u, %u, %u, %u)", j, l.from, l.out_port, l.to,
             l.in_port);
    if (l.from >= k || l.to >= k) return chain_refuse("%s names a stage outside the chain", name);
    if (l.to <= l.from) return chain_refuse("%s goes backward", name);
    if (l.out_port >= ch->st[l.from].nd)
      return chain_refuse("%s leaves from a port stage %u does not have", name, l.from);
    if (l.in_port > 0xFFFFu) return chain_refuse("%s arrives on a port beyond 16 bits", name);
    if (ch->st[l.to].in.size() == VP_TX_MERGE_MAX)
      return chain_refuse("%s: stage %u has more than %d inbound links", name, l.to,
                          VP_TX_MERGE_MAX);
    ch->st[l.to].in.push_back({l.from, l.out_port, l.in_port});
    ch->st[l.from].out.push_back({l.out_port, l.to});
  }
  for (uint32_t t = 1; t < k; t++) {
    if (ch->st[t].in.empty()) return chain_refuse("stage %u has no inbound link", t);
    if (ch->st[t].in.size() < 2) continue;
    for (const ChainInbound &in : ch->st[t].in) {
      uint32_t named = 0;
      for (const ChainOutbound &o : ch->st[in.from].out) named += o.out_port == in.out_port;
      if (named > 1)
        return chain_refuse("port %u of stage %u feeds stage %u, which merges, and has another "
                            "link", in.out_port, in.from, t);
    }
  }
  // vp_tx_return's actions: a linked port is skipped, an exit is its number,
  // anything else a drop
  std::vector<uint32_t> exits_of(k, 0);
  for (uint32_t s = 0; s < k; s++) {
    for (uint32_t d = 0; d < VP_MAX_DEVICES; d++) ch->st[s].ret_port[d] = VP_RET_DROP;
    for (const ChainOutbound &o : ch->st[s].out) ch->st[s].ret_port[o.out_port] = VP_RET_SKIP;
  }
  for (uint32_t j = 0; j < cfg->n_exits; j++) {
    const vp_chain_exit &e = cfg->exits[j];
    char name[96];
    snprintf(name, sizeof name, "exit %u (%u, %u) -> %u", j, e.stage, e.port, e.ext_port);
    if (e.stage >= k || e.port >= ch->st[e.stage].nd)
      return chain_refuse("%s names a port its stage does not have", name);
    ChainStage &s = ch->st[e.stage];
    if (s.ret_port[e.port] == VP_RET_SKIP) return chain_refuse("%s names a linked port", name);
    if (e.ext_port > 0xFFFFu) return chain_refuse("%s is beyond 16 bits", name);
    if (s.ret_port[e.port] == VP_RET_DROP) exits_of[e.stage]++;  // (a port named twice counts once)
    s.ret_port[e.port] = e.ext_port;
  }
  for (uint32_t s = 0; s < k; s++)
    ch->st[s].ret_flood = exits_of[s] == ch->st[s].nd ? (uint32_t)VP_FLOOD_FRAME
                          : s == 0                    ? VP_RET_SKIP
                                                      : VP_RET_DROP;
  if (hipSetDevice(ch->gpu) != hipSuccess) return VP_EIO;
  VP_HIP(hipHostMalloc((void **)&ch->h_pin, chain_pin_bytes(k), hipHostMallocDefault));
  VP_TRY(chain_reserve(ch, ch->stats_m, sizeof(vp_tx_return_stats) * k));
  guard.c = nullptr;
  *out = ch;
  return 0;
}

extern "C" int vp_chain_create(const vp_chain_config *cfg, vp_chain **out) {
  if (!cfg || !out) return VP_EINVAL;
  const uint32_t k = cfg->n_stages;
  if (k == 0 || k > VP_CHAIN_MAX_STAGES) return VP_EINVAL;
  if (!cfg->stages || (!cfg->links && cfg->n_links) || (!cfg->exits && cfg->n_exits))
    return VP_EINVAL;
  for (uint32_t s = 0; s < k; s++)
    if (!cfg->stages[s]) return VP_EINVAL;
  if (cfg->cable != VP_CABLE_SLOTS && cfg->cable != VP_CABLE_STREAM) return VP_EINVAL;
  // (the contexts are read from here on)
  try {
    return chain_create(cfg, out);
  } catch (const std::bad_alloc &) {  // (no exception crosses the C boundary)
    chain_refuse("out of host memory");
    return VP_ENOMEM;
  }
}

extern "C" void vp_chain_destroy(vp_chain *ch) { chain_free(ch); }

extern "C" int vp_chain_run(vp_chain *ch, const vp_dev_batch *batch, void *stream) {
  if (!ch || !batch) return VP_EINVAL;
  VP_TRY(chain_batch_check(batch, false));
  if (hipSetDevice(ch->gpu) != hipSuccess) return VP_EIO;
  hipStream_t q = stream ? (hipStream_t)stream : ch->st[0].ctx->stream;
  VP_TRY(chain_run(ch, batch, q));
  return chain_drained(ch, q);
}

extern "C" int vp_chain_view_get(vp_chain *ch, uint32_t stage, vp_chain_view *out) {
  if (!ch || !out || stage >= ch->st.size()) return VP_EINVAL;
  *out = ch->st[stage].v;
  return 0;
}

extern "C" int vp_chain_process_device(vp_chain *ch, const vp_dev_batch *batch,
                                       vp_tx_return_stats *stats, void *stream) {
  if (!ch || !batch) return VP_EINVAL;
  VP_TRY(chain_batch_check(batch, true));
  if (hipSetDevice(ch->gpu) != hipSuccess) return VP_EIO;
  hipStream_t q = stream ? (hipStream_t)stream : ch->st[0].ctx->stream;
  VP_TRY(chain_run(ch, batch, q));
  const uint32_t k = (uint32_t)ch->st.size();
  if (stats) *stats = vp_tx_return_stats{};
  if (!batch->n) return chain_drained(ch, q);
  vp_tx_return_stats *d_stats = (vp_tx_return_stats *)ch->stats_m.p;
  // (a stage nothing reached makes no return call: its counts are zero)
  VP_HIP(hipMemsetAsync(d_stats, 0, sizeof(vp_tx_return_stats) * k, q));
  for (uint32_t si = 0; si < k; si++) {
    const ChainStage &s = ch->st[si];
    if (s.v.n == 0) continue;
    const vp_dev_batch from = chain_batch(s);
    vp_tx_way_home way{};
    way.home = s.v.origin;  // (stage 0: the in-place form)
    for (uint32_t d = 0; d < VP_MAX_DEVICES; d++) way.port[d] = s.ret_port[d];
    way.on_drop = VP_RET_DROP;
    way.on_flood = s.ret_flood;
    way.on_bad = VP_RET_DROP;
    way.stats = d_stats + si;
    VP_TRY(vp_tx_return(s.ctx, &from, batch, &way, q));
  }
  if (stats) {
    vp_tx_return_stats *h = (vp_tx_return_stats *)ch->h_pin;
    VP_HIP(hipMemcpyAsync(h, d_stats, sizeof(vp_tx_return_stats) * k, hipMemcpyDeviceToHost, q));
    VP_TRY(chain_drained(ch, q));
    for (uint32_t si = 0; si < k; si++) {
      stats->returned += h[si].returned;
      stats->dropped += h[si].dropped;
      stats->skipped += h[si].skipped;
      stats->dup += h[si].dup;
      stats->bad_home += h[si].bad_home;
    }
  } else {
    VP_TRY(chain_drained(ch, q));
  }
  return 0;
}
