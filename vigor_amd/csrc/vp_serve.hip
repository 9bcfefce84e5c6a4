// vp_process_one's mailbox, host side (ServeBox, vp_internal.h), for any
// context whose NF has a resident kernel -- vignat (nat_serve, vp_nat.hip),
// vigfw (fw_serve, vp_fw.hip), vigbridge (bridge_serve, vp_bridge.hip),
// vigpol (pol_serve, vp_pol.hip) and viglb (lb_serve, vp_lb.hip, the one with
// two expiring tables). Launching the kernel, waiting for an answer,
// relaunching after an idle exit, stopping it before any other entry point
// touches the table, yielding the GPU's hardware queues between contexts, and
// the requests themselves: one packet (serve_process_one) and a small burst
// (serve_process_burst), the NFs told apart by their ServeNf alone. The
// device side's shared half is vp_serve_dev.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "vp_internal.h"
#include "vp_table.h"

namespace vp {

// Contexts whose server may run: stopped at exit, before the runtime's own
// teardown (the kernel would otherwise keep the stream busy until its idle
// exit).
static std::mutex g_srv_mu;
static std::vector<vp_ctx *> g_srv;
static void serve_stop_all() {
  std::vector<vp_ctx *> v;
  {
    std::lock_guard<std::mutex> g(g_srv_mu);
    v = g_srv;
  }
  for (vp_ctx *c : v) serve_stop(c);
}

bool serve_prof() {  // VIGPATH_SERVE_PROF
  static const bool on = [] {
    const char *e = getenv("VIGPATH_SERVE_PROF");
    return e && atoi(e);
  }();
  return on;
}

// The server of c leaves (a leave request, then the stream drains); the
// caller holds c->srv_mu. Does not touch g_srv.
static hipError_t serve_halt(vp_ctx *c) {
  ServeBox *bx = c->sbox;
  const uint32_t req = ++c->srv_req;
  bx->msg[0][0] = kServeLeave;
  __atomic_store_n(&bx->msg[0][3], req, __ATOMIC_RELEASE);
  const hipError_t e = hipStreamSynchronize(c->stream);
  // (the kernel is gone: the leave request counts as answered for the next one)
  __atomic_store_n(&bx->ans, (uint64_t)req, __ATOMIC_RELEASE);
  c->srv_on = false;
  if (serve_prof() && c->srv_prof[5] > 0) {  // (vignat's stage clock)
    const double n = c->srv_prof[5];
    fprintf(stderr,
            "vigpath serve: %.0f packets, us/packet: host call %.2f, bell->seen %.2f "
            "(idle poll), load %.2f, packet %.2f (LAN: hash %.2f, table %.2f, rewrite %.2f), "
            "store+answer %.2f; shader clock %.0f MHz\n",
            n, c->srv_prof[0] / n, c->srv_prof[1] / n, c->srv_prof[2] / n, c->srv_prof[3] / n,
            c->srv_prof[6] / std::max(1.0, c->srv_prof[9]),
            c->srv_prof[7] / std::max(1.0, c->srv_prof[9]),
            c->srv_prof[8] / std::max(1.0, c->srv_prof[9]), c->srv_prof[4] / n,
            c->srv_prof[10] / std::max(1e-9, c->srv_prof[3]));
    for (double &x : c->srv_prof) x = 0;
  }
  return e;
}

int serve_stop(vp_ctx *c) {
  if (!c) return 0;
  std::lock_guard<std::recursive_mutex> sg(c->srv_mu);
  if (!c->srv_on) return 0;
  const hipError_t e = serve_halt(c);
  {
    std::lock_guard<std::mutex> g(g_srv_mu);
    g_srv.erase(std::remove(g_srv.begin(), g_srv.end(), c), g_srv.end());
  }
  VP_HIP(e);
  return 0;
}

void serve_free(vp_ctx *c) {
  serve_stop(c);
  if (c->sbox) hipHostFree(c->sbox);
  c->sbox = nullptr;
}

// Another context's resident server on this GPU may share a hardware queue
// with c->stream (GPU_MAX_HW_QUEUES streams' worth): c's server would then
// wait behind it until its idle exit. Stop those first (contexts served by
// another thread right now keep theirs: try_lock).
static void serve_yield(vp_ctx *c) {
  // (under g_srv_mu throughout: a listed context is not destroyed meanwhile,
  // as vp_destroy's serve_stop unlists it under the same lock first)
  std::lock_guard<std::mutex> g(g_srv_mu);
  for (size_t i = 0; i < g_srv.size();) {
    vp_ctx *x = g_srv[i];
    if (x == c || x->gpu != c->gpu || !x->srv_mu.try_lock()) {
      i++;
      continue;
    }
    if (x->srv_on) serve_halt(x);  // (an error shows at x's next call)
    x->srv_mu.unlock();
    g_srv.erase(g_srv.begin() + (ptrdiff_t)i);
  }
}

// The polling parameters every server takes (kernel flags bits 10-23,
// serve_poll), as measured on the MI355X through nf.c's loop:
// the first poll after an answer waits kServeAfter wall-clock ticks of 10 ns
// (45: 4.59-4.65 us per packet, 60: 4.73-4.83, 0: 5.41-5.80,
// profiles/r06o_serve_after.txt, r06p_serve_after_sweep.txt);
constexpr uint32_t kServeAfter = 45;
// the delay adapts, from there (fixed against adaptive from 0 / 45 / 90:
// profiles/r06r_serve_adaptive.txt);
constexpr uint32_t kServeAdapt = 1;
// and grows by kServeUp ticks after a request it missed (4 to 24 within the
// run-to-run spread, profiles/r06aj_serve_up.txt).
constexpr uint32_t kServeUp = 8;

// Launch c's resident kernel on c->stream: the polling parameters, then the
// NF's own launcher.
static int serve_launch(vp_ctx *c) {
  serve_yield(c);
  ServeBox *dbox = nullptr;
  VP_HIP(hipHostGetDevicePointer((void **)&dbox, c->sbox, 0));
  const uint32_t flags = (kServeAfter << 10) | (kServeAdapt << 18) | (kServeUp << 19);
  const NfOps *nf = nf_ops(c->kind);
  if (!nf) return state_fail("no resident kernel for NF kind %d", c->kind);
  VP_TRY(nf->serve_launch(c, dbox, flags));
  c->srv_stats.launches += 1;
  if (!c->srv_on) {
    static std::once_flag once;
    std::call_once(once, [] { atexit(serve_stop_all); });
    std::lock_guard<std::mutex> g(g_srv_mu);
    g_srv.push_back(c);
  }
  c->srv_on = true;
  return 0;
}

bool serve_off() {  // VIGPATH_SERVE=0
  static const bool off = [] {
    const char *e = getenv("VIGPATH_SERVE");
    return e && !atoi(e);
  }();
  return off;
}

uint32_t serve_burst_limit(uint32_t dflt) {  // VIGPATH_SERVE_BURST
  static const int v = [] {
    const char *e = getenv("VIGPATH_SERVE_BURST");
    return e ? std::max(0, atoi(e)) : -1;
  }();
  return v < 0 ? dflt : (uint32_t)v;
}

// ------------------------------------------------------ the touch journal --
// Expiry inside the resident kernel (vp_serve_dev.h). The
// expiry time E of a table's cutoff, cutoff(t) = t - E in u64 arithmetic
// (vignat's and vigbridge's 32-bit wrap inside it, vigpol's 64-bit
// burst * 1e9 / rate, viglb's two 64-bit lifetimes). An NF with a second
// expiring table (viglb: table2 / cutoff2) has a journal per table; the two
// are seeded, dropped and seeded again together.
typedef int64_t (*CutoffFn)(const vp_ctx *c, int64_t t);
static uint64_t serve_expire_e(const vp_ctx *c, CutoffFn cutoff) {
  return (uint64_t)0 - (uint64_t)cutoff(c, 0);
}
static bool serve_jr_on(const vp_ctx *c, const ServeNf &nf) {
  return (c->*nf.table).jr_on && (!nf.table2 || (c->*nf.table2).jr_on);
}

// Whether c's kernel may expire: the NF has the walk,
// VIGPATH_SERVE_EXPIRE is not 0, vignat polls with one wave (the journal's
// control words live in that wave's registers), and no table's E is negative
// (a packet would then expire the entry it has just touched).
static bool serve_journal_ok(const vp_ctx *c, const ServeNf &nf) {
  static const bool off = [] {
    const char *e = getenv("VIGPATH_SERVE_EXPIRE");
    return e && !atoi(e);
  }();
  static const bool waves = [] {
    const char *e = getenv("VIGPATH_SERVE_WAVES");
    const int v = e ? atoi(e) : 1;
    return v == 2 || v == 4;
  }();
  return nf.journal && !off && !(waves && c->kind == KIND_NAT) &&
         (int64_t)serve_expire_e(c, nf.cutoff) >= 0 &&
         (!nf.table2 || (int64_t)serve_expire_e(c, nf.cutoff2) >= 0);
}

JournalDev serve_journal_dev(const vp_ctx *c, const ServeNf &nf, bool second) {
  const FlowTable &t = c->*(second ? nf.table2 : nf.table);
  if (!t.jr_on) return JournalDev{};
  return JournalDev{t.jr, t.jrec, t.jr_n, tbl_purge_bound(t),
                    serve_expire_e(c, second ? nf.cutoff2 : nf.cutoff)};
}

// A request found an expiry due while the journal was off: it takes the
// pipeline, and the next launch seeds the journal (serve_ready).
static void serve_handed(vp_ctx *c, const ServeNf &nf) {
  if (!nf.journal) return;
  c->srv_exp.handed += 1;
  if (serve_journal_ok(c, nf)) c->jr_want = true;
}

// What a journal request's answer says beside its results: `expired` entries
// left in its walk (viglb: in its two walks); kOneTombs / kBurstTombs (tombs):
// a table passed the purge bound, so the kernel stops for the pipeline's own
// check -- of both tables when there are two: the check reads the control block
// back first and is cheap -- and is launched again by the next request. The
// journal stays: a rebuild moves entries, not stamps.
static int serve_expired(vp_ctx *c, const ServeNf &nf, uint32_t expired, bool tombs) {
  if (expired) {
    c->srv_exp.expired += expired;
    c->srv_exp.walks += 1;
  }
  if (!tombs) return 0;
  VP_TRY(serve_stop(c));
  VP_HIP(hipSetDevice(c->gpu));
  VP_TRY(tbl_check_tombs(c, c->*nf.table));
  return nf.table2 ? tbl_check_tombs(c, c->*nf.table2) : 0;
}

// A ring is full: stop, and the launch that follows seeds it again from the
// table, on all CUs -- the journal's compaction (viglb: of both rings).
static int serve_reseed(vp_ctx *c, const ServeNf &nf) {
  VP_TRY(serve_stop(c));
  (c->*nf.table).jr_on = false;
  if (nf.table2) (c->*nf.table2).jr_on = false;
  c->jr_want = true;
  return serve_ready(c);
}

// An expiry is due and the journal is off. If the context's last fallback was
// a due expiry (jr_want: the bounce is behind it), the journal is seeded now
// and the request served; else this request is the bounce.
static int serve_seed_now(vp_ctx *c) {
  if (!c->jr_want) return 0;
  VP_TRY(serve_stop(c));
  return serve_ready(c);
}

// The mailbox exists and the server runs (the caller holds c->srv_mu).
int serve_ready(vp_ctx *c) {
  if (!c->sbox || !c->srv_on) VP_HIP(hipSetDevice(c->gpu));  // (HIP calls below)
  if (!c->sbox) {
    VP_HIP(hipHostMalloc((void **)&c->sbox, sizeof(ServeBox),
                         hipHostMallocCoherent | hipHostMallocMapped));
    memset(c->sbox, 0, sizeof(ServeBox));
    c->srv_req = 0;
    int khz = 0;
    VP_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->gpu));
    const char *e = getenv("VIGPATH_SERVE_IDLE_MS");
    c->srv_idle_ms = e ? std::max(1, atoi(e)) : 20;
    c->srv_idle = (uint64_t)std::max(khz, 1) * c->srv_idle_ms;
  }
  if (!c->srv_on) {
    // the context's last fallback was a due expiry: from this launch on the
    // kernel expires itself, from a journal of the table as it is now
    if (c->jr_want) {
      const ServeNf &nf = nf_ops(c->kind)->serve;
      c->jr_want = false;
      for (FlowTable vp_ctx::*m : {nf.table, nf.table2}) {
        if (!m || (c->*m).jr_on) continue;
        VP_TRY(tbl_journal_seed(c, c->*m));
        c->srv_exp.seeds += 1;  // (tables seeded: viglb's two count 2)
      }
    }
    // the batch path may leave a timestamp fold running: the server is
    // queued behind it on the same stream
    VP_TRY(serve_launch(c));
  }
  return 0;
}

// Wait for the answer to request `req`: chunk 0's tag, then the other chunks'
// (`need`: as many as the answer takes), each chunk's bytes final once its tag
// is the request's. A kernel that left (idle) before it saw the request is
// launched again.
int serve_wait(vp_ctx *c, uint32_t req, uint32_t need) {
  ServeBox *bx = c->sbox;
  auto last = std::chrono::steady_clock::now();
  auto answered = [&]() {
    for (uint32_t k = 0; k < need; k++)
      if (__atomic_load_n(&bx->amsg[k][3], __ATOMIC_ACQUIRE) != req) return false;
    return true;
  };
  uint32_t spins = 0;
  while (!answered()) {
    __builtin_ia32_pause();
    if (++spins & 255) continue;  // (the clock read every 256 spins, not each)
    const auto nw = std::chrono::steady_clock::now();
    if (nw - last < std::chrono::microseconds(200)) continue;
    last = nw;
    // the kernel left (idle) before it saw the request: launch it again
    VP_HIP(hipSetDevice(c->gpu));
    const hipError_t q = hipStreamQuery(c->stream);
    if (q == hipErrorNotReady) continue;
    VP_HIP(q);
    if (answered()) continue;
    VP_TRY(serve_launch(c));
  }
  return 0;
}

// vignat's stage clock (VIGPATH_SERVE_PROF) for the packet just answered: the
// host call since h0 and the device's stamps (wall clock ticks, 100 MHz).
static void serve_prof_add(vp_ctx *c, std::chrono::steady_clock::time_point h0) {
  const double us_tick = 1e3 / (double)(c->srv_idle / c->srv_idle_ms);
  c->srv_prof[0] +=
      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h0).count();
  const uint64_t *p = c->sbox->prof;
  c->srv_prof[1] += us_tick * (double)(p[1] - p[0]);
  c->srv_prof[2] += us_tick * (double)(p[2] - p[1]);
  if (p[3] && p[4]) {  // (register-path LAN packets: hash | table | rewrite)
    c->srv_prof[6] += us_tick * (double)(p[3] - p[2]);
    c->srv_prof[7] += us_tick * (double)(p[4] - p[3]);
    c->srv_prof[8] += us_tick * (double)(p[5] - p[4]);
    c->srv_prof[9] += 1;
  }
  c->srv_prof[3] += us_tick * (double)(p[6] - p[2]);
  c->srv_prof[4] += us_tick * (double)(p[7] - p[6]);
  c->srv_prof[10] += (double)(p[9] - p[8]);  // (shader cycles over `packet`: MHz)
  c->srv_prof[5] += 1;
}

int serve_process_one(vp_ctx *c, const ServeNf &nf, uint16_t in_dev, uint8_t *frame,
                      uint16_t len, int64_t now, uint16_t *out) {
  std::lock_guard<std::recursive_mutex> sg(c->srv_mu);
  FlowTable &t = c->*nf.table;
  FlowTable *t2 = nf.table2 ? &(c->*nf.table2) : nullptr;
  // times that do not go back, a frame the mailbox holds
  const bool ok = !serve_off() && !c->comm && len <= kServeFrame && now >= 0 &&
                  now >= c->last_now;
  if (!ok) {
    VP_TRY(serve_stop(c));
    return 1;
  }
  // no expiry due at this packet on either table (run_batch's test for a
  // segment of one, each table against its own floor) -- or the kernel
  // expires itself (the journal is on)
  const bool due = nf.cutoff(c, now) > (int64_t)std::min<uint64_t>(t.ts_floor, (uint64_t)now) ||
                   (t2 && nf.cutoff2(c, now) >
                              (int64_t)std::min<uint64_t>(t2->ts_floor, (uint64_t)now));
  if (due && !serve_jr_on(c, nf)) VP_TRY(serve_seed_now(c));  // (after a bounce: seeded, then served)
  if (due && !serve_jr_on(c, nf)) {
    serve_handed(c, nf);
    VP_TRY(serve_stop(c));
    return 1;
  }
  const bool prof = nf.prof && serve_prof();
  const auto h0 = prof ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
  ServeBox *bx = nullptr;
  uint32_t res = 0, got = 0, back = 0;
  bool via_frame = false;
  for (int attempt = 0;; attempt++) {
    VP_TRY(serve_ready(c));
    bx = c->sbox;
    // the request: a frame longer than the chunks hold goes whole through
    // `frame` before them and comes back there (nf.one_whole), or only its
    // first nf.one_in bytes go
    const uint32_t req = ++c->srv_req;
    via_frame = nf.one_whole && len > kServeInline;
    got = via_frame ? 0u : std::min<uint32_t>(len, nf.one_in);
    if (via_frame) memcpy(bx->frame, frame, len);
    uint32_t m[3 * kServeChunks];
    const uint32_t need = serve_pack(m, len | ((uint32_t)in_dev << 16), now, frame, got);
    serve_post(bx, m, need, req);
    // the answer: chunk 0, and the chunks that bring the frame bytes back -- as
    // many as the request took, chunk 1 alone (bytes 0-11), or none
    back = std::min(got, nf.one_back);
    VP_TRY(serve_wait(c, req, 1 + (back + 11) / 12));
    // out | fresh << 16 | kOneFresh2 | kOneDeclined | kOneFull | kOneTombs
    res = bx->amsg[0][0];
    if (!(res & kOneFull)) break;
    // the journal's ring is full and nothing was done: seeded again, then
    // the same packet once more (it fits: at most cap records of >= 2 cap)
    if (attempt) return state_fail("journal full right after a seed");
    VP_TRY(serve_reseed(c, nf));
  }
  const bool jr = serve_jr_on(c, nf);
  if (res & kOneDeclined) {
    // the packet itself wrote nothing: the batch path, as an ineligible one
    // (the walk in front of it is done and counted; the pipeline's own expiry
    // at this packet finds nothing left due)
    c->srv_stats.declined += 1;
    if (jr) VP_TRY(serve_expired(c, nf, bx->amsg[0][1], (res & kOneTombs) != 0));
    VP_TRY(serve_stop(c));
    return 1;
  }
  if (via_frame)
    memcpy(frame, bx->frame, len);
  else
    serve_unpack(bx, frame, back);
  *out = (uint16_t)res;
  if ((res >> 16) & 1u) t.ts_floor = std::min<uint64_t>(t.ts_floor, (uint64_t)now);
  if (t2 && (res & kOneFresh2)) t2->ts_floor = std::min<uint64_t>(t2->ts_floor, (uint64_t)now);
  c->seq += 1;
  c->last_now = now;
  c->srv_stats.packets_one += 1;
  if (prof) serve_prof_add(c, h0);
  if (jr) VP_TRY(serve_expired(c, nf, bx->amsg[0][1], (res & kOneTombs) != 0));
  return 0;
}

int serve_process_burst(vp_ctx *c, const ServeNf &nf, const vp_mbuf_batch *b, uint32_t first,
                        uint32_t count, uint32_t *served) {
  *served = 0;
  std::lock_guard<std::recursive_mutex> sg(c->srv_mu);
  const uint32_t limit = serve_burst_limit(nf.burst_route);
  if (serve_off() || c->comm || count == 0 || count > limit) return 1;
  FlowTable &t = c->*nf.table;
  auto at = [&](uint32_t i) {
    return b->now ? b->now[first + i] : b->now0 + (int64_t)(first + i) * b->now_step;
  };
  // the whole range or none of it: frames the mailbox holds, times that do
  // not go back, and no expiry due anywhere in it -- the cutoff is monotone in
  // time and flows born in the range are stamped >= its first time, so the
  // last packet's cutoff against the floor as the range finds it decides
  const int64_t n0 = at(0), n1 = at(count - 1);
  if (n0 < 0 || n0 < c->last_now) return 1;
  int64_t prev = n0;
  for (uint32_t i = 0; i < count; i++) {
    const int64_t ti = at(i);
    if (b->len[first + i] > kServeFrame || ti < prev) return 1;
    prev = ti;
  }
  FlowTable *t2 = nf.table2 ? &(c->*nf.table2) : nullptr;  // (the same, on its own floor)
  // (with the journal on the kernel expires itself, and serves a request up
  // to the packet at which the next expiry falls due)
  const bool due =
      nf.cutoff(c, n1) > (int64_t)std::min<uint64_t>(t.ts_floor, (uint64_t)n0) ||
      (t2 && nf.cutoff2(c, n1) > (int64_t)std::min<uint64_t>(t2->ts_floor, (uint64_t)n0));
  if (due && !serve_jr_on(c, nf)) VP_TRY(serve_seed_now(c));  // (after a bounce: seeded, then served)
  if (due && !serve_jr_on(c, nf)) {
    serve_handed(c, nf);
    return 1;
  }
  int reseeds = 0;
  for (uint32_t a0 = 0; a0 < count;) {
    VP_TRY(serve_ready(c));  // (stopped by a purge or a seed in between: launched again)
    ServeBox *bx = c->sbox;
    uint32_t m = std::min(kServeBurst, count - a0);
    // the body first, then the tagged chunk that announces it (ServeBox)
    for (uint32_t i = 0; i < m; i++) {
      const uint32_t p = first + a0 + i;
      if (b->len[p])
        memcpy(bx->bframe[i], b->frames[p], std::min<uint32_t>(b->len[p], nf.burst_in));
      bx->bmeta[i] = b->len[p] | ((uint32_t)b->in_dev[p] << 16);
      bx->bnow[i] = at(a0 + i);
    }
    const uint32_t req = ++c->srv_req;
    const uint32_t op[3] = {kServeBurstOp | (m << 16), 0, 0};
    serve_post(bx, op, 1, req);
    VP_TRY(serve_wait(c, req, 1));
    const uint32_t st = bx->amsg[0][0];
    const bool jr = serve_jr_on(c, nf);
    if (st == kBurstFull && jr) {  // nothing of it was done: seeded again, once more
      if (reseeds++) return state_fail("journal full right after a seed");
      VP_TRY(serve_reseed(c, nf));
      continue;
    }
    if ((st & 0xFFu) != kBurstServed) {
      // a byte-path frame, or viglb's erasure: none of its packets was done (a
      // walk in front of the erasure is, and is counted)
      c->srv_stats.declined += 1;
      if (jr) VP_TRY(serve_expired(c, nf, bx->amsg[0][2], (st & kBurstTombs) != 0));
      return 1;
    }
    reseeds = 0;
    // the packets served: all of them, or with the journal on those before
    // the one at which an expiry falls due (the rest is the next request)
    const uint32_t asked = m;
    if (jr) m = std::min(std::max(bx->amsg[0][1], 1u), m);
    bool fresh = false, fresh2 = false;
    for (uint32_t i = 0; i < m; i++) {
      const uint32_t p = first + a0 + i, r = bx->bout[i];
      b->out_dev[p] = (uint16_t)r;
      fresh |= (r >> 16) & 1u;
      fresh2 |= (r & kOneFresh2) != 0;
      // (only rewritten frames come back, and only the bytes a rewrite can change)
      if ((r >> 17) & 1u)
        memcpy(b->frames[p], bx->bframe[i], std::min<uint32_t>(b->len[p], nf.burst_back));
    }
    if (fresh) t.ts_floor = std::min<uint64_t>(t.ts_floor, (uint64_t)at(a0));
    if (t2 && fresh2) t2->ts_floor = std::min<uint64_t>(t2->ts_floor, (uint64_t)at(a0));
    c->seq += m;
    c->last_now = at(a0 + m - 1);
    c->srv_stats.bursts += 1;
    c->srv_stats.burst_packets += m;
    *served += m;
    if (jr) {
      if (m < asked) c->srv_exp.splits += 1;
      VP_TRY(serve_expired(c, nf, bx->amsg[0][2], (st & kBurstTombs) != 0));
    }
    a0 += m;
  }
  return 0;
}

}  // namespace vp
