// vp_process_one's mailbox, host side (ServeBox, vp_internal.h): the parts
// that serve any context whose NF has a resident kernel -- vignat (nat_serve,
// vp_nat.hip) and vigfw (fw_serve, vp_fw.hip). Launching the kernel, waiting
// for an answer, relaunching after an idle exit, stopping it before any other
// entry point touches the table, and yielding the GPU's hardware queues
// between contexts. What a request holds and how an answer is read is the
// NF's own (nat_process_one / nat_process_burst, fw_process_one /
// fw_process_burst).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "vp_internal.h"

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

// Launch c's resident kernel on c->stream: the polling parameters every
// server takes (kernel flags bits 10-23), then the NF's own launcher.
static int serve_launch(vp_ctx *c) {
  serve_yield(c);
  ServeBox *dbox = nullptr;
  VP_HIP(hipHostGetDevicePointer((void **)&dbox, c->sbox, 0));
  static const uint32_t after = [] {  // (wall-clock ticks of 10 ns, < 256)
    const char *e = getenv("VIGPATH_SERVE_AFTER");
    // (45: 4.59-4.65 us per packet, 60: 4.73-4.83, 0: 5.41-5.80 through
    // nf.c's loop, profiles/r06o_serve_after.txt, r06p_serve_after_sweep.txt)
    return e ? (uint32_t)std::min(255, std::max(0, atoi(e))) : 45u;
  }();
  static const uint32_t up = [] {  // (VIGPATH_SERVE_UP: ticks added after a late poll)
    const char *e = getenv("VIGPATH_SERVE_UP");
    return e ? (uint32_t)std::min(31, std::max(1, atoi(e))) : 8u;
  }();
  static const uint32_t adapt = [] {  // VIGPATH_SERVE_ADAPT=0: a fixed delay
    const char *e = getenv("VIGPATH_SERVE_ADAPT");
    return e && !atoi(e) ? 0u : 1u;
  }();
  const uint32_t flags = (after << 10) | (adapt << 18) | (up << 19);
  switch (c->kind) {
    case KIND_NAT:
      VP_TRY(nat_serve_launch(c, dbox, flags));
      break;
    case KIND_FW:
      VP_TRY(fw_serve_launch(c, dbox, flags));
      break;
    default:
      return state_fail("no resident kernel for NF kind %d", c->kind);
  }
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

}  // namespace vp
