// Memory-shape ceiling of the 64-byte classify tile (vp_probe_slots[_w],
// include/vigpath.h): the same persistent grid and access shape as
// nat_classify64 -- 4 blocks of 256 threads per CU (or one of 1024 threads,
// as nat_classify64w; or two of 512), each block a contiguous
// range of 64-slot tiles, its four waves interleaved over it, every load and
// store instruction 1 KiB contiguous through a buffer resource, the tile
// kernels' cache policy (kTilePolicy, vp_device.h: nt loads, sc1 nt stores; or
// the pair vp_probe_slots_p is given) -- with none of its work: each slot is read
// and (store != 0) written back in place. bench.py times it on the box it
// measures the classify kernel on, so the kernel's distance from the fastest
// possible pass over its bytes is a driver-measured number.
// (tools/slot_probe.hip is the stand-alone form with more variants.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "vp_device.h"
#include "vp_internal.h"

namespace vp {

typedef unsigned v4u __attribute__((ext_vector_type(4)));

// N = 16-byte chunks per slot; ST: store the slot back; W waves per block
// (4: nat_classify64's four 256-thread blocks per CU; 16: nat_classify64w's
// one 1024-thread block; 8: two 512-thread waves per SIMD)
// (split: as the 1024-thread vignat tiles, tile_split(), vp_internal.h)
// LP, SP: the cache policy of the loads and of the stores (the aux bits of
// the buffer instructions, vp_device.h; the default is the tile kernels')
template <uint32_t N, bool ST, uint32_t W = 4, int LP = policy_ld(kTilePolicy),
          int SP = policy_st(kTilePolicy)>
__global__ __launch_bounds__(64 * W, 16 / W) void probe_slots(uint4 *buf, uint32_t tiles,
                                                             uint32_t *sink, uint32_t split) {
  const uint32_t lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t per_b = (tiles + gridDim.x - 1) / gridDim.x;
  const uint32_t ks = W == 16 && (split == 2 || split == 4) ? split : 1u;
  const uint32_t tstep = W / ks, per_s = (per_b + ks - 1) / ks, sub = wv / tstep;
  const uint32_t tend = min(tiles, blockIdx.x * per_b + min(per_b, (sub + 1) * per_s));
  v4u acc = {0, 0, 0, 0};
  for (uint32_t tile = blockIdx.x * per_b + sub * per_s + (wv - sub * tstep); tile < tend;
       tile += tstep) {
    uint4 *g = buf + (size_t)tile * 64 * N;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(g, 0, 64 * N * 16, 0x00020000);
    v4u d[N];
#pragma unroll
    for (uint32_t j = 0; j < N; j++)
      d[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((64 * j + lane) * 16), 0, LP);
#pragma unroll
    for (uint32_t j = 0; j < N; j++) acc += d[j];
    if constexpr (ST) {
#pragma unroll
      for (uint32_t j = 0; j < N; j++)  // (the bytes as read: the buffer is unchanged)
        __builtin_amdgcn_raw_buffer_store_b128(d[j], rs, (int)((64 * j + lane) * 16), 0, SP);
    }
  }
  // (keeps the loads; never true for a buffer the caller filled with frames)
  if (acc.x == 0x9E3779B9u && acc.y == 0x7F4A7C15u) sink[0] = acc.z;
}

}  // namespace vp

using namespace vp;

typedef void (*ProbeKernel)(uint4 *, uint32_t, uint32_t *, uint32_t);
template <uint32_t W>
static ProbeKernel probe_kernel(uint32_t slot, int store) {
  return slot == 64 ? (store ? probe_slots<4, true, W> : probe_slots<4, false, W>)
                    : (store ? probe_slots<8, true, W> : probe_slots<8, false, W>);
}

// The policy ladder's kernels (vp_probe_slots_p): 64-byte slots, 4 or 16
// waves per block. (Without stores one instance per load policy.)
template <uint32_t W, int LP>
static ProbeKernel probe_kernel_sp(int store, int sp) {
  if (!store) return probe_slots<4, false, W, LP, 0>;
  return sp == kAuxSc1             ? probe_slots<4, true, W, LP, kAuxSc1>
         : sp == (kAuxSc1 | kAuxNt) ? probe_slots<4, true, W, LP, kAuxSc1 | kAuxNt>
         : sp == kAuxNt             ? probe_slots<4, true, W, LP, kAuxNt>
                                    : probe_slots<4, true, W, LP, 0>;
}
template <uint32_t W>
static ProbeKernel probe_kernel_lp(int store, int lp, int sp) {
  return lp == 0        ? probe_kernel_sp<W, 0>(store, sp)
         : lp == kAuxNt ? probe_kernel_sp<W, kAuxNt>(store, sp)
         : lp == kAuxSc1 ? probe_kernel_sp<W, kAuxSc1>(store, sp)
                         : probe_kernel_sp<W, kAuxSc0 | kAuxSc1>(store, sp);
}

extern "C" int vp_probe_slots_p(void *frames, uint32_t n, uint32_t slot, int store, int waves,
                                int load_policy, int store_policy, int reps, float *ms) {
  if (!frames || !ms || reps < 1 || (n & 63) || n == 0 || (slot != 64 && slot != 128) ||
      ((uintptr_t)frames & 15) || (waves != 4 && waves != 8 && waves != 12 && waves != 16))
    return VP_EINVAL;
  const int lp = load_policy, sp = store_policy;
  if ((lp != 0 && lp != kAuxNt && lp != kAuxSc1 && lp != (kAuxSc0 | kAuxSc1)) ||
      (sp != 0 && sp != kAuxNt && sp != kAuxSc1 && sp != (kAuxSc1 | kAuxNt)))
    return VP_EINVAL;
  const bool dflt = lp == policy_ld(kTilePolicy) && sp == policy_st(kTilePolicy);
  // (other policies: the ladder's shapes only)
  if (!dflt && (slot != 64 || (waves != 4 && waves != 16))) return VP_EINVAL;
  const ProbeKernel k = !dflt         ? (waves == 16 ? probe_kernel_lp<16>(store, lp, sp)
                                                     : probe_kernel_lp<4>(store, lp, sp))
                        : waves == 16 ? probe_kernel<16>(slot, store)
                        : waves == 12 ? probe_kernel<12>(slot, store)
                        : waves == 8  ? probe_kernel<8>(slot, store)
                                      : probe_kernel<4>(slot, store);
  const int threads = 64 * waves, cap = std::max(1, 16 / waves);  // blocks per CU at most
  int dev = 0, cus = 0, per = 0;
  VP_HIP(hipGetDevice(&dev));
  VP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  VP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void *)k, threads, 0));
  const uint32_t grid = (uint32_t)(cus * (per > cap ? cap : per < 1 ? 1 : per));
  const uint32_t split = tile_split();
  hipStream_t s = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  uint32_t *sink = nullptr;
  int rc = 0;
  float t = 0.f;
  auto fail = [&](hipError_t e, int line) { return hip_fail(e, "vp_probe_slots", __FILE__, line); };
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) != hipSuccess) return fail(e, __LINE__);
  if ((e = hipEventCreate(&a)) != hipSuccess || (e = hipEventCreate(&b)) != hipSuccess ||
      (e = hipMalloc((void **)&sink, 16)) != hipSuccess) {
    rc = fail(e, __LINE__);
    goto out;
  }
  for (int i = 0; i < 2; i++) k<<<grid, threads, 0, s>>>((uint4 *)frames, n / 64, sink, split);
  // each launch timed by its own dispatch's timestamps, as the classify
  // kernel is (launch_timed, vp_internal.h)
  for (int i = 0; i < reps; i++) {
    float one = 0.f;
    if ((e = launch_timed(k, dim3(grid), dim3(threads), s, a, b, (uint4 *)frames, n / 64,
                          sink, split)) != hipSuccess ||
        (e = hipEventSynchronize(b)) != hipSuccess ||
        (e = hipEventElapsedTime(&one, a, b)) != hipSuccess) {
      rc = fail(e, __LINE__);
      goto out;
    }
    t += one;
  }
  *ms = t / (float)reps;
out:
  if (s) hipStreamSynchronize(s);
  if (sink) hipFree(sink);
  if (a) hipEventDestroy(a);
  if (b) hipEventDestroy(b);
  if (s) hipStreamDestroy(s);
  return rc;
}

extern "C" int vp_probe_slots_w(void *frames, uint32_t n, uint32_t slot, int store, int waves,
                                int reps, float *ms) {
  return vp_probe_slots_p(frames, n, slot, store, waves, policy_ld(kTilePolicy),
                          policy_st(kTilePolicy), reps, ms);
}

extern "C" int vp_probe_slots(void *frames, uint32_t n, uint32_t slot, int store, int reps,
                              float *ms) {
  return vp_probe_slots_w(frames, n, slot, store, 4, reps, ms);
}
