// laser_amd/csrc/capi_internal.h -- what the host-side translation units of liblaser_hip.so share: capi.cpp (the extern "C" boundary),
// gemm_route.cpp (which kernel family runs a GEMM), prepack.cpp (pre-packed operands), sharded.cpp, foreach.cpp.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>

#include "../../include/laser_hip.h"
#include "common.h"

namespace laser_hip {
// ---- errors and initialisation (capi.cpp) ----
// set the thread-local error message (printf-style) and return `code`
int fail(int code, const char *fmt, ...);
// the same with a message of any length (a compiler log)
int fail_text(int code, const std::string &text);
int ensure_init();
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      const char *why_ = asm_error_detail();                                                  \
      return fail(LASER_HIP_E_HIP, "%s failed: %s%s%s (%s:%d)", #expr, hipGetErrorString(e_), \
                  why_[0] ? ": " : "", why_, __FILE__, __LINE__);                             \
    }                                                                                         \
  } while (0)
extern std::mutex g_mu;  // guards initialisation and the registries (pre-pack panel cache, storage free list)

// ---- run-time knobs (include/laser_hip.h documents each under its option name) ----
struct Context {
  std::atomic<bool> ready{false};  // read lock-free on every call, written once under g_mu
  int device = -1;
  std::string arch;
  // set by one thread, read by every call on every thread -> relaxed atomics (a knob flipped while a call is in flight applies to
  // that call or the next, never tears)
  std::atomic<int> float_mode{LASER_HIP_F32_LASER_ORDER};
  std::atomic<int> f32_cfg{-1};
  std::atomic<bool> f64_mfma{true}, i32_mfma{true}, i64_mfma{true}, narrow_mfma{true};
  std::atomic<bool> zc_poll{true};           // "zero_copy_poll"
  std::atomic<bool> host_pipeline_2d{true};
  std::atomic<int> slice_parallel_min{2};
  std::atomic<int64_t> slice_parallel_tiles{0};
  std::atomic<bool> slice_parallel{true}, skinny{true}, conv_implicit{true};
  std::atomic<int> shard_devices{1};      // laser_hip_set_shard_devices
};
extern Context g_ctx;
inline bool laser_order_now() { return g_ctx.float_mode == LASER_HIP_F32_LASER_ORDER; }
int f32_cfg_now();  // the f32 tile configuration pinned for this thread's launches (-1 = none: the heuristic and every kernel family)
extern std::atomic<int> g_last_narrow_mfma;  // gemm_route.cpp

// The device the host-pointer entry points use ON THIS THREAD (-1 = the library's default device).  The sharded
// host path sets it in its per-GPU worker threads.
void api_set_thread_device(int device);
int api_thread_device();
// Tile-configuration override for the f32 launches made BY THIS THREAD (-2 = none: the process-wide setting applies).
// (Forces the compiler-scheduled kernel of that configuration: tests and tuning sweeps.)
void api_set_thread_f32_config(int cfg);
// Tile-class pin of the hand-scheduled f32 kernels for the launches made BY THIS THREAD (option "asm_tile"'s values; -2 = none).
void api_set_thread_asm_tile(int tile_class);

// ---- host-pointer entry points (capi.cpp) ----
// RAII guard of a host-pointer entry point: makes its device current for the calling thread (another host thread
// using the host-pointer API would otherwise run on device 0 with this device's buffers), serialises on that device's
// mutex and makes the device's cached scratch (scratch_get) this thread's.
struct DeviceCtx;
struct HostCall {
  int rc = LASER_HIP_OK;
  DeviceCtx *d = nullptr;
  DeviceCtx *prev = nullptr;
  int caller_dev = -1;  // the caller's current device, restored on exit: an application thread driving another GPU must
                        // not find itself on the library's device after a host-pointer call
  HostCall();
  ~HostCall();
  HostCall(const HostCall &) = delete;
  HostCall &operator=(const HostCall &) = delete;
};
// the device's cached scratch buffer of role `slot`, grown to `bytes` (valid while a HostCall guard is alive)
int scratch_get(int slot, size_t bytes, void **out);

// Lowest / highest element offset touched by an R x C strided view (strides may be negative).
inline void view_span(int64_t R, int64_t C, int64_t rs, int64_t cs, int64_t *lo, int64_t *hi) {
  const int64_t r = (R - 1) * rs, c = (C - 1) * cs;
  *lo = std::min<int64_t>(0, r) + std::min<int64_t>(0, c);
  *hi = std::max<int64_t>(0, r) + std::max<int64_t>(0, c);
}
template <typename T>
GemmArgs<T> make_args(int64_t batch, int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA,
                      int64_t csA, int64_t bsA, const T *B, int64_t rsB, int64_t csB, int64_t bsB, T beta,
                      T *C, int64_t rsC, int64_t csC, int64_t bsC) {
  GemmArgs<T> a;
  memset(&a, 0, sizeof a);
  a.M = M; a.N = N; a.K = K;
  a.alpha = alpha; a.beta = beta;
  a.A = A; a.rsA = rsA; a.csA = csA; a.bsA = bsA;
  a.B = B; a.rsB = rsB; a.csB = csB; a.bsB = bsB;
  a.C = C; a.rsC = rsC; a.csC = csC; a.bsC = bsC;
  a.Mext = M; a.Next = N; a.Kext = K;
  a.batch = (int32_t)batch;
  return a;
}

// ---- gemm_route.cpp: which kernel family runs a problem on a stream (float, double, int32_t, int64_t, int8_t, int16_t) ----
template <typename T>
hipError_t run_gemm(const GemmArgs<T> &a, hipStream_t s);
// the small-matrix kernel on operands that live in host memory mapped into the device (gemm_host's zero-copy staging)
template <typename T>
hipError_t run_small_mapped(const GemmArgs<T> &a, hipStream_t s);

// ---- prepack.cpp: pre-packed operands (the same six element types) ----
template <typename T>
int64_t prepack_bytes(bool is_a, int64_t M, int64_t N, int64_t K);
template <typename T>
int prepack_dev(bool is_a, void *d_dst, int64_t M, int64_t N, int64_t K, const T *src, int64_t rs, int64_t cs, void *stream);
template <typename T>
int prepack_host(bool is_a, void *dst, int64_t M, int64_t N, int64_t K, const T *src, int64_t rs, int64_t cs);
template <typename T>
int packed_dev(int64_t M, int64_t N, int64_t K, T alpha, const void *dA, const void *dB, T beta, T *dC, int64_t rsC, int64_t csC,
               void *stream);
template <typename T>
int packed_host(int64_t M, int64_t N, int64_t K, T alpha, const void *pA, const void *pB, T beta, T *C, int64_t rsC, int64_t csC);
int prepack_release(void *packed);
void panel_cache_clear_locked();  // (g_mu held) laser_hip_finalize: every cached device panel goes

// ---- sharded.cpp ----
// ranks of the RCCL communicator the last GATHER_RCCL call used (ncclCommCount); 0 = none yet
int64_t api_shard_rccl_ranks();
// host-pointer gemm_strided cut into one row range per GPU (ndev <= 0: every visible GPU)
template <typename T>
int api_sharded_host(int ndev, int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA, int64_t csA, const T *B,
                     int64_t rsB, int64_t csB, T beta, T *C, int64_t rsC, int64_t csC);
// ---- foreach.cpp: hiprtc compiles made in this process, and the kernel variant of the last laser_hip_foreach_dev launch ----
int64_t api_foreach_compiles();
int api_last_foreach_variant();
}  // namespace laser_hip
