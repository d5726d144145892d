// laser_amd/csrc/capi.cpp -- the extern "C" boundary of liblaser_hip.so (include/laser_hip.h).
//
// Host-pointer entry points reproduce Laser's blocking call semantics (caller owns every pointer,
// the call returns when C is final); `_dev` entry points are the device-resident, stream-ordered
// path that benchmarks and multi-GPU code use.  No CPU compute fallback exists anywhere in this
// library: without a usable gfx950 device every compute entry point returns LASER_HIP_E_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <atomic>
#include <chrono>
#include <mutex>
#include <type_traits>
#include <thread>
#include <string>
#include <unordered_map>
#include <vector>

#include "capi_internal.h"
#include "../../include/laser_hip_select.h"
#include "normal_core.h"
#include "philox_core.h"
#include "random_plan.h"
#include "sampler_plan.h"
#include "scan_plan.h"
#include "bias_grad_plan.h"
#include "embedding_plan.h"
#include "optim_plan.h"
#include "layer_norm_plan.h"
#include "select_plan.h"
#include "attention_plan.h"
#include "softmax_axis_plan.h"
#include "softmax_rows_plan.h"

using namespace laser_hip;

namespace laser_hip {
std::mutex g_mu;
Context g_ctx;
static thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
int fail_text(int code, const std::string &text) {
  g_err = text;
  return code;
}

// Per-DEVICE state of the host-pointer paths: cached scratch (one growing buffer per role), the streams of the
// upload / compute / download pipeline, and a mutex that serialises the host-pointer calls using THIS device.  One
// process may drive every GPU of the node (the sharded entry points run one host thread per device), so none of this
// is per process.
struct DeviceCtx {
  int device = -1;
  std::mutex mu;
  hipStream_t s_up = nullptr, s_comp = nullptr, s_down = nullptr;
  void *scratch[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  size_t scratch_sz[6] = {0, 0, 0, 0, 0, 0};
  uint32_t zc_seq = 0;  // sequence number of the zero-copy path's completion flags (never 0 in a flag)
  void *zc = nullptr;  // pinned host buffer mapped into the device: zero-copy staging of the small-problem host path
  size_t zc_sz = 0;
};
namespace {
constexpr int kMaxDevices = 16;
DeviceCtx g_dev[kMaxDevices];
// The device a host-pointer call on this thread uses: -1 = the library's default device (laser_hip_init); the
// sharded entry points set it in their per-device worker threads.
thread_local int tl_device = -1;
thread_local int tl_f32_cfg = -2;  // per-thread override of g_ctx.f32_cfg (-2 = none), api_set_thread_f32_config
thread_local DeviceCtx *tl_dev = nullptr;  // valid while a HostCall guard is alive

int ensure_init_locked(int device) {
  if (g_ctx.ready && (device < 0 || device == g_ctx.device)) return LASER_HIP_OK;
  // (a later init with another ordinal only moves the DEFAULT device of the host-pointer entry points: scratch,
  // streams and kernel attributes are kept per device, nothing of the previous device is reused)
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(LASER_HIP_E_NODEVICE, "no HIP device available (%s)",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0) {
    HIP_TRY(hipGetDevice(&device));
  } else {
    if (device >= n || device >= kMaxDevices) return fail(LASER_HIP_E_INVALID, "device %d out of range (%d devices)", device, n);
    HIP_TRY(hipSetDevice(device));
  }
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  std::string arch = prop.gcnArchName;
  // gcnArchName looks like "gfx950:sramecc+:xnack-"; this library carries gfx950 code objects only
  if (arch.rfind("gfx950", 0) != 0)
    return fail(LASER_HIP_E_NODEVICE, "device %d is %s; liblaser_hip is built for gfx950 (MI355X) only",
                device, arch.c_str());
  g_ctx.arch = arch.substr(0, arch.find(':'));
  g_ctx.device = device;
  g_ctx.ready = true;
  return LASER_HIP_OK;
}
}  // namespace

int f32_cfg_now() { return tl_f32_cfg >= -1 ? tl_f32_cfg : g_ctx.f32_cfg.load(); }
void api_set_thread_device(int device) { tl_device = device; }
void api_set_thread_f32_config(int cfg) { tl_f32_cfg = cfg; }
void api_set_thread_asm_tile(int tile_class) { asm_set_thread_tile(tile_class); }
int api_thread_device() { return tl_device; }

int ensure_init() {
  if (g_ctx.ready) return LASER_HIP_OK;
  std::lock_guard<std::mutex> lk(g_mu);
  return ensure_init_locked(-1);
}

HostCall::HostCall() {
  if (hipGetDevice(&caller_dev) != hipSuccess) caller_dev = -1;
  const int dev = tl_device >= 0 ? tl_device : g_ctx.device;
  if (dev < 0 || dev >= kMaxDevices) {
    rc = fail(LASER_HIP_E_INVALID, "device %d outside 0..%d", dev, kMaxDevices - 1);
    return;
  }
  const hipError_t e = hipSetDevice(dev);
  if (e != hipSuccess) {
    rc = fail(LASER_HIP_E_HIP, "hipSetDevice(%d): %s", dev, hipGetErrorString(e));
    return;
  }
  d = &g_dev[dev];
  d->mu.lock();
  d->device = dev;
  prev = tl_dev;
  tl_dev = d;
}
HostCall::~HostCall() {
  if (d) {
    tl_dev = prev;
    d->mu.unlock();
  }
  if (caller_dev >= 0) (void)hipSetDevice(caller_dev);
}

int scratch_get(int slot, size_t bytes, void **out) {
  DeviceCtx &D = *tl_dev;
  if (bytes == 0) bytes = 16;
  if (D.scratch_sz[slot] < bytes) {
    if (D.scratch[slot]) HIP_TRY(hipFree(D.scratch[slot]));
    D.scratch[slot] = nullptr;
    D.scratch_sz[slot] = 0;
    size_t want = bytes + bytes / 8;  // a little headroom so slowly growing sizes do not thrash
    HIP_TRY(hipMalloc(&D.scratch[slot], want));
    D.scratch_sz[slot] = want;
  }
  *out = D.scratch[slot];
  return LASER_HIP_OK;
}
}  // namespace laser_hip

namespace {

// Pinned, device-mapped host staging for small host-pointer problems (<= kZeroCopyMax bytes of operands): the kernel
// reads A and B from it and writes C into it across PCIe -- one round trip, because the small-matrix kernel issues all
// of a block's loads up front -- instead of three blocking hipMemcpy calls (~10-15 us each for 64 KiB).
constexpr size_t kZeroCopyMax = (size_t)1 << 20;
int zero_copy_get(size_t bytes, void **out) {
  DeviceCtx &D = *tl_dev;
  if (D.zc_sz < bytes) {
    if (D.zc) HIP_TRY(hipHostFree(D.zc));
    D.zc = nullptr;
    D.zc_sz = 0;
    const size_t want = std::max<size_t>(bytes, (size_t)256 << 10);
    HIP_TRY(hipHostMalloc(&D.zc, want, hipHostMallocDefault));
    memset(D.zc, 0, want);  // completion flags live here: a fresh buffer must not hold a value that looks like a sequence number
    D.zc_sz = want;
  }
  *out = D.zc;
  return LASER_HIP_OK;
}

int pipeline_streams() {
  DeviceCtx &D = *tl_dev;
  if (!D.s_up) {
    HIP_TRY(hipStreamCreateWithFlags(&D.s_up, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&D.s_comp, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&D.s_down, hipStreamNonBlocking));
  }
  return LASER_HIP_OK;
}


// Fused epilogue request (device pointers): bias == nullptr and act == 0 means "plain gemm_strided".
template <typename T>
struct Epi {
  const T *bias = nullptr;
  int64_t rs = 0, cs = 0, bs = 0;
  int act = 0;
  int pre = 0;     // fused prologue: bit 0 = relu on A's elements, bit 1 = relu on B's (LASER_HIP_PRE_RELU_A / _B >> 8)
  bool on() const { return bias != nullptr || act != 0 || pre != 0; }
};
// the `activation` argument of the _ex_ entry points: low byte = activation, bits 8 / 9 = fused prologue
template <typename T>
Epi<T> make_epi(const T *bias, int64_t rs, int64_t cs, int act) {
  Epi<T> e;
  e.bias = bias; e.rs = rs; e.cs = cs;
  e.act = act & 0xff;
  e.pre = (act >> 8) & 3;
  if (act & ~0x3ff) e.act = -1;      // unknown bits: rejected by epi_check
  return e;
}
template <typename T>
int epi_check(const Epi<T> *e) {
  if (!e) return LASER_HIP_OK;
  if (e->act < LASER_HIP_ACT_NONE || e->act > LASER_HIP_ACT_SIGMOID) return fail(LASER_HIP_E_INVALID, "unknown activation %d", e->act);
  if (!std::is_floating_point<T>::value) return fail(LASER_HIP_E_INVALID, "fused epilogue is float32/float64 only");
  if (std::is_same<T, double>::value && !g_ctx.f64_mfma && (e->bias || e->act))
    return fail(LASER_HIP_E_INVALID, "fused epilogue needs the f64 MFMA kernel (laser_hip_set_option(\"f64_mfma\", 1))");
  return LASER_HIP_OK;
}
template <typename T>
void epi_apply(GemmArgs<T> &a, const Epi<T> *e) {
  if (!e) return;
  a.bias = e->bias; a.rsBias = e->rs; a.csBias = e->cs; a.bsBias = e->bs; a.act = e->act;
  a.preA = e->pre & 1; a.preB = (e->pre >> 1) & 1;
}

template <typename T>
int gemm_dev(int64_t batch, int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA, int64_t csA,
             int64_t bsA, const T *B, int64_t rsB, int64_t csB, int64_t bsB, T beta, T *C, int64_t rsC,
             int64_t csC, int64_t bsC, void *stream, const Epi<T> *epi = nullptr) {
  if (M < 0 || N < 0 || K < 0 || batch < 0) return fail(LASER_HIP_E_INVALID, "negative dimension");
  if (int rc = epi_check<T>(epi)) return rc;
  if (int rc = ensure_init()) return rc;
  // K == 0: the reference's pc loop never runs, C is left untouched even if beta != 1 (gemm.nim:150)
  if (M == 0 || N == 0 || K == 0 || batch == 0) return LASER_HIP_OK;
  if (!A || !B || !C) return fail(LASER_HIP_E_INVALID, "null operand pointer");
  if (batch > 65535) return fail(LASER_HIP_E_INVALID, "batch > 65535");
  GemmArgs<T> a = make_args<T>(batch, M, N, K, alpha, A, rsA, csA, bsA, B, rsB, csB, bsB, beta, C, rsC, csC, bsC);
  epi_apply(a, epi);
  HIP_TRY(run_gemm<T>(a, (hipStream_t)stream));
  return LASER_HIP_OK;
}

// Pipelined host path (see gemm_host): row panels of A (R rows) x column panels of B (W columns; W >= N is one column
// panel).  The uploads grow the computable region as a square -- B_0, A_0, then whichever of the next A row panel / B
// column panel keeps (rows up)/M ~ (cols up)/N -- so the first tile multiplies after one panel of each.  Every upload
// releases a row or column STRIP of C as one launch (the new row panel x every column already up, or the new column
// panel x every row already up: 12 launches at 8192^3, growing with what is on the device -- one launch per TILE left
// three quarters of the chip idle, 17.7 ms vs 15.5 ms for row panels only), and a helper thread copies every finished
// strip back while later panels are still arriving (PCIe is full duplex).  Elements of C are independent and each is ONE
// chain over all of K, so the arithmetic is unchanged.  With one column panel all of B goes first and each A row panel
// releases a full-width strip.
// Row panels of A and C and full-width strips are span copies with the caller's strides: the row panels must not
// overlap, strides may otherwise be negative or non-unit.  More than one column panel needs unit column strides: the
// column panels of B and the partial-width strips of C are pitched 2-D copies.  dA0/dB0/dC0 are the device addresses of
// element (0,0) of each operand inside the cached scratch.
template <typename T>
int gemm_host_pipelined(int64_t M, int64_t N, int64_t K, int64_t R, int64_t W, T alpha, const T *A, int64_t rsA,
                        int64_t csA, const T *B, int64_t rsB, int64_t csB, T beta, T *C, int64_t rsC, int64_t csC,
                        const T *dA0, const T *dB0, T *dC0, bool c_up) {
  if (int rc = pipeline_streams()) return rc;
  DeviceCtx &D = *tl_dev;
  const int nI = (int)((M + R - 1) / R), nJ = (int)((N + W - 1) / W);
  const int64_t ca = (K - 1) * csA, cc = (N - 1) * csC;
  // rows [r0, r1) of A or C (c = offset of the last column from the first) as one span copy between element-(0,0) pointers
  auto copy_rows = [](T *dst, const T *src, int64_t r0, int64_t r1, int64_t rs, int64_t c, hipMemcpyKind kind, hipStream_t s) {
    const int64_t lo = r0 * rs + std::min<int64_t>(0, c), hi = (r1 - 1) * rs + std::max<int64_t>(0, c);
    return hipMemcpyAsync(dst + lo, src + lo, (size_t)(hi - lo + 1) * sizeof(T), kind, s);
  };
  struct Strip { int64_t r0, r1, c0, c1; hipEvent_t done; };
  std::vector<hipEvent_t> events;  // every event made here; finish destroys them
  std::mutex qm;
  std::condition_variable qcv;
  std::deque<Strip> queue;
  bool closed = false;
  hipError_t down_err = hipSuccess;
  const int device = D.device;
  const hipStream_t s_down = D.s_down;
  std::thread downloader([&]() {
    (void)hipSetDevice(device);
    for (;;) {
      Strip t;
      {
        std::unique_lock<std::mutex> lk(qm);
        qcv.wait(lk, [&] { return !queue.empty() || closed; });
        if (queue.empty()) return;
        t = queue.front();
        queue.pop_front();
      }
      // (asynchronous copy on its own stream + synchronise, not a blocking hipMemcpy: beside the uploads of s_up the
      // blocking form gets 26 GB/s each way, this one 46 -- scripts/pcie_probe.py, pageable memory)
      hipError_t e = hipEventSynchronize(t.done);
      if (e == hipSuccess) {
        if (t.c0 == 0 && t.c1 == N)
          e = copy_rows(C, dC0, t.r0, t.r1, rsC, cc, hipMemcpyDeviceToHost, s_down);
        else
          e = hipMemcpy2DAsync(C + t.r0 * rsC + t.c0, (size_t)rsC * sizeof(T), dC0 + t.r0 * rsC + t.c0, (size_t)rsC * sizeof(T),
                               (size_t)(t.c1 - t.c0) * sizeof(T), (size_t)(t.r1 - t.r0), hipMemcpyDeviceToHost, s_down);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(s_down);
      if (e != hipSuccess && down_err == hipSuccess) down_err = e;
    }
  });
  auto finish = [&]() {
    {
      std::lock_guard<std::mutex> lk(qm);
      closed = true;
    }
    qcv.notify_all();
    downloader.join();
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
  };
  auto new_event = [&](hipEvent_t *ev) {
    const hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) events.push_back(*ev);
    return e;
  };
#define PIPE_TRY(expr)                                                                                        \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess) {                                                                                   \
      finish();                                                                                               \
      (void)hipDeviceSynchronize();                                                                           \
      return fail(LASER_HIP_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    }                                                                                                         \
  } while (0)
  int a_up = 0, b_up = 0;
  while (a_up < nI || b_up < nJ) {
    // one upload: B first, then keep the uploaded fractions level (ties go to A: its panels are the cheaper, contiguous copies)
    const bool take_b = b_up < nJ && (a_up >= nI || b_up == 0 || (int64_t)b_up * nI < (int64_t)a_up * nJ);
    Strip t;
    if (take_b) {
      t.c0 = b_up * W; t.c1 = std::min<int64_t>(N, t.c0 + W);
      t.r0 = 0; t.r1 = std::min<int64_t>(M, a_up * R);
      if (nJ == 1) {  // all of B: its span, whatever its strides
        int64_t blo, bhi;
        view_span(K, N, rsB, csB, &blo, &bhi);
        PIPE_TRY(hipMemcpyAsync((T *)dB0 + blo, B + blo, (size_t)(bhi - blo + 1) * sizeof(T), hipMemcpyHostToDevice, D.s_up));
      } else {
        PIPE_TRY(hipMemcpy2DAsync((T *)dB0 + t.c0, (size_t)rsB * sizeof(T), B + t.c0, (size_t)rsB * sizeof(T), (size_t)(t.c1 - t.c0) * sizeof(T),
                                  (size_t)K, hipMemcpyHostToDevice, D.s_up));
      }
      b_up++;
    } else {  // a row panel of A, and of C when it is read
      t.r0 = a_up * R; t.r1 = std::min<int64_t>(M, t.r0 + R);
      t.c0 = 0; t.c1 = std::min<int64_t>(N, b_up * W);
      PIPE_TRY(copy_rows((T *)dA0, A, t.r0, t.r1, rsA, ca, hipMemcpyHostToDevice, D.s_up));
      if (c_up) PIPE_TRY(copy_rows(dC0, C, t.r0, t.r1, rsC, cc, hipMemcpyHostToDevice, D.s_up));
      a_up++;
    }
    if (t.r1 <= t.r0 || t.c1 <= t.c0) continue;  // the very first upload has no partner yet
    hipEvent_t up;
    PIPE_TRY(new_event(&up));
    PIPE_TRY(hipEventRecord(up, D.s_up));
    PIPE_TRY(hipStreamWaitEvent(D.s_comp, up, 0));  // s_up is in order: this event covers every earlier upload too
    GemmArgs<T> a = make_args<T>(1, t.r1 - t.r0, t.c1 - t.c0, K, alpha, dA0 + t.r0 * rsA, rsA, csA, 0, dB0 + t.c0 * csB, rsB, csB, 0,
                                 beta, dC0 + t.r0 * rsC + t.c0 * csC, rsC, csC, 0);
    PIPE_TRY(run_gemm<T>(a, D.s_comp));
    PIPE_TRY(new_event(&t.done));
    PIPE_TRY(hipEventRecord(t.done, D.s_comp));
    {
      std::lock_guard<std::mutex> lk(qm);
      queue.push_back(t);
    }
    qcv.notify_one();
  }
#undef PIPE_TRY
  finish();
  if (down_err != hipSuccess) return fail(LASER_HIP_E_HIP, "D2H of a C strip failed: %s", hipGetErrorString(down_err));
  return LASER_HIP_OK;
}

// Host-pointer gemm_strided: stage the touched span of each operand, run, copy the C span back.
template <typename T>
int gemm_host(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA, int64_t csA, const T *B,
              int64_t rsB, int64_t csB, T beta, T *C, int64_t rsC, int64_t csC, const Epi<T> *hepi = nullptr) {
  if (M < 0 || N < 0 || K < 0) return fail(LASER_HIP_E_INVALID, "negative dimension");
  if (int rc = epi_check<T>(hepi)) return rc;
  if (int rc = ensure_init()) return rc;
  if (M == 0 || N == 0 || K == 0) return LASER_HIP_OK;
  if (!A || !B || !C) return fail(LASER_HIP_E_INVALID, "null operand pointer");
  // laser_hip_set_shard_devices(n != 1): a large plain gemm_strided call is cut into row ranges over n GPUs (rows of
  // C are independent, gemm.nim:160-176, so the arithmetic is unchanged).  Not for calls that already ARE a shard
  // (tl_device set by the sharded entry point's worker thread) and not worth it below ~4 tile rows per GPU.
  if (sizeof(T) >= 4 && g_ctx.shard_devices != 1 && tl_device < 0 && !(hepi && hepi->on())) {   // (no sharded form for int8 / int16)
    int ndev = g_ctx.shard_devices;
    if (ndev <= 0 && hipGetDeviceCount(&ndev) != hipSuccess) ndev = 1;
    if (ndev > 1 && M >= (int64_t)1024 * ndev && (double)M * (double)N * (double)K >= 64.0 * 1024 * 1024 * 1024)
      return api_sharded_host<T>(ndev, M, N, K, alpha, A, rsA, csA, B, rsB, csB, beta, C, rsC, csC);
  }
  HostCall hc;
  if (hc.rc) return hc.rc;
  int64_t alo, ahi, blo, bhi, clo, chi;
  view_span(M, K, rsA, csA, &alo, &ahi);
  view_span(K, N, rsB, csB, &blo, &bhi);
  view_span(M, N, rsC, csC, &clo, &chi);
  const size_t an = (size_t)(ahi - alo + 1), bn = (size_t)(bhi - blo + 1), cn = (size_t)(chi - clo + 1);
  // small problems (BASELINE configs[0], fp32 128^3): zero-copy through the pinned staging buffer
  {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t ab = up(an * sizeof(T)), bb = up(bn * sizeof(T)), cb = up(cn * sizeof(T));
    const bool has_epi = hepi && hepi->on();
    if (!has_epi && f32_cfg_now() < 0 && ab + bb + cb <= kZeroCopyMax && gemm_small_takes((int)sizeof(T), M, N, K, 1, true) &&
        std::is_floating_point<T>::value) {
      // completion flags, one per workgroup (= per 32x32 / 16x16 block of C; at most 256 by the dispatch rule), behind C
      const int mb = sizeof(T) == 4 ? 32 : 16;
      const size_t nblk = (size_t)((M + mb - 1) / mb) * (size_t)((N + mb - 1) / mb);
      const size_t fb = up(nblk * sizeof(uint32_t));
      void *z;
      if (int rc = zero_copy_get(ab + bb + cb + fb, &z)) return rc;
      if (int rc = pipeline_streams()) return rc;
      T *hA = (T *)z, *hB = (T *)((char *)z + ab), *hC = (T *)((char *)z + ab + bb);
      volatile uint32_t *flags = (volatile uint32_t *)((char *)z + ab + bb + cb);
      // the flag words sit where an earlier call of another shape kept payload: a stale word that happens to equal this
      // call's sequence number would read as "block done" -- clear them before the launch
      for (size_t i = 0; i < nblk; i++) flags[i] = 0;
      memcpy(hA, A + alo, an * sizeof(T));
      memcpy(hB, B + blo, bn * sizeof(T));
      const bool c_in = (beta != (T)0) || cn != (size_t)M * (size_t)N;  // read, or a span with gaps that belong to the caller
      if (c_in) memcpy(hC, C + clo, cn * sizeof(T));
      GemmArgs<T> a = make_args<T>(1, M, N, K, alpha, hA - alo, rsA, csA, 0, hB - blo, rsB, csB, 0, beta, hC - clo, rsC, csC, 0);
      uint32_t seq = ++tl_dev->zc_seq;
      if (seq == 0) seq = ++tl_dev->zc_seq;  // flags hold the sequence number of the call that set them; 0 = never
      if (g_ctx.zc_poll) {
        a.done_flags = (uint32_t *)flags;
        a.done_seq = seq;
      }
      HIP_TRY(run_small_mapped<T>(a, tl_dev->s_comp));
      // Wait for the blocks' flags in mapped memory instead of synchronising the stream (the runtime's completion path
      // costs more than this kernel).  Bounded: after ~2 ms of polling fall back to the synchronise, which also reports
      // a failed launch.
      bool polled = false;
      if (g_ctx.zc_poll) {
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        size_t i = 0;
        for (unsigned spins = 0; i < nblk; spins++) {
          if (flags[i] == seq) { i++; continue; }
          if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() > t_end) break;
          __builtin_ia32_pause();
        }
        polled = i == nblk;
        std::atomic_thread_fence(std::memory_order_acquire);
      }
      if (!polled) HIP_TRY(hipStreamSynchronize(tl_dev->s_comp));
      memcpy(C + clo, hC, cn * sizeof(T));
      return LASER_HIP_OK;
    }
  }
  void *dA, *dB, *dC;
  if (int rc = scratch_get(0, an * sizeof(T), &dA)) return rc;
  if (int rc = scratch_get(1, bn * sizeof(T), &dB)) return rc;
  if (int rc = scratch_get(2, cn * sizeof(T), &dC)) return rc;
  // C must be uploaded when it is read (beta != 0) or when its span has gaps that belong to the
  // caller (so the copy-back restores them unchanged).  A dense C with beta == 0 is write-only.
  const bool c_dense = (cn == (size_t)M * (size_t)N);
  const bool c_up = (beta != (T)0 || !c_dense);
  const T *dA0 = (const T *)dA - alo, *dB0 = (const T *)dB - blo;
  T *dC0 = (T *)dC - clo;

  // Large problems: stream panels so PCIe and the kernel overlap (gemm_host_pipelined).  Row panels only need rows of A
  // and C that do not overlap.
  auto iabs = [](int64_t v) { return v < 0 ? -v : v; };
  const bool panels_disjoint = rsA > 0 && rsC > 0 && rsA >= iabs(csA) * (K - 1) + 1 && rsC >= iabs(csC) * (N - 1) + 1;
  // fused epilogue: hepi->bias is a HOST view here; its span goes to the device next to the operands
  Epi<T> depi;
  const bool fused = hepi && hepi->on();
  if (fused) {
    depi = *hepi;
    if (hepi->bias) {
      int64_t lo, hi;
      view_span(M, N, hepi->rs, hepi->cs, &lo, &hi);
      void *dbias;
      if (int rc = scratch_get(5, (size_t)(hi - lo + 1) * sizeof(T), &dbias)) return rc;
      HIP_TRY(hipMemcpy(dbias, hepi->bias + lo, (size_t)(hi - lo + 1) * sizeof(T), hipMemcpyHostToDevice));
      depi.bias = (const T *)dbias - lo;
    }
  }
  const int64_t R = std::max<int64_t>(256, (M / 8 + 255) / 256 * 256);  // ~8 row panels of whole 256-row tiles
  const int64_t W = std::max<int64_t>(256, (N / 4 + 255) / 256 * 256);  // ~4 column panels of whole 256-column tiles
  // both operands and C row-major-like, and big enough that B's upload is worth hiding: column panels as well.  Pinned
  // (or registered) B and C only: their column panels / strips move as pitched 2-D copies, which are DMA transfers from
  // pinned memory but row-by-row staging from pageable memory (8192^3: 15.0 ms in one harness, 23 ms in another, against
  // 15.7 ms for row panels only -- profiles/r02/host_pipeline_v2.jsonl, configs_v19.jsonl)
  auto pinned = [](const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
      (void)hipGetLastError();  // an ordinary pageable pointer is "invalid value" to the runtime: not an error here
      return false;
    }
    return at.type == hipMemoryTypeHost;
  };
  if (!fused && g_ctx.host_pipeline_2d && pinned(B) && pinned(C) && csA == 1 && csB == 1 && csC == 1 && rsA >= K && rsB >= N && rsC >= N && M >= 2048 &&
      N >= 2048 && bn * sizeof(T) >= ((size_t)32 << 20) && (an + bn + cn) * sizeof(T) >= ((size_t)128 << 20))
    return gemm_host_pipelined<T>(M, N, K, R, W, alpha, A, rsA, csA, B, rsB, csB, beta, C, rsC, csC, dA0, dB0, dC0, c_up);
  if (!fused && panels_disjoint && M >= 2048 && (an + bn + cn) * sizeof(T) >= ((size_t)64 << 20))  // row panels only
    return gemm_host_pipelined<T>(M, N, K, R, N, alpha, A, rsA, csA, B, rsB, csB, beta, C, rsC, csC, dA0, dB0, dC0, c_up);

  HIP_TRY(hipMemcpy(dA, A + alo, an * sizeof(T), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dB, B + blo, bn * sizeof(T), hipMemcpyHostToDevice));
  if (c_up) HIP_TRY(hipMemcpy(dC, C + clo, cn * sizeof(T), hipMemcpyHostToDevice));
  GemmArgs<T> a = make_args<T>(1, M, N, K, alpha, dA0, rsA, csA, 0, dB0, rsB, csB, 0, beta, dC0, rsC, csC, 0);
  if (fused) epi_apply(a, &depi);
  HIP_TRY(run_gemm<T>(a, nullptr));
  HIP_TRY(hipMemcpy(C + clo, dC, cn * sizeof(T), hipMemcpyDeviceToHost));  // synchronises
  return LASER_HIP_OK;
}


// device tensor storage: live blocks (ptr -> rounded size) and the free list keyed by size
constexpr size_t kStorageCacheMax = (size_t)32 << 30;
// live blocks: ptr -> key; free list keyed by the same key = rounded size | device ordinal << 56 (a block is only
// ever handed back to a caller on the device it was allocated on)
std::unordered_map<void *, size_t> g_live_storage;
// A cached block remembers the stream it was allocated on and an event recorded on that stream when it was freed: whoever
// takes the block next is ordered behind that event ON THE DEVICE (nothing, on the same stream), never by a host wait.
// done == nullptr: the event could not be made or recorded -- the taker falls back to hipDeviceSynchronize.
struct FreeBlock {
  void *p;
  hipStream_t owner;
  hipEvent_t done;
};
std::unordered_map<void *, hipStream_t> g_storage_owner;
std::unordered_map<size_t, std::vector<FreeBlock>> g_free_storage;
inline void free_block_release(const FreeBlock &b) {
  if (b.done) (void)hipEventDestroy(b.done);
  (void)hipFree(b.p);
  g_live_storage.erase(b.p);
  g_storage_owner.erase(b.p);
}
inline size_t storage_key(size_t rounded, int dev) { return rounded | ((size_t)(dev & 0xff) << 56); }
inline size_t storage_size(size_t key) { return key & (((size_t)1 << 56) - 1); }
size_t g_free_storage_bytes = 0;
void storage_trim() {
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto &kv : g_free_storage)
    for (const FreeBlock &b : kv.second) free_block_release(b);
  g_free_storage.clear();
  g_free_storage_bytes = 0;
}

// ---- transposes ------------------------------------------------------------------------------------
int transpose_host(void *dst, const void *src, int64_t N, int64_t NR, int64_t NC, int elem) {
  if (N < 0 || NR < 0 || NC < 0) return fail(LASER_HIP_E_INVALID, "negative dimension");
  if (int rc = ensure_init()) return rc;
  const size_t bytes = (size_t)N * NR * NC * elem;
  if (bytes == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "null pointer");
  HostCall hc;
  if (hc.rc) return hc.rc;
  void *ds, *dd;
  if (int rc = scratch_get(0, bytes, &ds)) return rc;
  if (int rc = scratch_get(2, bytes, &dd)) return rc;
  HIP_TRY(hipMemcpy(ds, src, bytes, hipMemcpyHostToDevice));
  HIP_TRY(launch_transpose_batched(dd, ds, N, NR, NC, elem, nullptr));
  HIP_TRY(hipMemcpy(dst, dd, bytes, hipMemcpyDeviceToHost));
  return LASER_HIP_OK;
}

// ---- convolution -------------------------------------------------------------------------------------
void out_hw(int64_t iH, int64_t iW, int64_t kH, int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW,
            int64_t *oH, int64_t *oW) {
  // conv2d_common.nim:43-44 with dilation 1
  *oH = 1 + (iH + 2 * pH - kH) / sH;
  *oW = 1 + (iW + 2 * pW - kW) / sW;
}

int conv_check(int64_t iN, int64_t iC, int64_t iH, int64_t iW, int64_t c_out, int64_t c_in, int64_t kH, int64_t kW,
               int64_t pH, int64_t pW, int64_t sH, int64_t sW) {
  if (iN < 0 || iC <= 0 || iH <= 0 || iW <= 0 || c_out <= 0 || kH <= 0 || kW <= 0 || pH < 0 || pW < 0)
    return fail(LASER_HIP_E_INVALID, "bad convolution shape");
  if (c_in != iC) return fail(LASER_HIP_E_INVALID, "kernel c_in (%lld) != input channels (%lld)", (long long)c_in, (long long)iC);
  // conv2d_common.nim:33-34: doAssert 0 < sH and sH < iH (same for W)
  if (!(0 < sH && sH < iH && 0 < sW && sW < iW)) return fail(LASER_HIP_E_INVALID, "strides must satisfy 0 < s < input size");
  if (iH + 2 * pH < kH || iW + 2 * pW < kW) return fail(LASER_HIP_E_INVALID, "kernel larger than padded input");
  return LASER_HIP_OK;
}

// The implicit-GEMM loader keeps 8-bit row/column validity bitmaps and 32-bit in-image offsets:
// kernels up to 8x8 and images below 2^30 elements; anything else goes through the explicit workspace.
bool conv_takes_implicit(int64_t iC, int64_t iH, int64_t iW, int64_t kH, int64_t kW, int64_t pH, int64_t pW,
                         int64_t sH, int64_t sW) {
  int64_t oH, oW;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, &oH, &oW);
  const int64_t reach = (oH * sH + kH + pH) * iW + oW * sW + kW + pW;  // largest |window origin| offset
  return g_ctx.conv_implicit && kH <= 8 && kW <= 8 && iC * iH * iW + reach < (1ll << 30) && iC * kH * kW < (1ll << 30);
}

std::atomic<int> g_conv_1x1_implicit{0};   // option "conv_1x1_implicit" (probes): no GEMM shortcut for 1x1 / stride 1 / pad 0

int conv_dev(float *dout, const float *din, int64_t iN, int64_t iC, int64_t iH, int64_t iW, const float *dker,
             int64_t c_out, int64_t kH, int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *dws,
             hipStream_t s, const float *dbias = nullptr, int act = 0) {
  // per-output-channel bias = one value per row of the [C_out x oH*oW] product, shared by all images
  Epi<float> epi;
  epi.bias = dbias; epi.rs = 1; epi.cs = 0; epi.bs = 0; epi.act = act;
  if (int rc = epi_check<float>(&epi)) return rc;
  int64_t oH, oW;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, &oH, &oW);
  const int64_t M = c_out, K = iC * kH * kW, N = oH * oW;
  // 1x1 shortcut (conv2d_im2col.nim:121,128,151-153): the input already is the [K, N] matrix --
  // taken only for stride 1 / no padding, where that is actually true.
  // (option conv_1x1_implicit = 1, probes: the 1x1 / stride 1 / no padding case through the implicit-GEMM kernels as well)
  const bool direct = (kH * kW == 1) && pH == 0 && pW == 0 && sH == 1 && sW == 1 && !g_conv_1x1_implicit;
  if (!direct && conv_takes_implicit(iC, iH, iW, kH, kW, pH, pW, sH, sW)) {
    // implicit GEMM: im2col's index arithmetic runs inside the B-tile loader, nothing is materialised
    GemmArgs<float> a = make_args<float>(iN, M, N, K, 1.0f, dker, K, 1, 0, din, 0, 1, iC * iH * iW, 0.0f, dout, N, 1, M * N);
    a.cH = (int32_t)iH; a.cW = (int32_t)iW; a.ckH = (int32_t)kH; a.ckW = (int32_t)kW; a.coW = (int32_t)oW;
    a.cpH = (int32_t)pH; a.cpW = (int32_t)pW; a.csH = (int32_t)sH; a.csW = (int32_t)sW;
    epi_apply(a, &epi);
    HIP_TRY(launch_conv_implicit_f32(a, f32_cfg_now(), laser_order_now(), s));
    return LASER_HIP_OK;
  }
  const float *Bm = din;
  int64_t bsB = iC * iH * iW;
  if (!direct) {
    if (!dws) return fail(LASER_HIP_E_INVALID, "explicit im2col path needs a workspace");
    HIP_TRY(launch_im2col_f32(dws, oH, oW, din, iN, iC, iH, iW, kH, kW, pH, pW, sH, sW, s));
    Bm = dws;
    bsB = K * N;
  }
  // O[n] (M x N) = F (M x K) . W[n] (K x N), alpha = 1, beta = 0 (conv2d_im2col.nim:104-105,161-166);
  // all images in ONE batched launch: A = filter shared by every image (batch stride 0)
  GemmArgs<float> a = make_args<float>(iN, M, N, K, 1.0f, dker, K, 1, 0, Bm, N, 1, bsB, 0.0f, dout, N, 1, M * N);
  epi_apply(a, &epi);
  HIP_TRY(run_gemm<float>(a, s));
  return LASER_HIP_OK;
}

// cblas enums: benchmarks/third_party/blas.nim:12-16
template <typename T>
int cblas_gemm(int order, int tA, int tB, int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t lda,
                      const T *B, int64_t ldb, T beta, T *C, int64_t ldc) {
  if ((order != 101 && order != 102) || tA < 111 || tA > 113 || tB < 111 || tB > 113)
    return fail(LASER_HIP_E_INVALID, "bad cblas order/transpose enum");
  const bool rowm = order == 101;
  // op(X)[r,c]: row-major no-trans -> (ld,1); row-major trans -> (1,ld); col-major swaps them
  auto strides = [&](bool trans, int64_t ld, int64_t *rs, int64_t *cs) {
    const bool r_contig_c = rowm != trans;  // element [r, c+1] adjacent
    *rs = r_contig_c ? ld : 1;
    *cs = r_contig_c ? 1 : ld;
  };
  int64_t rsA, csA, rsB, csB;
  strides(tA != 111, lda, &rsA, &csA);
  strides(tB != 111, ldb, &rsB, &csB);
  const int64_t rsC = rowm ? ldc : 1, csC = rowm ? 1 : ldc;
  return gemm_host<T>(M, N, K, alpha, A, rsA, csA, B, rsB, csB, beta, C, rsC, csC);
}


}  // namespace

// =====================================================================================================
namespace {
template <typename U>
int copy_strided_api(void *dst, const int64_t *ds, const void *src, const int64_t *ss, const int64_t *shape,
                            int rank, void *stream) {
  if (rank < 0 || rank > kMaxRank) return fail(LASER_HIP_E_INVALID, "rank %d outside 0..%d (LASER_MAXRANK)", rank, kMaxRank);
  if (rank > 0 && (!ds || !ss || !shape)) return fail(LASER_HIP_E_INVALID, "null shape/strides");
  int64_t total = 1;
  for (int d = 0; d < rank; d++) {
    if (shape[d] < 0) return fail(LASER_HIP_E_INVALID, "negative extent");
    total *= shape[d];
  }
  if (int rc = ensure_init()) return rc;
  if (total == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "null buffer");
  // both sides C-contiguous: a plain device-to-device copy
  bool contiguous = true;
  int64_t run = 1;
  for (int d = rank - 1; d >= 0; d--) {
    if (shape[d] != 1 && (ds[d] != run || ss[d] != run)) contiguous = false;
    run *= shape[d];
  }
  if (contiguous) {
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)total * sizeof(U), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LASER_HIP_OK;
  }
  HIP_TRY(launch_copy_strided<U>((U *)dst, ds, (const U *)src, ss, shape, rank, (hipStream_t)stream));
  return LASER_HIP_OK;
}
}  // namespace

extern "C" {

int laser_hip_init(int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  return ensure_init_locked(device);
}

int laser_hip_finalize(void) {
  // lock order everywhere: a device's mutex BEFORE g_mu (the host-pointer entry points hold their device's mutex when
  // they touch the registries) -- so the per-device state is released first, one device at a time, then the registries
  for (DeviceCtx &D : g_dev) {
    std::lock_guard<std::mutex> dl(D.mu);
    if (D.device < 0) continue;
    (void)hipSetDevice(D.device);
    for (int i = 0; i < 6; i++) {
      if (D.scratch[i]) (void)hipFree(D.scratch[i]);
      D.scratch[i] = nullptr;
      D.scratch_sz[i] = 0;
    }
    if (D.s_up) {
      (void)hipStreamDestroy(D.s_up);
      (void)hipStreamDestroy(D.s_comp);
      (void)hipStreamDestroy(D.s_down);
      D.s_up = D.s_comp = D.s_down = nullptr;
    }
    if (D.zc) (void)hipHostFree(D.zc);
    D.zc = nullptr;
    D.zc_sz = 0;
    D.device = -1;
  }
  asm_kernels_release();
  scratch_pools_trim();
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_ctx.device >= 0) (void)hipSetDevice(g_ctx.device);
  panel_cache_clear_locked();
  if (g_ctx.device >= 0) (void)hipSetDevice(g_ctx.device);
  for (auto &kv : g_free_storage)
    for (const FreeBlock &b : kv.second) free_block_release(b);
  g_free_storage.clear();
  g_free_storage_bytes = 0;
  g_ctx.ready = false;
  return LASER_HIP_OK;
}

const char *laser_hip_last_error(void) { return g_err.c_str(); }
const char *laser_hip_version(void) { return "laser_hip 0.2.0 (gfx950)"; }
int laser_hip_abi_version(void) { return LASER_HIP_ABI_VERSION; }
int laser_hip_plan_f32(int64_t M, int64_t N, int64_t K, int laser_order, int cus, int64_t *out8) {
  if (!out8) return fail(LASER_HIP_E_INVALID, "null pointer");
  if (asm_plan_f32(M, N, K, laser_order, cus, out8)) return fail(LASER_HIP_E_INVALID, "laser_hip_plan_f32: bad shape or CU count");
  return LASER_HIP_OK;
}
int laser_hip_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
const char *laser_hip_arch(void) {
  if (ensure_init()) return "";
  return g_ctx.arch.c_str();
}

int laser_hip_set_float_mode(int mode) {
  if (mode != LASER_HIP_F32_LASER_ORDER && mode != LASER_HIP_F32_FAST) return fail(LASER_HIP_E_INVALID, "bad float mode");
  g_ctx.float_mode = mode;
  return LASER_HIP_OK;
}
int laser_hip_get_float_mode(void) { return g_ctx.float_mode; }
int laser_hip_set_f32_config(int cfg) {
  if (cfg >= gemm_f32_config_count()) return fail(LASER_HIP_E_INVALID, "bad f32 config index");
  g_ctx.f32_cfg = cfg < 0 ? -1 : cfg;
  return LASER_HIP_OK;
}
int laser_hip_f32_config_count(void) { return gemm_f32_config_count(); }
}  // extern "C"
// ---- options: every tuning / A-B switch behind ONE entry point (name, value); diagnostics behind laser_hip_get_option ----
// One row per name (the header documents each; unknown names are an error, never silently ignored): how to read it, how to write
// it (nothing: a read-only diagnostic), and what a written value becomes.  The variables stay beside the code that reads them.
namespace {
enum OptionRule {
  kOnOff,   // any non-zero value becomes 1
  kClamp,   // into [lo, hi]
  kOrElse,  // [lo, hi] as it is, anything else becomes `other`
};
struct Option {
  const char *name;
  int64_t (*get)();
  void (*set)(int);
  OptionRule rule;
  int lo, hi, other;
};
constexpr int kNoLimit = 2147483647;
#define LH_VAR(v) [] { return (int64_t)(v); }, [](int x) { (v) = x; }
#define LH_READ_ONLY(expr) [] { return (int64_t)(expr); }, nullptr, kOnOff, 0, 0, 0
const Option kOptions[] = {
  {"f32_asm", LH_VAR(g_f32_asm), kClamp, 0, 2},
  {"f64_asm", LH_VAR(g_f64_asm), kClamp, 0, 2},
  {"i32_asm", LH_VAR(g_i32_asm), kClamp, 0, 2},
  {"int_group_m", LH_VAR(g_int_group_m), kClamp, 1, 64},
  {"f64_mfma", LH_VAR(g_ctx.f64_mfma), kOnOff},
  {"i32_mfma", LH_VAR(g_ctx.i32_mfma), kOnOff},
  {"i64_mfma", LH_VAR(g_ctx.i64_mfma), kOnOff},
  {"narrow_mfma", LH_VAR(g_ctx.narrow_mfma), kOnOff},
  {"conv_implicit", LH_VAR(g_ctx.conv_implicit), kOnOff},
  {"conv_patch", LH_VAR(g_conv_patch), kOnOff},
  {"conv_direct", LH_VAR(g_conv_direct), kClamp, 0, 3},
  {"conv_kslice", LH_VAR(g_conv_kslice), kOnOff},
  {"conv_tail", LH_VAR(g_conv_tail), kOnOff},
  {"conv_cut_always", LH_VAR(g_conv_cut_always), kOnOff},
  {"conv_1x1_implicit", LH_VAR(g_conv_1x1_implicit), kOnOff},
  {"conv_walk", LH_VAR(g_conv_walk), kClamp, 0, 65535},
  {"host_pipeline_2d", LH_VAR(g_ctx.host_pipeline_2d), kOnOff},
  {"zero_copy_poll", LH_VAR(g_ctx.zc_poll), kOnOff},
  {"skinny", LH_VAR(g_ctx.skinny), kOnOff},
  {"small_path", LH_VAR(g_small_path), kOnOff},
  {"split_tail", LH_VAR(g_split_tail), kOnOff},
  {"slice_parallel", LH_VAR(g_ctx.slice_parallel), kOnOff},
  {"slice_parallel_min", LH_VAR(g_ctx.slice_parallel_min), kClamp, 2, kNoLimit},
  {"slice_parallel_tiles", LH_VAR(g_ctx.slice_parallel_tiles), kClamp, 0, kNoLimit},
  {"asm_plan", LH_VAR(g_asm_plan), kClamp, 0, 4},
  {"asm_kernel", LH_VAR(g_asm_kernel), kClamp, -1, kNoLimit},
  {"asm_tile", LH_VAR(g_asm_tile), kOrElse, 0, 9, -1},
  {"thread_asm_tile", [] { return (int64_t)asm_get_thread_tile(); }, asm_set_thread_tile, kOrElse, -1, 9, -2},  // thread-local
  {"asm_wgs", LH_VAR(g_asm_wgs), kClamp, 0, kNoLimit},
  {"asm_slice", LH_VAR(g_asm_slice), kClamp, 0, kNoLimit},
  {"asm_group_m", LH_VAR(g_asm_group_m), kClamp, 0, kNoLimit},
  {"asm_noseed", LH_VAR(g_asm_noseed), kOnOff},
  {"asm_test_giveup", LH_VAR(g_asm_giveup), kOnOff},
  {"im2col_band", LH_VAR(g_im2col_band), kClamp, 0, kNoLimit},
  // diagnostics of the last launch, and counters
  {"last_f32_config", LH_READ_ONLY(g_last_f32_cfg)},
  {"last_f32_asm", LH_READ_ONLY(g_last_f32_asm)},
  {"last_f64_asm", LH_READ_ONLY(g_last_f64_asm)},
  {"last_i32_asm", LH_READ_ONLY(g_last_i32_asm)},
  {"last_narrow_mfma", LH_READ_ONLY(g_last_narrow_mfma)},
  {"last_split", LH_READ_ONLY(g_last_split)},
  {"last_conv_tail", LH_READ_ONLY(g_last_conv_tail)},
  {"last_asm_wgs", LH_READ_ONLY(g_last_asm_wgs)},
  {"last_asm_rem", LH_READ_ONLY(g_last_asm_rem)},
  {"last_asm_slices", LH_READ_ONLY(g_last_asm_slices)},
  {"last_asm_group_m", LH_READ_ONLY(g_last_asm_group_m)},
  {"last_foreach_variant", LH_READ_ONLY(api_last_foreach_variant())},
  {"last_reduce_variant", LH_READ_ONLY(g_last_reduce_variant)},
  {"last_softmax_kernel", LH_READ_ONLY(g_last_softmax_kernel)},
  {"foreach_compiles", LH_READ_ONLY(api_foreach_compiles())},
  {"asm_fixup_timeouts", LH_READ_ONLY(asm_fixup_timeouts())},  // synchronises the device when there is one, -1 without
  {"shard_rccl_ranks", LH_READ_ONLY(api_shard_rccl_ranks())},
};
#undef LH_VAR
#undef LH_READ_ONLY
const Option *find_option(const char *name) {
  for (const Option &o : kOptions)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
}  // namespace
extern "C" {
int laser_hip_set_option(const char *name, int value) {
  if (!name) return fail(LASER_HIP_E_INVALID, "set_option: null name");
  const Option *o = find_option(name);
  if (!o || !o->set) return fail(LASER_HIP_E_INVALID, "set_option: unknown option '%s'", name);
  switch (o->rule) {
    case kOnOff: value = value != 0; break;
    case kClamp: value = value < o->lo ? o->lo : value > o->hi ? o->hi : value; break;
    case kOrElse: value = value < o->lo || value > o->hi ? o->other : value; break;
  }
  o->set(value);
  return LASER_HIP_OK;
}
int laser_hip_get_option(const char *name, int64_t *value) {
  if (!name || !value) return fail(LASER_HIP_E_INVALID, "get_option: null argument");
  const Option *o = find_option(name);
  if (!o) return fail(LASER_HIP_E_INVALID, "get_option: unknown option '%s'", name);
  *value = o->get();
  return LASER_HIP_OK;
}
int laser_hip_set_shard_devices(int ndev) {  // host-pointer gemm_strided over ndev GPUs (1 = off, 0 = every visible GPU)
  if (ndev < 0 || ndev > kMaxDevices) return fail(LASER_HIP_E_INVALID, "shard devices outside 0..%d", kMaxDevices);
  g_ctx.shard_devices = ndev;
  return LASER_HIP_OK;
}
int laser_hip_get_shard_devices(void) { return g_ctx.shard_devices; }
const char *laser_hip_f32_config_name(int cfg) { return gemm_f32_config_name(cfg); }

// S = the C type alpha and beta travel in: T itself, or int32_t for int8 / int16 (uint8 / uint16 on the same bits), reduced mod 2^8 / 2^16
#define LH_DEF_GEMM(SFX, T, S)                                                                                \
  int laser_hip_gemm_strided_##SFX(int64_t M, int64_t N, int64_t K, S alpha, const T *A, int64_t rsA,         \
                                   int64_t csA, const T *B, int64_t rsB, int64_t csB, S beta, T *C,           \
                                   int64_t rsC, int64_t csC) {                                                \
    return gemm_host<T>(M, N, K, (T)alpha, A, rsA, csA, B, rsB, csB, (T)beta, C, rsC, csC);                   \
  }                                                                                                           \
  int laser_hip_gemm_strided_##SFX##_dev(int64_t M, int64_t N, int64_t K, S alpha, const T *A, int64_t rsA,   \
                                         int64_t csA, const T *B, int64_t rsB, int64_t csB, S beta, T *C,     \
                                         int64_t rsC, int64_t csC, void *stream) {                            \
    return gemm_dev<T>(1, M, N, K, (T)alpha, A, rsA, csA, 0, B, rsB, csB, 0, (T)beta, C, rsC, csC, 0, stream); \
  }                                                                                                           \
  int laser_hip_gemm_strided_batched_##SFX##_dev(                                                             \
      int64_t batch, int64_t M, int64_t N, int64_t K, S alpha, const T *A, int64_t rsA, int64_t csA,          \
      int64_t bsA, const T *B, int64_t rsB, int64_t csB, int64_t bsB, S beta, T *C, int64_t rsC, int64_t csC, \
      int64_t bsC, void *stream) {                                                                            \
    return gemm_dev<T>(batch, M, N, K, (T)alpha, A, rsA, csA, bsA, B, rsB, csB, bsB, (T)beta, C, rsC, csC,    \
                       bsC, stream);                                                                          \
  }                                                                                                           \
  int64_t laser_hip_gemm_prepackA_mem_required_##SFX(int64_t M, int64_t N, int64_t K) {                       \
    return prepack_bytes<T>(true, M, N, K);                                                                   \
  }                                                                                                           \
  int64_t laser_hip_gemm_prepackB_mem_required_##SFX(int64_t M, int64_t N, int64_t K) {                       \
    return prepack_bytes<T>(false, M, N, K);                                                                  \
  }                                                                                                           \
  int laser_hip_gemm_prepackA_##SFX(void *dst, int64_t M, int64_t N, int64_t K, const T *A, int64_t rs,       \
                                    int64_t cs) {                                                             \
    return prepack_host<T>(true, dst, M, N, K, A, rs, cs);                                                    \
  }                                                                                                           \
  int laser_hip_gemm_prepackB_##SFX(void *dst, int64_t M, int64_t N, int64_t K, const T *B, int64_t rs,       \
                                    int64_t cs) {                                                             \
    return prepack_host<T>(false, dst, M, N, K, B, rs, cs);                                                   \
  }                                                                                                           \
  int laser_hip_gemm_packed_##SFX(int64_t M, int64_t N, int64_t K, S alpha, const void *pA, const void *pB,   \
                                  S beta, T *C, int64_t rsC, int64_t csC) {                                   \
    return packed_host<T>(M, N, K, (T)alpha, pA, pB, (T)beta, C, rsC, csC);                                   \
  }                                                                                                           \
  int laser_hip_gemm_prepackA_##SFX##_dev(void *d, int64_t M, int64_t N, int64_t K, const T *A, int64_t rs,   \
                                          int64_t cs, void *stream) {                                         \
    return prepack_dev<T>(true, d, M, N, K, A, rs, cs, stream);                                               \
  }                                                                                                           \
  int laser_hip_gemm_prepackB_##SFX##_dev(void *d, int64_t M, int64_t N, int64_t K, const T *B, int64_t rs,   \
                                          int64_t cs, void *stream) {                                         \
    return prepack_dev<T>(false, d, M, N, K, B, rs, cs, stream);                                              \
  }                                                                                                           \
  int laser_hip_gemm_packed_##SFX##_dev(int64_t M, int64_t N, int64_t K, S alpha, const void *dA,             \
                                        const void *dB, S beta, T *dC, int64_t rsC, int64_t csC,              \
                                        void *stream) {                                                       \
    return packed_dev<T>(M, N, K, (T)alpha, dA, dB, (T)beta, dC, rsC, csC, stream);                           \
  }
LH_DEF_GEMM(f32, float, float)
LH_DEF_GEMM(f64, double, double)
LH_DEF_GEMM(i32, int32_t, int32_t)
LH_DEF_GEMM(i64, int64_t, int64_t)
LH_DEF_GEMM(i8, int8_t, int32_t)
LH_DEF_GEMM(i16, int16_t, int32_t)
#undef LH_DEF_GEMM

int laser_hip_gemm_prepack_release(void *packed) { return prepack_release(packed); }

#define LH_DEF_TR(SFX, ELEM)                                                                                  \
  int laser_hip_transpose2d_copy_##SFX(void *dst, const void *src, int64_t NR, int64_t NC) {                  \
    return transpose_host(dst, src, 1, NR, NC, ELEM);                                                         \
  }                                                                                                           \
  int laser_hip_transpose2d_batched_##SFX(void *dst, const void *src, int64_t N, int64_t NR, int64_t NC) {    \
    return transpose_host(dst, src, N, NR, NC, ELEM);                                                         \
  }                                                                                                           \
  int laser_hip_nchw2nhwc_##SFX(void *dst, const void *src, int64_t N, int64_t C, int64_t H, int64_t W) {     \
    return transpose_host(dst, src, N, C, H * W, ELEM); /* swapaxes.nim:98 */                                 \
  }                                                                                                           \
  int laser_hip_nhwc2nchw_##SFX(void *dst, const void *src, int64_t N, int64_t C, int64_t H, int64_t W) {     \
    return transpose_host(dst, src, N, H * W, C, ELEM); /* swapaxes.nim:112 */                                \
  }                                                                                                           \
  int laser_hip_transpose2d_batched_##SFX##_dev(void *dst, const void *src, int64_t N, int64_t NR,            \
                                                int64_t NC, void *stream) {                                   \
    if (N < 0 || NR < 0 || NC < 0) return fail(LASER_HIP_E_INVALID, "negative dimension");                    \
    if (int rc = ensure_init()) return rc;                                                                    \
    if (N == 0 || NR == 0 || NC == 0) return LASER_HIP_OK;                                                    \
    if (!dst || !src) return fail(LASER_HIP_E_INVALID, "null pointer");                                       \
    HIP_TRY(launch_transpose_batched(dst, src, N, NR, NC, ELEM, (hipStream_t)stream));                        \
    return LASER_HIP_OK;                                                                                      \
  }
LH_DEF_TR(b32, 4)
LH_DEF_TR(b64, 8)
LH_DEF_TR(b16, 2)
LH_DEF_TR(b8, 1)
#undef LH_DEF_TR

int laser_hip_conv2d_out_shape(int64_t iN, int64_t iC, int64_t iH, int64_t iW, int64_t c_out, int64_t c_in,
                               int64_t kH, int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW,
                               int64_t *oN, int64_t *oC, int64_t *oH, int64_t *oW) {
  if (int rc = conv_check(iN, iC, iH, iW, c_out, c_in, kH, kW, pH, pW, sH, sW)) return rc;
  *oN = iN;
  *oC = c_out;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, oH, oW);
  return LASER_HIP_OK;
}

int64_t laser_hip_im2col_workspace_size(int64_t iN, int64_t iC, int64_t iH, int64_t iW, int64_t c_out,
                                        int64_t c_in, int64_t kH, int64_t kW, int64_t pH, int64_t pW,
                                        int64_t sH, int64_t sW) {
  (void)iN; (void)c_out; (void)c_in;
  if (sH <= 0 || sW <= 0) return 0;
  int64_t oH, oW;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, &oH, &oW);
  return iC * kH * kW * oH * oW;  // conv2d_im2col.nim:19-20
}

// im2col*[T] (conv2d_im2col.nim:42-88) is generic in the element type: pure data movement, one kernel per element size
static int im2col_api_dev(void *dws, int64_t oH, int64_t oW, const void *din, int64_t batch, int64_t iC, int64_t iH, int64_t iW,
                          int64_t kH, int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, int elem, void *stream) {
  if (int rc = ensure_init()) return rc;
  if (!dws || !din) return fail(LASER_HIP_E_INVALID, "null pointer");
  if (oH < 0 || oW < 0 || batch < 0 || iC <= 0 || iH <= 0 || iW <= 0 || kH <= 0 || kW <= 0 || pH < 0 || pW < 0 || sH <= 0 || sW <= 0)
    return fail(LASER_HIP_E_INVALID, "bad shape");
  HIP_TRY(launch_im2col(dws, oH, oW, din, batch, iC, iH, iW, kH, kW, pH, pW, sH, sW, elem, (hipStream_t)stream));
  return LASER_HIP_OK;
}
static int im2col_api_host(void *ws, int64_t oH, int64_t oW, const void *in, int64_t iC, int64_t iH, int64_t iW, int64_t kH, int64_t kW,
                           int64_t pH, int64_t pW, int64_t sH, int64_t sW, int elem) {
  if (int rc = ensure_init()) return rc;
  if (!ws || !in) return fail(LASER_HIP_E_INVALID, "null pointer");
  if (oH < 0 || oW < 0 || iC <= 0 || iH <= 0 || iW <= 0 || kH <= 0 || kW <= 0 || pH < 0 || pW < 0 || sH <= 0 || sW <= 0)
    return fail(LASER_HIP_E_INVALID, "bad shape");
  HostCall hc;
  if (hc.rc) return hc.rc;
  const size_t ib = (size_t)iC * iH * iW * elem, wb = (size_t)iC * kH * kW * oH * oW * elem;
  if (wb == 0) return LASER_HIP_OK;
  void *di, *dw;
  if (int rc = scratch_get(0, ib, &di)) return rc;
  if (int rc = scratch_get(4, wb, &dw)) return rc;
  HIP_TRY(hipMemcpy(di, in, ib, hipMemcpyHostToDevice));
  HIP_TRY(launch_im2col(dw, oH, oW, di, 1, iC, iH, iW, kH, kW, pH, pW, sH, sW, elem, nullptr));
  HIP_TRY(hipMemcpy(ws, dw, wb, hipMemcpyDeviceToHost));
  return LASER_HIP_OK;
}
#define LH_DEF_IM2COL(SFX, T)                                                                                               \
  int laser_hip_im2col_##SFX##_dev(T *dws, int64_t oH, int64_t oW, const T *din, int64_t batch, int64_t iC, int64_t iH,      \
                                   int64_t iW, int64_t kH, int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW,       \
                                   void *stream) {                                                                           \
    return im2col_api_dev(dws, oH, oW, din, batch, iC, iH, iW, kH, kW, pH, pW, sH, sW, (int)sizeof(T), stream);              \
  }                                                                                                                          \
  int laser_hip_im2col_##SFX(T *ws, int64_t oH, int64_t oW, const T *in, int64_t iC, int64_t iH, int64_t iW, int64_t kH,     \
                             int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW) {                                   \
    return im2col_api_host(ws, oH, oW, in, iC, iH, iW, kH, kW, pH, pW, sH, sW, (int)sizeof(T));                              \
  }
LH_DEF_IM2COL(f32, float)
LH_DEF_IM2COL(f64, double)
#undef LH_DEF_IM2COL

static int conv2d_api_dev(float *dout, const float *din, int64_t iN, int64_t iC, int64_t iH,
                                    int64_t iW, const float *dker, int64_t c_out, int64_t c_in, int64_t kH,
                                    int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *dws,
                                    int64_t dws_elems, const float *dbias, int act, void *stream) {
  if (int rc = conv_check(iN, iC, iH, iW, c_out, c_in, kH, kW, pH, pW, sH, sW)) return rc;
  if (int rc = ensure_init()) return rc;
  if (iN == 0) return LASER_HIP_OK;
  if (!dout || !din || !dker) return fail(LASER_HIP_E_INVALID, "null pointer");
  if (iN > 65535) return fail(LASER_HIP_E_INVALID, "batch > 65535");
  hipStream_t s = (hipStream_t)stream;
  const bool direct = (kH * kW == 1) && pH == 0 && pW == 0 && sH == 1 && sW == 1;
  if (direct || conv_takes_implicit(iC, iH, iW, kH, kW, pH, pW, sH, sW))  // nothing is materialised
    return conv_dev(dout, din, iN, iC, iH, iW, dker, c_out, kH, kW, pH, pW, sH, sW, nullptr, s, dbias, act);
  // Explicit im2col path (kernels larger than 8x8, huge images, laser_hip_set_conv_implicit(0)).  The caller's
  // workspace follows the REFERENCE's contract -- one image, im2col_workspace_size elements
  // (conv2d_im2col.nim:19-20, reused between batches :99) -- so it is used as what it is: a caller that hands
  // over iN images' worth gets them all expanded in one pass, one image's worth is looped over image by image,
  // anything smaller is rejected, and no workspace means stream-ordered library scratch (never a buffer shared
  // between streams).
  int64_t oH, oW;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, &oH, &oW);
  const int64_t w1 = iC * kH * kW * oH * oW;
  if (dws && dws_elems >= 0 && dws_elems < w1)
    return fail(LASER_HIP_E_INVALID, "im2col workspace holds %lld elements, one image needs %lld", (long long)dws_elems, (long long)w1);
  float *own = nullptr;
  int64_t imgs = iN;  // images expanded per pass
  if (!dws) {
    while (imgs > 1 && (double)imgs * (double)w1 * 4.0 > 2.0e9) imgs = (imgs + 1) / 2;  // bound the scratch
    HIP_TRY(scratch_alloc_async((void **)&own, (size_t)imgs * (size_t)w1 * 4, s));
    dws = own;
  } else {
    // capacity unknown (the plain entry points): the reference's contract is ONE image's worth -> image by image
    imgs = dws_elems >= 0 ? std::max<int64_t>(1, std::min<int64_t>(iN, dws_elems / w1)) : 1;
  }
  int rc = LASER_HIP_OK;
  for (int64_t n0 = 0; n0 < iN && rc == LASER_HIP_OK; n0 += imgs) {
    const int64_t nb = std::min<int64_t>(imgs, iN - n0);
    rc = conv_dev(dout + n0 * c_out * oH * oW, din + n0 * iC * iH * iW, nb, iC, iH, iW, dker, c_out, kH, kW, pH, pW, sH, sW,
                  dws, s, dbias, act);
  }
  if (own) {
    const hipError_t e = scratch_free_async(own, s);
    if (rc == LASER_HIP_OK && e != hipSuccess) rc = fail(LASER_HIP_E_HIP, "scratch_free_async: %s", hipGetErrorString(e));
  }
  return rc;
}
int laser_hip_conv2d_im2col_f32_dev(float *dout, const float *din, int64_t iN, int64_t iC, int64_t iH,
                                    int64_t iW, const float *dker, int64_t c_out, int64_t c_in, int64_t kH,
                                    int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *dws,
                                    void *stream) {
  return conv2d_api_dev(dout, din, iN, iC, iH, iW, dker, c_out, c_in, kH, kW, pH, pW, sH, sW, dws, -1, nullptr, 0, stream);
}
int laser_hip_conv2d_im2col_ex_f32_dev(float *dout, const float *din, int64_t iN, int64_t iC, int64_t iH,
                                       int64_t iW, const float *dker, int64_t c_out, int64_t c_in, int64_t kH,
                                       int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *dws,
                                       const float *dbias, int act, void *stream) {
  return conv2d_api_dev(dout, din, iN, iC, iH, iW, dker, c_out, c_in, kH, kW, pH, pW, sH, sW, dws, -1, dbias, act, stream);
}

static int conv2d_api_host(float *out, const float *in, int64_t iN, int64_t iC, int64_t iH, int64_t iW,
                                const float *ker, int64_t c_out, int64_t c_in, int64_t kH, int64_t kW,
                                int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *pworkspace,
                                const float *bias, int act) {
  if (int rc = conv_check(iN, iC, iH, iW, c_out, c_in, kH, kW, pH, pW, sH, sW)) return rc;
  if (int rc = ensure_init()) return rc;
  if (iN == 0) return LASER_HIP_OK;
  if (!out || !in || !ker) return fail(LASER_HIP_E_INVALID, "null pointer");
  if (iN > 65535) return fail(LASER_HIP_E_INVALID, "batch > 65535");
  HostCall hc;
  if (hc.rc) return hc.rc;
  int64_t oH, oW;
  out_hw(iH, iW, kH, kW, pH, pW, sH, sW, &oH, &oW);
  const size_t ib = (size_t)iN * iC * iH * iW * 4, kb = (size_t)c_out * iC * kH * kW * 4;
  const size_t ob = (size_t)iN * c_out * oH * oW * 4, w1 = (size_t)iC * kH * kW * oH * oW * 4;
  void *di, *dk, *dout, *dws;
  const bool direct = (kH * kW == 1) && pH == 0 && pW == 0 && sH == 1 && sW == 1;
  const bool implicit = conv_takes_implicit(iC, iH, iW, kH, kW, pH, pW, sH, sW);
  if (int rc = scratch_get(0, ib, &di)) return rc;
  if (int rc = scratch_get(1, kb, &dk)) return rc;
  if (int rc = scratch_get(2, ob, &dout)) return rc;
  if (int rc = scratch_get(4, implicit ? w1 : w1 * iN, &dws)) return rc;
  HIP_TRY(hipMemcpy(di, in, ib, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dk, ker, kb, hipMemcpyHostToDevice));
  void *dbias = nullptr;
  if (bias) {
    if (int rc = scratch_get(5, (size_t)c_out * 4, &dbias)) return rc;
    HIP_TRY(hipMemcpy(dbias, bias, (size_t)c_out * 4, hipMemcpyHostToDevice));
  }
  if (int rc = conv_dev((float *)dout, (const float *)di, iN, iC, iH, iW, (const float *)dk, c_out, kH, kW, pH,
                        pW, sH, sW, (float *)dws, nullptr, (const float *)dbias, act))
    return rc;
  HIP_TRY(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
  // like the reference, the caller's workspace ends up holding the LAST image's im2col matrix
  if (pworkspace && !direct && w1 > 0) {
    const char *src = (const char *)dws + (size_t)(iN - 1) * w1;
    if (implicit) {  // nothing was materialised: expand just the last image for the caller
      HIP_TRY(launch_im2col_f32((float *)dws, oH, oW, (const float *)di + (size_t)(iN - 1) * iC * iH * iW, 1, iC, iH, iW,
                                kH, kW, pH, pW, sH, sW, nullptr));
      src = (const char *)dws;
    }
    HIP_TRY(hipMemcpy(pworkspace, src, w1, hipMemcpyDeviceToHost));
  }
  return LASER_HIP_OK;
}

int laser_hip_conv2d_im2col_f32(float *out, const float *in, int64_t iN, int64_t iC, int64_t iH, int64_t iW,
                                const float *ker, int64_t c_out, int64_t c_in, int64_t kH, int64_t kW,
                                int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *pworkspace) {
  return conv2d_api_host(out, in, iN, iC, iH, iW, ker, c_out, c_in, kH, kW, pH, pW, sH, sW, pworkspace, nullptr, 0);
}
int laser_hip_conv2d_im2col_ex_f32(float *out, const float *in, int64_t iN, int64_t iC, int64_t iH, int64_t iW,
                                   const float *ker, int64_t c_out, int64_t c_in, int64_t kH, int64_t kW,
                                   int64_t pH, int64_t pW, int64_t sH, int64_t sW, float *pworkspace,
                                   const float *bias, int act) {
  return conv2d_api_host(out, in, iN, iC, iH, iW, ker, c_out, c_in, kH, kW, pH, pW, sH, sW, pworkspace, bias, act);
}

#define LH_DEF_GEMM_EX(SFX, T)                                                                                \
  int laser_hip_gemm_strided_ex_##SFX(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA,      \
                                      int64_t csA, const T *B, int64_t rsB, int64_t csB, T beta, T *C,        \
                                      int64_t rsC, int64_t csC, const T *bias, int64_t rsBias,                \
                                      int64_t csBias, int act) {                                              \
    const Epi<T> e = make_epi<T>(bias, rsBias, csBias, act);                                                  \
    return gemm_host<T>(M, N, K, alpha, A, rsA, csA, B, rsB, csB, beta, C, rsC, csC, &e);                     \
  }                                                                                                           \
  int laser_hip_gemm_strided_ex_##SFX##_dev(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA, \
                                            int64_t csA, const T *B, int64_t rsB, int64_t csB, T beta, T *C,  \
                                            int64_t rsC, int64_t csC, const T *bias, int64_t rsBias,          \
                                            int64_t csBias, int act, void *stream) {                          \
    const Epi<T> e = make_epi<T>(bias, rsBias, csBias, act);                                                  \
    return gemm_dev<T>(1, M, N, K, alpha, A, rsA, csA, 0, B, rsB, csB, 0, beta, C, rsC, csC, 0, stream, &e);  \
  }
LH_DEF_GEMM_EX(f32, float)
LH_DEF_GEMM_EX(f64, double)
#undef LH_DEF_GEMM_EX

// ---- device tensor storage -- laser/tensor/allocator.nim, initialization.nim -----------------------
// Freed storages are kept on a per-size free list (exact match of the 256-byte-rounded size, at most
// kStorageCacheMax bytes in total) so that chains of tensor-producing calls do not pay hipMalloc / hipFree -- a
// device allocation costs ~100 us, more than a 2048^3 product.  Reused blocks are zero-filled again: the contract
// stays allocShared0's.  laser_hip_storage_trim() / laser_hip_finalize() release the list.
static int storage_alloc(void **d, int64_t bytes, hipStream_t stream, bool ordered) {
  if (!d || bytes < 0) return fail(LASER_HIP_E_INVALID, "storage_alloc: bad argument");
  if (int rc = ensure_init()) return rc;
  *d = nullptr;
  if (bytes == 0) return LASER_HIP_OK;
  const size_t want = ((size_t)bytes + 255) & ~(size_t)255;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const size_t key = storage_key(want, dev);
  FreeBlock taken = {nullptr, nullptr, nullptr};
  {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_free_storage.find(key);
    if (it != g_free_storage.end() && !it->second.empty()) {
      // the newest block this stream freed itself, if there is one (no wait at all), else the newest of the size
      auto &list = it->second;
      size_t pick = list.size() - 1;
      for (size_t k = list.size(); ordered && k-- > 0;)
        if (list[k].owner == stream && list[k].done) {
          pick = k;
          break;
        }
      taken = list[pick];
      *d = taken.p;
      list.erase(list.begin() + (ptrdiff_t)pick);
      g_free_storage_bytes -= want;
      g_storage_owner[*d] = ordered ? stream : nullptr;
    }
  }
  // A recycled block may still be read by work queued on its owner's stream when the owner dropped it (hipFree would have
  // waited for the device; the free list does not).  The stream-ordered form stays asynchronous: the same stream needs
  // nothing (its zero fill queues behind that work), another stream waits for the event of the free on the device.  The
  // plain form waits for that event on the host, as it waits for its zero fill.
  if (*d) {
    hipError_t e = hipSuccess;
    if (!taken.done) e = hipDeviceSynchronize();
    else if (!ordered) e = hipEventSynchronize(taken.done);
    else if (stream != taken.owner) e = hipStreamWaitEvent(stream, taken.done, 0);
    if (taken.done) (void)hipEventDestroy(taken.done);
    if (e != hipSuccess) return fail(LASER_HIP_E_HIP, "storage_alloc (reuse): %s", hipGetErrorString(e));
  }
  if (!*d) {
    hipError_t e = hipMalloc(d, want);  // hipMalloc is 256-byte aligned >= LASER_MEM_ALIGN
    if (e != hipSuccess) {             // out of memory: give the cached blocks back and retry once
      storage_trim();
      e = hipMalloc(d, want);
    }
    if (e != hipSuccess) return fail(LASER_HIP_E_HIP, "hipMalloc(%zu): %s", want, hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(g_mu);
    g_live_storage[*d] = key;
    g_storage_owner[*d] = ordered ? stream : nullptr;
  }
  // zero fill (allocShared0): ordered on the caller's stream -- the stream the tensor's first kernel will run on --
  // or, for the plain entry point, completed before returning (PyTorch-style side streams are non-blocking: a fill
  // left running on the NULL stream could land after, or beside, the first kernel that writes the block)
  hipError_t e = hipMemsetAsync(*d, 0, (size_t)bytes, stream);
  if (e == hipSuccess && !ordered) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return fail(LASER_HIP_E_HIP, "zero fill: %s", hipGetErrorString(e));
  return LASER_HIP_OK;
}
int laser_hip_storage_alloc(void **d, int64_t bytes) { return storage_alloc(d, bytes, nullptr, false); }
int laser_hip_storage_alloc_stream(void **d, int64_t bytes, void *stream) { return storage_alloc(d, bytes, (hipStream_t)stream, true); }
int laser_hip_storage_free(void *d) {
  if (!d) return LASER_HIP_OK;
  if (int rc = ensure_init()) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_live_storage.find(d);
  if (it == g_live_storage.end()) return fail(LASER_HIP_E_INVALID, "storage_free: not a laser_hip storage");
  const size_t key = it->second, sz = storage_size(key);
  if (g_free_storage_bytes + sz <= kStorageCacheMax) {
    FreeBlock b = {d, nullptr, nullptr};
    auto ow = g_storage_owner.find(d);
    if (ow != g_storage_owner.end()) b.owner = ow->second;
    // everything queued so far on the owner's stream may still use the block
    if (hipEventCreateWithFlags(&b.done, hipEventDisableTiming) != hipSuccess) b.done = nullptr;
    if (b.done && hipEventRecord(b.done, b.owner) != hipSuccess) {
      (void)hipEventDestroy(b.done);
      b.done = nullptr;
    }
    if (!b.done) (void)hipGetLastError();
    g_free_storage[key].push_back(b);
    g_free_storage_bytes += sz;
    return LASER_HIP_OK;
  }
  g_live_storage.erase(it);
  g_storage_owner.erase(d);
  HIP_TRY(hipFree(d));
  return LASER_HIP_OK;
}
int laser_hip_storage_trim(void) {
  if (int rc = ensure_init()) return rc;
  storage_trim();
  return LASER_HIP_OK;
}
// Host <-> device copies of a storage, ORDERED on `stream` (after the kernels already queued there that produce or
// still read the block) and complete when the call returns.  The plain forms use the NULL stream, which does not
// wait for non-blocking streams: a caller that computes on its own stream passes that stream here.
int laser_hip_storage_upload_stream(void *d, const void *h, int64_t bytes, void *stream) {
  if (bytes < 0 || (bytes > 0 && (!d || !h))) return fail(LASER_HIP_E_INVALID, "storage_upload: bad argument");
  if (int rc = ensure_init()) return rc;
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(d, h, (size_t)bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  return LASER_HIP_OK;
}
int laser_hip_storage_download_stream(void *h, const void *d, int64_t bytes, void *stream) {
  if (bytes < 0 || (bytes > 0 && (!d || !h))) return fail(LASER_HIP_E_INVALID, "storage_download: bad argument");
  if (int rc = ensure_init()) return rc;
  if (bytes) {
    HIP_TRY(hipMemcpyAsync(h, d, (size_t)bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  }
  return LASER_HIP_OK;
}
int laser_hip_storage_upload(void *d, const void *h, int64_t bytes) { return laser_hip_storage_upload_stream(d, h, bytes, nullptr); }
int laser_hip_storage_download(void *h, const void *d, int64_t bytes) { return laser_hip_storage_download_stream(h, d, bytes, nullptr); }
int laser_hip_storage_set_zero(void *d, int64_t bytes, void *stream) {
  if (bytes < 0 || (bytes > 0 && !d)) return fail(LASER_HIP_E_INVALID, "storage_set_zero: bad argument");
  if (int rc = ensure_init()) return rc;
  if (bytes) HIP_TRY(hipMemsetAsync(d, 0, (size_t)bytes, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_copy_strided_b32_dev(void *dst, const int64_t *ds, const void *src, const int64_t *ss,
                                   const int64_t *shape, int rank, void *stream) {
  return copy_strided_api<uint32_t>(dst, ds, src, ss, shape, rank, stream);
}
int laser_hip_copy_strided_b64_dev(void *dst, const int64_t *ds, const void *src, const int64_t *ss,
                                   const int64_t *shape, int rank, void *stream) {
  return copy_strided_api<uint64_t>(dst, ds, src, ss, shape, rank, stream);
}

}  // extern "C"  (a template follows)

// ---- elementwise map over strided views: the device twin of forEach (map_strided.hip) ---------------------------
namespace {
template <typename T>
int map_api(int op, bool binary, T *dst, const int64_t *ds, const T *a, const int64_t *as, const T *b, const int64_t *bs,
            const int64_t *shape, int rank, T alpha, T beta, void *stream) {
  if (rank < 0 || rank > kMaxRank) return fail(LASER_HIP_E_INVALID, "rank %d outside 0..%d (LASER_MAXRANK)", rank, kMaxRank);
  const bool is_bin = op >= LASER_HIP_MAP_ADD && op <= LASER_HIP_MAP_AXPBY && op != 35;   // (35: the removed DIV -- never a silent copy)
  const bool is_un = op >= LASER_HIP_MAP_COPY && op <= LASER_HIP_MAP_SQUARE;
  if (binary ? !is_bin : !is_un) return fail(LASER_HIP_E_INVALID, "map op %d is not a %s op", op, binary ? "binary" : "unary");
  const int nin = binary ? 2 : (op == LASER_HIP_MAP_FILL ? 0 : 1);
  if (rank > 0 && (!ds || !shape || (nin >= 1 && !as) || (nin >= 2 && !bs))) return fail(LASER_HIP_E_INVALID, "null shape/strides");
  int64_t total = 1;
  for (int d = 0; d < rank; d++) {
    if (shape[d] < 0) return fail(LASER_HIP_E_INVALID, "negative extent");
    total *= shape[d];
  }
  if (int rc = ensure_init()) return rc;
  if (total == 0) return LASER_HIP_OK;
  if (!dst || (nin >= 1 && !a) || (nin >= 2 && !b)) return fail(LASER_HIP_E_INVALID, "null buffer");
  HIP_TRY(launch_map_strided<T>(op, nin, dst, ds, a, as, b, bs, shape, rank, alpha, beta, (hipStream_t)stream));
  return LASER_HIP_OK;
}
}  // namespace

extern "C" {

#define LH_DEF_MAP(SFX, T)                                                                                              \
  int laser_hip_map_strided_unary_##SFX##_dev(int op, T *dst, const int64_t *ds, const T *a, const int64_t *as,          \
                                              const int64_t *shape, int rank, T alpha, T beta, void *stream) {           \
    return map_api<T>(op, false, dst, ds, a, as, nullptr, nullptr, shape, rank, alpha, beta, stream);                    \
  }                                                                                                                     \
  int laser_hip_map_strided_binary_##SFX##_dev(int op, T *dst, const int64_t *ds, const T *a, const int64_t *as,         \
                                               const T *b, const int64_t *bs, const int64_t *shape, int rank,            \
                                               T alpha, T beta, void *stream) {                                         \
    return map_api<T>(op, true, dst, ds, a, as, b, bs, shape, rank, alpha, beta, stream);                                \
  }
LH_DEF_MAP(f32, float)
LH_DEF_MAP(f64, double)
LH_DEF_MAP(i32, int32_t)
LH_DEF_MAP(i64, int64_t)
#undef LH_DEF_MAP

// ---- reductions: laser/primitives/reductions.nim:48-116 in reduce_core.h's order (reduce.hip) --------------------------
}  // extern "C"  (templates follow)
namespace {
template <typename T>
int reduce_api(int op, const T *src, const int64_t *strides, const int64_t *shape, int rank, T *out, void *stream) {
  if (rank < 0 || rank > kMaxRank) return fail(LASER_HIP_E_INVALID, "reduce: rank %d outside 0..%d (LASER_MAXRANK)", rank, kMaxRank);
  if (rank > 0 && (!strides || !shape)) return fail(LASER_HIP_E_INVALID, "reduce: null shape / strides");
  int64_t total = 1;
  for (int d = 0; d < rank; d++) {
    if (shape[d] < 0) return fail(LASER_HIP_E_INVALID, "reduce: negative extent");
    total *= shape[d];
  }
  if (int rc = ensure_init()) return rc;
  if (!out || (total > 0 && !src)) return fail(LASER_HIP_E_INVALID, "reduce: null buffer");
  HIP_TRY(launch_reduce<T>(op, src, strides, shape, rank, out, (hipStream_t)stream));
  return LASER_HIP_OK;
}
// the host-pointer form: through device scratch, synchronous; the same kernels and so the same bits as the _dev form
int reduce_host_f32(int op, const float *data, int64_t len, float *out) {
  if (len < 0 || !out || (len > 0 && !data)) return fail(LASER_HIP_E_INVALID, "reduce: bad argument");
  if (int rc = ensure_init()) return rc;
  HostCall hc;
  if (hc.rc) return hc.rc;
  void *d_src, *d_out;
  if (int rc = scratch_get(0, (size_t)len * sizeof(float), &d_src)) return rc;
  if (int rc = scratch_get(2, sizeof(float), &d_out)) return rc;
  if (len) HIP_TRY(hipMemcpy(d_src, data, (size_t)len * sizeof(float), hipMemcpyHostToDevice));
  const int64_t stride = 1;
  HIP_TRY(launch_reduce<float>(op, (const float *)d_src, &stride, &len, 1, (float *)d_out, nullptr));
  HIP_TRY(hipMemcpy(out, d_out, sizeof(float), hipMemcpyDeviceToHost));
  return LASER_HIP_OK;
}
}  // namespace
extern "C" {
#define LH_DEF_REDUCE(SFX, T)                                                                                           \
  int laser_hip_reduce_sum_##SFX##_dev(const T *src, const int64_t *st, const int64_t *shape, int rank, T *out,       \
                                       void *stream) {                                                                 \
    return reduce_api<T>(0, src, st, shape, rank, out, stream);                                                       \
  }                                                                                                                   \
  int laser_hip_reduce_min_##SFX##_dev(const T *src, const int64_t *st, const int64_t *shape, int rank, T *out,       \
                                       void *stream) {                                                                 \
    return reduce_api<T>(1, src, st, shape, rank, out, stream);                                                       \
  }                                                                                                                   \
  int laser_hip_reduce_max_##SFX##_dev(const T *src, const int64_t *st, const int64_t *shape, int rank, T *out,       \
                                       void *stream) {                                                                 \
    return reduce_api<T>(2, src, st, shape, rank, out, stream);                                                       \
  }
LH_DEF_REDUCE(f32, float)
LH_DEF_REDUCE(f64, double)
LH_DEF_REDUCE(i32, int32_t)
LH_DEF_REDUCE(i64, int64_t)
#undef LH_DEF_REDUCE
int laser_hip_reduce_sum_f32(const float *data, int64_t len, float *out) { return reduce_host_f32(0, data, len, out); }
int laser_hip_reduce_min_f32(const float *data, int64_t len, float *out) { return reduce_host_f32(1, data, len, out); }
int laser_hip_reduce_max_f32(const float *data, int64_t len, float *out) { return reduce_host_f32(2, data, len, out); }

// ---- the elementwise functions on pointwise.h: lexp, llog, the activations with their gradients, lsin / lcos ---------------
// The checks their device entry points share, over nops operands of which strides[0 .. ndst - 1] belong to destinations.
static int pointwise_check(const char *what, int ndst, int nops, const int64_t *const *strides, const int64_t *shape, int rank,
                           int64_t *total) {
  if (rank < 0 || rank > kMaxRank) return fail(LASER_HIP_E_INVALID, "%s: rank %d outside 0..%d (LASER_MAXRANK)", what, rank, kMaxRank);
  if (rank > 0 && !shape) return fail(LASER_HIP_E_INVALID, "%s: null shape / strides", what);
  for (int i = 0; i < nops && rank > 0; i++)
    if (!strides[i]) return fail(LASER_HIP_E_INVALID, "%s: null shape / strides", what);
  *total = 1;
  for (int d = 0; d < rank; d++) {
    if (shape[d] < 0) return fail(LASER_HIP_E_INVALID, "%s: negative extent", what);
    for (int i = 0; i < ndst; i++)
      if (shape[d] > 1 && strides[i][d] == 0) return fail(LASER_HIP_E_INVALID, "%s: stride 0 on a destination (dimension %d)", what, d);
    *total *= shape[d];
  }
  return LASER_HIP_OK;
}
// a device entry point with one source and one destination, around its launch_*_f32
typedef std::function<hipError_t(float *, const int64_t *, const float *, const int64_t *, const int64_t *, int, hipStream_t)> UnaryLaunch;
static int unary_dev(const char *what, float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                     void *stream, const UnaryLaunch &launch) {
  const int64_t *st[2] = {ds, ss};
  int64_t total;
  if (int rc = pointwise_check(what, 1, 2, st, shape, rank, &total)) return rc;
  if (int rc = ensure_init()) return rc;
  if (total == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "%s: null buffer", what);
  HIP_TRY(launch(dst, ds, src, ss, shape, rank, (hipStream_t)stream));
  return LASER_HIP_OK;
}
// the host-pointer form of the same: through device scratch, in place there, synchronous; the same kernel as the _dev form
static int unary_host(const char *what, float *dst, const float *src, int64_t len, const UnaryLaunch &launch) {
  if (len < 0 || (len > 0 && (!dst || !src))) return fail(LASER_HIP_E_INVALID, "%s: bad argument", what);
  if (int rc = ensure_init()) return rc;
  if (len == 0) return LASER_HIP_OK;
  HostCall hc;
  if (hc.rc) return hc.rc;
  void *d_buf;
  if (int rc = scratch_get(0, (size_t)len * sizeof(float), &d_buf)) return rc;
  HIP_TRY(hipMemcpy(d_buf, src, (size_t)len * sizeof(float), hipMemcpyHostToDevice));
  const int64_t stride = 1;
  HIP_TRY(launch((float *)d_buf, &stride, (const float *)d_buf, &stride, &len, 1, nullptr));
  HIP_TRY(hipMemcpy(dst, d_buf, (size_t)len * sizeof(float), hipMemcpyDeviceToHost));
  return LASER_HIP_OK;
}

// ---- lexp and the row softmax: laser/primitives/simd_math/exp_log_*.nim (exp_core.h, exp_softmax.hip) -----------------
int laser_hip_exp_f32_dev(float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                          void *stream) {
  return unary_dev("exp", dst, ds, src, ss, shape, rank, stream, launch_exp_f32);
}
int laser_hip_exp_f32(float *dst, const float *src, int64_t len) { return unary_host("exp", dst, src, len, launch_exp_f32); }
int laser_hip_softmax_rows_f32_dev(float *dst, int64_t dst_row_stride, const float *src, int64_t src_row_stride, int64_t rows,
                                   int64_t n, void *stream) {
  if (n < 1 || n > LASER_HIP_SOFTMAX_MAX_N) return fail(LASER_HIP_E_INVALID, "softmax: row length %lld outside 1..2^26", (long long)n);
  if (rows < 0) return fail(LASER_HIP_E_INVALID, "softmax: negative row count");
  if (dst_row_stride < n || src_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "softmax: row strides %lld / %lld below the row length %lld", (long long)dst_row_stride,
                (long long)src_row_stride, (long long)n);
  if (dst == src && dst_row_stride != src_row_stride) return fail(LASER_HIP_E_INVALID, "softmax: in place needs equal row strides");
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "softmax: null buffer");
  HIP_TRY(launch_softmax_rows_f32(dst, dst_row_stride, src, src_row_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}

int laser_hip_softmax_axis_f32_dev(float *dst, int64_t dst_outer_stride, int64_t dst_axis_stride, const float *src,
                                   int64_t src_outer_stride, int64_t src_axis_stride, int64_t outer, int64_t n, int64_t inner,
                                   void *stream) {
  if (n < 1 || inner < 1 || outer < 0)
    return fail(LASER_HIP_E_INVALID, "softmax_axis: outer %lld, n %lld, inner %lld (outer >= 0, n >= 1, inner >= 1)", (long long)outer,
                (long long)n, (long long)inner);
  if (dst_axis_stride < inner || src_axis_stride < inner)
    return fail(LASER_HIP_E_INVALID, "softmax_axis: axis strides %lld / %lld below inner %lld", (long long)dst_axis_stride,
                (long long)src_axis_stride, (long long)inner);
  const bool rows = inner == 1 && dst_axis_stride == 1 && src_axis_stride == 1;
  if (n > (rows ? LASER_HIP_SOFTMAX_MAX_N : LASER_HIP_SOFTMAX_AXIS_MAX_N))
    return fail(LASER_HIP_E_INVALID,
                rows ? "softmax_axis: axis length %lld outside 1..2^26"
                     : "softmax_axis: axis length %lld past 2^20 on a strided axis (one workgroup walks a whole column; splitting a "
                       "column over workgroups is not built)",
                (long long)n);
  if (outer > 1) {
    const __int128 ext_d = (__int128)(n - 1) * dst_axis_stride + inner, ext_s = (__int128)(n - 1) * src_axis_stride + inner;
    if (dst_outer_stride < ext_d || src_outer_stride < ext_s)
      return fail(LASER_HIP_E_INVALID, "softmax_axis: outer strides %lld / %lld below (n - 1) * axis stride + inner",
                  (long long)dst_outer_stride, (long long)src_outer_stride);
  }
  if (dst == src && (dst_axis_stride != src_axis_stride || (outer > 1 && dst_outer_stride != src_outer_stride)))
    return fail(LASER_HIP_E_INVALID, "softmax_axis: in place needs equal strides");
  if (int rc = ensure_init()) return rc;
  if (outer == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "softmax_axis: null buffer");
  if (rows)  // a single row has no row stride to speak of
    HIP_TRY(launch_softmax_rows_f32(dst, outer > 1 ? dst_outer_stride : n, src, outer > 1 ? src_outer_stride : n, outer, n,
                                    (hipStream_t)stream));
  else
    HIP_TRY(launch_softmax_axis_f32(dst, dst_outer_stride, dst_axis_stride, src, src_outer_stride, src_axis_stride, outer, n, inner,
                                    (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_softmax_axis_plan(int64_t outer, int64_t n, int64_t inner, int vec, int cus, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "softmax_axis_plan: null out4");
  long long p[4];
  if (lh_softmax_axis_plan(outer, n, inner, vec, cus, p) != 0)
    return fail(LASER_HIP_E_INVALID, "softmax_axis_plan: outer %lld, n %lld, inner %lld outside what softmax_axis takes", (long long)outer,
                (long long)n, (long long)inner);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}

// ---- llog, logsumexp, log-softmax and the softmax cross-entropy (log_core.h, log_softmax.hip, softmax_rows_plan.h) --------
int laser_hip_log_f32_dev(float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                          void *stream) {
  return unary_dev("log", dst, ds, src, ss, shape, rank, stream, launch_log_f32);
}
int laser_hip_log_f32(float *dst, const float *src, int64_t len) { return unary_host("log", dst, src, len, launch_log_f32); }
// ---- relu, ltanh, lsigmoid and their gradients from the output (act_core.h, activation.hip) -----------------------------------
static int act_code_check(const char *what, int act) {
  if (act != LASER_HIP_ACT_RELU && act != LASER_HIP_ACT_TANH && act != LASER_HIP_ACT_SIGMOID)
    return fail(LASER_HIP_E_INVALID, "%s: act %d is not LASER_HIP_ACT_RELU, _TANH or _SIGMOID", what, act);
  return LASER_HIP_OK;
}
int laser_hip_act_f32_dev(int act, float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                          void *stream) {
  if (int rc = act_code_check("act", act)) return rc;
  return unary_dev("act", dst, ds, src, ss, shape, rank, stream, [act](auto... a) { return launch_act_f32(act, a...); });
}
int laser_hip_act_f32(int act, float *dst, const float *src, int64_t len) {
  if (int rc = act_code_check("act", act)) return rc;
  return unary_host("act", dst, src, len, [act](auto... a) { return launch_act_f32(act, a...); });
}
int laser_hip_act_grad_f32_dev(int act, float *dx, const int64_t *dxs, const float *dy, const int64_t *dys, const float *y,
                               const int64_t *ys, const int64_t *shape, int rank, void *stream) {
  if (int rc = act_code_check("act_grad", act)) return rc;
  const int64_t *st[3] = {dxs, dys, ys};
  int64_t total;
  if (int rc = pointwise_check("act_grad", 1, 3, st, shape, rank, &total)) return rc;
  if (int rc = ensure_init()) return rc;
  if (total == 0) return LASER_HIP_OK;
  if (!dx || !dy || !y) return fail(LASER_HIP_E_INVALID, "act_grad: null buffer");
  HIP_TRY(launch_act_grad_f32(act, dx, dxs, dy, dys, y, ys, shape, rank, (hipStream_t)stream));
  return LASER_HIP_OK;
}
// ---- dense-layer backward: dz = dy * f'(y) and the bias gradient in one pass (act_grad_core.h, dense_grad.hip, bias_grad_plan.h) ---
int laser_hip_bias_grad_f32_dev(float *db, int64_t db_stride, float *dz, int64_t dz_row_stride, const float *dy, int64_t dy_row_stride,
                                const float *y, int64_t y_row_stride, int64_t rows, int64_t n, int act, void *stream) {
  if (rows < 0 || n < 0 || rows > LASER_HIP_BIAS_GRAD_MAX_ROWS)
    return fail(LASER_HIP_E_INVALID, "bias_grad: rows %lld, n %lld (0 <= rows <= 2^26, n >= 0)", (long long)rows, (long long)n);
  if (act != LASER_HIP_ACT_NONE && act != LASER_HIP_ACT_RELU && act != LASER_HIP_ACT_TANH && act != LASER_HIP_ACT_SIGMOID)
    return fail(LASER_HIP_E_INVALID, "bias_grad: act %d is not LASER_HIP_ACT_NONE, _RELU, _TANH or _SIGMOID", act);
  const bool has_y = act != LASER_HIP_ACT_NONE;
  if (dy_row_stride < n || (dz && dz_row_stride < n) || (has_y && y_row_stride < n))
    return fail(LASER_HIP_E_INVALID, "bias_grad: row strides %lld (dz) / %lld (dy) / %lld (y) below n %lld", (long long)dz_row_stride,
                (long long)dy_row_stride, (long long)y_row_stride, (long long)n);
  if (dz && ((dz == dy && dz_row_stride != dy_row_stride) || (has_y && dz == y && dz_row_stride != y_row_stride)))
    return fail(LASER_HIP_E_INVALID, "bias_grad: dz in place over dy or y needs equal row strides");
  long long plan[4];
  if (lh_bias_grad_plan(rows, n, 0, 0, plan) != 0)
    return fail(LASER_HIP_E_INVALID, "bias_grad: rows %lld x n %lld is past what the chunk partials can address", (long long)rows,
                (long long)n);
  // (what is never touched may be null: everything when n == 0, dy and y when rows == 0)
  if (n > 0 && (!db || (rows > 0 && (!dy || (has_y && !y))))) return fail(LASER_HIP_E_INVALID, "bias_grad: null buffer");
  if (int rc = ensure_init()) return rc;
  if (n == 0) return LASER_HIP_OK;
  HIP_TRY(launch_bias_grad_f32(db, db_stride, dz, dz_row_stride, dy, dy_row_stride, y, y_row_stride, rows, n, act, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_bias_grad_last_kernel(void) { return g_last_bias_grad_kernel; }
int laser_hip_bias_grad_plan(int64_t rows, int64_t n, int vec, int cus, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "bias_grad_plan: null out4");
  long long p[4];
  if (lh_bias_grad_plan(rows, n, vec, cus, p) != 0)
    return fail(LASER_HIP_E_INVALID, "bias_grad_plan: rows %lld, n %lld outside what bias_grad takes", (long long)rows, (long long)n);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}
// ---- layer normalization forward and backward (layer_norm.hip, layer_norm_plan.h) -------------------------------------------------
int laser_hip_layer_norm_f32_dev(float *y, int64_t y_row_stride, float *mean, int64_t mean_stride, float *rstd, int64_t rstd_stride,
                                 const float *x, int64_t x_row_stride, const float *gamma, int64_t gamma_stride, const float *beta,
                                 int64_t beta_stride, int64_t rows, int64_t n, float eps, void *stream) {
  if (rows < 0 || n < 1 || n > LASER_HIP_LAYER_NORM_MAX_N)
    return fail(LASER_HIP_E_INVALID, "layer_norm: rows %lld, n %lld (rows >= 0, 1 <= n <= 2^26)", (long long)rows, (long long)n);
  if (!(eps >= 0.0f)) return fail(LASER_HIP_E_INVALID, "layer_norm: eps %g (eps >= 0 is needed)", (double)eps);
  if (y_row_stride < n || x_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "layer_norm: row strides %lld (y) / %lld (x) below n %lld", (long long)y_row_stride,
                (long long)x_row_stride, (long long)n);
  if ((mean && mean_stride < 1) || (rstd && rstd_stride < 1))
    return fail(LASER_HIP_E_INVALID, "layer_norm: strides %lld (mean) / %lld (rstd) below 1", (long long)mean_stride, (long long)rstd_stride);
  if (y && y == x && y_row_stride != x_row_stride) return fail(LASER_HIP_E_INVALID, "layer_norm: y in place over x needs equal row strides");
  if (rows > 0 && (!y || !x)) return fail(LASER_HIP_E_INVALID, "layer_norm: null buffer");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_layer_norm_f32(y, y_row_stride, mean, mean_stride, rstd, rstd_stride, x, x_row_stride, gamma, gamma_stride, beta,
                                beta_stride, rows, n, eps, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_layer_norm_grad_f32_dev(float *dx, int64_t dx_row_stride, float *dgamma, int64_t dgamma_stride, float *dbeta,
                                      int64_t dbeta_stride, const float *dy, int64_t dy_row_stride, const float *x, int64_t x_row_stride,
                                      const float *mean, int64_t mean_stride, const float *rstd, int64_t rstd_stride, const float *gamma,
                                      int64_t gamma_stride, int64_t rows, int64_t n, void *stream) {
  if (rows < 0 || n < 1 || n > LASER_HIP_LAYER_NORM_MAX_N)
    return fail(LASER_HIP_E_INVALID, "layer_norm_grad: rows %lld, n %lld (rows >= 0, 1 <= n <= 2^26)", (long long)rows, (long long)n);
  if (!dx && !dgamma && !dbeta) return fail(LASER_HIP_E_INVALID, "layer_norm_grad: none of dx, dgamma and dbeta is asked for");
  if ((dgamma || dbeta) && rows > LASER_HIP_LAYER_NORM_MAX_ROWS)
    return fail(LASER_HIP_E_INVALID, "layer_norm_grad: rows %lld with a parameter gradient (rows <= 2^26)", (long long)rows);
  if (dy_row_stride < n || x_row_stride < n || (dx && dx_row_stride < n))
    return fail(LASER_HIP_E_INVALID, "layer_norm_grad: row strides %lld (dx) / %lld (dy) / %lld (x) below n %lld", (long long)dx_row_stride,
                (long long)dy_row_stride, (long long)x_row_stride, (long long)n);
  if ((dgamma && dgamma_stride < 1) || (dbeta && dbeta_stride < 1))
    return fail(LASER_HIP_E_INVALID, "layer_norm_grad: strides %lld (dgamma) / %lld (dbeta) below 1", (long long)dgamma_stride,
                (long long)dbeta_stride);
  if (dx && ((dx == dy && dx_row_stride != dy_row_stride) || (dx == x && dx_row_stride != x_row_stride)))
    return fail(LASER_HIP_E_INVALID, "layer_norm_grad: dx in place over dy or x needs equal row strides");
  if (rows > 0 && (!dy || !x || !mean || !rstd)) return fail(LASER_HIP_E_INVALID, "layer_norm_grad: null buffer");
  if (int rc = ensure_init()) return rc;
  // the column sums first: they read dy and x as they came, and dx may overwrite either
  HIP_TRY(launch_layer_norm_param_grads_f32(dgamma, dgamma_stride, dbeta, dbeta_stride, dy, dy_row_stride, x, x_row_stride, mean,
                                            mean_stride, rstd, rstd_stride, rows, n, (hipStream_t)stream));
  if (dx)
    HIP_TRY(launch_layer_norm_dx_f32(dx, dx_row_stride, dy, dy_row_stride, x, x_row_stride, mean, mean_stride, rstd, rstd_stride, gamma,
                                     gamma_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_layer_norm_plan(int64_t rows, int64_t n, int vec, int what, int64_t *out) {
  if (!out) return fail(LASER_HIP_E_INVALID, "layer_norm_plan: null out");
  long long p[4];
  if (lh_layer_norm_plan(rows, n, vec, what, p) != 0)
    return fail(LASER_HIP_E_INVALID, "layer_norm_plan: rows %lld, n %lld, what %d outside what layer_norm takes", (long long)rows,
                (long long)n, what);
  for (int i = 0; i < 4; i++) out[i] = p[i];
  return LASER_HIP_OK;
}
int laser_hip_layer_norm_last_kernel(int what) { return what >= 0 && what < 3 ? (int)g_last_layer_norm_kernel[what] : -1; }
// ---- row top-k, argmax and the row gather (select.hip, select_plan.h; include/laser_hip_select.h) ----------------------------------
namespace {
// [p, p + bytes) and [q, q + qbytes) share a byte
bool select_overlap(const void *p, long long bytes, const void *q, long long qbytes) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && bytes > 0 && qbytes > 0 && a < b + (uintptr_t)qbytes && b < a + (uintptr_t)bytes;
}
// bytes from the base of a (rows, len) operand of 4-byte elements to its end (rows >= 1)
long long select_span(int64_t rows, int64_t stride, int64_t len) { return ((rows - 1) * (rows > 1 ? stride : 0) + len) * 4; }
int select_sizes(const char *fn, int64_t rows, int64_t n) {
  if (rows < 0 || rows > LASER_HIP_SELECT_MAX_ROWS)
    return fail(LASER_HIP_E_INVALID, "%s: rows %lld (0 <= rows <= 2^26 is needed)", fn, (long long)rows);
  if (n < 1 || n > LASER_HIP_SELECT_MAX_N) return fail(LASER_HIP_E_INVALID, "%s: row length %lld (1 <= n <= 2^24 is needed)", fn, (long long)n);
  return LASER_HIP_OK;
}
}  // namespace
int laser_hip_topk_rows_f32_dev(float *d_vals, int64_t vals_row_stride, int32_t *d_idx, int64_t idx_row_stride, const float *d_src,
                                int64_t src_row_stride, int64_t rows, int64_t n, int64_t k, int largest, void *stream) {
  if (int rc = select_sizes("topk", rows, n)) return rc;
  if (k < 1 || k > n || k > LASER_HIP_SELECT_MAX_K)
    return fail(LASER_HIP_E_INVALID, "topk: k %lld (1 <= k <= min(n, 1024) is needed; n %lld)", (long long)k, (long long)n);
  if (largest != 0 && largest != 1) return fail(LASER_HIP_E_INVALID, "topk: largest %d (0 or 1)", largest);
  if (rows == 0) return LASER_HIP_OK;
  if (!d_vals && !d_idx) return fail(LASER_HIP_E_INVALID, "topk: neither values nor indices are asked for");
  if (!d_src) return fail(LASER_HIP_E_INVALID, "topk: null source");
  if (rows > 1 && (src_row_stride < n || (d_vals && vals_row_stride < k) || (d_idx && idx_row_stride < k)))
    return fail(LASER_HIP_E_INVALID, "topk: row strides %lld (source, >= n %lld) / %lld (values) / %lld (indices, >= k %lld)",
                (long long)src_row_stride, (long long)n, (long long)vals_row_stride, (long long)idx_row_stride, (long long)k);
  const long long src_bytes = select_span(rows, src_row_stride, n);
  if (select_overlap(d_vals, select_span(rows, vals_row_stride, k), d_src, src_bytes) ||
      select_overlap(d_idx, select_span(rows, idx_row_stride, k), d_src, src_bytes))
    return fail(LASER_HIP_E_INVALID, "topk: an output overlaps the source (no overlap is allowed)");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_topk_rows_f32(d_vals, vals_row_stride, d_idx, idx_row_stride, d_src, src_row_stride, rows, n, k, largest,
                               (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_argmax_rows_f32_dev(int32_t *d_idx, int64_t idx_stride, float *d_val, int64_t val_stride, const float *d_src,
                                  int64_t src_row_stride, int64_t rows, int64_t n, int largest, void *stream) {
  if (int rc = select_sizes("argmax", rows, n)) return rc;
  if (largest != 0 && largest != 1) return fail(LASER_HIP_E_INVALID, "argmax: largest %d (0 or 1)", largest);
  if (rows == 0) return LASER_HIP_OK;
  if (!d_idx || !d_src) return fail(LASER_HIP_E_INVALID, "argmax: null buffer");
  if (rows > 1 && (src_row_stride < n || idx_stride < 1 || (d_val && val_stride < 1)))
    return fail(LASER_HIP_E_INVALID, "argmax: strides %lld (source, >= n %lld) / %lld (indices) / %lld (values, >= 1)",
                (long long)src_row_stride, (long long)n, (long long)idx_stride, (long long)val_stride);
  const long long src_bytes = select_span(rows, src_row_stride, n);
  if (select_overlap(d_idx, select_span(rows, idx_stride, 1), d_src, src_bytes) ||
      select_overlap(d_val, select_span(rows, val_stride, 1), d_src, src_bytes))
    return fail(LASER_HIP_E_INVALID, "argmax: an output overlaps the source (no overlap is allowed)");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_argmax_rows_f32(d_idx, idx_stride, d_val, val_stride, d_src, src_row_stride, rows, n, largest, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_take_rows_i32_dev(int32_t *d_out, int64_t out_row_stride, const int32_t *d_src, int64_t src_row_stride,
                                const int32_t *d_j, int64_t j_row_stride, int64_t rows, int64_t m, int64_t num, void *stream) {
  if (int rc = select_sizes("take_rows", rows, m)) return rc;
  if (num < 0 || num > LASER_HIP_SELECT_MAX_N) return fail(LASER_HIP_E_INVALID, "take_rows: num %lld (0 <= num <= 2^24 is needed)", (long long)num);
  if (rows == 0 || num == 0) return LASER_HIP_OK;
  if (!d_out || !d_src || !d_j) return fail(LASER_HIP_E_INVALID, "take_rows: null buffer");
  if (rows > 1 && (src_row_stride < m || out_row_stride < num || j_row_stride < num))
    return fail(LASER_HIP_E_INVALID, "take_rows: row strides %lld (source, >= m %lld) / %lld (out) / %lld (j, >= num %lld)",
                (long long)src_row_stride, (long long)m, (long long)out_row_stride, (long long)j_row_stride, (long long)num);
  const long long out_bytes = select_span(rows, out_row_stride, num);
  if (select_overlap(d_out, out_bytes, d_src, select_span(rows, src_row_stride, m)) ||
      select_overlap(d_out, out_bytes, d_j, select_span(rows, j_row_stride, num)))
    return fail(LASER_HIP_E_INVALID, "take_rows: out overlaps src or j (no overlap is allowed)");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_take_rows_i32(d_out, out_row_stride, d_src, src_row_stride, d_j, j_row_stride, rows, m, num, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_topk_plan(int64_t rows, int64_t n, int64_t k, int vec, int64_t *out3) {
  if (!out3) return fail(LASER_HIP_E_INVALID, "topk_plan: null out3");
  long long p[3];
  if (lh_topk_plan(rows, n, k, vec, p) != 0)
    return fail(LASER_HIP_E_INVALID, "topk_plan: rows %lld, n %lld, k %lld outside 0..2^26, 1..2^24, 1..min(n, 1024)", (long long)rows,
                (long long)n, (long long)k);
  for (int i = 0; i < 3; i++) out3[i] = p[i];
  return LASER_HIP_OK;
}
int laser_hip_topk_last_kernel(void) { return g_last_topk_kernel; }
// ---- the softmax gradient from the output (softmax_grad.hip; lh_softmax_grad_rows_plan in softmax_rows_plan.h) --------------------
int laser_hip_softmax_grad_rows_f32_dev(float *dx, int64_t dx_row_stride, const float *dy, int64_t dy_row_stride, const float *y,
                                        int64_t y_row_stride, int64_t rows, int64_t n, void *stream) {
  if (n < 1 || n > LASER_HIP_SOFTMAX_MAX_N) return fail(LASER_HIP_E_INVALID, "softmax_grad: row length %lld outside 1..2^26", (long long)n);
  if (rows < 0) return fail(LASER_HIP_E_INVALID, "softmax_grad: negative row count");
  if (dx_row_stride < n || dy_row_stride < n || y_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "softmax_grad: row strides %lld (dx) / %lld (dy) / %lld (y) below the row length %lld",
                (long long)dx_row_stride, (long long)dy_row_stride, (long long)y_row_stride, (long long)n);
  if (dx && ((dx == dy && dx_row_stride != dy_row_stride) || (dx == y && dx_row_stride != y_row_stride)))
    return fail(LASER_HIP_E_INVALID, "softmax_grad: dx in place over dy or y needs equal row strides");
  if (rows > 0 && (!dx || !dy || !y)) return fail(LASER_HIP_E_INVALID, "softmax_grad: null buffer");
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  HIP_TRY(launch_softmax_grad_rows_f32(dx, dx_row_stride, dy, dy_row_stride, y, y_row_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_softmax_grad_plan(int64_t rows, int64_t n, int vec, int64_t *out3) {
  if (!out3) return fail(LASER_HIP_E_INVALID, "softmax_grad_plan: null out3");
  long long p[3];
  if (lh_softmax_grad_rows_plan(rows, n, vec, p) != 0)
    return fail(LASER_HIP_E_INVALID, "softmax_grad_plan: rows %lld, n %lld outside what softmax_grad takes", (long long)rows, (long long)n);
  for (int i = 0; i < 3; i++) out3[i] = p[i];
  return LASER_HIP_OK;
}
int laser_hip_softmax_grad_last_kernel(void) { return g_last_softmax_grad_kernel; }
// ---- the fused attention forward (attention.hip, attention_plan.h) ----------------------------------------------------------------
namespace {
// the limits of "Attention", each with its own text
int attention_sizes(const char *who, int64_t bh_b, int64_t bh_h, int64_t tq, int64_t tk, int64_t d, int64_t dv, int causal) {
  if (bh_b < 0 || bh_h < 0) return fail(LASER_HIP_E_INVALID, "%s: batch %lld, heads %lld (both >= 0)", who, (long long)bh_b, (long long)bh_h);
  if (tq < 0) return fail(LASER_HIP_E_INVALID, "%s: Tq %lld (Tq >= 0)", who, (long long)tq);
  if (tk < 1 || tk > LASER_HIP_ATTENTION_MAX_KEYS)
    return fail(LASER_HIP_E_INVALID, "%s: Tk %lld outside 1..LASER_HIP_ATTENTION_MAX_KEYS = %d", who, (long long)tk, LASER_HIP_ATTENTION_MAX_KEYS);
  if (d < 1 || d > LASER_HIP_ATTENTION_MAX_D)
    return fail(LASER_HIP_E_INVALID, "%s: d %lld outside 1..LASER_HIP_ATTENTION_MAX_D = %d", who, (long long)d, LASER_HIP_ATTENTION_MAX_D);
  if (dv < 1 || dv > LASER_HIP_ATTENTION_MAX_D)
    return fail(LASER_HIP_E_INVALID, "%s: dv %lld outside 1..LASER_HIP_ATTENTION_MAX_D = %d", who, (long long)dv, LASER_HIP_ATTENTION_MAX_D);
  if (causal && tq > tk) return fail(LASER_HIP_E_INVALID, "%s: causal with Tq %lld > Tk %lld", who, (long long)tq, (long long)tk);
  long long p[5];
  if (bh_h != 0 && bh_b > (1ll << 40) / bh_h) return fail(LASER_HIP_E_INVALID, "%s: batch * heads past 2^40", who);
  if (lh_attention_plan(bh_b * bh_h, tq, tk, d, dv, causal, 1, p) != 0)
    return fail(LASER_HIP_E_INVALID, "%s: batch * heads * ceil(Tq / %d) past 2^40 query blocks", who, LH_ATTENTION_BM);
  return LASER_HIP_OK;
}
// strides {batch, head, position} of an operand of (B, H, T, width): none negative, rows apart by at least their length
int attention_strides(const char *name, const int64_t *st, int64_t t, int64_t width) {
  if (!st) return fail(LASER_HIP_E_INVALID, "attention: null strides of %s", name);
  if (st[0] < 0 || st[1] < 0 || st[2] < 0 || (t > 1 && st[2] < width))
    return fail(LASER_HIP_E_INVALID, "attention: strides {%lld, %lld, %lld} of %s (none negative, position stride >= %lld)", (long long)st[0],
                (long long)st[1], (long long)st[2], name, (long long)width);
  return LASER_HIP_OK;
}
}  // namespace
int laser_hip_attention_f32_dev(float *d_out, const int64_t *out_strides, const float *d_q, const int64_t *q_strides, const float *d_k,
                                const int64_t *k_strides, const float *d_v, const int64_t *v_strides, float *d_probs,
                                const int64_t *probs_strides, float *d_row_max, float *d_row_sum, int64_t batch, int64_t heads,
                                int64_t tq, int64_t tk, int64_t d, int64_t dv, float scale, int causal, void *stream) {
  if (int rc = attention_sizes("attention", batch, heads, tq, tk, d, dv, causal)) return rc;
  if (!d_out && !d_probs && !d_row_max && !d_row_sum)
    return fail(LASER_HIP_E_INVALID, "attention: none of out, probs, row_max and row_sum is asked for");
  if (int rc = attention_strides("q", q_strides, tq, d)) return rc;
  if (int rc = attention_strides("k", k_strides, tk, d)) return rc;
  if (int rc = attention_strides("v", v_strides, tk, dv)) return rc;
  if (d_out)
    if (int rc = attention_strides("out", out_strides, tq, dv)) return rc;
  if (d_probs)
    if (int rc = attention_strides("probs", probs_strides, tq, tk)) return rc;
  const bool any = batch > 0 && heads > 0 && tq > 0;
  if (any && (!d_q || !d_k || !d_v)) return fail(LASER_HIP_E_INVALID, "attention: null buffer");
  const void *outs[4] = {d_out, d_probs, d_row_max, d_row_sum}, *ins[3] = {d_q, d_k, d_v};
  for (int i = 0; i < 4; i++) {
    for (int j = 0; j < 3; j++)
      if (outs[i] && outs[i] == ins[j]) return fail(LASER_HIP_E_INVALID, "attention: an output may not overlap an input");
    for (int j = 0; j < i; j++)
      if (outs[i] && outs[i] == outs[j]) return fail(LASER_HIP_E_INVALID, "attention: the outputs may not overlap each other");
  }
  if (int rc = ensure_init()) return rc;
  if (!any) return LASER_HIP_OK;
  HIP_TRY(launch_attention_f32(d_out, out_strides, d_q, q_strides, d_k, k_strides, d_v, v_strides, d_probs, probs_strides, d_row_max,
                               d_row_sum, batch, heads, tq, tk, d, dv, scale, causal, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_attention_plan(int64_t bh, int64_t tq, int64_t tk, int64_t d, int64_t dv, int causal, int vec, int64_t *out5) {
  if (!out5) return fail(LASER_HIP_E_INVALID, "attention_plan: null out5");
  long long p[5];
  if (lh_attention_plan(bh, tq, tk, d, dv, causal, vec, p) != 0)
    return fail(LASER_HIP_E_INVALID, "attention_plan: bh %lld, Tq %lld, Tk %lld, d %lld, dv %lld, causal %d outside what attention takes",
                (long long)bh, (long long)tq, (long long)tk, (long long)d, (long long)dv, causal);
  for (int i = 0; i < 5; i++) out5[i] = p[i];
  return LASER_HIP_OK;
}
int laser_hip_attention_last_kernel(void) { return g_last_attention_kernel; }
// ---- the embedding layer: row gather, stable grouping by id, deterministic gradient (embedding.hip, embedding_plan.h) ------------
namespace {
int embedding_sizes(const char *who, int64_t tokens, int64_t vocab, int64_t dim) {
  if (tokens < 0 || tokens > LASER_HIP_EMBEDDING_MAX_TOKENS || vocab < 0 || vocab > LASER_HIP_EMBEDDING_MAX_VOCAB || dim < 0)
    return fail(LASER_HIP_E_INVALID, "%s: tokens %lld, vocab %lld, dim %lld (0 <= tokens <= 2^26, 0 <= vocab <= 2^30, dim >= 0)", who,
                (long long)tokens, (long long)vocab, (long long)dim);
  return LASER_HIP_OK;
}
}  // namespace
int laser_hip_embedding_f32_dev(float *y, int64_t y_row_stride, const float *w, int64_t w_row_stride, const int32_t *idx, int64_t tokens,
                                int64_t vocab, int64_t dim, void *stream) {
  if (int rc = embedding_sizes("embedding", tokens, vocab, dim)) return rc;
  if (y_row_stride < dim || w_row_stride < dim)
    return fail(LASER_HIP_E_INVALID, "embedding: row strides %lld (y) / %lld (w) below dim %lld", (long long)y_row_stride,
                (long long)w_row_stride, (long long)dim);
  // (what is never touched may be null: idx without tokens, y and w without tokens or columns, w without a vocabulary)
  if (tokens > 0 && (!idx || (dim > 0 && (!y || (vocab > 0 && !w))))) return fail(LASER_HIP_E_INVALID, "embedding: null buffer");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_embedding_f32(y, y_row_stride, w, w_row_stride, idx, tokens, vocab, dim, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_embedding_group_i32_dev(int32_t *order, int32_t *starts, const int32_t *idx, int64_t tokens, int64_t vocab, void *stream) {
  if (int rc = embedding_sizes("embedding_group", tokens, vocab, 0)) return rc;
  if (!starts || (tokens > 0 && (!order || !idx))) return fail(LASER_HIP_E_INVALID, "embedding_group: null buffer");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_embedding_group_i32(order, starts, idx, tokens, vocab, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_embedding_grad_f32_dev(float *dw, int64_t dw_row_stride, const float *dy, int64_t dy_row_stride, const int32_t *idx,
                                     const int32_t *order, const int32_t *starts, int64_t tokens, int64_t vocab, int64_t dim,
                                     void *stream) {
  if (int rc = embedding_sizes("embedding_grad", tokens, vocab, dim)) return rc;
  if (dw_row_stride < dim || dy_row_stride < dim)
    return fail(LASER_HIP_E_INVALID, "embedding_grad: row strides %lld (dw) / %lld (dy) below dim %lld", (long long)dw_row_stride,
                (long long)dy_row_stride, (long long)dim);
  if ((order == nullptr) != (starts == nullptr))
    return fail(LASER_HIP_E_INVALID, "embedding_grad: d_order and d_starts are given together or not at all");
  // (dW has no element without a vocabulary or columns: nothing is touched then; dy, idx and order only with tokens)
  if (vocab > 0 && dim > 0 && (!dw || (tokens > 0 && (!dy || !idx)))) return fail(LASER_HIP_E_INVALID, "embedding_grad: null buffer");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_embedding_grad_f32(dw, dw_row_stride, dy, dy_row_stride, idx, order, starts, tokens, vocab, dim, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_embedding_plan(int64_t tokens, int64_t vocab, int64_t dim, int vec, int cus, int64_t *out8) {
  if (!out8) return fail(LASER_HIP_E_INVALID, "embedding_plan: null out8");
  long long p[8];
  if (lh_embedding_plan(tokens, vocab, dim, vec, cus, p) != 0)
    return fail(LASER_HIP_E_INVALID, "embedding_plan: tokens %lld, vocab %lld, dim %lld outside what embedding takes", (long long)tokens,
                (long long)vocab, (long long)dim);
  for (int i = 0; i < 8; i++) out8[i] = p[i];
  return LASER_HIP_OK;
}
int laser_hip_embedding_last_kernel(int what) { return what >= 0 && what < 4 ? (int)g_last_embedding_kernel[what] : -1; }
// ---- optimizer steps over a list of tensors and the global gradient norm (optim_core.h, optim.hip, optim_plan.h) ---------------
// the list of a step or of the norm: judged before a device is looked for
static int optim_list(const char *fn, const int64_t *lens, int count, const void *const *const *lists, const char *const *names, int nlists) {
  if (count < 0 || count > LASER_HIP_OPTIM_MAX_COUNT) return fail(LASER_HIP_E_INVALID, "%s: count %d (0 <= count <= 65536)", fn, count);
  if (count == 0) return LASER_HIP_OK;
  if (!lens) return fail(LASER_HIP_E_INVALID, "%s: null lens", fn);
  for (int a = 0; a < nlists; a++)
    if (!lists[a]) return fail(LASER_HIP_E_INVALID, "%s: null list %s", fn, names[a]);
  for (int k = 0; k < count; k++) {
    if (lens[k] < 0 || lens[k] > LASER_HIP_OPTIM_MAX_LEN)
      return fail(LASER_HIP_E_INVALID, "%s: lens[%d] = %lld (0 <= len <= 2^26)", fn, k, (long long)lens[k]);
    for (int a = 0; a < nlists && lens[k] > 0; a++)
      if (!lists[a][k]) return fail(LASER_HIP_E_INVALID, "%s: %s[%d] is null with lens[%d] = %lld", fn, names[a], k, k, (long long)lens[k]);
  }
  return LASER_HIP_OK;
}
int laser_hip_sgd_step_f32_dev(float *const *d_w, const float *const *d_g, float *const *d_m, const int64_t *lens, int count, float lr,
                               float mu, float wd, int nesterov, float gscale, const float *d_clip, void *stream) {
  if (!d_m && (mu != 0.0f || nesterov))
    return fail(LASER_HIP_E_INVALID, "sgd_step: mu %g, nesterov %d without a momentum list", (double)mu, nesterov);
  const void *const *lists[3] = {(const void *const *)d_w, (const void *const *)d_g, (const void *const *)d_m};
  const char *names[3] = {"d_w", "d_g", "d_m"};
  if (int rc = optim_list("sgd_step", lens, count, lists, names, d_m ? 3 : 2)) return rc;
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_sgd_step_f32(d_w, d_g, d_m, lens, count, lr, mu, wd, nesterov, gscale, d_clip, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_adam_step_f32_dev(float *const *d_w, const float *const *d_g, float *const *d_m, float *const *d_v, const int64_t *lens,
                                int count, float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                                float gscale, const float *d_clip, void *stream) {
  const void *const *lists[4] = {(const void *const *)d_w, (const void *const *)d_g, (const void *const *)d_m, (const void *const *)d_v};
  const char *names[4] = {"d_w", "d_g", "d_m", "d_v"};
  if (int rc = optim_list("adam_step", lens, count, lists, names, 4)) return rc;
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_adam_step_f32(d_w, d_g, d_m, d_v, lens, count, lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale, d_clip,
                               (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_grad_norm_f32_dev(float *d_norm, float *d_clip, const float *const *d_g, const int64_t *lens, int count, float max_norm,
                                void *stream) {
  if (!d_norm && !d_clip) return fail(LASER_HIP_E_INVALID, "grad_norm: neither d_norm nor d_clip is asked for");
  if (!(max_norm >= 0.0f)) return fail(LASER_HIP_E_INVALID, "grad_norm: max_norm %g (max_norm >= 0 is needed; +Inf is allowed)", (double)max_norm);
  const void *const *lists[1] = {(const void *const *)d_g};
  const char *names[1] = {"d_g"};
  if (int rc = optim_list("grad_norm", lens, count, lists, names, 1)) return rc;
  if (int rc = ensure_init()) return rc;
  HIP_TRY(launch_grad_norm_f32(d_norm, d_clip, d_g, lens, count, max_norm, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_adam_bias_correction(float beta, int64_t step, float *out) {
  if (!out) return fail(LASER_HIP_E_INVALID, "adam_bias_correction: null out");
  if (step < 1) return fail(LASER_HIP_E_INVALID, "adam_bias_correction: step %lld (step >= 1 is needed)", (long long)step);
  *out = optim_bias_correction(beta, step);
  return LASER_HIP_OK;
}
int laser_hip_optim_plan(int what, const int64_t *lens, int count, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "optim_plan: null out4");
  long long p[4];
  if (lh_optim_plan(what, lens, count, p) != 0)
    return fail(LASER_HIP_E_INVALID, "optim_plan: what %d, count %d or a length outside what the optimizer steps take", what, count);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}
// ---- lsin, lcos and both at once (sincos_core.h, sincos.hip) ---------------------------------------------------------------------
int laser_hip_sin_f32_dev(float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                          void *stream) {
  return unary_dev("sin", dst, ds, src, ss, shape, rank, stream, launch_sin_f32);
}
int laser_hip_cos_f32_dev(float *dst, const int64_t *ds, const float *src, const int64_t *ss, const int64_t *shape, int rank,
                          void *stream) {
  return unary_dev("cos", dst, ds, src, ss, shape, rank, stream, launch_cos_f32);
}
int laser_hip_sincos_f32_dev(float *sin_dst, const int64_t *sin_strides, float *cos_dst, const int64_t *cos_strides, const float *src,
                             const int64_t *ss, const int64_t *shape, int rank, void *stream) {
  const int64_t *st[3] = {sin_strides, cos_strides, ss};
  int64_t total;
  if (int rc = pointwise_check("sincos", 2, 3, st, shape, rank, &total)) return rc;
  if (int rc = ensure_init()) return rc;
  if (total == 0) return LASER_HIP_OK;
  if (!sin_dst || !cos_dst || !src) return fail(LASER_HIP_E_INVALID, "sincos: null buffer");
  if (sin_dst == cos_dst) return fail(LASER_HIP_E_INVALID, "sincos: the two destinations are the same buffer");
  HIP_TRY(launch_sincos_f32(sin_dst, sin_strides, cos_dst, cos_strides, src, ss, shape, rank, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_sin_f32(float *dst, const float *src, int64_t len) { return unary_host("sin", dst, src, len, launch_sin_f32); }
int laser_hip_cos_f32(float *dst, const float *src, int64_t len) { return unary_host("cos", dst, src, len, launch_cos_f32); }
// the checks the three row entry points share, in the order of the softmax entry point
static int rows_check(const char *what, int64_t src_row_stride, int64_t rows, int64_t n) {
  if (n < 1 || n > LASER_HIP_SOFTMAX_MAX_N) return fail(LASER_HIP_E_INVALID, "%s: row length %lld outside 1..2^26", what, (long long)n);
  if (rows < 0) return fail(LASER_HIP_E_INVALID, "%s: negative row count", what);
  if (src_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "%s: source row stride %lld below the row length %lld", what, (long long)src_row_stride, (long long)n);
  return LASER_HIP_OK;
}
int laser_hip_logsumexp_rows_f32_dev(float *dst, int64_t dst_stride, const float *src, int64_t src_row_stride, int64_t rows,
                                     int64_t n, void *stream) {
  if (int rc = rows_check("logsumexp", src_row_stride, rows, n)) return rc;
  if (dst_stride < 1) return fail(LASER_HIP_E_INVALID, "logsumexp: destination stride %lld below 1", (long long)dst_stride);
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "logsumexp: null buffer");
  HIP_TRY(launch_logsumexp_rows_f32(dst, dst_stride, src, src_row_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_log_softmax_rows_f32_dev(float *dst, int64_t dst_row_stride, const float *src, int64_t src_row_stride, int64_t rows,
                                       int64_t n, void *stream) {
  if (int rc = rows_check("log_softmax", src_row_stride, rows, n)) return rc;
  if (dst_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "log_softmax: destination row stride %lld below the row length %lld", (long long)dst_row_stride,
                (long long)n);
  if (dst == src && dst_row_stride != src_row_stride) return fail(LASER_HIP_E_INVALID, "log_softmax: in place needs equal row strides");
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!dst || !src) return fail(LASER_HIP_E_INVALID, "log_softmax: null buffer");
  HIP_TRY(launch_log_softmax_rows_f32(dst, dst_row_stride, src, src_row_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_softmax_xent_rows_f32_dev(float *loss, int64_t loss_stride, float *grad, int64_t grad_row_stride, const float *src,
                                        int64_t src_row_stride, const int32_t *labels, int64_t rows, int64_t n, float scale,
                                        void *stream) {
  if (int rc = rows_check("softmax_xent", src_row_stride, rows, n)) return rc;
  if (!loss && !grad) return fail(LASER_HIP_E_INVALID, "softmax_xent: neither a loss nor a gradient to write");
  if (loss && loss_stride < 1) return fail(LASER_HIP_E_INVALID, "softmax_xent: loss stride %lld below 1", (long long)loss_stride);
  if (grad && grad_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "softmax_xent: gradient row stride %lld below the row length %lld", (long long)grad_row_stride,
                (long long)n);
  if (grad == src) return fail(LASER_HIP_E_INVALID, "softmax_xent: the gradient may not overwrite the logits (x[label] is read from them)");
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!src || !labels) return fail(LASER_HIP_E_INVALID, "softmax_xent: null buffer");
  HIP_TRY(launch_softmax_xent_rows_f32(loss, loss_stride, grad, grad_row_stride, src, src_row_stride, labels, rows, n, scale,
                                       (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_softmax_rows_plan(int64_t rows, int64_t n, int vec, int64_t *out3) {
  if (!out3) return fail(LASER_HIP_E_INVALID, "softmax_rows_plan: null out3");
  long long p[3];
  if (lh_softmax_rows_plan(rows, n, vec, p) != 0)
    return fail(LASER_HIP_E_INVALID, "softmax_rows_plan: rows %lld, n %lld outside what the row entry points take", (long long)rows,
                (long long)n);
  for (int i = 0; i < 3; i++) out3[i] = p[i];
  return LASER_HIP_OK;
}

// ---- the F+tree weighted sampler: benchmarks/random_sampling/fenwicktree.nim (sampler.hip, sampler_plan.h) ---------------
int laser_hip_sampler_tree_elems(int64_t n, int64_t *elems) {
  if (!elems) return fail(LASER_HIP_E_INVALID, "sampler_tree_elems: null elems");
  long long e;
  if (lh_sampler_tree_elems(n, &e) != 0) return fail(LASER_HIP_E_INVALID, "sampler: row length %lld outside 1..2^24", (long long)n);
  *elems = e;
  return LASER_HIP_OK;
}
int laser_hip_sampler_plan(int64_t rows, int64_t n, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "sampler_plan: null out4");
  long long p[4];
  if (lh_sampler_plan(rows, n, p) != 0)
    return fail(LASER_HIP_E_INVALID, "sampler_plan: rows %lld, n %lld outside what sampler_build takes", (long long)rows, (long long)n);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}
// the checks every sampler call shares, in the order of the softmax entry points; `count` is m or k (1 where there is none)
static int sampler_args(const char *what, int64_t tree_row_stride, int64_t rows, int64_t n, int64_t count) {
  long long elems;
  if (lh_sampler_tree_elems(n, &elems) != 0) return fail(LASER_HIP_E_INVALID, "%s: row length %lld outside 1..2^24", what, (long long)n);
  if (rows < 0 || count < 0) return fail(LASER_HIP_E_INVALID, "%s: negative count", what);
  if (tree_row_stride < elems)
    return fail(LASER_HIP_E_INVALID, "%s: tree row stride %lld below the %lld elements of a tree of %lld leaves", what,
                (long long)tree_row_stride, elems, (long long)n);
  return LASER_HIP_OK;
}
int laser_hip_sampler_build_f32_dev(float *tree, int64_t tree_row_stride, const float *w, int64_t w_row_stride, int64_t rows, int64_t n,
                                    void *stream) {
  if (int rc = sampler_args("sampler_build", tree_row_stride, rows, n, 1)) return rc;
  if (w_row_stride < n)
    return fail(LASER_HIP_E_INVALID, "sampler_build: weight row stride %lld below the row length %lld", (long long)w_row_stride, (long long)n);
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!tree || !w) return fail(LASER_HIP_E_INVALID, "sampler_build: null buffer");
  HIP_TRY(launch_sampler_build_f32(tree, tree_row_stride, w, w_row_stride, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_sampler_sample_f32_dev(int32_t *idx, const float *tree, int64_t tree_row_stride, const float *u01, int64_t rows, int64_t n,
                                     int64_t m, void *stream) {
  if (int rc = sampler_args("sampler_sample", tree_row_stride, rows, n, m)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || m == 0) return LASER_HIP_OK;
  if (!idx || !tree || !u01) return fail(LASER_HIP_E_INVALID, "sampler_sample: null buffer");
  HIP_TRY(launch_sampler_sample_f32(idx, tree, tree_row_stride, u01, rows, n, m, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_sampler_sample_remove_f32_dev(int32_t *idx, float *tree, int64_t tree_row_stride, const float *u01, int64_t rows, int64_t n,
                                            int64_t k, void *stream) {
  if (int rc = sampler_args("sampler_sample_remove", tree_row_stride, rows, n, k)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || k == 0) return LASER_HIP_OK;
  if (!idx || !tree || !u01) return fail(LASER_HIP_E_INVALID, "sampler_sample_remove: null buffer");
  HIP_TRY(launch_sampler_sample_remove_f32(idx, tree, tree_row_stride, u01, rows, n, k, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_sampler_update_f32_dev(float *tree, int64_t tree_row_stride, const int32_t *elem, const float *weight, int64_t rows,
                                     int64_t n, void *stream) {
  if (int rc = sampler_args("sampler_update", tree_row_stride, rows, n, 1)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0) return LASER_HIP_OK;
  if (!tree || !elem || !weight) return fail(LASER_HIP_E_INVALID, "sampler_update: null buffer");
  HIP_TRY(launch_sampler_update_f32(tree, tree_row_stride, elem, weight, rows, n, (hipStream_t)stream));
  return LASER_HIP_OK;
}

int laser_hip_sampler_sample_rng_f32_dev(int32_t *idx, const float *tree, int64_t tree_row_stride, int64_t seed, int64_t subseq,
                                         int64_t offset, int64_t rows, int64_t n, int64_t m, void *stream) {
  if (int rc = sampler_args("sampler_sample_rng", tree_row_stride, rows, n, m)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || m == 0) return LASER_HIP_OK;
  if (!idx || !tree) return fail(LASER_HIP_E_INVALID, "sampler_sample_rng: null buffer");
  HIP_TRY(launch_sampler_sample_rng_f32(idx, tree, tree_row_stride, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, rows, n, m,
                                        (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_sampler_sample_remove_rng_f32_dev(int32_t *idx, float *tree, int64_t tree_row_stride, int64_t seed, int64_t subseq,
                                                int64_t offset, int64_t rows, int64_t n, int64_t k, void *stream) {
  if (int rc = sampler_args("sampler_sample_remove_rng", tree_row_stride, rows, n, k)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || k == 0) return LASER_HIP_OK;
  if (!idx || !tree) return fail(LASER_HIP_E_INVALID, "sampler_sample_remove_rng: null buffer");
  HIP_TRY(launch_sampler_sample_remove_rng_f32(idx, tree, tree_row_stride, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, rows, n, k,
                                               (hipStream_t)stream));
  return LASER_HIP_OK;
}

// ---- row cumsum, searchsorted and the inverse-CDF sampler: bench_multinomial_samplers.nim (scan.hip, scan_core.h, scan_plan.h)
int laser_hip_cumsum_plan(int64_t rows, int64_t n, int elem_size, int cus, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "cumsum_plan: null out4");
  long long p[4];
  if (lh_scan_plan(rows, n, elem_size, cus, p) != 0)
    return fail(LASER_HIP_E_INVALID, "cumsum_plan: rows %lld, n %lld, element size %d outside what cumsum takes", (long long)rows,
                (long long)n, elem_size);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}
// the checks every call of this section shares, in the order of the sampler entry points; `count` is m or k (1 where there is
// none), s0 / s1 the row strides of the call (n where it has fewer than two)
static int scan_args(const char *what, int64_t rows, int64_t n, int64_t count, int64_t s0, int64_t s1) {
  if (n < 1 || n > LH_SCAN_MAX_N) return fail(LASER_HIP_E_INVALID, "%s: row length %lld outside 1..2^24", what, (long long)n);
  if (rows < 0 || count < 0) return fail(LASER_HIP_E_INVALID, "%s: negative count", what);
  if (s0 < n || s1 < n)
    return fail(LASER_HIP_E_INVALID, "%s: row stride %lld below the row length %lld", what, (long long)(s0 < n ? s0 : s1), (long long)n);
  return LASER_HIP_OK;
}
#define LASER_HIP_DEF_SCAN(SFX, T)                                                                                                  \
  int laser_hip_cumsum_##SFX##_dev(T *dst, int64_t dst_row_stride, const T *src, int64_t src_row_stride, int64_t rows, int64_t n,   \
                                   void *stream) {                                                                                  \
    if (int rc = scan_args("cumsum_" #SFX, rows, n, 1, dst_row_stride, src_row_stride)) return rc;                                  \
    if (int rc = ensure_init()) return rc;                                                                                          \
    if (rows == 0) return LASER_HIP_OK;                                                                                             \
    if (!dst || !src) return fail(LASER_HIP_E_INVALID, "cumsum_" #SFX ": null buffer");                                             \
    HIP_TRY(launch_cumsum_##SFX(dst, dst_row_stride, src, src_row_stride, rows, n, (hipStream_t)stream));                           \
    return LASER_HIP_OK;                                                                                                            \
  }                                                                                                                                 \
  int laser_hip_searchsorted_##SFX##_dev(int32_t *idx, const T *a, int64_t a_row_stride, const T *v, int64_t rows, int64_t n,       \
                                         int64_t m, int right, void *stream) {                                                      \
    if (int rc = scan_args("searchsorted_" #SFX, rows, n, m, a_row_stride, n)) return rc;                                           \
    if (int rc = ensure_init()) return rc;                                                                                          \
    if (rows == 0 || m == 0) return LASER_HIP_OK;                                                                                   \
    if (!idx || !a || !v) return fail(LASER_HIP_E_INVALID, "searchsorted_" #SFX ": null buffer");                                   \
    HIP_TRY(launch_searchsorted_##SFX(idx, a, a_row_stride, v, rows, n, m, right, (hipStream_t)stream));                            \
    return LASER_HIP_OK;                                                                                                            \
  }
LASER_HIP_DEF_SCAN(f32, float)
LASER_HIP_DEF_SCAN(f64, double)
LASER_HIP_DEF_SCAN(i32, int32_t)
LASER_HIP_DEF_SCAN(i64, int64_t)
#undef LASER_HIP_DEF_SCAN
int laser_hip_cdf_sample_f32_dev(int32_t *idx, const float *cdf, int64_t cdf_row_stride, const float *u01, int64_t rows, int64_t n,
                                 int64_t m, void *stream) {
  if (int rc = scan_args("cdf_sample", rows, n, m, cdf_row_stride, n)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || m == 0) return LASER_HIP_OK;
  if (!idx || !cdf || !u01) return fail(LASER_HIP_E_INVALID, "cdf_sample: null buffer");
  HIP_TRY(launch_cdf_sample_f32(idx, cdf, cdf_row_stride, u01, rows, n, m, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_cdf_sample_remove_f32_dev(int32_t *idx, float *w, int64_t w_row_stride, float *cdf, int64_t cdf_row_stride,
                                        const float *u01, int64_t rows, int64_t n, int64_t k, void *stream) {
  if (int rc = scan_args("cdf_sample_remove", rows, n, k, w_row_stride, cdf_row_stride)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || k == 0) return LASER_HIP_OK;
  if (!idx || !w || !cdf || !u01) return fail(LASER_HIP_E_INVALID, "cdf_sample_remove: null buffer");
  HIP_TRY(launch_cdf_sample_remove_f32(idx, w, w_row_stride, cdf, cdf_row_stride, u01, rows, n, k, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_cdf_sample_rng_f32_dev(int32_t *idx, const float *cdf, int64_t cdf_row_stride, int64_t seed, int64_t subseq,
                                     int64_t offset, int64_t rows, int64_t n, int64_t m, void *stream) {
  if (int rc = scan_args("cdf_sample_rng", rows, n, m, cdf_row_stride, n)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || m == 0) return LASER_HIP_OK;
  if (!idx || !cdf) return fail(LASER_HIP_E_INVALID, "cdf_sample_rng: null buffer");
  HIP_TRY(launch_cdf_sample_rng_f32(idx, cdf, cdf_row_stride, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, rows, n, m,
                                    (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_cdf_sample_remove_rng_f32_dev(int32_t *idx, float *w, int64_t w_row_stride, float *cdf, int64_t cdf_row_stride,
                                            int64_t seed, int64_t subseq, int64_t offset, int64_t rows, int64_t n, int64_t k,
                                            void *stream) {
  if (int rc = scan_args("cdf_sample_remove_rng", rows, n, k, w_row_stride, cdf_row_stride)) return rc;
  if (int rc = ensure_init()) return rc;
  if (rows == 0 || k == 0) return LASER_HIP_OK;
  if (!idx || !w || !cdf) return fail(LASER_HIP_E_INVALID, "cdf_sample_remove_rng: null buffer");
  HIP_TRY(launch_cdf_sample_remove_rng_f32(idx, w, w_row_stride, cdf, cdf_row_stride, (uint64_t)seed, (uint64_t)subseq,
                                           (uint64_t)offset, rows, n, k, (hipStream_t)stream));
  return LASER_HIP_OK;
}

// ---- random numbers: Philox4x32-10, the uniform and the normal fills (random.hip, philox_core.h, normal_core.h, random_plan.h)
int laser_hip_random_plan(int64_t n, int words_per_elem, int64_t offset, int dst_misaligned, int cus, int64_t *out4) {
  if (!out4) return fail(LASER_HIP_E_INVALID, "random_plan: null out4");
  long long p[4];
  if (lh_random_plan(n, words_per_elem, (uint64_t)offset, dst_misaligned, cus, p) != 0)
    return fail(LASER_HIP_E_INVALID, "random_plan: n %lld outside 0..2^60 or %d words per element (1 or 2)", (long long)n, words_per_elem);
  for (int i = 0; i < 4; i++) out4[i] = p[i];
  return LASER_HIP_OK;
}
// the checks every fill shares, in the order of the sampler entry points: arguments (`range_ok`: the bounds), the device,
// n = 0, a null pointer; 0 = launch, -1 = done with nothing to do, else the error
static int random_args(const char *what, const void *dst, int64_t n, bool range_ok) {
  if (n < 0 || n > LH_RANDOM_MAX_N) return fail(LASER_HIP_E_INVALID, "%s: n %lld outside 0..2^60", what, (long long)n);
  if (!range_ok) return fail(LASER_HIP_E_INVALID, "%s: lo, hi and hi - lo must be finite and lo <= hi", what);
  if (int rc = ensure_init()) return rc;
  if (n == 0) return -1;
  if (!dst) return fail(LASER_HIP_E_INVALID, "%s: null buffer", what);
  return LASER_HIP_OK;
}
int laser_hip_random_bits_u32_dev(uint32_t *dst, int64_t n, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (int rc = random_args("random_bits_u32", dst, n, true)) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_bits_u32(dst, n, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_random_uniform_f32_dev(float *dst, int64_t n, float lo, float hi, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (int rc = random_args("random_uniform_f32", dst, n, lh_uniform_range_ok_f32(lo, hi))) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_uniform_f32(dst, n, lo, hi, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_random_uniform_f64_dev(double *dst, int64_t n, double lo, double hi, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (int rc = random_args("random_uniform_f64", dst, n, lh_uniform_range_ok_f64(lo, hi))) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_uniform_f64(dst, n, lo, hi, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_random_uniform_i32_dev(int32_t *dst, int64_t n, int32_t lo, int32_t hi, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (int rc = random_args("random_uniform_i32", dst, n, lo <= hi)) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_uniform_i32(dst, n, lo, hi, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_random_uniform_i64_dev(int64_t *dst, int64_t n, int64_t lo, int64_t hi, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (int rc = random_args("random_uniform_i64", dst, n, lo <= hi)) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_uniform_i64(dst, n, lo, hi, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}
int laser_hip_random_normal_f32_dev(float *dst, int64_t n, float mean, float std, int64_t seed, int64_t subseq, int64_t offset, void *stream) {
  if (n >= 0 && n <= LH_RANDOM_MAX_N && !lh_normal_params_ok_f32(mean, std))
    return fail(LASER_HIP_E_INVALID, "random_normal_f32: mean must be finite, std finite and >= 0");
  if (int rc = random_args("random_normal_f32", dst, n, true)) return rc < 0 ? LASER_HIP_OK : rc;
  HIP_TRY(launch_random_normal_f32(dst, n, mean, std, (uint64_t)seed, (uint64_t)subseq, (uint64_t)offset, (hipStream_t)stream));
  return LASER_HIP_OK;
}

// ---- pinned host memory for the host-pointer entry points -----------------------------------------------------------
// Laser leaves buffer management to the caller ("creating or reusing buffers is left at the discretion of the
// high-level lib", Design.md:5-7).  The host-pointer entry points work on any memory; from PAGEABLE memory every
// hipMemcpy is staged or pinned on the fly by the runtime.  A tensor allocator that wants the full PCIe rate allocates
// its buffers here (or registers what it already has): the same entry points then run their uploads / downloads as
// direct asynchronous DMA.  Nothing else changes; results are identical.
int laser_hip_host_alloc(void **host_ptr, int64_t bytes) {
  if (!host_ptr || bytes < 0) return fail(LASER_HIP_E_INVALID, "host_alloc: bad argument");
  if (int rc = ensure_init()) return rc;
  *host_ptr = nullptr;
  if (bytes == 0) return LASER_HIP_OK;
  HIP_TRY(hipHostMalloc(host_ptr, (size_t)bytes, hipHostMallocDefault));
  return LASER_HIP_OK;
}
int laser_hip_host_free(void *host_ptr) {
  if (!host_ptr) return LASER_HIP_OK;
  HIP_TRY(hipHostFree(host_ptr));
  return LASER_HIP_OK;
}
int laser_hip_host_register(void *host_ptr, int64_t bytes) {
  if (!host_ptr || bytes <= 0) return fail(LASER_HIP_E_INVALID, "host_register: bad argument");
  if (int rc = ensure_init()) return rc;
  HIP_TRY(hipHostRegister(host_ptr, (size_t)bytes, hipHostRegisterDefault));
  return LASER_HIP_OK;
}
int laser_hip_host_unregister(void *host_ptr) {
  if (!host_ptr) return fail(LASER_HIP_E_INVALID, "host_unregister: null pointer");
  HIP_TRY(hipHostUnregister(host_ptr));
  return LASER_HIP_OK;
}

int laser_hip_cblas_sgemm(int order, int tA, int tB, int64_t M, int64_t N, int64_t K, float alpha, const float *A,
                          int64_t lda, const float *B, int64_t ldb, float beta, float *C, int64_t ldc) {
  return cblas_gemm<float>(order, tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
}
int laser_hip_cblas_dgemm(int order, int tA, int tB, int64_t M, int64_t N, int64_t K, double alpha,
                          const double *A, int64_t lda, const double *B, int64_t ldb, double beta, double *C,
                          int64_t ldc) {
  return cblas_gemm<double>(order, tA, tB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
}

}  // extern "C"
