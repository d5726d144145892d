// laser_amd/csrc/common.h -- shared host/device declarations of liblaser_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gemm_args.h"

namespace laser_hip {

// Stream-ordered scratch (packing passes, limb planes, slice partials): hipMallocFromPoolAsync on a pool THIS LIBRARY owns (one per
// device, made on first use, destroyed by laser_hip_finalize), with a release threshold of 4 GiB -- at the default (0) every
// synchronisation hands a pool's free memory back to the driver and the next call pays for mapping it again (a packed 4096^3 product
// timed 4 calls per synchronise lost 60 us per call to that: profiles/r04/colmajor_a_probe_v1.jsonl against configs_v5.jsonl).  The
// device's DEFAULT pool belongs to the host application and its other libraries: its threshold is never touched.
// Given back with scratch_free_async (below).  A runtime that cannot make a pool: plain hipMallocAsync.
struct ScratchPools {
  std::atomic<hipMemPool_t> pool[64] = {};
  std::atomic<unsigned long long> failed{0};     // one bit per device ordinal whose pool could not be made
};
inline ScratchPools g_scratch_pools;
inline hipError_t scratch_pool_alloc(void **p, size_t bytes, hipStream_t s);

// In front of the pool, a cache of idle blocks per (device, stream).  A block that scratch_free_async takes back is handed
// out again ONLY on the stream it was freed on, so stream order alone separates its users: no event, no wait, no runtime call.
// It is there because hipFreeAsync waits ON THE HOST when the block it frees was allocated from a free that has not completed
// yet -- the second scratch-taking call queued on a stream that is still busy with (or blocked before) the first would stall
// its caller until the stream drains, which `_dev` calls never do (seen: two reductions queued behind a blocked stream, the
// second returned only when the stream ran; tests/test_gpu_stream_order.py).  A stream that is being captured bypasses the
// cache: its allocations and frees become nodes of the graph, as before.  Idle blocks above kScratchIdleMax go back to the pool.
struct ScratchCache {
  struct Block {
    void *p;
    size_t bytes;
  };
  std::mutex mu;
  std::map<std::pair<int, hipStream_t>, std::vector<Block>> idle;
  std::unordered_map<void *, size_t> owned;     // every block handed out through the cache or idle in it -> its size
  size_t idle_bytes = 0;
};
inline ScratchCache g_scratch_cache;
constexpr size_t kScratchIdleMax = (size_t)4 << 30;
inline bool scratch_capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
    (void)hipGetLastError();
    return true;      // (unknown: the conservative path)
  }
  return cap != hipStreamCaptureStatusNone;
}
inline hipError_t scratch_alloc_async(void **p, size_t bytes, hipStream_t s) {
  if (scratch_capturing(s)) return scratch_pool_alloc(p, bytes, s);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return scratch_pool_alloc(p, bytes, s);
  const size_t want = (std::max<size_t>(bytes, 1) + 4095) & ~(size_t)4095;
  {
    std::lock_guard<std::mutex> lk(g_scratch_cache.mu);
    auto it = g_scratch_cache.idle.find({dev, s});
    if (it != g_scratch_cache.idle.end()) {
      auto &list = it->second;
      size_t best = list.size();
      for (size_t k = 0; k < list.size(); k++)      // the smallest block that fits, and not one far too large
        if (list[k].bytes >= want && list[k].bytes <= 4 * want + ((size_t)1 << 20) && (best == list.size() || list[k].bytes < list[best].bytes))
          best = k;
      if (best != list.size()) {
        *p = list[best].p;
        g_scratch_cache.idle_bytes -= list[best].bytes;
        list.erase(list.begin() + (ptrdiff_t)best);
        return hipSuccess;
      }
    }
  }
  const hipError_t e = scratch_pool_alloc(p, want, s);
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_scratch_cache.mu);
    g_scratch_cache.owned[*p] = want;
  }
  return e;
}
// The end of a scratch block's use on `s`, the stream it was allocated on: everything that reads or writes it is queued.
inline hipError_t scratch_free_async(void *p, hipStream_t s) {
  if (p == nullptr) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_scratch_cache.mu);
    auto it = g_scratch_cache.owned.find(p);
    if (it != g_scratch_cache.owned.end()) {
      int dev = 0;
      const size_t bytes = it->second;
      if (!scratch_capturing(s) && hipGetDevice(&dev) == hipSuccess && g_scratch_cache.idle_bytes + bytes <= kScratchIdleMax) {
        g_scratch_cache.idle[{dev, s}].push_back({p, bytes});
        g_scratch_cache.idle_bytes += bytes;
        return hipSuccess;
      }
      g_scratch_cache.owned.erase(it);
    }
  }
  return hipFreeAsync(p, s);
}
inline hipError_t scratch_pool_alloc(void **p, size_t bytes, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || (g_scratch_pools.failed.load(std::memory_order_relaxed) >> dev & 1ull))
    return hipMallocAsync(p, bytes, s);
  hipMemPool_t pool = g_scratch_pools.pool[dev].load(std::memory_order_acquire);
  if (pool == nullptr) {
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t made = nullptr;
    if (hipMemPoolCreate(&made, &props) != hipSuccess || made == nullptr) {
      (void)hipGetLastError();
      g_scratch_pools.failed.fetch_or(1ull << dev, std::memory_order_relaxed);
      return hipMallocAsync(p, bytes, s);
    }
    uint64_t keep = (uint64_t)4 << 30;
    (void)hipMemPoolSetAttribute(made, hipMemPoolAttrReleaseThreshold, &keep);
    hipMemPool_t expect = nullptr;
    if (g_scratch_pools.pool[dev].compare_exchange_strong(expect, made, std::memory_order_acq_rel)) {
      pool = made;
    } else {      // another host thread made this device's pool first
      (void)hipMemPoolDestroy(made);
      pool = expect;
    }
  }
  return hipMallocFromPoolAsync(p, bytes, pool, s);
}
// laser_hip_finalize: the pools go (every device is idle by then; what they kept returns to the driver)
inline void scratch_pools_trim() {
  {
    std::lock_guard<std::mutex> lk(g_scratch_cache.mu);
    for (auto &kv : g_scratch_cache.idle)
      for (const ScratchCache::Block &b : kv.second) {
        (void)hipFree(b.p);
        g_scratch_cache.owned.erase(b.p);
      }
    g_scratch_cache.idle.clear();
    g_scratch_cache.idle_bytes = 0;
  }
  for (int dev = 0; dev < 64; dev++) {
    hipMemPool_t pool = g_scratch_pools.pool[dev].exchange(nullptr, std::memory_order_acq_rel);
    if (pool != nullptr) (void)hipMemPoolDestroy(pool);
  }
  g_scratch_pools.failed.store(0, std::memory_order_relaxed);
}

// One-time-per-DEVICE initialisation of a kernel (hipFuncSetAttribute acts on the current device's instance of the
// function): a single process may drive all 8 GPUs of a node (the sharded entry points), so "done" is a bit per
// device ordinal, not a per-process flag.
struct PerDeviceOnce {
  std::atomic<uint64_t> mask{0};
  template <typename F>
  hipError_t run(F &&f) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (mask.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = f();
    if (e == hipSuccess) mask.fetch_or(bit, std::memory_order_release);
    return e;
  }
};

// How an operand tile is brought from HBM into its LDS panel image (the GPU analogue of
// pack_A_mc_kc / pack_B_kc_nc, gemm_packing.nim:24-94 -- strides are resolved HERE).
enum LoadMode : int {
  LOAD_VEC_X = 0,  // unit stride along the tile's M/N dimension, 16-B vector loads, full tiles
  LOAD_VEC_K = 1,  // unit stride along k, 16-B vector loads + transposing LDS write, full tiles
  LOAD_GEN_X = 2,  // any strides / ragged edges, scalar predicated loads, lanes run along M/N
  LOAD_GEN_K = 3,  // any strides / ragged edges, scalar predicated loads, lanes run along k
  // 16-B vector loads on ragged problems (extents multiples of 4, not of the tile): addresses are
  // clamped into the operand, quads beyond K are replaced by zeros (Laser zero-pads its panels the
  // same way, gemm_packing.nim:46-55,85-94; rows/cols beyond M/N only feed outputs never stored)
  LOAD_VEC_X_EDGE = 4,
  LOAD_VEC_K_EDGE = 5,
  // B operand only: im2col fused into the loader (implicit-GEMM convolution), lanes run along
  // the output pixel index j = oh*oW + ow, predicated gathers from the NCHW image, zeros for padding
  LOAD_IM2COL = 6,
  LOAD_CONV_PATCH = 7,  // implicit-GEMM conv, B from an LDS-resident input patch: the tile's input rows are loaded once
                        // (contiguous 16-B pieces) and the kH*kW shifted views are gathered by the fragment reads
};

// LOAD_CONV_PATCH geometry for a BK x BN tile: channels a K-tile can touch, input rows reached by BN consecutive output
// pixels (upper bound), and the patch row stride in floats (input column j at index 4 + j).  The row stride is the
// smallest multiple of 4 >= W + 8 that keeps the 32 lanes of a fragment read on 32 distinct LDS banks when their 32
// consecutive output pixels wrap from one output row to the next: the wrap moves the address by PWs*sH - (oW-1)*sW,
// which must be = sW (mod 32).  (With W + 8 = 64 at the 56x56 shape every patch row starts on bank 0 and the wrapped
// lanes collide 2-way: SQ_LDS_BANK_CONFLICT = 13 % of the LDS cycles, profiles/r02/rocprof_conv_c4.)  Returns false if
// no stride fits the B region of an LDS stage (budget = BK*BN - BK - 4 floats).
struct ConvPatchGeom {
  int chm, rp, pws;
};
inline bool conv_patch_geom(int BK, int BN, int W, int oW, int kH, int kW, int sH, int sW, ConvPatchGeom *g) {
  const int khw = kH * kW;
  g->chm = (BK + khw - 2) / khw + 1;
  g->rp = ((BN - 1) / oW + 1) * sH + kH;
  const int64_t budget = (int64_t)BK * BN - BK - 4;
  g->pws = W + 8;
  if ((int64_t)g->chm * g->rp * g->pws > budget) return false;
  for (int p = W + 8; p <= W + 40; p += 4)
    if ((p * sH - oW * sW) % 32 == 0 && (int64_t)g->chm * g->rp * p <= budget) {
      g->pws = p;
      break;
    }
  return true;
}

hipError_t launch_gemm_f32(const GemmArgs<float> &args, int cfg, bool laser_order, hipStream_t s);
hipError_t launch_gemm_f64(const GemmArgs<double> &args, bool laser_order, hipStream_t s);
// float32, unit column strides on A and C, B row-major-like or passed transposed, any alpha / beta / K, enough tiles to fill the
// chip: the hand-scheduled assembly kernels (gemm_f32_asm.cpp, laser_amd/asmgen/); hipErrorNotSupported = not that class, use launch_gemm_f32
hipError_t launch_gemm_f32_asm(const GemmArgs<float> &args, bool laser_order, hipStream_t s);
// implicit-GEMM convolution on the same framework (3x3 kernel, stride 1, padding 0 or 1): output pixels [0, args.N) of every image
hipError_t launch_conv_f32_asm(const GemmArgs<float> &args, bool laser_order, hipStream_t s);
int64_t conv_asm_plan_cut(const GemmArgs<float> &args, bool laser_order);   // pixel cut for an assembly main launch (-1: not its class, 0: none)
int asm_plan_f32(int64_t M, int64_t N, int64_t K, int laser_order, int cus, int64_t out[8]);   // diagnostics: kernel + launch plan for a device of `cus` CUs (no device touched)
const char *asm_error_detail();   // the assembly launcher's explanation of the error it just returned on this thread ("" = none)
int64_t asm_fixup_timeouts();  // diagnostics: fix-ups of cut launches that gave up waiting (0 in a correct run; synchronises the device)
void asm_kernels_release();   // unload the assembly kernels' code objects (laser_hip_finalize)
hipError_t launch_gemm_f64_asm(const GemmArgs<double> &args, bool laser_order, hipStream_t s);
extern std::atomic<int> g_f64_asm, g_last_f64_asm;
hipError_t launch_gemm_i32_asm(const GemmArgs<int32_t> &args, void *ws, hipStream_t s);
hipError_t launch_gemm_i64_asm(const GemmArgs<int64_t> &args, void *ws, hipStream_t s);
extern std::atomic<int> g_i32_asm, g_last_i32_asm, g_int_group_m;
// (the option variables below: include/laser_hip.h documents each under its name -- g_x is option "x", g_last_x is "last_x")
extern std::atomic<int> g_asm_tile;
void asm_set_thread_tile(int tile_class);   // per-thread pin of the same (-2 = none)
int asm_get_thread_tile();
int asm_tile_pin_now();                     // the pin this thread's launches see (-1 = none)
extern std::atomic<int> g_asm_plan, g_asm_kernel, g_asm_wgs, g_asm_slice, g_asm_noseed, g_asm_group_m, g_asm_giveup;   // ("asm_test_giveup")
extern std::atomic<int> g_last_asm_wgs, g_last_asm_slices, g_last_asm_group_m, g_last_asm_rem;
extern std::atomic<int> g_f32_asm, g_last_f32_asm;
// args.B = NCHW input, args.bsB = C*H*W, args.c* = geometry, N = oH*oW, K = C*kH*kW; A = filter
hipError_t launch_conv_implicit_f32(const GemmArgs<float> &args, int cfg, bool laser_order, hipStream_t s);
int gemm_f32_config_count();
const char *gemm_f32_config_name(int cfg);

// matrix-vector-like problems (M <= 8 or N <= 8) as an HBM stream; hipErrorNotSupported = not skinny, use the tiled kernels
template <typename T>
hipError_t launch_gemm_skinny(const GemmArgs<T> &args, bool laser_order, int kc_elems, hipStream_t s);
// small-matrix path (gemm_small.hip): one wave per 32x32 (f64: 16x16) block of C, operands loaded straight into the
// MFMA operand registers; hipErrorNotSupported = not a small problem, use the tiled kernels.  float32 / float64.
template <typename T>
hipError_t launch_gemm_small(const GemmArgs<T> &args, bool laser_order, int kc_elems, hipStream_t s, bool mapped = false);
extern std::atomic<int> g_small_path;
// the dispatch rule of launch_gemm_small (mapped: the operands live in host memory mapped into the device)
bool gemm_small_takes(int elem_size, int64_t M, int64_t N, int64_t K, int64_t batch, bool mapped = false);
template <typename T>
hipError_t launch_gemm_valu(const GemmArgs<T> &args, bool laser_order, hipStream_t s);

// int32 GEMM on the int8 matrix cores (signed 8-bit limb decomposition, bit-exact mod 2^32);
// ws = device scratch of gemm_i32_mfma_workspace_bytes(M, N, K) bytes, valid on stream s.
size_t gemm_i32_mfma_workspace_bytes(int64_t M, int64_t N, int64_t K);
hipError_t launch_gemm_i32_mfma(const GemmArgs<int32_t> &args, void *ws, hipStream_t s);
// int64 GEMM on the int8 matrix cores (eight signed 8-bit limbs, 36 limb products, bit-exact mod 2^64; K in chunks of
// 8192 per launch); ws = device scratch of gemm_i64_mfma_workspace_bytes(M, N, K) bytes, valid on stream s.
size_t gemm_i64_mfma_workspace_bytes(int64_t M, int64_t N, int64_t K);
hipError_t launch_gemm_i64_mfma(const GemmArgs<int64_t> &args, void *ws, hipStream_t s);

// int8 / int16 GEMM (uint8 / uint16 on the same bits) on the int8 matrix cores, bit-exact mod 2^8 / 2^16 (gemm_narrow_mfma.hip):
// one / two int8 digit planes per operand.  K <= NARROW_MAX_K per launch (the dispatcher chunks longer K);
// ws = device scratch of gemm_narrow_mfma_workspace_bytes<T>(M, N, K) bytes, valid on stream s.
constexpr int64_t NARROW_MAX_K = 16384;
template <typename T>
size_t gemm_narrow_mfma_workspace_bytes(int64_t M, int64_t N, int64_t K);
template <typename T>
hipError_t launch_gemm_narrow_mfma(const GemmArgs<T> &args, void *ws, hipStream_t s);
extern std::atomic<int> g_conv_direct, g_conv_patch, g_conv_walk, g_conv_cut_always, g_conv_tail, g_conv_kslice, g_last_conv_tail;
hipError_t launch_conv_direct_small_f32(const GemmArgs<float> &a, hipStream_t s);
hipError_t launch_conv_tail_f32(const GemmArgs<float> &a, int kc, hipStream_t s);
extern std::atomic<int> g_split_tail, g_last_f32_cfg;   // ("last_f32_config")
extern std::atomic<int64_t> g_last_split;
hipError_t launch_transpose_batched(void *dst, const void *src, int64_t N, int64_t NR, int64_t NC,
                                    int elem_size, hipStream_t s);
hipError_t launch_transpose_pitched(void *dst, int64_t ld_dst, const void *src, int64_t ld_src, int64_t NR, int64_t NC, int elem_size,
                                    hipStream_t s);
extern std::atomic<int> g_im2col_band;
hipError_t launch_im2col(void *ws, int64_t oH, int64_t oW, const void *in, int64_t batch, int64_t C, int64_t H, int64_t W, int64_t kH,
                         int64_t kW, int64_t pH, int64_t pW, int64_t sH, int64_t sW, int elem_size, hipStream_t s);
hipError_t launch_im2col_f32(float *ws, int64_t oH, int64_t oW, const float *in, int64_t batch,
                             int64_t C, int64_t H, int64_t W, int64_t kH, int64_t kW, int64_t pH,
                             int64_t pW, int64_t sH, int64_t sW, hipStream_t s);
// dst[r*ld + c] = (r < R && c < Ccols) ? src[r*rs + c*cs] : 0 for r < Rpad, c < Cpad
// ordered combine of per-kc-slice partial products W[nsl][M][N] into C (slice-parallel GEMM)
template <typename E>
hipError_t launch_combine_slices(E *C, int64_t rsC, int64_t csC, const E *W, int64_t M, int64_t N, int nsl, E alpha, E beta,
                                 hipStream_t s);
// rank-N strided element copy (tensor deepCopy / copyFrom); LASER_MAXRANK = 6 (laser/dynamic_stack_arrays.nim:6)
constexpr int kMaxRank = 6;
template <typename T>
hipError_t launch_copy_strided(T *dst, const int64_t *dstrides, const T *src, const int64_t *sstrides,
                               const int64_t *shape, int rank, hipStream_t s);
// elementwise map over strided rank <= 6 views (map_strided.hip): dst = f(a [, b]); nin = operands read (0: fill)
template <typename T>
hipError_t launch_map_strided(int op, int nin, T *dst, const int64_t *dstrides, const T *a, const int64_t *astrides, const T *b,
                              const int64_t *bstrides, const int64_t *shape, int rank, T alpha, T beta, hipStream_t s);
// Dimension merging of the strided traversals: extent-1 dimensions dropped, a dimension pair merged when it is contiguous on
// every one of the nops operands (strides[i * rank + d]); never permutes.  Writes the merged strides st[i][..] and extents
// sh[..], returns the merged rank (>= 1).
int merge_dims(int nops, const int64_t *strides, const int64_t *shape, int rank, int64_t (*st)[kMaxRank], int64_t *sh);
// reductions in reduce_core.h's order (reduce.hip): op 0 sum, 1 min, 2 max; the result to the device address `out`
template <typename T>
hipError_t launch_reduce(int op, const T *src, const int64_t *strides, const int64_t *shape, int rank, T *out, hipStream_t s);
extern std::atomic<int> g_last_reduce_variant;
// The levels of a reduction of n elements (reduce.hip; forEachReduce uses it too).  level0(blocks, dst) launches the first
// level (E = e0 elements per lane and step), one partial per workgroup into dst; partials(in, count, blocks, dst) reduces an
// array of `count` accumulators of acc_size bytes.  Intermediate arrays live in stream-ordered scratch.
typedef std::function<hipError_t(int64_t blocks, void *dst)> ReduceLevel0;
typedef std::function<hipError_t(const void *in, int64_t count, int64_t blocks, void *dst)> ReducePartials;
hipError_t reduce_levels(int64_t n, int e0, int acc_size, void *out, hipStream_t s, const ReduceLevel0 &level0,
                         const ReducePartials &partials);
// lexp over strided views (exp_softmax.hip; exp_core.h is the definition of lexp) and the deterministic row softmax (the kSm
// ending of log_softmax.hip's row kernels)
hipError_t launch_exp_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s);
hipError_t launch_softmax_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                   hipStream_t s);
// the softmax along a strided axis of (outer, n, inner), inner unit-stride (softmax_axis.hip; softmax_axis_plan.h picks the kernel)
hipError_t launch_softmax_axis_f32(float *dst, int64_t dst_outer_stride, int64_t dst_axis_stride, const float *src,
                                   int64_t src_outer_stride, int64_t src_axis_stride, int64_t outer, int64_t n, int64_t inner,
                                   hipStream_t s);
extern std::atomic<int> g_last_softmax_kernel;
// llog over strided views, and logsumexp, log-softmax and the softmax cross-entropy over rows (log_softmax.hip; log_core.h is
// the definition of llog, softmax_rows_plan.h picks the kernel).  The cross-entropy writes loss, grad or both (null: not that one).
hipError_t launch_log_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s);
hipError_t launch_logsumexp_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                     hipStream_t s);
hipError_t launch_log_softmax_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                       hipStream_t s);
hipError_t launch_softmax_xent_rows_f32(float *loss, int64_t loss_stride, float *grad, int64_t grad_stride, const float *src,
                                        int64_t sstride, const int32_t *labels, int64_t rows, int64_t n, float scale, hipStream_t s);
// relu, ltanh and lsigmoid over strided views and their gradients from the forward output (activation.hip; act_core.h is the
// definition of ltanh and lsigmoid); act is LASER_HIP_ACT_RELU / TANH / SIGMOID, anything else hipErrorInvalidValue
hipError_t launch_act_f32(int act, float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s);
hipError_t launch_act_grad_f32(int act, float *dx, const int64_t *dxstrides, const float *dy, const int64_t *dystrides, const float *y,
                               const int64_t *ystrides, const int64_t *shape, int rank, hipStream_t s);
// the backward pass of a dense layer's activation and bias (dense_grad.hip; act_grad_core.h is the rule, bias_grad_plan.h the
// launch plan): dz = the gradient rule of (dy, y), or dy for LASER_HIP_ACT_NONE, stored unless dz is null, and db = its column sums
hipError_t launch_bias_grad_f32(float *db, int64_t db_stride, float *dz, int64_t dz_row_stride, const float *dy, int64_t dy_row_stride,
                                const float *y, int64_t y_row_stride, int64_t rows, int64_t n, int act, hipStream_t s);
extern std::atomic<int> g_last_bias_grad_kernel;
// layer normalization over the rows of a matrix (layer_norm.hip; layer_norm_plan.h is the launch plan): the forward pass
// (mean, rstd, gamma and beta may each be null), dx from the saved statistics, and the column sums dgamma and dbeta (either
// may be null).  g_last_layer_norm_kernel[what]: the plan's kernel code of the last launch of each
hipError_t launch_layer_norm_f32(float *y, int64_t y_row_stride, float *mean, int64_t mean_stride, float *rstd, int64_t rstd_stride,
                                 const float *x, int64_t x_row_stride, const float *gamma, int64_t gamma_stride, const float *beta,
                                 int64_t beta_stride, int64_t rows, int64_t n, float eps, hipStream_t s);
hipError_t launch_layer_norm_dx_f32(float *dx, int64_t dx_row_stride, const float *dy, int64_t dy_row_stride, const float *x,
                                    int64_t x_row_stride, const float *mean, int64_t mean_stride, const float *rstd, int64_t rstd_stride,
                                    const float *gamma, int64_t gamma_stride, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_layer_norm_param_grads_f32(float *dgamma, int64_t dgamma_stride, float *dbeta, int64_t dbeta_stride, const float *dy,
                                             int64_t dy_row_stride, const float *x, int64_t x_row_stride, const float *mean,
                                             int64_t mean_stride, const float *rstd, int64_t rstd_stride, int64_t rows, int64_t n,
                                             hipStream_t s);
extern std::atomic<int> g_last_layer_norm_kernel[3];
// the gradient of the row softmax from its output (softmax_grad.hip; lh_softmax_grad_rows_plan in softmax_rows_plan.h picks
// the kernel), and the fused attention forward (attention.hip; attention_plan.h is the launch plan): strides are
// {batch, head, position} in elements; o, probs, row_max and row_sum may each be null
hipError_t launch_softmax_grad_rows_f32(float *dx, int64_t dx_row_stride, const float *dy, int64_t dy_row_stride, const float *y,
                                        int64_t y_row_stride, int64_t rows, int64_t n, hipStream_t s);
extern std::atomic<int> g_last_softmax_grad_kernel;
hipError_t launch_attention_f32(float *o, const int64_t *os, const float *q, const int64_t *qs, const float *k, const int64_t *ks,
                                const float *v, const int64_t *vs, float *probs, const int64_t *ps, float *row_max, float *row_sum,
                                int64_t batch, int64_t heads, int64_t tq, int64_t tk, int64_t d, int64_t dv, float scale, int causal,
                                hipStream_t s);
extern std::atomic<int> g_last_attention_kernel;
// the embedding layer (embedding.hip; embedding_plan.h is the launch plan): the row gather, the stable grouping of the token
// positions by id, and the gradient (order and starts both null: grouped here, in stream-ordered scratch).
// g_last_embedding_kernel[what]: laser_hip_embedding_last_kernel's answers
hipError_t launch_embedding_f32(float *y, int64_t y_row_stride, const float *w, int64_t w_row_stride, const int32_t *idx, int64_t tokens,
                                int64_t vocab, int64_t dim, hipStream_t s);
hipError_t launch_embedding_group_i32(int32_t *order, int32_t *starts, const int32_t *idx, int64_t tokens, int64_t vocab, hipStream_t s);
hipError_t launch_embedding_grad_f32(float *dw, int64_t dw_row_stride, const float *dy, int64_t dy_row_stride, const int32_t *idx,
                                     const int32_t *order, const int32_t *starts, int64_t tokens, int64_t vocab, int64_t dim,
                                     hipStream_t s);
extern std::atomic<int> g_last_embedding_kernel[4];
// row selection (select.hip; select_plan.h is the launch plan; include/laser_hip_select.h): the k first elements of every row in
// the key order with their columns (vals or idx may be null), the first element alone in one pass (val may be null), and the
// row gather out[r, c] = src[r, j[r, c]].  g_last_topk_kernel: the plan's code of the last top-k launch, + 8 for an argmax launch
hipError_t launch_topk_rows_f32(float *vals, int64_t vals_row_stride, int32_t *idx, int64_t idx_row_stride, const float *src,
                                int64_t src_row_stride, int64_t rows, int64_t n, int64_t k, int largest, hipStream_t s);
hipError_t launch_argmax_rows_f32(int32_t *idx, int64_t idx_stride, float *val, int64_t val_stride, const float *src,
                                  int64_t src_row_stride, int64_t rows, int64_t n, int largest, hipStream_t s);
hipError_t launch_take_rows_i32(int32_t *out, int64_t out_row_stride, const int32_t *src, int64_t src_row_stride, const int32_t *j,
                                int64_t j_row_stride, int64_t rows, int64_t m, int64_t num, hipStream_t s);
extern std::atomic<int> g_last_topk_kernel;
// the optimizer steps over a list of tensors and the global gradient norm (optim.hip; optim_core.h is the arithmetic,
// optim_plan.h the launch plan): the pointer lists are host arrays of device pointers, m may be null for SGD, d_clip may be null
hipError_t launch_sgd_step_f32(float *const *w, const float *const *g, float *const *m, const int64_t *lens, int count, float lr, float mu,
                               float wd, int nesterov, float gscale, const float *d_clip, hipStream_t s);
hipError_t launch_adam_step_f32(float *const *w, const float *const *g, float *const *m, float *const *v, const int64_t *lens, int count,
                                float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2, float gscale,
                                const float *d_clip, hipStream_t s);
hipError_t launch_grad_norm_f32(float *d_norm, float *d_clip, const float *const *g, const int64_t *lens, int count, float max_norm,
                                hipStream_t s);
// 1 - beta^step of optim_core.h (host only; it lives in optim.hip, which is compiled with contraction off)
float optim_bias_correction(float beta, int64_t step);
// lsin, lcos and both from one reduction over strided views (sincos.hip; sincos_core.h is the definition)
hipError_t launch_sin_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s);
hipError_t launch_cos_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s);
hipError_t launch_sincos_f32(float *sin_dst, const int64_t *sin_strides, float *cos_dst, const int64_t *cos_strides, const float *src,
                             const int64_t *sstrides, const int64_t *shape, int rank, hipStream_t s);
// the F+tree weighted sampler (sampler.hip; sampler_plan.h picks the build kernel): tree images of 2 P elements per row
hipError_t launch_sampler_build_f32(float *tree, int64_t tree_row_stride, const float *w, int64_t w_row_stride, int64_t rows, int64_t n,
                                    hipStream_t s);
hipError_t launch_sampler_sample_f32(int32_t *idx, const float *tree, int64_t tree_row_stride, const float *u01, int64_t rows, int64_t n,
                                     int64_t m, hipStream_t s);
hipError_t launch_sampler_sample_remove_f32(int32_t *idx, float *tree, int64_t tree_row_stride, const float *u01, int64_t rows, int64_t n,
                                            int64_t k, hipStream_t s);
hipError_t launch_sampler_update_f32(float *tree, int64_t tree_row_stride, const int32_t *elem, const float *weight, int64_t rows,
                                     int64_t n, hipStream_t s);
// the same draws with u01[row, j] made in the kernel from word offset + row * m + j of the Philox stream (philox_core.h)
hipError_t launch_sampler_sample_rng_f32(int32_t *idx, const float *tree, int64_t tree_row_stride, uint64_t seed, uint64_t subseq,
                                         uint64_t offset, int64_t rows, int64_t n, int64_t m, hipStream_t s);
hipError_t launch_sampler_sample_remove_rng_f32(int32_t *idx, float *tree, int64_t tree_row_stride, uint64_t seed, uint64_t subseq,
                                                uint64_t offset, int64_t rows, int64_t n, int64_t k, hipStream_t s);
// the row prefix sum, the sorted search and the inverse-CDF sampler (scan.hip; scan_core.h is the order, scan_plan.h the launch plan)
hipError_t launch_cumsum_f32(float *dst, int64_t ds, const float *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_cumsum_f64(double *dst, int64_t ds, const double *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_cumsum_i32(int32_t *dst, int64_t ds, const int32_t *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_cumsum_i64(int64_t *dst, int64_t ds, const int64_t *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s);
hipError_t launch_searchsorted_f32(int32_t *idx, const float *a, int64_t as, const float *v, int64_t rows, int64_t n, int64_t m, int right,
                                   hipStream_t s);
hipError_t launch_searchsorted_f64(int32_t *idx, const double *a, int64_t as, const double *v, int64_t rows, int64_t n, int64_t m, int right,
                                   hipStream_t s);
hipError_t launch_searchsorted_i32(int32_t *idx, const int32_t *a, int64_t as, const int32_t *v, int64_t rows, int64_t n, int64_t m,
                                   int right, hipStream_t s);
hipError_t launch_searchsorted_i64(int32_t *idx, const int64_t *a, int64_t as, const int64_t *v, int64_t rows, int64_t n, int64_t m,
                                   int right, hipStream_t s);
hipError_t launch_cdf_sample_f32(int32_t *idx, const float *cdf, int64_t cs, const float *u01, int64_t rows, int64_t n, int64_t m,
                                 hipStream_t s);
hipError_t launch_cdf_sample_rng_f32(int32_t *idx, const float *cdf, int64_t cs, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     int64_t rows, int64_t n, int64_t m, hipStream_t s);
hipError_t launch_cdf_sample_remove_f32(int32_t *idx, float *w, int64_t ws, float *cdf, int64_t cs, const float *u01, int64_t rows,
                                        int64_t n, int64_t k, hipStream_t s);
hipError_t launch_cdf_sample_remove_rng_f32(int32_t *idx, float *w, int64_t ws, float *cdf, int64_t cs, uint64_t seed, uint64_t subseq,
                                            uint64_t offset, int64_t rows, int64_t n, int64_t k, hipStream_t s);
// fills with uniform random numbers (random.hip; philox_core.h is the generator, random_plan.h the launch plan)
hipError_t launch_random_bits_u32(uint32_t *dst, int64_t n, uint64_t seed, uint64_t subseq, uint64_t offset, hipStream_t s);
hipError_t launch_random_uniform_f32(float *dst, int64_t n, float lo, float hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s);
hipError_t launch_random_uniform_f64(double *dst, int64_t n, double lo, double hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s);
hipError_t launch_random_uniform_i32(int32_t *dst, int64_t n, int32_t lo, int32_t hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s);
hipError_t launch_random_uniform_i64(int64_t *dst, int64_t n, int64_t lo, int64_t hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s);
// the normal fill (normal_core.h): Box-Muller pairs on the same streams, one word per element
hipError_t launch_random_normal_f32(float *dst, int64_t n, float mean, float std, uint64_t seed, uint64_t subseq, uint64_t offset,
                                    hipStream_t s);
template <typename T>
hipError_t launch_pack_pad(T *dst, int64_t Rpad, int64_t Cpad, const T *src, int64_t R,
                           int64_t Ccols, int64_t rs, int64_t cs, hipStream_t s, int relu = 0);

}  // namespace laser_hip
