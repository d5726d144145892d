// laser_amd/csrc/log_softmax.hip -- llog over strided device views, and the row kernels: the deterministic row softmax
// (include/laser_hip.h, "exp and row softmax") and what takes logits to a loss, logsumexp, log-softmax and the softmax
// cross-entropy with integer labels (include/laser_hip.h, "log, logsumexp, log-softmax and cross-entropy").
//
// llog is log_core.h's, lexp exp_core.h's.  For a row, m = the maximum under lh_reduce_max and s = the sum of lexp(x[j] - m)
// in reduce_core.h's order applied to the row as a 1-D array of n float32 (E = 4, W = 256 lanes, R = 8 steps, init +0), so
// every result is a function of the row's values, n (and the label) alone.  Three lane mappings, chosen by n alone
// (softmax_rows_plan.h), each with a 16-byte-vector instance (row bases 16-byte aligned) and a single-element one: same
// values, same order.  Only the endings differ:
//   kLse   per_row[row] = m + llog(s)                          (m = +-Inf: m itself)
//   kLsm   y[j] = (x[j] - m) - llog(s)                         two separately rounded subtractions
//   kXent  loss = llog(s) - (x[label] - m),  grad[j] = (lexp(x[j] - m) / s - [j == label]) * scale;  either may be absent.
//          label -1: +0 everywhere; any other label outside [0, n): NaN everywhere
//   kSm    y[j] = lexp(x[j] - m) / s                           the softmax; the division is __fdiv_rn
// s >= 1 (the maximal element adds lexp(0) = 1), so llog(s) >= 0 with no cancellation.
//   LogOp               the elementwise llog as an Op of pointwise.h, which holds the kernels, the grid and the vector choice;
//                       no table in LDS: llog's 256 bytes of constants stay in two cache lines
//   rows_wave_kernel    n <= 1024: one wave per row, four rows per workgroup.  Lane l holds the order's lanes l, l + 64,
//                       l + 128, l + 192 (four elements each), folds lanes 128 and 64 apart in registers and the rest with
//                       cross-lane moves; the row never leaves the registers.
//   rows_block_kernel   n <= 8192 (one chunk): one workgroup per row, lane t = the order's lane t, 8 steps x 4 elements in
//                       registers between the passes; the lane fold goes through LDS.
//   rows_long_kernel    longer rows: one workgroup walks the row's chunks: the maximum, the chunk partials of the sum (folded
//                       by the same rule from LDS), then (kLsm, kSm, kXent with grad) once more for the results.
//                       LDS: 4 KiB table + 1 KiB fold scratch + 32 KiB partials
// Every kernel copies the 4 KiB table of lexp into LDS once per workgroup and gathers from there (exp_softmax.hip says why).
// No workgroup waits on another; no atomics, no flags.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "log_core.h"
#include "pointwise.h"
#include "softmax_common.h"
#include "softmax_rows_plan.h"

#pragma clang fp contract(off)

static_assert(LH_SOFTMAX_ROWS_MAX_WORKGROUPS == LH_SOFTMAX_MAX_WORKGROUPS, "one cap for every row kernel");
static_assert(LH_SOFTMAX_ROWS_CHUNK_N == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of the order");

namespace laser_hip {
namespace {

// ---- log ----------------------------------------------------------------------------------------------------------------
struct LogOp : PointwiseOp<1, 1> {
  __device__ __forceinline__ void apply(const float (&x)[1], float (&y)[1]) const { y[0] = lh_log(x[0]); }
};

// ---- the row kernels ----------------------------------------------------------------------------------------------------
enum { kLse = 0, kLsm = 1, kXent = 2, kSm = 3 };

struct RowArgs {
  float *row_out;  // kLsm: y; kXent: grad or null
  long long ostride;
  float *per_row;  // kLse: the logsumexp; kXent: loss or null
  long long pstride;
  const float *src;
  long long sstride;
  const int *labels;  // kXent
  float scale;        // kXent
  long long rows, n;
};

__device__ __forceinline__ float lse_of(const float m, const float s) {
  const float inf = __builtin_inff();
  return (m == inf || m == -inf) ? m : m + lh_log(s);
}

// kXent: the label of `row`; for a label outside [0, n) the row is finished here by `lanes` lanes (`lane` of them this one):
// +0 for -1 ("ignore"), NaN for anything else.  The branch is uniform over the lanes that share the row.
__device__ __forceinline__ bool xent_label(const RowArgs &a, const long long row, const int lane, const int lanes, int &lab) {
  lab = a.labels[row];
  if (lab >= 0 && lab < a.n) return true;
  const float v = lab == -1 ? 0.0f : __builtin_nanf("");
  if (a.per_row && lane == 0) a.per_row[row * a.pstride] = v;
  if (a.row_out) {
    float *y = a.row_out + row * a.ostride;
    for (long long j = lane; j < a.n; j += lanes) y[j] = v;
  }
  return false;
}

template <bool VEC, int OP>
__global__ void __launch_bounds__(256) rows_wave_kernel(const RowArgs a) {
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int lane = threadIdx.x & 63;
  const int n = (int)a.n;
  const float ninf = -__builtin_inff();
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += (long long)gridDim.x * 4) {
    const float *x = a.src + row * a.sstride;
    int lab = 0;
    if (OP == kXent && !xent_label(a, row, lane, 64, lab)) continue;
    float e[4][4];
    float m = ninf;
#pragma unroll
    for (int k = 0; k < 4; k++) {  // the order's lane lane + 64 k, step 0
      load4<VEC>(x, k * 256 + lane * 4, n, ninf, e[k]);
#pragma unroll
      for (int j = 0; j < 4; j++) m = lh_reduce_max(m, e[k][j]);
    }
    m = wave_max(m);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = e[k][j] - m;
        p[j] = k * 256 + lane * 4 + j < n ? lh_exp_with(d, lut) : 0.0f;
        e[k][j] = OP == kLsm ? d : p[j];
      }
      v[k] = (p[0] + p[2]) + (p[1] + p[3]);
    }
    const float s = __shfl(wave_fold((v[0] + v[2]) + (v[1] + v[3])), 0);
    if (OP == kLse) {
      if (lane == 0) a.per_row[row * a.pstride] = lse_of(m, s);
      continue;
    }
    if (OP == kXent) {
      if (a.per_row && lane == 0) a.per_row[row * a.pstride] = lh_log(s) - (x[lab] - m);
      if (!a.row_out) continue;
    }
    float *y = a.row_out + row * a.ostride;
    const float l = OP == kLsm ? lh_log(s) : 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (OP == kLsm) {
          e[k][j] = e[k][j] - l;
        } else if (OP == kSm) {
          e[k][j] = __fdiv_rn(e[k][j], s);
        } else {
          const float g = __fdiv_rn(e[k][j], s) - (k * 256 + lane * 4 + j == lab ? 1.0f : 0.0f);
          e[k][j] = g * a.scale;
        }
      }
      store4<VEC>(y, k * 256 + lane * 4, n, e[k]);
    }
  }
}

template <bool VEC, int OP>
__global__ void __launch_bounds__(256) rows_block_kernel(const RowArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ float red[260];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int t = threadIdx.x;
  const long long n = a.n;  // (64-bit as load4 / store4 take it: 13 to 26 fewer registers than an int in the kLse and kSm instances)
  const float ninf = -__builtin_inff();
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.src + row * a.sstride;
    int lab = 0;
    if (OP == kXent && !xent_label(a, row, t, 256, lab)) continue;
    float e[R][4];
    float m = ninf;
#pragma unroll
    for (int r = 0; r < R; r++) {
      load4<VEC>(x, r * 1024 + t * 4, n, ninf, e[r]);
#pragma unroll
      for (int j = 0; j < 4; j++) m = lh_reduce_max(m, e[r][j]);
    }
    m = block_max(m, red);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = e[r][j] - m;
        const float p = r * 1024 + t * 4 + j < n ? lh_exp_with(d, lut) : 0.0f;
        acc[j] = acc[j] + p;
        e[r][j] = OP == kLsm ? d : p;
      }
    }
    const float s = block_sum(acc, red);
    if (OP == kLse) {
      if (t == 0) a.per_row[row * a.pstride] = lse_of(m, s);
      continue;
    }
    if (OP == kXent) {
      if (a.per_row && t == 0) a.per_row[row * a.pstride] = lh_log(s) - (x[lab] - m);
      if (!a.row_out) continue;
    }
    float *y = a.row_out + row * a.ostride;
    const float l = OP == kLsm ? lh_log(s) : 0.0f;
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (OP == kLsm) {
          e[r][j] = e[r][j] - l;
        } else if (OP == kSm) {
          e[r][j] = __fdiv_rn(e[r][j], s);
        } else {
          const float g = __fdiv_rn(e[r][j], s) - (r * 1024 + t * 4 + j == lab ? 1.0f : 0.0f);
          e[r][j] = g * a.scale;
        }
      }
      store4<VEC>(y, r * 1024 + t * 4, n, e[r]);
    }
  }
}

template <bool VEC, int OP>
__global__ void __launch_bounds__(256) rows_long_kernel(const RowArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ float red[260];
  __shared__ float part[kChunk];  // the chunk partials of a row: n <= 2^26 leaves at most 8192, one chunk of the next level
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int t = threadIdx.x;
  const long long n = a.n;
  const float ninf = -__builtin_inff();
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.src + row * a.sstride;
    int lab = 0;
    if (OP == kXent && !xent_label(a, row, t, 256, lab)) continue;
    float m = ninf;
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float q[4];
      load4<VEC>(x, base, n, ninf, q);
#pragma unroll
      for (int j = 0; j < 4; j++) m = lh_reduce_max(m, q[j]);
    }
    m = block_max(m, red);
    for (int c = 0; c < chunks; c++) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long base = (long long)c * kChunk + r * 1024 + t * 4;
        float q[4];
        load4<VEC>(x, base, n, 0.0f, q);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = acc[j] + (base + j < n ? lh_exp_with(q[j] - m, lut) : 0.0f);
      }
      const float p = block_sum(acc, red);
      if (t == 0) part[c] = p;
    }
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = r * 1024 + t * 4 + j;
        acc[j] = acc[j] + (i < chunks ? part[i] : 0.0f);
      }
    }
    const float s = block_sum(acc, red);  // (its barriers also keep part[] until every lane has read it)
    if (OP == kLse) {
      if (t == 0) a.per_row[row * a.pstride] = lse_of(m, s);
      continue;
    }
    if (OP == kXent) {
      if (a.per_row && t == 0) a.per_row[row * a.pstride] = lh_log(s) - (x[lab] - m);
      if (!a.row_out) continue;
    }
    float *y = a.row_out + row * a.ostride;
    const float l = OP == kLsm ? lh_log(s) : 0.0f;
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float q[4];
      load4<VEC>(x, base, n, 0.0f, q);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = q[j] - m;
        if (OP == kLsm) {
          q[j] = d - l;
        } else if (OP == kSm) {
          q[j] = __fdiv_rn(lh_exp_with(d, lut), s);
        } else {
          const float g = __fdiv_rn(lh_exp_with(d, lut), s) - (base + j == lab ? 1.0f : 0.0f);
          q[j] = g * a.scale;
        }
      }
      store4<VEC>(y, base, n, q);
    }
  }
}

// `code`: where the plan's kernel code goes once the launch is made (null: nowhere)
template <int OP>
hipError_t launch_rows(const RowArgs &a, const bool vec, hipStream_t s, int *code = nullptr) {
  if (a.rows == 0) return hipSuccess;
  long long p[3];
  if (lh_softmax_rows_plan(a.rows, a.n, vec ? 1 : 0, p) != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)p[1]);
  switch ((int)p[0]) {
#define LH_ROWS_CASE(CODE, K, V) \
  case CODE:                     \
    hipLaunchKernelGGL((K<V, OP>), grid, dim3(256), 0, s, a); \
    break;
    LH_ROWS_CASE(0, rows_wave_kernel, true)
    LH_ROWS_CASE(1, rows_block_kernel, true)
    LH_ROWS_CASE(2, rows_long_kernel, true)
    LH_ROWS_CASE(4, rows_wave_kernel, false)
    LH_ROWS_CASE(5, rows_block_kernel, false)
    LH_ROWS_CASE(6, rows_long_kernel, false)
#undef LH_ROWS_CASE
    default:
      return hipErrorInvalidValue;
  }
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess && code) *code = (int)p[0];
  return e;
}

// 16-byte vectors need every row operand of a call to pass this
bool rows_aligned(const void *p, int64_t stride, int64_t rows) { return (uintptr_t)p % 16 == 0 && (rows == 1 || stride % 4 == 0); }

}  // namespace

hipError_t launch_log_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s) {
  return launch_pointwise<LogOp>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
}

hipError_t launch_softmax_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                   hipStream_t s) {
  RowArgs a = {};
  a.row_out = dst;
  a.ostride = dstride;
  a.src = src;
  a.sstride = sstride;
  a.rows = rows;
  a.n = n;
  int code = -1;
  const hipError_t e = launch_rows<kSm>(a, rows_aligned(src, sstride, rows) && rows_aligned(dst, dstride, rows), s, &code);
  if (code >= 0) g_last_softmax_kernel = code;  // (option "last_softmax_kernel")
  return e;
}

hipError_t launch_logsumexp_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                     hipStream_t s) {
  RowArgs a = {};
  a.per_row = dst;
  a.pstride = dstride;
  a.src = src;
  a.sstride = sstride;
  a.rows = rows;
  a.n = n;
  return launch_rows<kLse>(a, rows_aligned(src, sstride, rows), s);
}

hipError_t launch_log_softmax_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                       hipStream_t s) {
  RowArgs a = {};
  a.row_out = dst;
  a.ostride = dstride;
  a.src = src;
  a.sstride = sstride;
  a.rows = rows;
  a.n = n;
  return launch_rows<kLsm>(a, rows_aligned(src, sstride, rows) && rows_aligned(dst, dstride, rows), s);
}

hipError_t launch_softmax_xent_rows_f32(float *loss, int64_t loss_stride, float *grad, int64_t grad_stride, const float *src,
                                        int64_t sstride, const int32_t *labels, int64_t rows, int64_t n, float scale, hipStream_t s) {
  RowArgs a = {};
  a.row_out = grad;
  a.ostride = grad_stride;
  a.per_row = loss;
  a.pstride = loss_stride;
  a.src = src;
  a.sstride = sstride;
  a.labels = labels;
  a.scale = scale;
  a.rows = rows;
  a.n = n;
  return launch_rows<kXent>(a, rows_aligned(src, sstride, rows) && (!grad || rows_aligned(grad, grad_stride, rows)), s);
}

}  // namespace laser_hip
