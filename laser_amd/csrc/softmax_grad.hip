// laser_amd/csrc/softmax_grad.hip -- the gradient of the row softmax from its OUTPUT (include/laser_hip.h, "Softmax
// gradient"): for a row of n, D = the sum of the rounded products dy[j] * y[j] in reduce_core.h's order applied to the row as
// a 1-D array of n float32 (E = 4, W = 256 lanes, R = 8 steps, init +0), then dx[j] = y[j] * (dy[j] - D), a rounded
// subtraction and a rounded multiplication.  Every result is a function of the row's values and n alone.
//
// The three lane mappings of the softmax rows (log_softmax.hip), chosen by n alone (lh_softmax_grad_rows_plan in
// softmax_rows_plan.h), each with a 16-byte-vector instance and a single-element one:
//   grad_wave_kernel    n <= 1024: one wave per row, four rows per workgroup; the row never leaves the registers
//   grad_block_kernel   n <= 8192 (one chunk): one workgroup per row, both rows in registers between the passes
//   grad_long_kernel    longer rows: one workgroup walks the row's chunks for the chunk partials, folds them by the same rule
//                       from LDS and walks the row once more for the results
// The products can be negative or -0, so the leaves add them to the order's init (+0 + -0 is +0); an element past the row's
// end is skipped, which leaves +0.  dx may be dy or y: every element is read and written by the same lane, and the sum is
// complete before the first store of a row.  No workgroup waits on another; no atomics, no flags.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/laser_hip.h"
#include "common.h"
#include "softmax_common.h"
#include "softmax_rows_plan.h"

#pragma clang fp contract(off)

namespace laser_hip {

std::atomic<int> g_last_softmax_grad_kernel{-1};

namespace {

struct GradArgs {
  float *dx;
  long long xstride;
  const float *dy;
  long long dstride;
  const float *y;
  long long ystride;
  long long rows, n;
};

template <bool VEC>
__global__ void __launch_bounds__(256) grad_wave_kernel(const GradArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = (int)a.n;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += (long long)gridDim.x * 4) {
    const float *dy = a.dy + row * a.dstride;
    const float *y = a.y + row * a.ystride;
    float g[4][4], p[4][4], v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // the order's lane lane + 64 k, step 0
      load4<VEC>(dy, k * 256 + lane * 4, n, 0.0f, g[k]);
      load4<VEC>(y, k * 256 + lane * 4, n, 0.0f, p[k]);
      float q[4];
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = k * 256 + lane * 4 + j < n ? 0.0f + g[k][j] * p[k][j] : 0.0f;
      v[k] = (q[0] + q[2]) + (q[1] + q[3]);
    }
    const float D = __shfl(wave_fold((v[0] + v[2]) + (v[1] + v[3])), 0);
    float *dx = a.dx + row * a.xstride;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
      for (int j = 0; j < 4; j++) g[k][j] = p[k][j] * (g[k][j] - D);
      store4<VEC>(dx, k * 256 + lane * 4, n, g[k]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) grad_block_kernel(const GradArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  const int t = threadIdx.x;
  const long long n = a.n;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *dy = a.dy + row * a.dstride;
    const float *y = a.y + row * a.ystride;
    float g[R][4], p[R][4];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
      load4<VEC>(dy, r * 1024 + t * 4, n, 0.0f, g[r]);
      load4<VEC>(y, r * 1024 + t * 4, n, 0.0f, p[r]);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (r * 1024 + t * 4 + j < n) acc[j] = acc[j] + g[r][j] * p[r][j];
    }
    const float D = block_sum(acc, red);
    float *dx = a.dx + row * a.xstride;
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) g[r][j] = p[r][j] * (g[r][j] - D);
      store4<VEC>(dx, r * 1024 + t * 4, n, g[r]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) grad_long_kernel(const GradArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  __shared__ float part[kChunk];  // the chunk partials of a row: n <= 2^26 leaves at most 8192, one chunk of the next level
  const int t = threadIdx.x;
  const long long n = a.n;
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *dy = a.dy + row * a.dstride;
    const float *y = a.y + row * a.ystride;
    __syncthreads();  // the last readers of part[] are done
    for (int c = 0; c < chunks; c++) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long base = (long long)c * kChunk + r * 1024 + t * 4;
        float g[4], p[4];
        load4<VEC>(dy, base, n, 0.0f, g);
        load4<VEC>(y, base, n, 0.0f, p);
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (base + j < n) acc[j] = acc[j] + g[j] * p[j];
      }
      const float s = block_sum(acc, red);
      if (t == 0) part[c] = s;
    }
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = r * 1024 + t * 4 + j;
        if (i < chunks) acc[j] = acc[j] + part[i];
      }
    }
    const float D = block_sum(acc, red);
    float *dx = a.dx + row * a.xstride;
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float g[4], p[4];
      load4<VEC>(dy, base, n, 0.0f, g);
      load4<VEC>(y, base, n, 0.0f, p);
#pragma unroll
      for (int j = 0; j < 4; j++) g[j] = p[j] * (g[j] - D);
      store4<VEC>(dx, base, n, g);
    }
  }
}

bool grad_aligned(const void *p, int64_t stride, int64_t rows) { return (uintptr_t)p % 16 == 0 && (rows == 1 || stride % 4 == 0); }

}  // namespace

hipError_t launch_softmax_grad_rows_f32(float *dx, int64_t dx_row_stride, const float *dy, int64_t dy_row_stride, const float *y,
                                        int64_t y_row_stride, int64_t rows, int64_t n, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  GradArgs a = {dx, dx_row_stride, dy, dy_row_stride, y, y_row_stride, rows, n};
  const bool vec = grad_aligned(dx, dx_row_stride, rows) && grad_aligned(dy, dy_row_stride, rows) && grad_aligned(y, y_row_stride, rows);
  long long p[3];
  if (lh_softmax_grad_rows_plan(rows, n, vec ? 1 : 0, p) != 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)p[1]);
  switch ((int)p[0]) {
#define LH_GRAD_CASE(CODE, K, V) \
  case CODE:                     \
    hipLaunchKernelGGL((K<V>), grid, dim3(256), 0, s, a); \
    break;
    LH_GRAD_CASE(0, grad_wave_kernel, true)
    LH_GRAD_CASE(1, grad_block_kernel, true)
    LH_GRAD_CASE(2, grad_long_kernel, true)
    LH_GRAD_CASE(4, grad_wave_kernel, false)
    LH_GRAD_CASE(5, grad_block_kernel, false)
    LH_GRAD_CASE(6, grad_long_kernel, false)
#undef LH_GRAD_CASE
    default:
      return hipErrorInvalidValue;
  }
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_softmax_grad_kernel = (int)p[0];
  return e;
}

}  // namespace laser_hip
