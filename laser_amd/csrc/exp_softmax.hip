// laser_amd/csrc/exp_softmax.hip -- lexp over strided device views and the deterministic row softmax (include/laser_hip.h,
// "exp and row softmax"): the device form of laser/primitives/simd_math/exp_log_*.nim and of the softmax its README promises
// on top of it.
//
// lexp is exp_core.h's, the sum of a softmax row is reduce_core.h's order applied to the row as a 1-D array of n float32
// (E = 4, W = 256 lanes, R = 8 steps, init +0), so a row's result is a function of its values and n alone.  Every kernel
// copies the 4 KiB table into LDS once per workgroup (256 lanes x one 16-byte vector) and gathers from there: a wave's 64
// table indices are scattered, which LDS serves at a word per bank and cycle while the vector L1 would serialise cache lines.
// Workgroups are capped and stride over their work, so the table fill is paid once per workgroup, not once per row.
//   exp_vec_kernel        C-contiguous, both bases 16-byte aligned: one 16-byte vector per lane and step, scalar tail
//   exp_strided_kernel    rank <= 6, any element strides: logical index -> offsets, 64-bit (also the unaligned contiguous case)
//   softmax_wave_kernel   n <= 1024: one wave per row, four rows per workgroup.  Lane l holds the order's lanes l, l + 64,
//                         l + 128, l + 192 (four elements each), folds lanes 128 and 64 apart in registers and the rest with
//                         cross-lane moves; the row never leaves the registers.
//   softmax_block_kernel  n <= 8192 (one chunk): one workgroup per row, lane t = the order's lane t, 8 steps x 4 elements in
//                         registers between the passes; the lane fold goes through LDS.
//   softmax_long_kernel   longer rows: one workgroup walks the row's chunks three times (max; chunk partials of the sum,
//                         folded by the same rule from LDS; lexp again and the division).
// The VEC instances move 16-byte vectors (row bases 16-byte aligned), the others single elements: same values, same order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/laser_hip.h"
#include "common.h"
#include "softmax_common.h"

namespace laser_hip {

std::atomic<int> g_last_softmax_kernel{-1};

namespace {

// ---- exp ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) exp_vec_kernel(float *dst, const float *src, const long long n) {
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const long long nvec = n / 4, step = (long long)gridDim.x * 256;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long v = gid; v < nvec; v += step) {
    F4 x = ((const F4 *)src)[v];
#pragma unroll
    for (int j = 0; j < 4; j++) x.v[j] = lh_exp_with(x.v[j], lut);
    ((F4 *)dst)[v] = x;
  }
  const long long t = nvec * 4 + gid;  // the last n % 4 elements
  if (t < n) dst[t] = lh_exp_with(src[t], lut);
}

struct ExpArgs {
  float *dst;
  const float *src;
  long long n, rank;
  long long shape[kMaxRank], sd[kMaxRank], ss[kMaxRank];  // merged extents and element strides
};

__global__ void __launch_bounds__(256) exp_strided_kernel(const ExpArgs a) {
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += step) {
    long long rem = i, od = 0, os = 0;
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      if (d < a.rank) {
        const long long q = d ? rem / a.shape[d] : 0, idx = rem - q * a.shape[d];
        od += idx * a.sd[d];
        os += idx * a.ss[d];
        rem = q;
      }
    }
    a.dst[od] = lh_exp_with(a.src[os], lut);
  }
}

// ---- softmax ------------------------------------------------------------------------------------------------------------
// (load4 / store4, the maxima and the folds of the order: softmax_common.h, shared with softmax_axis.hip)
template <bool VEC>
__global__ void __launch_bounds__(256) softmax_wave_kernel(float *dst, const long long dstride, const float *src, const long long sstride,
                                                           const long long rows, const int n) {
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int lane = threadIdx.x & 63;
  const float ninf = -__builtin_inff();
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
    const float *x = src + row * sstride;
    float *y = dst + row * dstride;
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
#pragma unroll
      for (int j = 0; j < 4; j++) e[k][j] = k * 256 + lane * 4 + j < n ? lh_exp_with(e[k][j] - m, lut) : 0.0f;
      v[k] = (e[k][0] + e[k][2]) + (e[k][1] + e[k][3]);
    }
    const float s = __shfl(wave_fold((v[0] + v[2]) + (v[1] + v[3])), 0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
      for (int j = 0; j < 4; j++) e[k][j] = __fdiv_rn(e[k][j], s);
      store4<VEC>(y, k * 256 + lane * 4, n, e[k]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) softmax_block_kernel(float *dst, const long long dstride, const float *src, const long long sstride,
                                                            const long long rows, const int n) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ float red[260];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int t = threadIdx.x;
  const float ninf = -__builtin_inff();
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const float *x = src + row * sstride;
    float *y = dst + row * dstride;
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
        e[r][j] = r * 1024 + t * 4 + j < n ? lh_exp_with(e[r][j] - m, lut) : 0.0f;
        acc[j] = acc[j] + e[r][j];
      }
    }
    const float s = block_sum(acc, red);
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) e[r][j] = __fdiv_rn(e[r][j], s);
      store4<VEC>(y, r * 1024 + t * 4, n, e[r]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) softmax_long_kernel(float *dst, const long long dstride, const float *src, const long long sstride,
                                                           const long long rows, const long long n) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ float red[260];
  __shared__ float part[kChunk];  // the chunk partials of a row: n <= 2^26 leaves at most 8192, one chunk of the next level
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  const int t = threadIdx.x;
  const float ninf = -__builtin_inff();
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    const float *x = src + row * sstride;
    float *y = dst + row * dstride;
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
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float q[4];
      load4<VEC>(x, base, n, 0.0f, q);
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = __fdiv_rn(lh_exp_with(q[j] - m, lut), s);
      store4<VEC>(y, base, n, q);
    }
  }
}

}  // namespace

hipError_t launch_exp_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s) {
  int64_t both[2 * kMaxRank], st[2][kMaxRank] = {}, sh[kMaxRank] = {};
  int64_t n = 1;
  for (int d = 0; d < rank; d++) {
    both[d] = dstrides[d];
    both[rank + d] = sstrides[d];
    n *= shape[d];
  }
  if (n == 0) return hipSuccess;
  const int r = merge_dims(2, both, shape, rank, st, sh);
  const bool contiguous = r == 1 && st[0][0] == 1 && st[1][0] == 1;
  if (contiguous && (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0) {
    const int64_t blocks = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n / 4 + 255) / 256));
    hipLaunchKernelGGL(exp_vec_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dst, src, (long long)n);
    return hipGetLastError();
  }
  ExpArgs a = {};
  a.dst = dst;
  a.src = src;
  a.n = n;
  a.rank = r;
  for (int d = 0; d < r; d++) {
    a.shape[d] = sh[d];
    a.sd[d] = st[0][d];
    a.ss[d] = st[1][d];
  }
  const int64_t blocks = std::min<int64_t>(kMaxBlocks, (n + 255) / 256);
  hipLaunchKernelGGL(exp_strided_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_softmax_rows_f32(float *dst, int64_t dstride, const float *src, int64_t sstride, int64_t rows, int64_t n,
                                   hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const bool vec = (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0 && (rows == 1 || (dstride % 4 == 0 && sstride % 4 == 0));
  int kernel;
#define LH_SOFTMAX_LAUNCH(K, BLOCKS, NT)                                                                                  \
  do {                                                                                                                    \
    const dim3 grid((unsigned)std::min<int64_t>(kMaxBlocks, (BLOCKS)));                                                   \
    if (vec)                                                                                                              \
      hipLaunchKernelGGL(K<true>, grid, dim3(256), 0, s, dst, (long long)dstride, src, (long long)sstride, (long long)rows, (NT)n); \
    else                                                                                                                  \
      hipLaunchKernelGGL(K<false>, grid, dim3(256), 0, s, dst, (long long)dstride, src, (long long)sstride, (long long)rows, (NT)n); \
  } while (0)
  if (n <= 1024) {
    kernel = 0;
    LH_SOFTMAX_LAUNCH(softmax_wave_kernel, (rows + 3) / 4, int);
  } else if (n <= kChunk) {
    kernel = 1;
    LH_SOFTMAX_LAUNCH(softmax_block_kernel, rows, int);
  } else {
    kernel = 2;
    LH_SOFTMAX_LAUNCH(softmax_long_kernel, rows, long long);
  }
#undef LH_SOFTMAX_LAUNCH
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_softmax_kernel = kernel + (vec ? 0 : 4);
  return e;
}

}  // namespace laser_hip
