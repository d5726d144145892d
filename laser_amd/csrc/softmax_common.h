// laser_amd/csrc/softmax_common.h -- what the row kernels (log_softmax.hip), the column-strip kernels
// (softmax_axis.hip, dense_grad.hip) and the elementwise template (pointwise.h: the vector types, the workgroup cap, the table copy) share:
// the 16-byte vector types, the table copy into LDS, the bounded 4-element loads and stores, the order-free maximum and the
// folds of reduce_core.h's order over the 256 lanes of a workgroup.  Device code only; every function is inlined.
#ifndef LASER_HIP_SOFTMAX_COMMON_H
#define LASER_HIP_SOFTMAX_COMMON_H

#include <hip/hip_runtime.h>

#include "exp_core.h"
#include "reduce_core.h"
#include "softmax_axis_plan.h"

static_assert(LH_REDUCE_LANES == 256 && LH_REDUCE_STEPS == 8, "the softmax kernels map lanes onto this order");

namespace laser_hip {
namespace {

constexpr int kChunk = LH_REDUCE_STEPS * LH_REDUCE_LANES * 4;  // elements of one chunk of the order (f32: E = 4)
constexpr int kMaxBlocks = LH_SOFTMAX_MAX_WORKGROUPS;           // 2048: 8 workgroups of 256 lanes on each of 256 CUs

struct alignas(16) F4 {
  float v[4];
};
struct alignas(16) U4 {
  unsigned int v[4];
};

__device__ __forceinline__ void lut_to_lds(unsigned int *lut) {
  for (int i = threadIdx.x; i < LH_EXP_LUT_SIZE / 4; i += blockDim.x) ((U4 *)lut)[i] = ((const U4 *)lh_exp_lut)[i];
  __syncthreads();
}

// elements base .. base + 3 of a row of n; `pad` where the row has ended
template <bool VEC>
__device__ __forceinline__ void load4(const float *x, const long long base, const long long n, const float pad, float (&q)[4]) {
  if (VEC && base + 4 <= n) {
    const F4 f = *(const F4 *)(x + base);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = f.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = base + j < n ? x[base + j] : pad;
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float *y, const long long base, const long long n, const float (&q)[4]) {
  if (VEC && base + 4 <= n) {
    F4 f;
#pragma unroll
    for (int j = 0; j < 4; j++) f.v[j] = q[j];
    *(F4 *)(y + base) = f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (base + j < n) y[base + j] = q[j];
  }
}

// the maximum does not depend on the order (lh_reduce_max): butterflies, every lane gets it
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) m = lh_reduce_max(m, __shfl_xor(m, h));
  return m;
}
// `red` holds 260 floats
__device__ __forceinline__ float block_max(float m, float *red) {
  m = wave_max(m);
  __syncthreads();  // the last readers of red are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  return lh_reduce_max(lh_reduce_max(red[0], red[1]), lh_reduce_max(red[2], red[3]));
}
// the order's fold of lanes 0 .. 63 of one wave: lane t merges lane t + h, h = 32, .., 1 (the result is lane 0's)
__device__ __forceinline__ float wave_fold(float v) {
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) v = v + __shfl_down(v, h);
  return v;
}
// the order's end of a chunk: the 4 accumulators of every lane folded by halving, then the 256 lanes; every lane gets it
__device__ __forceinline__ float block_sum(const float (&acc)[4], float *red) {
  const int t = threadIdx.x;
  float v = (acc[0] + acc[2]) + (acc[1] + acc[3]);
  __syncthreads();  // the last readers of red are done
  red[t] = v;
  __syncthreads();
  if (t < 64) {  // lanes 128 and 64 apart, then within the wave
    v = wave_fold((red[t] + red[t + 128]) + (red[t + 64] + red[t + 192]));
    if (t == 0) red[256] = v;
  }
  __syncthreads();
  return red[256];
}

// ---- the column-strip folds (softmax_axis.hip, dense_grad.hip): a lane owns 4 adjacent columns, CW / 4 lanes span a strip
// row, and row lane rl = tid / (CW / 4) holds the leaves a = q * 4 RL + 4 rl + p of each of its columns
// the order's fold over the row lanes: lane tid merges lane tid + h, h = 128, 64, .., LPR; the CW column results go to
// out[0 .. CW) (LDS), visible to every lane on return.  red4 holds 256 vectors.
template <int CW>
__device__ __forceinline__ void col_fold(const float (&v)[4], F4 *red4, float *out) {
#pragma clang fp contract(off)
  constexpr int LPR = CW / 4;
  const int t = threadIdx.x;
  F4 f;
#pragma unroll
  for (int j = 0; j < 4; j++) f.v[j] = v[j];
  __syncthreads();  // the last readers of red4 and of out are done
  red4[t] = f;
  __syncthreads();
  if (t < 64) {
    const F4 a = red4[t], b = red4[t + 128], c = red4[t + 64], d = red4[t + 192];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float s = (a.v[j] + b.v[j]) + (c.v[j] + d.v[j]);
#pragma unroll
      for (int h = 32; h >= LPR; h /= 2) s = s + __shfl_down(s, h);
      if (t < LPR) out[t * 4 + j] = s;
    }
  }
  __syncthreads();
}

// the leaves of one lane folded inside the lane: bits 1 and 0 of the leaf index (p), then the top bits (q).  The lane holds
// the first QU of its Q blocks of 4 leaves; the others took no element and are the order's init, +0
template <int Q, int QU>
__device__ __forceinline__ void lane_fold(const float (&e)[QU][4][4], float (&v)[4]) {
#pragma clang fp contract(off)
  float u[Q][4];
#pragma unroll
  for (int q = 0; q < Q; q++) {
#pragma unroll
    for (int j = 0; j < 4; j++) u[q][j] = 0.0f;
  }
#pragma unroll
  for (int q = 0; q < QU; q++) {
#pragma unroll
    for (int j = 0; j < 4; j++) u[q][j] = (e[q][0][j] + e[q][2][j]) + (e[q][1][j] + e[q][3][j]);
  }
#pragma unroll
  for (int h = Q / 2; h >= 1; h /= 2) {
#pragma unroll
    for (int q = 0; q < h; q++) {
#pragma unroll
      for (int j = 0; j < 4; j++) u[q][j] = u[q][j] + u[q + h][j];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = u[0][j];
}

}  // namespace
}  // namespace laser_hip

#endif  // LASER_HIP_SOFTMAX_COMMON_H
