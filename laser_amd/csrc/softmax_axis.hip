// laser_amd/csrc/softmax_axis.hip -- the softmax along a strided axis (include/laser_hip.h, "exp and row softmax"): the
// operand is (outer, n, inner), element (o, k, i) at base + o * outer_stride + k * axis_stride + i, and every column
// x[o, 0..n, i] gets exactly what softmax_rows gives the same values as a row: lh_reduce_max's maximum, lexp(x - m), the sum
// in reduce_core.h's order for a 1-D array of n float32, a correctly rounded division.
//
// A workgroup of 256 lanes owns a strip: CW = LH_SOFTMAX_AXIS_CW consecutive inner positions of one outer index, over all n.
// Lane tid = rl * LPR + l takes the 4 adjacent columns 4 l .. 4 l + 3 (LPR = CW / 4 lanes span a strip row: one run of CW * 4
// contiguous bytes, 16 bytes per lane) and is row lane rl of RL = 256 / LPR.  The columns never change lanes, so nothing is
// transposed through LDS; what crosses lanes are the folds, 16 bytes per lane (ds_write_b128 / ds_read_b128 on consecutive
// 16-byte slots: conflict-free) and cross-lane moves within a wave.
//
// The order, per column and chunk of 8192 rows: row k goes to leaf a = k mod 1024; the 1024 leaves are folded over the bits
// of a in the order 1, 0, 9, 8, .., 2 (higher index into lower).  Row lane rl holds the leaves a = q * 4 RL + 4 rl + p,
// p = 0 .. 3, q = 0 .. Q - 1 (Q = 1024 / (4 RL) = LPR): bits 1 and 0 of a are p, the top bits are q -- both fold inside the lane,
// in that order -- and the bits between are rl, which folds last: lane tid merges lane tid + h, h = 128, 64 (through LDS),
// 32, .., LPR (cross-lane moves).  The same tree as block_sum's, whichever CW.
//   softmax_axis_resident_kernel   n <= 2048 (CW = 16; 1024 for CW = 32): the lane keeps its RU x Q x 4 x 4 elements in
//                                  registers from the one read to the one write; a leaf takes RU = 1 or 2 elements 1024
//                                  rows apart.  (An instance with one block of 4 rows per lane for n <= 4 RL: the other
//                                  leaves are +0, and it needs a fraction of the registers.)
//   softmax_axis_stream_kernel     longer n: the maximum, then chunk by chunk the leaves (8 steps each) and the chunk's
//                                  partial into LDS, the partials folded by the same rule, then lexp again and the division
// The VEC instances move 16-byte vectors wherever 4 columns lie inside `inner`; the others single elements.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "softmax_axis_plan.h"
#include "softmax_common.h"

static_assert(LH_SOFTMAX_AXIS_CW == 16 || LH_SOFTMAX_AXIS_CW == 32, "a strip is 16 or 32 columns wide");
static_assert(LH_SOFTMAX_AXIS_RESIDENT_N == 1024 || LH_SOFTMAX_AXIS_RESIDENT_N == 2048, "the resident kernel holds 1 or 2 elements per leaf");
static_assert(LH_SOFTMAX_AXIS_MAX_N_PLAN == LASER_HIP_SOFTMAX_AXIS_MAX_N && laser_hip::kMaxBlocks == 2048, "plan and header agree");

namespace laser_hip {
namespace {

constexpr int kMaxParts = (int)(LASER_HIP_SOFTMAX_AXIS_MAX_N / kChunk);  // chunk partials of one column: 128

struct AxisArgs {
  float *dst;
  const float *src;
  long long dos, das, sos, sas;  // outer and axis strides of dst and src, in elements
  long long n, inner, per_outer, strips;
};

// 4 adjacent columns from column c of a row; FULL: the whole strip lies inside `inner` and rows are 16-byte aligned
template <bool FULL>
__device__ __forceinline__ void load_cols(const float *row, const long long c, const long long inner, float (&q)[4]) {
  if (FULL) {
    const F4 f = *(const F4 *)(row + c);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = f.v[j];
  } else {
    load4<false>(row, c, inner, 0.0f, q);
  }
}
template <bool FULL>
__device__ __forceinline__ void store_cols(float *row, const long long c, const long long inner, const float (&q)[4]) {
  if (FULL) {
    F4 f;
#pragma unroll
    for (int j = 0; j < 4; j++) f.v[j] = q[j];
    *(F4 *)(row + c) = f;
  } else {
    store4<false>(row, c, inner, q);
  }
}

// the maxima of a lane's 4 columns over all row lanes (any order: lh_reduce_max); wmax holds 4 * CW floats
template <int CW>
__device__ __forceinline__ void col_max(float (&m)[4], float *wmax) {
  constexpr int LPR = CW / 4;
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int h = 32; h >= LPR; h /= 2) m[j] = lh_reduce_max(m[j], __shfl_xor(m[j], h));
  }
  __syncthreads();  // the last readers of wmax are done
  if ((t & 63) < LPR) {
#pragma unroll
    for (int j = 0; j < 4; j++) wmax[(t >> 6) * CW + (t & 63) * 4 + j] = m[j];
  }
  __syncthreads();
  const float *w = wmax + (t % LPR) * 4;
#pragma unroll
  for (int j = 0; j < 4; j++)
    m[j] = lh_reduce_max(lh_reduce_max(w[j], w[CW + j]), lh_reduce_max(w[2 * CW + j], w[3 * CW + j]));
}

// QU: how many of the lane's Q blocks of 4 rows n reaches (n <= QU * 4 * RL): a short axis needs a fraction of the registers.
// RU: how many steps of 1024 rows n reaches (n <= RU * 1024): a leaf takes up to RU elements, in ascending row order.
template <int CW, bool FULL, int QU, int RU>
__device__ __forceinline__ void resident_strip(const AxisArgs &a, const float *x, float *y, const long long c, const unsigned int *lut,
                                               F4 *red4, float *wmax, float *sums) {
#pragma clang fp contract(off)
  constexpr int LPR = CW / 4, RL = 256 / LPR, Q = LPR;
  const int rl = threadIdx.x / LPR, l = threadIdx.x % LPR;
  const int n = (int)a.n;
  const float ninf = -__builtin_inff();
  float e[RU][QU][4][4];
  float m[4] = {ninf, ninf, ninf, ninf};
#pragma unroll
  for (int r = 0; r < RU; r++) {
#pragma unroll
    for (int q = 0; q < QU; q++) {
      if (r * 1024 + q * 4 * RL < n) {  // the same for every lane
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int row = r * 1024 + q * 4 * RL + rl * 4 + p;
          load_cols<FULL>(x + (long long)min(row, n - 1) * a.sas, c, a.inner, e[r][q][p]);  // a row past n repeats the last
#pragma unroll
          for (int j = 0; j < 4; j++) m[j] = lh_reduce_max(m[j], e[r][q][p][j]);
        }
      }
    }
  }
  col_max<CW>(m, wmax);
  // block by block of 4 leaves: a leaf starts at +0 and takes its elements in ascending row order; the 4 leaves of a block
  // fold at once (bits 1 and 0 of the leaf index), so only Q x 4 sums stay live
  float u[Q][4];
#pragma unroll
  for (int q = 0; q < Q; q++) {
#pragma unroll
    for (int j = 0; j < 4; j++) u[q][j] = 0.0f;
  }
#pragma unroll
  for (int q = 0; q < QU; q++) {
    float acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
      for (int j = 0; j < 4; j++) acc[p][j] = 0.0f;
#pragma unroll
      for (int r = 0; r < RU; r++) {
        if (r * 1024 + q * 4 * RL < n) {  // the same for every lane
          const bool valid = r * 1024 + q * 4 * RL + rl * 4 + p < n;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            e[r][q][p][j] = valid ? lh_exp_with(e[r][q][p][j] - m[j], lut) : 0.0f;
            acc[p][j] = acc[p][j] + e[r][q][p][j];
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) u[q][j] = (acc[0][j] + acc[2][j]) + (acc[1][j] + acc[3][j]);
  }
#pragma unroll
  for (int h = Q / 2; h >= 1; h /= 2) {  // the top bits of the leaf index
#pragma unroll
    for (int q = 0; q < h; q++) {
#pragma unroll
      for (int j = 0; j < 4; j++) u[q][j] = u[q][j] + u[q + h][j];
    }
  }
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; j++) v[j] = u[0][j];
  col_fold<CW>(v, red4, sums);
  float s[4];
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = sums[l * 4 + j];
#pragma unroll
  for (int r = 0; r < RU; r++) {
#pragma unroll
    for (int q = 0; q < QU; q++) {
      if (r * 1024 + q * 4 * RL < n) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int row = r * 1024 + q * 4 * RL + rl * 4 + p;
          if (row < n) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = __fdiv_rn(e[r][q][p][j], s[j]);
            store_cols<FULL>(y + (long long)row * a.das, c, a.inner, o);
          }
        }
      }
    }
  }
}

template <int CW, bool VEC, int QU, int RU>
__global__ void __launch_bounds__(256) softmax_axis_resident_kernel(const AxisArgs a) {
  constexpr int LPR = CW / 4;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ F4 red4[256];
  __shared__ float wmax[4 * CW];
  __shared__ float sums[CW];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  for (long long strip = blockIdx.x; strip < a.strips; strip += gridDim.x) {
    const long long o = strip / a.per_outer, i0 = (strip - o * a.per_outer) * CW;
    const long long c = i0 + (threadIdx.x % LPR) * 4;
    const float *x = a.src + o * a.sos;
    float *y = a.dst + o * a.dos;
    if (VEC && i0 + CW <= a.inner)
      resident_strip<CW, true, QU, RU>(a, x, y, c, lut, red4, wmax, sums);
    else
      resident_strip<CW, false, QU, RU>(a, x, y, c, lut, red4, wmax, sums);
  }
}

template <int CW, bool FULL>
__device__ __forceinline__ void stream_strip(const AxisArgs &a, const float *x, float *y, const long long c, const unsigned int *lut,
                                             F4 *red4, float *wmax, float *sums, float *part) {
#pragma clang fp contract(off)
  constexpr int LPR = CW / 4, RL = 256 / LPR, Q = LPR, U = 8;  // U rows in flight per lane in the first and last pass (16 measured: no faster)
  const int t = threadIdx.x, rl = t / LPR, l = t % LPR;
  const long long n = a.n;
  const float ninf = -__builtin_inff();
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (int i = t; i < kMaxParts * CW; i += 256) part[i] = 0.0f;  // (the folds below have barriers before part is written again)
  // 1. the maxima: any order; a row past n repeats the last one
  float m[4] = {ninf, ninf, ninf, ninf};
  for (long long row0 = 0; row0 < n; row0 += U * RL) {
    float q[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) load_cols<FULL>(x + min(row0 + u * RL + rl, n - 1) * a.sas, c, a.inner, q[u]);
#pragma unroll
    for (int u = 0; u < U; u++) {
#pragma unroll
      for (int j = 0; j < 4; j++) m[j] = lh_reduce_max(m[j], q[u][j]);
    }
  }
  col_max<CW>(m, wmax);
  // 2. the chunk partials of the sum
  for (int ch = 0; ch < chunks; ch++) {
    const long long k0 = (long long)ch * kChunk;
    const int rem = (int)min((long long)kChunk, n - k0);  // rows of this chunk
    float acc[Q][4][4];
#pragma unroll
    for (int q = 0; q < Q; q++) {
#pragma unroll
      for (int p = 0; p < 4; p++) {
#pragma unroll
        for (int j = 0; j < 4; j++) acc[q][p][j] = 0.0f;
      }
    }
    for (int r = 0; r < LH_REDUCE_STEPS && r * 1024 < rem; r++) {
#pragma unroll
      for (int q = 0; q < Q; q++) {
        if (r * 1024 + q * 4 * RL < rem) {  // the same for every lane
          float xq[4][4];
#pragma unroll
          for (int p = 0; p < 4; p++)
            load_cols<FULL>(x + (k0 + min(r * 1024 + q * 4 * RL + rl * 4 + p, rem - 1)) * a.sas, c, a.inner, xq[p]);
#pragma unroll
          for (int p = 0; p < 4; p++) {
            const bool valid = r * 1024 + q * 4 * RL + rl * 4 + p < rem;
#pragma unroll
            for (int j = 0; j < 4; j++) acc[q][p][j] = acc[q][p][j] + (valid ? lh_exp_with(xq[p][j] - m[j], lut) : 0.0f);
          }
        }
      }
    }
    float v[4];
    lane_fold<Q, Q>(acc, v);
    col_fold<CW>(v, red4, chunks > 1 ? part + ch * CW : sums);
  }
  // 3. more than one chunk: the partials of a column are one more array under the same rule (one leaf each: bits 1, 0, then
  //    6 .. 2; the leaves past the last partial are +0, and x + 0 = x for the sums here, which are never -0)
  if (chunks > 1) {
    if (t < CW) {
      float *p = part + t;
      const int used = (chunks + 3) / 4 * 4;
      for (int i = 0; i < used; i += 4) p[i * CW] = (p[i * CW] + p[(i + 2) * CW]) + (p[(i + 1) * CW] + p[(i + 3) * CW]);
      for (int h = kMaxParts / 2; h >= 4; h /= 2) {
        for (int i = 0; i < h && i + h < used; i += 4) p[i * CW] = p[i * CW] + p[(i + h) * CW];
      }
      sums[t] = p[0];
    }
    __syncthreads();
  }
  float s[4];
#pragma unroll
  for (int j = 0; j < 4; j++) s[j] = sums[l * 4 + j];
  // 4. lexp again and the division
  for (long long row0 = 0; row0 < n; row0 += U * RL) {
    float q[U][4];
#pragma unroll
    for (int u = 0; u < U; u++) load_cols<FULL>(x + min(row0 + u * RL + rl, n - 1) * a.sas, c, a.inner, q[u]);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const long long row = row0 + u * RL + rl;
      if (row < n) {
#pragma unroll
        for (int j = 0; j < 4; j++) q[u][j] = __fdiv_rn(lh_exp_with(q[u][j] - m[j], lut), s[j]);
        store_cols<FULL>(y + row * a.das, c, a.inner, q[u]);
      }
    }
  }
}

template <int CW, bool VEC>
__global__ void __launch_bounds__(256) softmax_axis_stream_kernel(const AxisArgs a) {
  constexpr int LPR = CW / 4;
  __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
  __shared__ F4 red4[256];
  __shared__ float wmax[4 * CW];
  __shared__ float sums[CW];
  __shared__ float part[kMaxParts * CW];
  unsigned int *lut = (unsigned int *)lut4;
  lut_to_lds(lut);
  for (long long strip = blockIdx.x; strip < a.strips; strip += gridDim.x) {
    const long long o = strip / a.per_outer, i0 = (strip - o * a.per_outer) * CW;
    const long long c = i0 + (threadIdx.x % LPR) * 4;
    const float *x = a.src + o * a.sos;
    float *y = a.dst + o * a.dos;
    if (VEC && i0 + CW <= a.inner)
      stream_strip<CW, true>(a, x, y, c, lut, red4, wmax, sums, part);
    else
      stream_strip<CW, false>(a, x, y, c, lut, red4, wmax, sums, part);
  }
}

}  // namespace

hipError_t launch_softmax_axis_f32(float *dst, int64_t dos, int64_t das, const float *src, int64_t sos, int64_t sas, int64_t outer,
                                   int64_t n, int64_t inner, hipStream_t s) {
  constexpr int CW = LH_SOFTMAX_AXIS_CW;
  if (outer == 0) return hipSuccess;
  // (a stride that is never applied -- the axis stride of n == 1, the outer stride of outer == 1 -- does not count)
  const bool vec = (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0 && (n == 1 || (das % 4 == 0 && sas % 4 == 0)) &&
                   (outer == 1 || (dos % 4 == 0 && sos % 4 == 0));
  long long plan[4];
  if (lh_softmax_axis_strip_plan(outer, n, inner, vec, 0, plan) != 0) return hipErrorInvalidValue;
  AxisArgs a;
  a.dst = dst;
  a.src = src;
  a.dos = dos;
  a.das = das;
  a.sos = sos;
  a.sas = sas;
  a.n = n;
  a.inner = inner;
  a.per_outer = (inner + CW - 1) / CW;
  a.strips = outer * a.per_outer;
  const dim3 grid((unsigned)plan[2]);
  const bool resident = plan[0] % 4 == 0;  // 8 or 12
  constexpr int Q = CW / 4, RL = 256 / Q;
  // the resident instances by the registers they need: one block of 4 rows per lane (n <= 4 RL), one element per leaf
  // (n <= 1024), and with 16-column strips two elements per leaf (n <= 2048: 128 values a lane)
  constexpr int RBIG = LH_SOFTMAX_AXIS_RESIDENT_N / 1024;
#define LH_AXIS_RESIDENT(V, QU, RU) hipLaunchKernelGGL((softmax_axis_resident_kernel<CW, V, QU, RU>), grid, dim3(256), 0, s, a)
  if (resident && n <= 4 * RL) {
    if (vec) LH_AXIS_RESIDENT(true, 1, 1); else LH_AXIS_RESIDENT(false, 1, 1);
  } else if (resident && n <= 1024) {
    if (vec) LH_AXIS_RESIDENT(true, Q, 1); else LH_AXIS_RESIDENT(false, Q, 1);
  } else if (resident) {
    if (vec) LH_AXIS_RESIDENT(true, Q, RBIG); else LH_AXIS_RESIDENT(false, Q, RBIG);
  } else if (vec)
    hipLaunchKernelGGL((softmax_axis_stream_kernel<CW, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((softmax_axis_stream_kernel<CW, false>), grid, dim3(256), 0, s, a);
#undef LH_AXIS_RESIDENT
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_softmax_kernel = (int)plan[0];
  return e;
}

}  // namespace laser_hip
