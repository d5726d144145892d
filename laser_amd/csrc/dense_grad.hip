// laser_amd/csrc/dense_grad.hip -- the backward pass of a dense layer's activation and bias in one read (include/laser_hip.h,
// "Dense-layer backward"): dz[r, j] = act_grad_core.h's rule of (dy[r, j], y[r, j]) and db[j] = the sum of dz[0..rows, j] in
// reduce_core.h's order for a 1-D array of `rows` float32 (E = 4, init +0) -- reduce_sum of the column.
//
// A workgroup of 256 lanes owns one unit at a time: a chunk of 8192 rows (one chunk of the order) by a strip of CW = 16
// columns; bias_grad_plan.h has the units, the grid and the launches.  Lane tid = rl * 4 + l takes the 4 adjacent columns
// 4 l .. 4 l + 3 of the strip (4 lanes span a strip row: one run of 64 contiguous bytes, 16 per lane) and is row lane rl of 64,
// exactly as softmax_axis.hip's streaming kernel maps its lanes.
//
// The order, per column and chunk: row k of the chunk goes to leaf a = k mod 1024; a leaf starts at +0 and takes its up to 8
// elements in ascending k; the 1024 leaves are folded over the bits of a in the order 1, 0, 9, 8, .., 2 (higher index into
// lower).  Row lane rl holds the leaves a = q * 256 + 4 rl + p, p = 0 .. 3, q = 0 .. 3, of each of its 4 columns: 64
// accumulators.  Bits 1 and 0 of a are p and bits 9 and 8 are q: both fold inside the lane, in that order (lane_fold); bits
// 7 .. 2 are rl, which folds last over the lanes (col_fold).  A chunk that is the whole column writes db; otherwise its
// partial goes to P[chunk, j], and P is one more such array: the same kernel, no activation, no dz, rows = chunks.
//
// No workgroup waits on another, nothing is atomic, every access is bounded by rows and n.  A row past the end is neither
// read nor written; its leaves keep +0 (adding +0 to a running sum changes nothing: a sum that started at +0 is never -0).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "act_grad_core.h"
#include "bias_grad_plan.h"
#include "common.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

static_assert(LH_BIAS_GRAD_CHUNK == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of rows is a chunk of the order");
static_assert(LH_BIAS_GRAD_CW == 16 && LH_BIAS_GRAD_MAX_WORKGROUPS == 2048, "the kernel's lane mapping and the plan agree");
static_assert(LH_BIAS_GRAD_MAX_ROWS == LASER_HIP_BIAS_GRAD_MAX_ROWS, "plan and header agree");
static_assert(LH_BIAS_GRAD_MAX_ROWS / LH_BIAS_GRAD_CHUNK <= LH_BIAS_GRAD_CHUNK, "the chunk partials of a column fit one chunk");

namespace laser_hip {

std::atomic<int> g_last_bias_grad_kernel{-1};

namespace {

constexpr int CW = LH_BIAS_GRAD_CW, LPR = CW / 4, RL = 256 / LPR, Q = 1024 / (4 * RL);

struct DenseGradArgs {
  float *out;          // the partial of chunk c and column j goes to out[c * out_chunk_stride + j * out_col_stride]
  long long out_chunk_stride, out_col_stride;
  float *dz;           // null: not stored
  const float *dy, *y;
  long long dzs, dys, ys;  // row strides in elements
  long long rows, n, strips, chunks;
  long long step_chunks, step_strips;  // gridDim.x / strips and gridDim.x % strips: from one unit of a workgroup to its next
};

// 4 adjacent columns of one row, p = the address of the first.  V: one 16-byte vector (the strip lies inside n, bases and row
// strides are multiples of 16 bytes); otherwise the first `cols` of them one by one.  A row that does not exist (`valid` false)
// is neither read nor written and loads as +0.
template <bool V>
__device__ __forceinline__ void load_row(const float *p, const int cols, const bool valid, float (&q)[4]) {
  if (V) {
    F4 f = {{0.0f, 0.0f, 0.0f, 0.0f}};
    if (valid) f = *(const F4 *)p;
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = f.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = valid && j < cols ? p[j] : 0.0f;
  }
}
template <bool V>
__device__ __forceinline__ void store_row(float *p, const int cols, const bool valid, const float (&q)[4]) {
  if (V) {
    F4 f;
#pragma unroll
    for (int j = 0; j < 4; j++) f.v[j] = q[j];
    if (valid) *(F4 *)p = f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (valid && j < cols) p[j] = q[j];
  }
}

// One unit: the chunk's rows k0 .. k0 + rem of the lane's 4 columns from column c.  V: as above; FULL: rem == 8192, no row is tested
template <int ACT, bool V, bool FULL>
__device__ __forceinline__ void grad_unit(const DenseGradArgs &a, const long long k0, const int rem, const long long c, F4 *red4,
                                          float *sums) {
  const int rl = threadIdx.x / LPR;
  const int cols = (int)max(0ll, min(4ll, a.n - c));
  const bool store = a.dz != nullptr;  // (the same for every lane)
  // Element offsets of the lane's first row of the current step; a step's 4 rows lie 0 .. 3 row strides below it, and the
  // next step 4 RL rows further.  The offsets are walked, and hidden from the compiler after every step: left to itself it
  // keeps the 16 (step, row) offsets of every operand of the 8-step loop in registers, 96 of them, and the 64 sums on top
  // leave one workgroup per CU.
  long long ody = (k0 + rl * 4) * a.dys + c, oy = (k0 + rl * 4) * a.ys + c, odz = (k0 + rl * 4) * a.dzs + c;
  float acc[Q][4][4];
#pragma unroll
  for (int q = 0; q < Q; q++) {
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
      for (int j = 0; j < 4; j++) acc[q][p][j] = 0.0f;
    }
  }
#pragma unroll 1
  for (int r = 0; r < LH_REDUCE_STEPS && (FULL || r * 1024 < rem); r++) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int row0 = r * 1024 + q * 4 * RL;  // the step's first row: the same for every lane
      if (FULL || row0 < rem) {
        float g[4][4], f[4][4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const bool valid = FULL || row0 + rl * 4 + p < rem;
          load_row<V>(a.dy + (ody + p * a.dys), cols, valid, g[p]);
          if (ACT != LASER_HIP_ACT_NONE) load_row<V>(a.y + (oy + p * a.ys), cols, valid, f[p]);
        }
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const bool valid = FULL || row0 + rl * 4 + p < rem;
          if (ACT != LASER_HIP_ACT_NONE) {
#pragma unroll
            for (int j = 0; j < 4; j++) g[p][j] = lh_act_grad<ACT>(g[p][j], f[p][j]);
          }
          if (store) store_row<V>(a.dz + (odz + p * a.dzs), cols, valid, g[p]);
#pragma unroll
          for (int j = 0; j < 4; j++) acc[q][p][j] = acc[q][p][j] + (valid ? g[p][j] : 0.0f);
        }
      }
      ody += 4 * RL * a.dys;
      oy += 4 * RL * a.ys;
      odz += 4 * RL * a.dzs;
      asm volatile("" : "+v"(ody), "+v"(oy), "+v"(odz));
    }
  }
  float v[4];
  lane_fold<Q, Q>(acc, v);
  col_fold<CW>(v, red4, sums);
}

template <int ACT, bool VEC>
__global__ void __launch_bounds__(256) dense_grad_kernel(const DenseGradArgs a) {
  __shared__ F4 red4[256];
  __shared__ float sums[CW];
  // unit = chunk * strips + strip, walked without a 64-bit division (its expansion is float arithmetic with fused
  // multiply-adds, which this file keeps out of its kernels): the grid is at most 2048, so the first unit divides in 32 bits
  long long ch = 0, strip = blockIdx.x;
  if (strip >= a.strips) {
    ch = blockIdx.x / (unsigned)a.strips;
    strip = blockIdx.x % (unsigned)a.strips;
  }
  for (; ch < a.chunks; ch += a.step_chunks, strip += a.step_strips) {
    if (strip >= a.strips) {
      strip -= a.strips;
      if (++ch >= a.chunks) break;
    }
    const long long c0 = strip * CW;
    const long long c = c0 + (threadIdx.x % LPR) * 4;
    const long long k0 = ch * LH_BIAS_GRAD_CHUNK;
    const int rem = (int)min((long long)LH_BIAS_GRAD_CHUNK, a.rows - k0);  // rows of this chunk (0 only when rows == 0)
    const bool full = rem == LH_BIAS_GRAD_CHUNK;
    if (VEC && c0 + CW <= a.n) {
      if (full) grad_unit<ACT, true, true>(a, k0, rem, c, red4, sums);
      else grad_unit<ACT, true, false>(a, k0, rem, c, red4, sums);
    } else {
      if (full) grad_unit<ACT, false, true>(a, k0, rem, c, red4, sums);
      else grad_unit<ACT, false, false>(a, k0, rem, c, red4, sums);
    }
    if (threadIdx.x < CW && c0 + threadIdx.x < a.n)
      a.out[ch * a.out_chunk_stride + (c0 + threadIdx.x) * a.out_col_stride] = sums[threadIdx.x];
  }
}

template <bool VEC>
hipError_t launch_instance(int act, const DenseGradArgs &a, unsigned grid, hipStream_t s) {
  switch (act) {
    case LASER_HIP_ACT_NONE: hipLaunchKernelGGL((dense_grad_kernel<LASER_HIP_ACT_NONE, VEC>), dim3(grid), dim3(256), 0, s, a); break;
    case LASER_HIP_ACT_RELU: hipLaunchKernelGGL((dense_grad_kernel<LASER_HIP_ACT_RELU, VEC>), dim3(grid), dim3(256), 0, s, a); break;
    case LASER_HIP_ACT_TANH: hipLaunchKernelGGL((dense_grad_kernel<LASER_HIP_ACT_TANH, VEC>), dim3(grid), dim3(256), 0, s, a); break;
    case LASER_HIP_ACT_SIGMOID:
      hipLaunchKernelGGL((dense_grad_kernel<LASER_HIP_ACT_SIGMOID, VEC>), dim3(grid), dim3(256), 0, s, a);
      break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

bool vec_ok(const void *p, long long stride, long long rows) {
  // (a row stride that is never applied -- at most one row -- does not count)
  return p == nullptr || ((uintptr_t)p % 16 == 0 && (rows <= 1 || stride % 4 == 0));
}

}  // namespace

hipError_t launch_bias_grad_f32(float *db, int64_t db_stride, float *dz, int64_t dzs, const float *dy, int64_t dys, const float *y,
                                int64_t ys, int64_t rows, int64_t n, int act, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (act == LASER_HIP_ACT_NONE) y = nullptr;
  const bool vec = vec_ok(dz, dzs, rows) && vec_ok(dy, dys, rows) && vec_ok(y, ys, rows);
  long long plan[4];
  if (lh_bias_grad_plan(rows, n, vec, 0, plan) != 0) return hipErrorInvalidValue;
  const long long chunks = rows == 0 ? 1 : (rows + LH_BIAS_GRAD_CHUNK - 1) / LH_BIAS_GRAD_CHUNK;
  DenseGradArgs a;
  a.dz = dz;
  a.dy = dy;
  a.y = y;
  a.dzs = dzs;
  a.dys = dys;
  a.ys = ys;
  a.rows = rows;
  a.n = n;
  a.strips = (n + CW - 1) / CW;
  a.chunks = chunks;
  a.step_chunks = plan[1] / a.strips;
  a.step_strips = plan[1] % a.strips;
  float *part = nullptr;
  if (plan[2] == 2) {
    const hipError_t e = scratch_alloc_async((void **)&part, (size_t)plan[3] * sizeof(float), s);
    if (e != hipSuccess) return e;
    a.out = part;
    a.out_chunk_stride = n;
    a.out_col_stride = 1;
  } else {
    a.out = db;
    a.out_chunk_stride = 0;
    a.out_col_stride = db_stride;
  }
  hipError_t e = vec ? launch_instance<true>(act, a, (unsigned)plan[1], s) : launch_instance<false>(act, a, (unsigned)plan[1], s);
  if (e == hipSuccess && part != nullptr) {
    // the chunk partials of a column are one more array under the same rule: rows = chunks <= 8192, one chunk
    DenseGradArgs b;
    b.out = db;
    b.out_chunk_stride = 0;
    b.out_col_stride = db_stride;
    b.dz = nullptr;
    b.dy = part;
    b.y = nullptr;
    b.dzs = b.ys = 0;
    b.dys = n;
    b.rows = chunks;
    b.n = n;
    b.strips = a.strips;
    b.chunks = 1;
    const unsigned grid = (unsigned)std::min<long long>(LH_BIAS_GRAD_MAX_WORKGROUPS, b.strips);
    b.step_chunks = grid / b.strips;
    b.step_strips = grid % b.strips;
    e = n % 4 == 0 ? launch_instance<true>(LASER_HIP_ACT_NONE, b, grid, s) : launch_instance<false>(LASER_HIP_ACT_NONE, b, grid, s);
  }
  if (part != nullptr) {
    const hipError_t f = scratch_free_async(part, s);
    if (e == hipSuccess) e = f;
  }
  if (e == hipSuccess) g_last_bias_grad_kernel = (int)plan[0];
  return e;
}

}  // namespace laser_hip
