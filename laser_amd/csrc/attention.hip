// laser_amd/csrc/attention.hip -- the fused attention forward (include/laser_hip.h, "Attention"): O = softmax(scale * Q K^T) V
// per (batch, head) slice, float32, with the score matrix never in global memory.  attention_plan.h is the launch plan.
//
// A workgroup of 4 waves owns BM = 32 query rows of one slice and strides over the units.  The Q block sits in LDS; the keys
// come in tiles of BN = 128, one K tile in LDS at a time, wave w taking keys 32 w .. 32 w + 31 of the tile.  A score block
// (32 rows x 32 keys per wave) is d / 2 v_mfma_f32_32x32x2_f32 from a zero accumulator: bit for bit the k-ascending fmaf
// chain from +0.  An odd d is padded with the pair (-0, 1): fma(-0, 1, c) is c for every c, -0 included.  Three sweeps:
//   1  the row maxima of s = scale * c under lh_reduce_max (order-free: per lane, across the 32 lanes of a row, across waves)
//   2  the row sums of e = lexp(s - m) in reduce_core.h's order applied to the row's n_i scores as a 1-D array.  The order has
//      1024 leaves per row and chunk of 8192: leaf kk takes elements kk, kk + 1024, .. of the chunk in ascending order.
//      Key tile `blk` of a step of 1024 keys gives lane (w, c) the leaf kk = 128 blk + 32 w + c of its 16 rows: 8 x 16
//      accumulators per lane, in registers.  At the end of a chunk the leaves fold by halving in the order's sequence:
//      kk + 2 and kk + 1 (the E = 4 accumulators of an order lane: two cross-lane moves), then the order lanes t = kk / 4:
//      t + 128, + 64, + 32 (blk: in registers), t + 16, + 8 (w: through LDS), t + 4, + 2, + 1 (c / 4: one lane per row).
//      Every e is +0 or positive, so a masked or absent element adds +0 where the order skips it: the same bits.
//   3  p = e / s (__fdiv_rn), +0 where masked, through LDS from the accumulator layout to the A-operand layout, and O += P V
//      on the same MFMA, wave w owning columns 32 w .. 32 w + 31 of O, V read from global memory (each lane row is 128
//      contiguous bytes) into 64 registers per lane before the tile's scores are computed.  Every 512 keys the chain's
//      accumulator is added to the running sum, unfused, and restarts at +0.  Keys past Tk in the last tile are the pair
//      (-0, 1) again.
// In causal mode the two score sweeps stop at the block's largest n_i; the third walks all Tk keys (include/laser_hip.h says
// why) but computes no score past it.  Scores at or past a row's n_i are never used: the MFMA computes them, a select drops them.
// Addresses past an operand are never formed into a load: the staging loops and the V fetch test the index first.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/laser_hip.h"
#include "attention_plan.h"
#include "common.h"
#include "gemm_mfma_kernel.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

static_assert(LH_ATTENTION_CHUNK == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of the order");
static_assert(LH_ATTENTION_BM == 32 && LH_ATTENTION_BN == 128 && LH_ATTENTION_MAX_D <= 128, "the lane mapping of attention.hip");
static_assert(LH_ATTENTION_MAX_CHUNKS == 8, "the second level folds two order lanes");

namespace laser_hip {

std::atomic<int> g_last_attention_kernel{-1};

namespace {

constexpr int BM = LH_ATTENTION_BM, BN = LH_ATTENTION_BN, PLD = LH_ATTENTION_P_LD, MAXC = LH_ATTENTION_MAX_CHUNKS;
using M32 = Mma<float>;

struct AttnArgs {
  float *o, *p, *rmax, *rsum;
  const float *q, *k, *v;
  long long os[3], ps[3], qs[3], ks[3], vs[3];  // element strides of batch, head, position
  long long heads, tq, units, qblocks;
  int tk, d, dv, causal;
  float scale;
};

// rows [t0, t0 + nrows) of an operand of `d` features into LDS rows of `ld` words, features d .. dp - 1 as `fpad`; rows at
// or past `tend` as zeros
template <bool VEC>
__device__ __forceinline__ void stage_rows(float *dst, const int ld, const float *src, const long long stride_t, const long long t0,
                                           const int nrows, const long long tend, const int d, const int dp, const float fpad) {
  const int g4 = (dp + 3) >> 2;
  for (int idx = threadIdx.x; idx < nrows * g4; idx += 256) {
    const int r = idx / g4, f = (idx - r * g4) * 4;
    float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t0 + r < tend) load4<VEC>(src + (t0 + r) * stride_t, f, d, fpad, q);
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (f + j < dp) dst[r * ld + f + j] = q[j];
  }
}

// the score block of this wave: rows of the Q block x keys 32 w .. 32 w + 31 of the K tile
__device__ __forceinline__ M32::Acc score_block(const float *Qs, const float *Ks, const int ld, const int dp, const int w, const int lane) {
  M32::Acc acc = {0};
  const float *qa = Qs + M32::lx(lane) * ld + M32::lk(lane);
  const float *kb = Ks + (w * 32 + M32::lx(lane)) * ld + M32::lk(lane);
  for (int s = 0; s < dp; s += 2) acc = M32::mma(qa[s], kb[s], acc);
  return acc;
}

template <bool VEC>
__global__ void __launch_bounds__(256) attention_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float at_lds[];
  const int d = a.d, dp = d + (d & 1), ld = dp | 1;  // (= lh_attention_ld(d), a host function)
  unsigned int *lut = (unsigned int *)at_lds;
  float *Qs = at_lds + LH_EXP_LUT_SIZE;
  float *Ks = Qs + BM * ld;
  float *Ps = Ks + BN * ld;
  float *wmax = Ps + BM * PLD;      // [4][BM]
  float *wsum = wmax + 4 * BM;      // [BM][4][8]
  float *part = wsum + BM * 32;     // [BM][MAXC]
  float *mrow = part + BM * MAXC;   // [BM]
  float *srow = mrow + BM;          // [BM]
  lut_to_lds(lut);
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, c = lane & 31, hi = lane >> 5;
  const int tk = a.tk, dv = a.dv;
  const float ninf = -__builtin_inff();
  const float scale = a.scale;

  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long bh = unit / a.qblocks, qb = unit - bh * a.qblocks;
    const long long b = bh / a.heads, h = bh - b * a.heads;
    const long long i0 = qb * BM;
    const int rows = (int)(a.tq - i0 < BM ? a.tq - i0 : BM);
    const float *q = a.q + b * a.qs[0] + h * a.qs[1];
    const float *k = a.k + b * a.ks[0] + h * a.ks[1];
    const float *v = a.v + b * a.vs[0] + h * a.vs[1];
    // row i sees keys [0, n_i): n_i = i + (Tk - Tq) + 1 in causal mode (Tq <= Tk there, so everything fits an int), else Tk
    const int off1 = a.causal ? (int)(i0 + (tk - a.tq) + 1) : 0;  // n of the block's first row
    int nmax = a.causal ? off1 + rows - 1 : tk;
    if (nmax > tk) nmax = tk;
    int nrow[16];  // n of this lane's 16 accumulator rows
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int n = a.causal ? off1 + M32::acc_row(r, lane) : tk;
      nrow[r] = n < tk ? n : tk;
    }

    __syncthreads();  // the last readers of Qs and of the scratch are done
    stage_rows<VEC>(Qs, ld, q, a.qs[2], i0, BM, a.tq, d, dp, -0.0f);

    // ---- sweep 1: the row maxima ----
    float m[16];
#pragma unroll
    for (int r = 0; r < 16; r++) m[r] = ninf;
    for (int j0 = 0; j0 < nmax; j0 += BN) {
      __syncthreads();
      stage_rows<VEC>(Ks, ld, k, a.ks[2], j0, BN, tk, d, dp, 1.0f);
      __syncthreads();
      const M32::Acc acc = score_block(Qs, Ks, ld, dp, w, lane);
      const int j = j0 + w * 32 + c;
#pragma unroll
      for (int r = 0; r < 16; r++)
        if (j < nrow[r]) m[r] = lh_reduce_max(m[r], scale * acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
#pragma unroll
      for (int x = 16; x >= 1; x /= 2) m[r] = lh_reduce_max(m[r], __shfl_xor(m[r], x));
      if (c == 0) wmax[w * BM + M32::acc_row(r, lane)] = m[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = M32::acc_row(r, lane);
      m[r] = lh_reduce_max(lh_reduce_max(wmax[row], wmax[BM + row]), lh_reduce_max(wmax[2 * BM + row], wmax[3 * BM + row]));
    }
    if (tid < BM) mrow[tid] = lh_reduce_max(lh_reduce_max(wmax[tid], wmax[BM + tid]), lh_reduce_max(wmax[2 * BM + tid], wmax[3 * BM + tid]));

    // ---- sweep 2: the row sums in the reduction order ----
    const int chunks = (nmax + LH_ATTENTION_CHUNK - 1) / LH_ATTENTION_CHUNK;
    for (int ch = 0; ch < chunks; ch++) {
      float leaf[8][16];
#pragma unroll
      for (int blk = 0; blk < 8; blk++) {
#pragma unroll
        for (int r = 0; r < 16; r++) leaf[blk][r] = 0.0f;
      }
      for (int step = 0; step < LH_REDUCE_STEPS; step++) {
        const int s0 = ch * LH_ATTENTION_CHUNK + step * 1024;
        if (s0 >= nmax) break;
#pragma unroll
        for (int blk = 0; blk < 8; blk++) {
          const int j0 = s0 + blk * BN;
          if (j0 < nmax) {  // (uniform over the workgroup)
            __syncthreads();
            stage_rows<VEC>(Ks, ld, k, a.ks[2], j0, BN, tk, d, dp, 1.0f);
            __syncthreads();
            const M32::Acc acc = score_block(Qs, Ks, ld, dp, w, lane);
            const int j = j0 + w * 32 + c;
#pragma unroll
            for (int r = 0; r < 16; r++) {
              const float e = j < nrow[r] ? lh_exp_with(scale * acc[r] - m[r], lut) : 0.0f;
              leaf[blk][r] = leaf[blk][r] + e;
            }
          }
        }
      }
      // the fold of the chunk's 1024 leaves of each row
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float u[8];
#pragma unroll
        for (int blk = 0; blk < 8; blk++) {
          float x = leaf[blk][r];
          x = x + __shfl_down(x, 2);  // accumulators j and j + 2 of an order lane
          x = x + __shfl_down(x, 1);  // then j and j + 1: lanes with c % 4 == 0 hold the order lane's value
          u[blk] = x;
        }
#pragma unroll
        for (int x = 4; x >= 1; x /= 2) {
#pragma unroll
          for (int blk = 0; blk < x; blk++) u[blk] = u[blk] + u[blk + x];
        }
        if ((c & 3) == 0) wsum[(M32::acc_row(r, lane) * 4 + w) * 8 + (c >> 2)] = u[0];
      }
      __syncthreads();
      if (tid < BM) {
        const float *x = wsum + tid * 32;
        float y[8];
#pragma unroll
        for (int i = 0; i < 8; i++) y[i] = (x[i] + x[16 + i]) + (x[8 + i] + x[24 + i]);
        part[tid * MAXC + ch] = ((y[0] + y[4]) + (y[2] + y[6])) + ((y[1] + y[5]) + (y[3] + y[7]));
      }
      __syncthreads();  // wsum is free for the next chunk, part[] is visible
    }
    if (tid < BM) {
      // the partials by the same rule: order lane 0 takes partials 0 .. 3, lane 1 partials 4 .. 7; absent ones are +0
      float pc[MAXC];
#pragma unroll
      for (int i = 0; i < MAXC; i++) pc[i] = i < chunks ? part[tid * MAXC + i] : 0.0f;
      const float s = ((pc[0] + pc[2]) + (pc[1] + pc[3])) + ((pc[4] + pc[6]) + (pc[5] + pc[7]));
      srow[tid] = s;
      if (tid < rows) {
        if (a.rmax) a.rmax[bh * a.tq + i0 + tid] = mrow[tid];
        if (a.rsum) a.rsum[bh * a.tq + i0 + tid] = s;
      }
    }
    __syncthreads();
    if (!a.o && !a.p) continue;

    // ---- sweep 3: P, and O = P V in 512-key slices ----
    float sum[16];
#pragma unroll
    for (int r = 0; r < 16; r++) sum[r] = srow[M32::acc_row(r, lane)];
    float *pg = a.p ? a.p + b * a.ps[0] + h * a.ps[1] : nullptr;
    M32::Acc oacc = {0}, orun = {0};
    const int col = w * 32 + c;
    const bool owns = a.o && w * 32 < dv;  // (uniform over the wave)
    for (int j0 = 0; j0 < tk; j0 += BN) {
      M32::Acc pv = {0};
      const int j = j0 + w * 32 + c;
      // this lane's B operands of the tile's P V steps, fetched ahead of the scores so that the loads fly under them
      float bv[BN / 2];
      if (owns) {
#pragma unroll
        for (int i = 0; i < BN / 2; i++) {
          const int key = j0 + 2 * i + hi;
          bv[i] = key < tk ? (col < dv ? v[key * a.vs[2] + col] : 0.0f) : 1.0f;
        }
      }
      if (j0 < nmax) {  // (uniform over the workgroup)
        __syncthreads();
        stage_rows<VEC>(Ks, ld, k, a.ks[2], j0, BN, tk, d, dp, 1.0f);
        __syncthreads();
        const M32::Acc acc = score_block(Qs, Ks, ld, dp, w, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) pv[r] = j < nrow[r] ? __fdiv_rn(lh_exp_with(scale * acc[r] - m[r], lut), sum[r]) : 0.0f;
      } else {
        __syncthreads();  // the last readers of Ps are done
      }
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = M32::acc_row(r, lane);
        Ps[row * PLD + w * 32 + c] = j < tk ? pv[r] : -0.0f;
        if (pg && row < rows && j < tk) pg[(i0 + row) * a.ps[2] + j] = pv[r];
      }
      if (!a.o) continue;
      __syncthreads();
      if (owns) {
        if (j0 > 0 && (j0 & 511) == 0) {  // a slice of 512 keys ends: S_0, then (.. + S_p), unfused
          if (j0 == 512) {
            orun = oacc;
          } else {
#pragma unroll
            for (int r = 0; r < 16; r++) orun[r] = orun[r] + oacc[r];
          }
#pragma unroll
          for (int r = 0; r < 16; r++) oacc[r] = 0.0f;
        }
        const float *pa = Ps + c * PLD + hi;
#pragma unroll
        for (int i = 0; i < BN / 2; i++) oacc = M32::mma(pa[2 * i], bv[i], oacc);
      }
    }
    if (owns) {
      if (tk > 512) {
#pragma unroll
        for (int r = 0; r < 16; r++) oacc[r] = orun[r] + oacc[r];
      }
      float *o = a.o + b * a.os[0] + h * a.os[1];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = M32::acc_row(r, lane);
        if (row < rows && col < dv) o[(i0 + row) * a.os[2] + col] = oacc[r];
      }
    }
  }
}

bool aligned16(const float *p, const int64_t *st) { return (uintptr_t)p % 16 == 0 && st[0] % 4 == 0 && st[1] % 4 == 0 && st[2] % 4 == 0; }

}  // namespace

hipError_t launch_attention_f32(float *o, const int64_t *os, const float *q, const int64_t *qs, const float *k, const int64_t *ks,
                                const float *v, const int64_t *vs, float *probs, const int64_t *ps, float *row_max, float *row_sum,
                                int64_t batch, int64_t heads, int64_t tq, int64_t tk, int64_t d, int64_t dv, float scale, int causal,
                                hipStream_t s) {
  const bool vec = aligned16(q, qs) && aligned16(k, ks);
  long long plan[5];
  if (lh_attention_plan(batch * heads, tq, tk, d, dv, causal, vec ? 1 : 0, plan) != 0) return hipErrorInvalidValue;
  if (plan[4] == 0) return hipSuccess;
  AttnArgs a = {};
  a.o = o, a.p = probs, a.rmax = row_max, a.rsum = row_sum, a.q = q, a.k = k, a.v = v;
  for (int i = 0; i < 3; i++) {
    a.os[i] = o ? os[i] : 0, a.ps[i] = probs ? ps[i] : 0;
    a.qs[i] = qs[i], a.ks[i] = ks[i], a.vs[i] = vs[i];
  }
  a.heads = heads, a.tq = tq, a.units = plan[4], a.qblocks = plan[4] / (batch * heads);
  a.tk = (int)tk, a.d = (int)d, a.dv = (int)dv, a.causal = causal ? 1 : 0, a.scale = scale;
  const void *kern = vec ? reinterpret_cast<const void *>(attention_kernel<true>) : reinterpret_cast<const void *>(attention_kernel<false>);
  hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan[3]);
  if (e != hipSuccess) return e;
  if (vec)
    hipLaunchKernelGGL(attention_kernel<true>, dim3((unsigned)plan[2]), dim3(256), (size_t)plan[3], s, a);
  else
    hipLaunchKernelGGL(attention_kernel<false>, dim3((unsigned)plan[2]), dim3(256), (size_t)plan[3], s, a);
  e = hipGetLastError();
  if (e == hipSuccess) g_last_attention_kernel = (int)plan[1];
  return e;
}

}  // namespace laser_hip
