// laser_amd/csrc/layer_norm.hip -- layer normalization over the rows of a matrix, forward and backward (include/laser_hip.h,
// "Layer normalization").  Every operation is one correctly rounded float32 operation (+ - x, __fdiv_rn, __builtin_sqrtf),
// never fused, and every sum runs in reduce_core.h's order (E = 4, W = 256 lanes, R = 8 steps, init +0): a row sum as
// reduce_sum of the row's n float32, a column sum as reduce_sum of the column's `rows` float32 (dense_grad.hip's order).
//
//   forward   mean = rsum(x) / nf;  d = x - mean;  var = rsum(d * d) / nf;  rstd = 1 / sqrt(var + eps);
//             y = ((d * rstd) * gamma) + beta        (gamma absent: no multiply; beta absent: no add)
//   dx        xhat = (x - mean) * rstd;  g = dy * gamma (or dy);  a = rsum(g) / nf;  b = rsum(g * xhat) / nf;
//             dx = ((g - a) - xhat * b) * rstd
//   params    dbeta[j] = csum(dy[:, j]),  dgamma[j] = csum(dy[:, j] * xhat[:, j])
//
// An accumulator of the order starts at +0 and ADDS its first element: +0 + -0 = +0, so a row of -0 has the sum +0 and the
// kernels write `0.0f + x` where the softmax kernels (whose terms are never -0) may skip it.  An accumulator that started at
// +0 is never -0 afterwards, so adding +0 for an element past the end changes nothing: that is how the tails are skipped.
//
// The row kernels (forward, dx) have log_softmax.hip's three lane mappings, chosen by n alone (layer_norm_plan.h), each with
// a 16-byte-vector instance and a single-element one: same values, same order.
//   *_wave_kernel    n <= 1024: one wave per row, four rows per workgroup.  Lane l holds the order's lanes l, l + 64, l + 128,
//                    l + 192 (four elements each); the row never leaves the registers, no LDS.
//   *_block_kernel   n <= 8192 (one chunk): one workgroup per row, lane t = the order's lane t, 8 steps x 4 elements in
//                    registers between the passes; the lane fold goes through LDS (block_sum).
//   *_long_kernel    longer rows: one workgroup walks the row's chunks.  Chunk c's partial is element c of the array of
//                    partials, which the order gives to lane (c mod 1024) / 4, accumulator c mod 4, in ascending c: that lane
//                    adds it as it appears (take_partial), so the partials need no table in LDS.  x is read once per pass:
//                    three passes forward (mean, variance, y), two backward (a and b together, dx).
// Results are stored after the last read of the same elements by the same lane, so y may be x and dx may be dy or x.
//
// The column kernel (dgamma, dbeta) is dense_grad.hip's: a workgroup owns a (chunk of 8192 rows) x (strip of CW columns) unit
// and a lane 4 adjacent columns of every 4 RL-th group of 4 rows; both sums come from one read of dy and x with two
// accumulator sets.  CW = LH_LAYER_NORM_CW = 8: 2 x 32 accumulators per lane (profiles/layer_norm/README.md).  Longer
// columns write their chunk partials to scratch, and those are folded as the bias gradient folds its own: by
// launch_bias_grad_f32 on the partial matrix.
//
// No workgroup waits on another, nothing is atomic, every access is bounded by rows and n.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "layer_norm_plan.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

static_assert(LH_LAYER_NORM_MAX_WORKGROUPS == LH_SOFTMAX_MAX_WORKGROUPS, "one cap for every row kernel");
static_assert(LH_LAYER_NORM_CHUNK == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of the order");
static_assert(LH_LAYER_NORM_MAX_N == LASER_HIP_LAYER_NORM_MAX_N && LH_LAYER_NORM_MAX_ROWS == LASER_HIP_LAYER_NORM_MAX_ROWS,
              "plan and header agree");
static_assert(LH_LAYER_NORM_MAX_ROWS / LH_LAYER_NORM_CHUNK <= LH_LAYER_NORM_CHUNK, "the chunk partials of a column fit one chunk");
static_assert(LH_LAYER_NORM_MAX_N / LH_LAYER_NORM_CHUNK <= LH_LAYER_NORM_CHUNK, "the chunk partials of a row fit one chunk");
static_assert(LH_LAYER_NORM_CW == 8 || LH_LAYER_NORM_CW == 16, "the column kernel's lane mapping");

namespace laser_hip {

std::atomic<int> g_last_layer_norm_kernel[3] = {{-1}, {-1}, {-1}};

namespace {

struct FwdArgs {
  float *y;
  long long ys;
  float *mean, *rstd;  // either may be null
  long long ms, rs;
  const float *x;
  long long xs;
  const float *gamma, *beta;  // either may be null
  long long gs, bs;
  long long rows, n;
  float eps;
};

struct DxArgs {
  float *dx;
  long long dxs;
  const float *dy, *x;
  long long dys, xs;
  const float *mean, *rstd;
  long long ms, rs;
  const float *gamma;  // may be null
  long long gs;
  long long rows, n;
};

// elements base .. base + 3 of gamma or beta: VEC: unit stride and a 16-byte aligned base; +0 where the row has ended
template <bool VEC>
__device__ __forceinline__ void load4p(const float *p, const long long stride, const long long base, const long long n, float (&q)[4]) {
  if (VEC) {
    load4<true>(p, base, n, 0.0f, q);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = base + j < n ? p[(base + j) * stride] : 0.0f;
  }
}

__device__ __forceinline__ float rstd_of(const float var, const float eps) { return __fdiv_rn(1.0f, __builtin_sqrtf(var + eps)); }

// y = xhat * gamma + beta for 4 elements from `base`, two roundings, either parameter absent
template <bool VEC>
__device__ __forceinline__ void affine4(const FwdArgs &a, const long long base, float (&q)[4]) {
  if (a.gamma) {
    float g[4];
    load4p<VEC>(a.gamma, a.gs, base, a.n, g);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = q[j] * g[j];
  }
  if (a.beta) {
    float b[4];
    load4p<VEC>(a.beta, a.bs, base, a.n, b);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = q[j] + b[j];
  }
}

// g = dy * gamma (dy itself without gamma) for 4 elements from `base`
template <bool VEC>
__device__ __forceinline__ void scale4(const DxArgs &a, const long long base, float (&q)[4]) {
  if (a.gamma) {
    float g[4];
    load4p<VEC>(a.gamma, a.gs, base, a.n, g);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = q[j] * g[j];
  }
}

// the order's fold of the 4 lanes l, l + 64, l + 128, l + 192 that one lane of a wave holds, then of the wave; every lane gets it
__device__ __forceinline__ float wave_sum(const float (&v)[4]) { return __shfl(wave_fold((v[0] + v[2]) + (v[1] + v[3])), 0); }

// a long row's second level: the partial p of chunk c joins accumulator c mod 4 of lane (c mod 1024) / 4
__device__ __forceinline__ void take_partial(float (&pacc)[4], const int c, const float p) {
  const bool mine = (int)threadIdx.x == ((c & 1023) >> 2);
#pragma unroll
  for (int j = 0; j < 4; j++) pacc[j] = pacc[j] + (mine && j == (c & 3) ? p : 0.0f);
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) ln_fwd_wave_kernel(const FwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = (int)a.n;
  const float nf = (float)a.n;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += (long long)gridDim.x * 4) {
    const float *x = a.x + row * a.xs;
    float e[4][4], v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {  // the order's lane lane + 64 k, step 0
      load4<VEC>(x, k * 256 + lane * 4, n, 0.0f, e[k]);
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; j++) p[j] = 0.0f + e[k][j];
      v[k] = (p[0] + p[2]) + (p[1] + p[3]);
    }
    const float mean = __fdiv_rn(wave_sum(v), nf);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      float p[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = e[k][j] - mean;
        e[k][j] = d;
        p[j] = 0.0f + (k * 256 + lane * 4 + j < n ? d * d : 0.0f);
      }
      v[k] = (p[0] + p[2]) + (p[1] + p[3]);
    }
    const float rstd = rstd_of(__fdiv_rn(wave_sum(v), nf), a.eps);
    if (lane == 0) {
      if (a.mean) a.mean[row * a.ms] = mean;
      if (a.rstd) a.rstd[row * a.rs] = rstd;
    }
    float *y = a.y + row * a.ys;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int base = k * 256 + lane * 4;
      if (base >= n) break;
#pragma unroll
      for (int j = 0; j < 4; j++) e[k][j] = e[k][j] * rstd;
      affine4<VEC>(a, base, e[k]);
      store4<VEC>(y, base, n, e[k]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) ln_fwd_block_kernel(const FwdArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  const int t = threadIdx.x;
  const long long n = a.n;
  const float nf = (float)a.n;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.x + row * a.xs;
    float e[R][4];
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
      load4<VEC>(x, r * 1024 + t * 4, n, 0.0f, e[r]);
#pragma unroll
      for (int j = 0; j < 4; j++) acc[j] = acc[j] + e[r][j];
    }
    const float mean = __fdiv_rn(block_sum(acc, red), nf);
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = 0.0f;
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float d = e[r][j] - mean;
        e[r][j] = d;
        acc[j] = acc[j] + (r * 1024 + t * 4 + j < n ? d * d : 0.0f);
      }
    }
    const float rstd = rstd_of(__fdiv_rn(block_sum(acc, red), nf), a.eps);
    if (t == 0) {
      if (a.mean) a.mean[row * a.ms] = mean;
      if (a.rstd) a.rstd[row * a.rs] = rstd;
    }
    float *y = a.y + row * a.ys;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const long long base = r * 1024 + t * 4;
      if (base >= n) break;
#pragma unroll
      for (int j = 0; j < 4; j++) e[r][j] = e[r][j] * rstd;
      affine4<VEC>(a, base, e[r]);
      store4<VEC>(y, base, n, e[r]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) ln_fwd_long_kernel(const FwdArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  const int t = threadIdx.x;
  const long long n = a.n;
  const float nf = (float)a.n;
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.x + row * a.xs;
    float pacc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < chunks; c++) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        float q[4];
        load4<VEC>(x, (long long)c * kChunk + r * 1024 + t * 4, n, 0.0f, q);
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = acc[j] + q[j];
      }
      take_partial(pacc, c, block_sum(acc, red));
    }
    const float mean = __fdiv_rn(block_sum(pacc, red), nf);
#pragma unroll
    for (int j = 0; j < 4; j++) pacc[j] = 0.0f;
    for (int c = 0; c < chunks; c++) {
      float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long base = (long long)c * kChunk + r * 1024 + t * 4;
        float q[4];
        load4<VEC>(x, base, n, 0.0f, q);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float d = q[j] - mean;
          acc[j] = acc[j] + (base + j < n ? d * d : 0.0f);
        }
      }
      take_partial(pacc, c, block_sum(acc, red));
    }
    const float rstd = rstd_of(__fdiv_rn(block_sum(pacc, red), nf), a.eps);
    if (t == 0) {
      if (a.mean) a.mean[row * a.ms] = mean;
      if (a.rstd) a.rstd[row * a.rs] = rstd;
    }
    float *y = a.y + row * a.ys;
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float q[4];
      load4<VEC>(x, base, n, 0.0f, q);
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = (q[j] - mean) * rstd;
      affine4<VEC>(a, base, q);
      store4<VEC>(y, base, n, q);
    }
  }
}

// ---- dx -----------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) ln_dx_wave_kernel(const DxArgs a) {
  const int lane = threadIdx.x & 63;
  const int n = (int)a.n;
  const float nf = (float)a.n;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += (long long)gridDim.x * 4) {
    const float *x = a.x + row * a.xs, *dy = a.dy + row * a.dys;
    const float mean = a.mean[row * a.ms], rstd = a.rstd[row * a.rs];
    float g[4][4], h[4][4], va[4], vb[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int base = k * 256 + lane * 4;
      load4<VEC>(dy, base, n, 0.0f, g[k]);
      load4<VEC>(x, base, n, 0.0f, h[k]);
      scale4<VEC>(a, base, g[k]);
      float p[4], q[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool in = base + j < n;
        h[k][j] = (h[k][j] - mean) * rstd;
        p[j] = 0.0f + (in ? g[k][j] : 0.0f);
        q[j] = 0.0f + (in ? g[k][j] * h[k][j] : 0.0f);
      }
      va[k] = (p[0] + p[2]) + (p[1] + p[3]);
      vb[k] = (q[0] + q[2]) + (q[1] + q[3]);
    }
    const float ca = __fdiv_rn(wave_sum(va), nf);
    const float cb = __fdiv_rn(wave_sum(vb), nf);
    float *dx = a.dx + row * a.dxs;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int base = k * 256 + lane * 4;
      if (base >= n) break;
#pragma unroll
      for (int j = 0; j < 4; j++) g[k][j] = ((g[k][j] - ca) - h[k][j] * cb) * rstd;
      store4<VEC>(dx, base, n, g[k]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) ln_dx_block_kernel(const DxArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  const int t = threadIdx.x;
  const long long n = a.n;
  const float nf = (float)a.n;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.x + row * a.xs, *dy = a.dy + row * a.dys;
    const float mean = a.mean[row * a.ms], rstd = a.rstd[row * a.rs];
    float g[R][4], h[R][4];
    float aa[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ab[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int r = 0; r < R; r++) {
      const long long base = r * 1024 + t * 4;
      load4<VEC>(dy, base, n, 0.0f, g[r]);
      load4<VEC>(x, base, n, 0.0f, h[r]);
      scale4<VEC>(a, base, g[r]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool in = base + j < n;
        h[r][j] = (h[r][j] - mean) * rstd;
        aa[j] = aa[j] + (in ? g[r][j] : 0.0f);
        ab[j] = ab[j] + (in ? g[r][j] * h[r][j] : 0.0f);
      }
    }
    const float ca = __fdiv_rn(block_sum(aa, red), nf);
    const float cb = __fdiv_rn(block_sum(ab, red), nf);
    float *dx = a.dx + row * a.dxs;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const long long base = r * 1024 + t * 4;
      if (base >= n) break;
#pragma unroll
      for (int j = 0; j < 4; j++) g[r][j] = ((g[r][j] - ca) - h[r][j] * cb) * rstd;
      store4<VEC>(dx, base, n, g[r]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) ln_dx_long_kernel(const DxArgs a) {
  constexpr int R = LH_REDUCE_STEPS;
  __shared__ float red[260];
  const int t = threadIdx.x;
  const long long n = a.n;
  const float nf = (float)a.n;
  const int chunks = (int)((n + kChunk - 1) / kChunk);
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const float *x = a.x + row * a.xs, *dy = a.dy + row * a.dys;
    const float mean = a.mean[row * a.ms], rstd = a.rstd[row * a.rs];
    float pa[4] = {0.0f, 0.0f, 0.0f, 0.0f}, pb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c = 0; c < chunks; c++) {
      float aa[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ab[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < R; r++) {
        const long long base = (long long)c * kChunk + r * 1024 + t * 4;
        float g[4], h[4];
        load4<VEC>(dy, base, n, 0.0f, g);
        load4<VEC>(x, base, n, 0.0f, h);
        scale4<VEC>(a, base, g);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const bool in = base + j < n;
          const float xh = (h[j] - mean) * rstd;
          aa[j] = aa[j] + (in ? g[j] : 0.0f);
          ab[j] = ab[j] + (in ? g[j] * xh : 0.0f);
        }
      }
      take_partial(pa, c, block_sum(aa, red));
      take_partial(pb, c, block_sum(ab, red));
    }
    const float ca = __fdiv_rn(block_sum(pa, red), nf);
    const float cb = __fdiv_rn(block_sum(pb, red), nf);
    float *dx = a.dx + row * a.dxs;
#pragma unroll 4
    for (long long base = t * 4; base < n; base += 1024) {
      float g[4], h[4];
      load4<VEC>(dy, base, n, 0.0f, g);
      load4<VEC>(x, base, n, 0.0f, h);
      scale4<VEC>(a, base, g);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float xh = (h[j] - mean) * rstd;
        g[j] = ((g[j] - ca) - xh * cb) * rstd;
      }
      store4<VEC>(dx, base, n, g);
    }
  }
}

// ---- dgamma and dbeta -----------------------------------------------------------------------------------------------------------
constexpr int CW = LH_LAYER_NORM_CW, LPR = CW / 4, RL = 256 / LPR, Q = 1024 / (4 * RL);

struct ParamArgs {
  float *outg, *outb;  // the partial of chunk c and column j goes to out[c * out_chunk_stride + j * out?_col_stride]
  long long out_chunk_stride, outg_col_stride, outb_col_stride;
  const float *dy, *x, *mean, *rstd;
  long long dys, xs, ms, rs;  // row strides in elements
  long long rows, n, strips, chunks;
  long long step_chunks, step_strips;  // gridDim.x / strips and gridDim.x % strips: from one unit of a workgroup to its next
};

// 4 adjacent columns of one row, as dense_grad.hip loads them: V: one 16-byte vector; otherwise the first `cols` one by one.
// A row that does not exist (`valid` false) is not read and loads as +0.
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

// One unit: the chunk's rows k0 .. k0 + rem of the lane's 4 columns from column c.  G, B: dgamma, dbeta wanted; FULL: rem == 8192
template <bool G, bool B, bool V, bool FULL>
__device__ __forceinline__ void param_unit(const ParamArgs &a, const long long k0, const int rem, const long long c, F4 *red4,
                                           float *sumg, float *sumb) {
  const int rl = threadIdx.x / LPR;
  const int cols = (int)max(0ll, min(4ll, a.n - c));
  // the offsets of the lane's first row of the current step are walked and hidden from the compiler after every step, as in
  // dense_grad.hip: otherwise every (step, row) offset of every operand stays in registers next to the sums
  long long ody = (k0 + rl * 4) * a.dys + c, ox = (k0 + rl * 4) * a.xs + c, om = (k0 + rl * 4) * a.ms, ors = (k0 + rl * 4) * a.rs;
  float accg[Q][4][4], accb[Q][4][4];
#pragma unroll
  for (int q = 0; q < Q; q++) {
#pragma unroll
    for (int p = 0; p < 4; p++) {
#pragma unroll
      for (int j = 0; j < 4; j++) accg[q][p][j] = accb[q][p][j] = 0.0f;
    }
  }
#pragma unroll 1
  for (int r = 0; r < LH_REDUCE_STEPS && (FULL || r * 1024 < rem); r++) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int row0 = r * 1024 + q * 4 * RL;  // the step's first row: the same for every lane
      if (FULL || row0 < rem) {
        float g[4][4], f[4][4], m[4], s[4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const bool valid = FULL || row0 + rl * 4 + p < rem;
          load_row<V>(a.dy + (ody + p * a.dys), cols, valid, g[p]);
          if (G) {
            load_row<V>(a.x + (ox + p * a.xs), cols, valid, f[p]);
            m[p] = valid ? a.mean[om + p * a.ms] : 0.0f;
            s[p] = valid ? a.rstd[ors + p * a.rs] : 0.0f;
          }
        }
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const bool valid = FULL || row0 + rl * 4 + p < rem;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            if (B) accb[q][p][j] = accb[q][p][j] + (valid ? g[p][j] : 0.0f);
            if (G) {
              const float xh = (f[p][j] - m[p]) * s[p];
              accg[q][p][j] = accg[q][p][j] + (valid && j < cols ? g[p][j] * xh : 0.0f);
            }
          }
        }
      }
      ody += 4 * RL * a.dys;
      ox += 4 * RL * a.xs;
      om += 4 * RL * a.ms;
      ors += 4 * RL * a.rs;
      asm volatile("" : "+v"(ody), "+v"(ox), "+v"(om), "+v"(ors));
    }
  }
  float v[4];
  if (G) {
    lane_fold<Q, Q>(accg, v);
    col_fold<CW>(v, red4, sumg);
  }
  if (B) {
    lane_fold<Q, Q>(accb, v);
    col_fold<CW>(v, red4, sumb);
  }
}

template <bool G, bool B, bool VEC>
__global__ void __launch_bounds__(256) ln_param_kernel(const ParamArgs a) {
  __shared__ F4 red4[256];
  __shared__ float sumg[CW], sumb[CW];
  // unit = chunk * strips + strip, walked without a 64-bit division, as dense_grad.hip walks its units: the grid is at most
  // 2048, so the first unit divides in 32 bits
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
    const long long k0 = ch * LH_LAYER_NORM_CHUNK;
    const int rem = (int)min((long long)LH_LAYER_NORM_CHUNK, a.rows - k0);  // rows of this chunk (0 only when rows == 0)
    const bool full = rem == LH_LAYER_NORM_CHUNK;
    if (VEC && c0 + CW <= a.n) {
      if (full) param_unit<G, B, true, true>(a, k0, rem, c, red4, sumg, sumb);
      else param_unit<G, B, true, false>(a, k0, rem, c, red4, sumg, sumb);
    } else {
      if (full) param_unit<G, B, false, true>(a, k0, rem, c, red4, sumg, sumb);
      else param_unit<G, B, false, false>(a, k0, rem, c, red4, sumg, sumb);
    }
    if (threadIdx.x < CW && c0 + threadIdx.x < a.n) {
      if (G) a.outg[ch * a.out_chunk_stride + (c0 + threadIdx.x) * a.outg_col_stride] = sumg[threadIdx.x];
      if (B) a.outb[ch * a.out_chunk_stride + (c0 + threadIdx.x) * a.outb_col_stride] = sumb[threadIdx.x];
    }
  }
}

template <bool VEC>
hipError_t launch_param_instance(const ParamArgs &a, unsigned grid, hipStream_t s) {
  if (a.outg && a.outb) hipLaunchKernelGGL((ln_param_kernel<true, true, VEC>), dim3(grid), dim3(256), 0, s, a);
  else if (a.outg) hipLaunchKernelGGL((ln_param_kernel<true, false, VEC>), dim3(grid), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((ln_param_kernel<false, true, VEC>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// 16-byte vectors need every operand of a call to pass this (a row stride that is never applied does not count)
bool vec_ok(const void *p, long long stride, long long rows) {
  return p == nullptr || ((uintptr_t)p % 16 == 0 && (rows <= 1 || stride % 4 == 0));
}
// gamma and beta: one row of n elements, which the vector instances read with unit stride
bool param_vec_ok(const void *p, long long stride, long long n) { return p == nullptr || ((uintptr_t)p % 16 == 0 && (n <= 1 || stride == 1)); }

}  // namespace

// the row launch of forward (PREFIX ln_fwd) or dx (ln_dx): the plan's instance of the three mappings on the plan's grid
#define LH_LN_ROWS_LAUNCH(WHAT, PREFIX)                                                         \
  if (a.rows == 0) return hipSuccess;                                                           \
  long long p[4];                                                                               \
  if (lh_layer_norm_plan(a.rows, a.n, vec ? 1 : 0, WHAT, p) != 0) return hipErrorInvalidValue;  \
  const dim3 grid((unsigned)p[1]);                                                              \
  switch ((int)p[0]) {                                                                          \
    case 0: hipLaunchKernelGGL((PREFIX##_wave_kernel<true>), grid, dim3(256), 0, s, a); break;   \
    case 1: hipLaunchKernelGGL((PREFIX##_block_kernel<true>), grid, dim3(256), 0, s, a); break;  \
    case 2: hipLaunchKernelGGL((PREFIX##_long_kernel<true>), grid, dim3(256), 0, s, a); break;   \
    case 4: hipLaunchKernelGGL((PREFIX##_wave_kernel<false>), grid, dim3(256), 0, s, a); break;  \
    case 5: hipLaunchKernelGGL((PREFIX##_block_kernel<false>), grid, dim3(256), 0, s, a); break; \
    case 6: hipLaunchKernelGGL((PREFIX##_long_kernel<false>), grid, dim3(256), 0, s, a); break;  \
    default: return hipErrorInvalidValue;                                                       \
  }                                                                                             \
  const hipError_t e = hipGetLastError();                                                       \
  if (e == hipSuccess) g_last_layer_norm_kernel[WHAT] = (int)p[0];                              \
  return e;

hipError_t launch_layer_norm_f32(float *y, int64_t ys, float *mean, int64_t ms, float *rstd, int64_t rs, const float *x, int64_t xs,
                                 const float *gamma, int64_t gs, const float *beta, int64_t bs, int64_t rows, int64_t n, float eps,
                                 hipStream_t s) {
  FwdArgs a;
  a.y = y;
  a.ys = ys;
  a.mean = mean;
  a.rstd = rstd;
  a.ms = ms;
  a.rs = rs;
  a.x = x;
  a.xs = xs;
  a.gamma = gamma;
  a.beta = beta;
  a.gs = gs;
  a.bs = bs;
  a.rows = rows;
  a.n = n;
  a.eps = eps;
  const bool vec = vec_ok(y, ys, rows) && vec_ok(x, xs, rows) && param_vec_ok(gamma, gs, n) && param_vec_ok(beta, bs, n);
  LH_LN_ROWS_LAUNCH(LH_LAYER_NORM_FORWARD, ln_fwd)
}

hipError_t launch_layer_norm_dx_f32(float *dx, int64_t dxs, const float *dy, int64_t dys, const float *x, int64_t xs, const float *mean,
                                    int64_t ms, const float *rstd, int64_t rs, const float *gamma, int64_t gs, int64_t rows, int64_t n,
                                    hipStream_t s) {
  DxArgs a;
  a.dx = dx;
  a.dxs = dxs;
  a.dy = dy;
  a.x = x;
  a.dys = dys;
  a.xs = xs;
  a.mean = mean;
  a.rstd = rstd;
  a.ms = ms;
  a.rs = rs;
  a.gamma = gamma;
  a.gs = gs;
  a.rows = rows;
  a.n = n;
  const bool vec = vec_ok(dx, dxs, rows) && vec_ok(dy, dys, rows) && vec_ok(x, xs, rows) && param_vec_ok(gamma, gs, n);
  LH_LN_ROWS_LAUNCH(LH_LAYER_NORM_DX, ln_dx)
}
#undef LH_LN_ROWS_LAUNCH

hipError_t launch_layer_norm_param_grads_f32(float *dgamma, int64_t dgs, float *dbeta, int64_t dbs, const float *dy, int64_t dys,
                                             const float *x, int64_t xs, const float *mean, int64_t ms, const float *rstd, int64_t rs,
                                             int64_t rows, int64_t n, hipStream_t s) {
  if (!dgamma && !dbeta) return hipSuccess;
  const bool vec = vec_ok(dy, dys, rows) && (!dgamma || vec_ok(x, xs, rows));
  long long plan[4];
  if (lh_layer_norm_plan(rows, n, vec, LH_LAYER_NORM_PARAMS, plan) != 0) return hipErrorInvalidValue;
  const long long chunks = rows == 0 ? 1 : (rows + LH_LAYER_NORM_CHUNK - 1) / LH_LAYER_NORM_CHUNK;
  ParamArgs a;
  a.dy = dy;
  a.x = x;
  a.mean = mean;
  a.rstd = rstd;
  a.dys = dys;
  a.xs = xs;
  a.ms = ms;
  a.rs = rs;
  a.rows = rows;
  a.n = n;
  a.strips = (n + CW - 1) / CW;
  a.chunks = chunks;
  a.step_chunks = plan[1] / a.strips;
  a.step_strips = plan[1] % a.strips;
  float *part = nullptr;
  if (chunks > 1) {  // one (chunks, n) matrix of partials for every sum asked for
    const size_t each = (size_t)chunks * (size_t)n;
    const hipError_t e = scratch_alloc_async((void **)&part, each * sizeof(float) * ((dgamma ? 1 : 0) + (dbeta ? 1 : 0)), s);
    if (e != hipSuccess) return e;
    a.outg = dgamma ? part : nullptr;
    a.outb = dbeta ? part + (dgamma ? each : 0) : nullptr;
    a.out_chunk_stride = n;
    a.outg_col_stride = a.outb_col_stride = 1;
  } else {
    a.outg = dgamma;
    a.outb = dbeta;
    a.out_chunk_stride = 0;
    a.outg_col_stride = dgs;
    a.outb_col_stride = dbs;
  }
  hipError_t e = vec ? launch_param_instance<true>(a, (unsigned)plan[1], s) : launch_param_instance<false>(a, (unsigned)plan[1], s);
  if (part != nullptr) {
    // the chunk partials of a column are one more array under the same rule, rows = chunks <= 8192: the bias gradient's
    // launch folds them (its "last kernel" record stays the last bias_grad call's)
    const int keep = g_last_bias_grad_kernel;
    if (e == hipSuccess && dgamma) e = launch_bias_grad_f32(dgamma, dgs, nullptr, 0, a.outg, n, nullptr, 0, chunks, n, LASER_HIP_ACT_NONE, s);
    if (e == hipSuccess && dbeta) e = launch_bias_grad_f32(dbeta, dbs, nullptr, 0, a.outb, n, nullptr, 0, chunks, n, LASER_HIP_ACT_NONE, s);
    g_last_bias_grad_kernel = keep;
    const hipError_t f = scratch_free_async(part, s);
    if (e == hipSuccess) e = f;
  }
  if (e == hipSuccess) g_last_layer_norm_kernel[LH_LAYER_NORM_PARAMS] = (int)plan[0];
  return e;
}

}  // namespace laser_hip
