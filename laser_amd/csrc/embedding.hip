// laser_amd/csrc/embedding.hip -- the embedding layer (include/laser_hip.h, "Embedding"): the row gather Y[t, :] = W[idx[t], :],
// the stable grouping of the token positions by id, and dW[v, j] = the sum of dY[t, j] over the tokens of id v, in token
// order, in reduce_core.h's order for a 1-D array (E = 4, init +0).  embedding_plan.h has the passes, the tiles and the launches.
//
// Gather.  A workgroup of 256 lanes owns 256 / LPR rows at a time, LPR = the lanes that span a row (a power of two, at most
// 256); a lane loads its row's id once and walks the row in steps of LPR 16-byte quads.  The bits travel as uint32.
//
// Grouping.  key(t) = idx[t] inside [0, vocab), else vocab.  One pass per 8-bit digit of the largest key, least significant
// first, each a stable counting sort of the current order: (1) every wave counts the digits of its tile of consecutive sort
// positions (LDS integer adds: a count does not depend on arrival order) and writes row `digit` of the (digit, tile) table;
// (2) the row cumsum of scan.hip turns the table, read as one row, into inclusive prefix sums -- integer sums, exact in
// any order; (3) the wave walks its tile again, 64 positions a step: a lane's slot is (prefix - count) of its (digit, tile)
// + the elements of that digit the wave has passed (a per-digit LDS counter, advanced by one lane per digit and step) +
// the lanes below it with the same digit (ballots over the digit's 8 bits).  Every term is a count of elements that precede
// in the current order, so the pass is stable and its output unique.  Keys are not stored: a pass reads idx through the
// order of the pass before (the first through the identity).  starts[v] is the lower-bound descent of scan_core.h for v
// over the sorted keys.  Nothing claims a slot atomically, no workgroup waits on another.
//
// Sums.  The tree of a segment of c occurrences: occurrence k goes to chunk k / 8192 and leaf a = k mod 1024 of it; a leaf
// starts at +0 and takes its elements in ascending k; the 1024 leaves fold over the bits of a in the order 1, 0, 9, 8, .., 2;
// chunk partials fold as one more such array.  A leaf is +0 + x, and a sum with a +0 term is never -0, so adding a +0
// partner (an empty leaf) is exact: the tree restricted to the occupied leaves has the same bits.
//   short_kernel, c <= 32 (and c = 0): a lane owns (id, 4 columns).  Leaves 0 .. 31 are 8 groups of 4; a group folds as
//     (l0 + l2) + (l1 + l3) (bits 1, 0), and the groups by halving, ((u0 + u4) + (u2 + u6)) + ((u1 + u5) + (u3 + u7)) (bits
//     4, 3, 2; the folds over bits 9 .. 5 add +0).  Lanes of one id read one run of a gathered row, 16 bytes each.
//   long_kernel, c > 32: a workgroup owns (4096 sorted positions, strip of 16 columns).  Its lanes find the long segments
//     that start in those positions (position p starts id v iff starts[v] == p) by ballots, and take them in position order.
//     A chunk is dense_grad.hip's unit with the rows gathered through `order`; the partial of chunk m goes to leaf m mod 1024
//     of an LDS array, which the same workgroup folds by the same rule.  A segment of one chunk writes its partial.
// Every id is written by exactly one of the two kernels; nothing is atomic; a lane's columns never mix with another's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "embedding_plan.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

static_assert(LH_EMBEDDING_CHUNK == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of occurrences is a chunk of the order");
static_assert(LH_EMBEDDING_MAX_TOKENS == LASER_HIP_EMBEDDING_MAX_TOKENS && LH_EMBEDDING_MAX_VOCAB == LASER_HIP_EMBEDDING_MAX_VOCAB,
              "plan and header agree");
static_assert(LH_EMBEDDING_MAX_TOKENS / LH_EMBEDDING_CHUNK <= LH_EMBEDDING_CHUNK, "the chunk partials of an id fit one chunk");
static_assert(LH_EMBEDDING_DIGIT_BITS == 8 && LH_EMBEDDING_SHORT == 32 && LH_EMBEDDING_CW == 16 && LH_EMBEDDING_PTILE == 16 * 256,
              "the kernels' lane mappings and the plan agree");
static_assert(LH_EMBEDDING_MAX_TILES * 256 <= LASER_HIP_SCAN_MAX_N, "the (digit, tile) table is one row of the cumsum");

namespace laser_hip {

std::atomic<int> g_last_embedding_kernel[4] = {{-1}, {-1}, {-1}, {-1}};

namespace {

constexpr int CW = LH_EMBEDDING_CW, LPR = CW / 4, RL = 256 / LPR, Q = 1024 / (4 * RL);
constexpr int kGridX = 65536, kGridY = 65535;

__device__ __forceinline__ int key_of(const int id, const int vocab) { return (unsigned)id < (unsigned)vocab ? id : vocab; }

// 4 adjacent columns from column c of a row of `dim`; a row that does not exist (`valid` false) is not read and loads as +0
template <bool VEC>
__device__ __forceinline__ void load_quad(const float *row, const long long c, const long long dim, const bool valid, float (&q)[4]) {
  if (VEC && c + 4 <= dim) {
    F4 f = {{0.0f, 0.0f, 0.0f, 0.0f}};
    if (valid) f = *(const F4 *)(row + c);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = f.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = valid && c + j < dim ? row[c + j] : 0.0f;
  }
}

// ---- the gather ---------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) embedding_kernel(unsigned int *y, const long long ys, const unsigned int *w, const long long ws,
                                                        const int *idx, const long long tokens, const int vocab, const long long dim,
                                                        const int lpr_log2) {
  const int lpr = 1 << lpr_log2, ipw = 256 >> lpr_log2;
  const int rl = threadIdx.x >> lpr_log2, ql = threadIdx.x & (lpr - 1);
  const long long quads = (dim + 3) >> 2;
  for (long long g = blockIdx.x; g * ipw < tokens; g += gridDim.x) {
    const long long t = g * ipw + rl;
    if (t >= tokens) continue;
    const int id = idx[t];  // once per row
    const bool ok = (unsigned)id < (unsigned)vocab;
    const unsigned int fill = id == -1 ? 0u : 0x7fc00000u;
    const unsigned int *src = w + (ok ? (long long)id : 0ll) * ws;
    unsigned int *dst = y + t * ys;
    for (long long q = ql; q < quads; q += lpr) {
      const long long c = q * 4;
      if (VEC && c + 4 <= dim) {
        U4 v = {{fill, fill, fill, fill}};
        if (ok) v = *(const U4 *)(src + c);
        *(U4 *)(dst + c) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (c + j < dim) dst[c + j] = ok ? src[c + j] : fill;
      }
    }
  }
}

// ---- the grouping -------------------------------------------------------------------------------------------------------------
// order_in null: the identity.  Wave `wv` of workgroup b owns tile 4 b + wv: sort positions [tile * tl, tile * (tl + 1))
__global__ void __launch_bounds__(256) embedding_hist_kernel(int *hist, const int *order_in, const int *idx, const int tokens,
                                                             const int vocab, const int shift, const int tile, const int tiles) {
  __shared__ int cnt[4][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = lane; i < 256; i += 64) cnt[wv][i] = 0;
  __syncthreads();
  const int tl = blockIdx.x * 4 + wv;
  if (tl < tiles) {
    const int end = min(tokens, (tl + 1) * tile);
    for (int i = tl * tile + lane; i < end; i += 64) {
      const int t = order_in ? order_in[i] : i;
      int d = 0;
      if ((unsigned)t < (unsigned)tokens) d = (key_of(idx[t], vocab) >> shift) & 255;
      atomicAdd(&cnt[wv][d], 1);  // an integer count: the same whatever the arrival order
    }
  }
  __syncthreads();
  if (tl < tiles)
    for (int i = lane; i < 256; i += 64) hist[i * tiles + tl] = cnt[wv][i];
}

// `scan` is the inclusive prefix sum of `hist` read as one row of 256 * tiles counters
__global__ void __launch_bounds__(256) embedding_scatter_kernel(int *order_out, const int *order_in, const int *idx, const int *hist,
                                                                const int *scan, const int tokens, const int vocab, const int shift,
                                                                const int tile, const int tiles) {
  __shared__ int base[4][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int tl = blockIdx.x * 4 + wv;
  if (tl < tiles)
    for (int i = lane; i < 256; i += 64) base[wv][i] = scan[i * tiles + tl] - hist[i * tiles + tl];
  __syncthreads();
  // (every wave walks all the steps, so that the workgroup's barriers are met by all: a wave past the end has no valid lane)
  for (int st = 0; st < tile; st += 64) {
    const int i = tl * tile + st + lane;
    int t = 0, d = 0;
    bool valid = tl < tiles && i < tokens;
    if (valid) {
      t = order_in ? order_in[i] : i;
      valid = (unsigned)t < (unsigned)tokens;
      if (valid) d = (key_of(idx[t], vocab) >> shift) & 255;
    }
    unsigned long long same = __ballot(valid);  // the valid lanes of this wave with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1;
      const unsigned long long bb = __ballot(bit);
      same &= bit ? bb : ~bb;
    }
    const int below = __popcll(same & ((1ull << lane) - 1ull));
    int pos = -1;
    if (valid) pos = base[wv][d] + below;
    __syncthreads();
    if (valid && below == 0) base[wv][d] += __popcll(same);  // one lane per digit: the lowest
    __syncthreads();
    if ((unsigned)pos < (unsigned)tokens) order_out[pos] = t;
  }
}

// starts[v], v = 0 .. vocab: the first sorted position whose key is >= v (scan_core.h's left-side descent)
__global__ void __launch_bounds__(256) embedding_starts_kernel(int *starts, const int *order, const int *idx, const int tokens,
                                                               const int vocab) {
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v <= vocab; v += (long long)gridDim.x * 256) {
    int lo = 0, count = tokens;
    while (count > 0) {
      const int step = count / 2, pos = lo + step;
      const int t = order[pos];
      const int k = (unsigned)t < (unsigned)tokens ? key_of(idx[t], vocab) : vocab;
      if (k < (int)v) {
        lo = pos + 1;
        count -= step + 1;
      } else {
        count = step;
      }
    }
    starts[v] = lo;
  }
}

// ---- the sums -----------------------------------------------------------------------------------------------------------------
struct GradArgs {
  float *dw;
  const float *dy;
  const int *idx, *order, *starts;
  long long dws, dys, dim;
  int tokens, vocab, lpr_log2;
};

template <bool VEC>
__global__ void __launch_bounds__(256) embedding_short_kernel(const GradArgs a) {
  const int lpr = 1 << a.lpr_log2, ipw = 256 >> a.lpr_log2;
  const int rl = threadIdx.x >> a.lpr_log2, ql = threadIdx.x & (lpr - 1);
  const long long quads = (a.dim + 3) >> 2;
  for (long long g = blockIdx.x; g * ipw < a.vocab; g += gridDim.x) {
    const long long v = g * ipw + rl;
    if (v >= a.vocab) continue;
    const int s = a.starts[v], c = a.starts[v + 1] - s;
    if (c > LH_EMBEDDING_SHORT) continue;  // the long-segment kernel's
    for (long long q = (long long)blockIdx.y * lpr + ql; q < quads; q += (long long)gridDim.y * lpr) {
      const long long col = q * 4;
      float u[8][4];
#pragma unroll
      for (int gr = 0; gr < 8; gr++) {
#pragma unroll
        for (int j = 0; j < 4; j++) u[gr][j] = 0.0f;
        if (gr * 4 < c) {
          float x[4][4];
#pragma unroll
          for (int p = 0; p < 4; p++) {
            bool valid = gr * 4 + p < c;
            int t = 0;
            if (valid) {
              t = a.order[s + gr * 4 + p];
              valid = (unsigned)t < (unsigned)a.tokens;
            }
            load_quad<VEC>(a.dy + (long long)t * a.dys, col, a.dim, valid, x[p]);
          }
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const float l0 = 0.0f + x[0][j], l1 = 0.0f + x[1][j], l2 = 0.0f + x[2][j], l3 = 0.0f + x[3][j];
            u[gr][j] = (l0 + l2) + (l1 + l3);
          }
        }
      }
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; j++) r[j] = ((u[0][j] + u[4][j]) + (u[2][j] + u[6][j])) + ((u[1][j] + u[5][j]) + (u[3][j] + u[7][j]));
      float *out = a.dw + v * a.dws;
      if (VEC && col + 4 <= a.dim) {
        F4 f;
#pragma unroll
        for (int j = 0; j < 4; j++) f.v[j] = r[j];
        *(F4 *)(out + col) = f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (col + j < a.dim) out[col + j] = r[j];
      }
    }
  }
}

// One chunk of a segment: occurrences pos0 .. pos0 + rem of the sorted order, the lane's 4 columns from column c; the 16
// column sums of the strip go to sums[] (dense_grad.hip's grad_unit with the rows gathered)
template <bool V>
__device__ __forceinline__ void chunk_unit(const GradArgs &a, const int pos0, const int rem, const long long c, F4 *red4, float *sums) {
  const int rl = threadIdx.x / LPR;
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
  for (int r = 0; r < LH_REDUCE_STEPS && r * 1024 < rem; r++) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      const int row0 = r * 1024 + q * 4 * RL;  // the step's first occurrence: the same for every lane
      if (row0 < rem) {
        float g[4][4];
#pragma unroll
        for (int p = 0; p < 4; p++) {
          const int k = row0 + rl * 4 + p;
          bool valid = k < rem;
          int t = 0;
          if (valid) {
            t = a.order[pos0 + k];
            valid = (unsigned)t < (unsigned)a.tokens;
          }
          load_quad<V>(a.dy + (long long)t * a.dys, c, a.dim, valid, g[p]);
        }
#pragma unroll
        for (int p = 0; p < 4; p++) {
#pragma unroll
          for (int j = 0; j < 4; j++) acc[q][p][j] = acc[q][p][j] + g[p][j];
        }
      }
    }
  }
  float v[4];
  lane_fold<Q, Q>(acc, v);
  col_fold<CW>(v, red4, sums);
}

template <bool VEC>
__global__ void __launch_bounds__(256) embedding_long_kernel(const GradArgs a) {
  __shared__ F4 red4[256];
  __shared__ float sums[CW];
  __shared__ unsigned long long masks[LH_EMBEDDING_PTILE / 64];
  __shared__ float leaves[1024 * CW];
  const int nvalid = min(a.starts[a.vocab], a.tokens);
  const int tile0 = blockIdx.x * LH_EMBEDDING_PTILE;
  if (tile0 >= nvalid) return;  // (the same for every lane)
  // which of this tile's positions start a long segment: position p starts id v iff starts[v] == p
  for (int j = 0; j < LH_EMBEDDING_PTILE / 256; j++) {
    const int p = tile0 + j * 256 + threadIdx.x;
    bool flag = false;
    if (p < nvalid) {
      const int t = a.order[p];
      if ((unsigned)t < (unsigned)a.tokens) {
        const int v = a.idx[t];
        if ((unsigned)v < (unsigned)a.vocab) flag = a.starts[v] == p && a.starts[v + 1] - p > LH_EMBEDDING_SHORT;
      }
    }
    const unsigned long long m = __ballot(flag);
    if ((threadIdx.x & 63) == 0) masks[j * 4 + (threadIdx.x >> 6)] = m;
  }
  __syncthreads();
  const long long strips = (a.dim + CW - 1) / CW;
  for (int mi = 0; mi < LH_EMBEDDING_PTILE / 64; mi++) {
    unsigned long long mask = masks[mi];  // (the same for every lane: the loops below are uniform)
    while (mask != 0) {
      const int p = tile0 + mi * 64 + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int v = a.idx[a.order[p]];
      const int c = min(a.starts[v + 1], nvalid) - p;
      const int chunks = (c + LH_EMBEDDING_CHUNK - 1) / LH_EMBEDDING_CHUNK;
      const int nleaves = min(chunks, 1024);
      for (long long strip = blockIdx.y; strip < strips; strip += gridDim.y) {
        const long long c0 = strip * CW;
        const long long col = c0 + (threadIdx.x % LPR) * 4;
        const bool vec = VEC && c0 + CW <= a.dim;
        if (chunks > 1) {
          __syncthreads();  // the last readers of leaves are done
          for (int i = threadIdx.x; i < nleaves * CW; i += 256) leaves[i] = 0.0f;
        }
        for (int m = 0; m < chunks; m++) {
          const int rem = min(LH_EMBEDDING_CHUNK, c - m * LH_EMBEDDING_CHUNK);
          if (vec) chunk_unit<true>(a, p + m * LH_EMBEDDING_CHUNK, rem, col, red4, sums);
          else chunk_unit<false>(a, p + m * LH_EMBEDDING_CHUNK, rem, col, red4, sums);
          // (col_fold begins and ends with a barrier: sums and the zeroed leaves are visible, and the next unit waits)
          if (threadIdx.x < CW) {
            if (chunks > 1) leaves[(m & 1023) * CW + threadIdx.x] = leaves[(m & 1023) * CW + threadIdx.x] + sums[threadIdx.x];
            else if (c0 + threadIdx.x < a.dim) a.dw[(long long)v * a.dws + c0 + threadIdx.x] = sums[threadIdx.x];
          }
        }
        if (chunks > 1) {
          // the chunk partials are one more array under the same rule: leaf a = q * 256 + 4 rl + p of the lane's 4 columns
          __syncthreads();
          const int rl = threadIdx.x / LPR, l = threadIdx.x % LPR;
          float acc[Q][4][4];
#pragma unroll
          for (int q = 0; q < Q; q++) {
#pragma unroll
            for (int pp = 0; pp < 4; pp++) {
              const int leaf = q * 4 * RL + rl * 4 + pp;
#pragma unroll
              for (int j = 0; j < 4; j++) acc[q][pp][j] = leaf < nleaves ? leaves[leaf * CW + l * 4 + j] : 0.0f;
            }
          }
          float f[4];
          lane_fold<Q, Q>(acc, f);
          col_fold<CW>(f, red4, sums);
          if (threadIdx.x < CW && c0 + threadIdx.x < a.dim) a.dw[(long long)v * a.dws + c0 + threadIdx.x] = sums[threadIdx.x];
        }
      }
    }
  }
}

bool vec_ok(const void *p, long long stride, long long rows) {
  // (a row stride that is never applied -- at most one row -- does not count)
  return p == nullptr || ((uintptr_t)p % 16 == 0 && (rows <= 1 || stride % 4 == 0));
}

// the lanes that span a row of `dim`: the power of two at or above its quads, at most 256
int lanes_per_row_log2(long long dim) {
  const long long quads = (dim + 3) / 4;
  int l = 0;
  while (l < 8 && (1ll << l) < quads) l++;
  return l;
}

unsigned grid_for(long long units, int cap) { return (unsigned)std::max<long long>(1, std::min<long long>(units, cap)); }

}  // namespace

hipError_t launch_embedding_f32(float *y, int64_t ys, const float *w, int64_t ws, const int32_t *idx, int64_t tokens, int64_t vocab,
                                int64_t dim, hipStream_t s) {
  if (tokens == 0 || dim == 0) return hipSuccess;
  const bool vec = vec_ok(y, ys, tokens) && vec_ok(w, ws, vocab);
  const int l = lanes_per_row_log2(dim);
  const long long groups = (tokens + (256 >> l) - 1) / (256 >> l);
  if (vec)
    hipLaunchKernelGGL(embedding_kernel<true>, dim3(grid_for(groups, kGridX)), dim3(256), 0, s, (unsigned int *)y, (long long)ys,
                       (const unsigned int *)w, (long long)ws, idx, (long long)tokens, (int)vocab, (long long)dim, l);
  else
    hipLaunchKernelGGL(embedding_kernel<false>, dim3(grid_for(groups, kGridX)), dim3(256), 0, s, (unsigned int *)y, (long long)ys,
                       (const unsigned int *)w, (long long)ws, idx, (long long)tokens, (int)vocab, (long long)dim, l);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_embedding_kernel[0] = vec ? 0 : 1;
  return e;
}

hipError_t launch_embedding_group_i32(int32_t *order, int32_t *starts, const int32_t *idx, int64_t tokens, int64_t vocab, hipStream_t s) {
  long long plan[8];
  if (lh_embedding_plan(tokens, vocab, 0, 0, 0, plan) != 0) return hipErrorInvalidValue;
  const int passes = (int)plan[0], tile = (int)plan[1];
  const int tiles = (int)((tokens + tile - 1) / tile);
  char *scratch = nullptr;
  hipError_t e = hipSuccess;
  if (tokens > 0) {
    e = scratch_alloc_async((void **)&scratch, (size_t)plan[6], s);
    if (e != hipSuccess) return e;
    int *hist = (int *)scratch, *scan = hist + 256ll * tiles, *tmp = scan + 256ll * tiles;
    // the last pass writes `order`: the buffers alternate backwards from it
    const int *src = nullptr;
    for (int p = 0; p < passes && e == hipSuccess; p++) {
      int *dst = (passes - 1 - p) % 2 == 0 ? order : tmp;
      const int shift = p * LH_EMBEDDING_DIGIT_BITS;
      hipLaunchKernelGGL(embedding_hist_kernel, dim3((unsigned)plan[2]), dim3(256), 0, s, hist, src, idx, (int)tokens, (int)vocab, shift,
                         tile, tiles);
      e = hipGetLastError();
      if (e == hipSuccess) e = launch_cumsum_i32(scan, 256ll * tiles, hist, 256ll * tiles, 1, 256ll * tiles, s);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(embedding_scatter_kernel, dim3((unsigned)plan[2]), dim3(256), 0, s, dst, src, idx, hist, scan, (int)tokens,
                           (int)vocab, shift, tile, tiles);
        e = hipGetLastError();
      }
      src = dst;
    }
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(embedding_starts_kernel, dim3(grid_for((vocab + 256) / 256, kGridX)), dim3(256), 0, s, starts, order, idx,
                       (int)tokens, (int)vocab);
    e = hipGetLastError();
  }
  if (scratch != nullptr) {
    const hipError_t f = scratch_free_async(scratch, s);
    if (e == hipSuccess) e = f;
  }
  if (e == hipSuccess) {
    g_last_embedding_kernel[1] = tokens == 0 ? 0 : passes;
    g_last_embedding_kernel[3] = tokens == 0 ? 0 : (int)plan[2];
  }
  return e;
}

hipError_t launch_embedding_grad_f32(float *dw, int64_t dws, const float *dy, int64_t dys, const int32_t *idx, const int32_t *order,
                                     const int32_t *starts, int64_t tokens, int64_t vocab, int64_t dim, hipStream_t s) {
  if (vocab == 0 || dim == 0) return hipSuccess;
  int *own = nullptr;
  hipError_t e = hipSuccess;
  if (order == nullptr) {
    e = scratch_alloc_async((void **)&own, (size_t)(tokens + vocab + 1) * sizeof(int), s);
    if (e != hipSuccess) return e;
    e = launch_embedding_group_i32(own + vocab + 1, own, idx, tokens, vocab, s);
    order = own + vocab + 1;
    starts = own;
  }
  const bool vec = vec_ok(dw, dws, vocab) && vec_ok(dy, dys, tokens);
  if (e == hipSuccess) {
    GradArgs a;
    a.dw = dw;
    a.dy = dy;
    a.idx = idx;
    a.order = order;
    a.starts = starts;
    a.dws = dws;
    a.dys = dys;
    a.dim = dim;
    a.tokens = (int)tokens;
    a.vocab = (int)vocab;
    a.lpr_log2 = lanes_per_row_log2(dim);
    const int lpr = 1 << a.lpr_log2;
    const long long groups = (vocab + (256 / lpr) - 1) / (256 / lpr), quads = (dim + 3) / 4;
    const dim3 gs(grid_for(groups, kGridX), grid_for((quads + lpr - 1) / lpr, kGridY));
    if (vec) hipLaunchKernelGGL(embedding_short_kernel<true>, gs, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(embedding_short_kernel<false>, gs, dim3(256), 0, s, a);
    e = hipGetLastError();
    if (e == hipSuccess) {
      const dim3 gl(grid_for((tokens + LH_EMBEDDING_PTILE - 1) / LH_EMBEDDING_PTILE, kGridX), grid_for((dim + CW - 1) / CW, kGridY));
      if (vec) hipLaunchKernelGGL(embedding_long_kernel<true>, gl, dim3(256), 0, s, a);
      else hipLaunchKernelGGL(embedding_long_kernel<false>, gl, dim3(256), 0, s, a);
      e = hipGetLastError();
    }
  }
  if (own != nullptr) {
    const hipError_t f = scratch_free_async(own, s);
    if (e == hipSuccess) e = f;
  }
  if (e == hipSuccess) g_last_embedding_kernel[2] = vec ? 0 : 1;
  return e;
}

}  // namespace laser_hip
