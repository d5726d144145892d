// laser_amd/csrc/select.hip -- row selection (include/laser_hip_select.h "Row top-k, argmax and top-k sampling"): for every row
// of a float32 matrix the k first elements in the key order with their columns, the first element alone, and the row gather
// that maps a draw among k candidates back to a column.  Only integers are compared:
//
//   key(x)     = bits ^ 0xFFFFFFFF when the sign bit is set, bits ^ 0x80000000 otherwise; complemented on load for largest = 0
//   composite  = key << 32 | (0xFFFFFFFF - column): unique within a row; descending composites = descending key, then
//                ascending column.  A composite is never 0, so 0 pads a sort network to its power of two.
//
// The top-k kernels have the three lane mappings of the other row kernels, chosen by n alone (select_plan.h), each with a
// 16-byte-vector instance and a single-element one: same values, same order.
//   topk_wave_kernel       n <= 256: one wave per row, four rows per workgroup.  A row this short is cheaper to sort whole than
//                          to select from: its composites go through the bitonic network on the next power of two >= n.
//   topk_resident_kernel   n <= 8192: one workgroup per row, 32 keys per lane loaded once; all passes run from registers.
//   topk_streaming_kernel  longer rows: one workgroup re-reads the row for each pass; five reads of the row in all.
// The selection of the two workgroup kernels: four passes over 8-bit digits, most significant first.  A pass counts the keys
// that still match the digits found so far into 256 integer bins in LDS (counts are integers: the arrival order of the adds
// cannot show) and scans the bins from the top to the digit at which the running count reaches what is still needed.  After
// the last pass the threshold key T is known, and `need`, the number of elements equal to T that are taken; the g = k - need
// keys above T are all taken.  The collection pass walks the row in column order: keys above T take the next free slot of
// [0, g) (an LDS counter: their slots are arbitrary, the sort below fixes the order), keys equal to T get their rank among the
// row's equals from a prefix count (inside the lane, across the wave by shuffles, across the waves and the earlier chunks by
// LDS), and the ranks below `need` go to slot g + rank: the tie pick is positional.  The k composites are then sorted by the
// bitonic network on the next power of two >= k and written out: column = 0xFFFFFFFF - low word, value bits from the key.
//
// argmax is one pass: the maximum of the composites (wave butterflies, then one LDS step across the four waves).
// No floating-point operation, no floating-point atomic, nothing waits on another workgroup; every access is bounded by
// rows, n and k.
#include <hip/hip_runtime.h>

#include "../../include/laser_hip.h"
#include "../../include/laser_hip_select.h"
#include "common.h"
#include "select_plan.h"
#include "softmax_common.h"

static_assert(LH_SELECT_MAX_WORKGROUPS == LH_SOFTMAX_MAX_WORKGROUPS, "one cap for every row kernel");
static_assert(LH_SELECT_MAX_N == LASER_HIP_SELECT_MAX_N && LH_SELECT_MAX_ROWS == LASER_HIP_SELECT_MAX_ROWS &&
                  LH_SELECT_MAX_K == LASER_HIP_SELECT_MAX_K,
              "plan and header agree");
static_assert(LH_SELECT_WAVE_N == 64 * 4 && LH_SELECT_RESIDENT_N == 256 * 8 * 4 && LH_SELECT_COLLECT_CHUNK == 256 * 4 * 4,
              "the lane mappings");

namespace laser_hip {

std::atomic<int> g_last_topk_kernel{-1};

namespace {

typedef unsigned long long u64;

struct TopkArgs {
  unsigned *vals;  // bit copies; may be null
  long long vs;
  int *idx;  // may be null
  long long is;
  const unsigned *x;
  long long xs;
  long long rows;
  int n, k;
  unsigned flip;  // 0: largest first; 0xFFFFFFFF: smallest first (the key complemented)
};

struct ArgmaxArgs {
  int *idx;
  long long is;
  unsigned *val;  // may be null
  long long vs;
  const unsigned *x;
  long long xs;
  long long rows;
  int n;
  unsigned flip;
};

__device__ __forceinline__ unsigned key_of(const unsigned b, const unsigned flip) {
  return (b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u)) ^ flip;
}
__device__ __forceinline__ unsigned bits_of(unsigned key, const unsigned flip) {
  key ^= flip;
  return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu);
}
__device__ __forceinline__ u64 composite(const unsigned key, const int col) { return ((u64)key << 32) | (0xFFFFFFFFu - (unsigned)col); }
__device__ __forceinline__ int col_of(const u64 c) { return (int)(0xFFFFFFFFu - (unsigned)c); }

// the bits of elements base .. base + 3 of a row of n; 0 where the row has ended (the callers never count those)
template <bool VEC>
__device__ __forceinline__ void load4u(const unsigned *x, const int base, const int n, unsigned (&q)[4]) {
  if (VEC && base + 4 <= n) {
    const U4 f = *(const U4 *)(x + base);
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = f.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = base + j < n ? x[base + j] : 0u;
  }
}

// buf[0 .. P) sorted descending by the bitonic network, P a power of two, by the G lanes of a group (`lane` in [0, G)); every
// lane of the workgroup calls it (the barriers), a group that is not `active` touches nothing.  Ends with a barrier.
template <int G>
__device__ __forceinline__ void sort_desc(u64 *buf, const int P, const int lane, const bool active) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      if (active) {
        for (int i = lane; i < P / 2; i += G) {
          const int pos = 2 * i - (i & (stride - 1));
          const u64 a = buf[pos], b = buf[pos + stride];
          if ((a < b) == ((pos & size) == 0)) {
            buf[pos] = b;
            buf[pos + stride] = a;
          }
        }
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ void store_result(const TopkArgs &a, const long long row, const int i, const u64 c) {
  if (a.vals) a.vals[row * a.vs + i] = bits_of((unsigned)(c >> 32), a.flip);
  if (a.idx) a.idx[row * a.is + i] = col_of(c);
}

// ---- n <= 256: a wave sorts its row ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) topk_wave_kernel(const TopkArgs a) {
  __shared__ u64 sbuf[4][LH_SELECT_WAVE_N];
  static_assert(sizeof(sbuf) == LH_SELECT_LDS_WAVE, "plan and kernel agree");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 *buf = sbuf[w];
  int P = 1;
  while (P < a.n) P <<= 1;
  // the trip count is the workgroup's (barriers inside): a wave past the last row idles through its trip
  for (long long row0 = (long long)blockIdx.x * 4; row0 < a.rows; row0 += (long long)gridDim.x * 4) {
    const long long row = row0 + w;
    const bool active = row < a.rows;
    if (active) {
      unsigned q[4];
      load4u<VEC>(a.x + row * a.xs, lane * 4, a.n, q);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int i = lane * 4 + j;
        if (i < P) buf[i] = i < a.n ? composite(key_of(q[j], a.flip), i) : 0ull;
      }
    }
    sort_desc<64>(buf, P, lane, active);
    if (active) {
      for (int i = lane; i < a.k; i += 64) store_result(a, row, i, buf[i]);
    }
    __syncthreads();  // the results are read before the next row is written
  }
}

// ---- the workgroup kernels --------------------------------------------------------------------------------------------------------
struct BlockLds {
  u64 buf[LH_SELECT_MAX_K];
  unsigned hist[256];
  unsigned wtot[2][8][4];  // [parity of the chunk][step][wave]: the wave's count of elements equal to the threshold
  unsigned sel[4];         // {digit, still needed inside it, slots taken by keys above the threshold, -}
};
static_assert(sizeof(BlockLds) == LH_SELECT_LDS_BLOCK, "plan and kernel agree");

// one more candidate key with this digit.  Every lane of the wave calls it (the ballots).  Float keys crowd into few top
// digits, and 64 adds to one bin serialise: up to two rounds in which the lanes that share the first candidate's digit add
// once, together; what is left adds lane by lane.  The bins end with the same integers either way.
__device__ __forceinline__ void hist_add(unsigned *hist, bool cand, const unsigned digit) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int round = 0; round < 2; round++) {
    const u64 live = __ballot(cand);
    if (live != 0) {
      const int first = __ffsll((long long)live) - 1;
      const unsigned d0 = __shfl(digit, first);
      const bool same = cand && digit == d0;
      const u64 m = __ballot(same);
      if (lane == first) atomicAdd(&hist[d0], (unsigned)__popcll(m));
      cand = cand && !same;
    }
  }
  if (cand) atomicAdd(&hist[digit], 1u);
}

// the bins are complete (a barrier since the last add): the digit at which the count from the top bin reaches `need`, and what
// is still needed inside that bin.  The bins hold at least `need` keys.  Ends with a barrier.
__device__ __forceinline__ void pick_digit(BlockLds &s, const unsigned need, unsigned &digit, unsigned &rem) {
  const int t = threadIdx.x;
  if (t < 64) {  // lane t: bins 4 t .. 4 t + 3
    unsigned c[4];
#pragma unroll
    for (int b = 0; b < 4; b++) c[b] = s.hist[4 * t + b];
    const unsigned own = (c[0] + c[1]) + (c[2] + c[3]);
    unsigned incl = own;  // own bins and every bin above them
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) {
      const unsigned v = __shfl_down(incl, h);
      if (t + h < 64) incl += v;
    }
    unsigned above = incl - own;
    if (above < need && need <= incl) {  // exactly one lane
      bool done = false;
#pragma unroll
      for (int b = 3; b >= 0; b--) {
        if (!done && above + c[b] >= need) {
          s.sel[0] = 4 * t + b;
          s.sel[1] = need - above;
          done = true;
        }
        if (!done) above += c[b];
      }
    }
  }
  __syncthreads();
  digit = s.sel[0];
  rem = s.sel[1];
}

// the collection of R steps of 1024 elements from column cbase: lane t holds columns cbase + 1024 r + 4 t + j.  T: the threshold
// key; need: how many elements equal to T are taken, the first in column order; g = k - need; eq_before: equals in the chunks
// before this one (in and out, the same in every lane).  One barrier, and wtot[par] is rewritten two chunks later.
template <int R>
__device__ __forceinline__ void collect_chunk(BlockLds &s, const unsigned (&key)[R][4], const int cbase, const int n, const unsigned T,
                                              const unsigned need, const unsigned g, const int par, unsigned &eq_before) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned wpre[R];  // equals in the lower lanes of the wave, per step
#pragma unroll
  for (int r = 0; r < R; r++) {
    unsigned c = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) c += (cbase + r * 1024 + t * 4 + j < n && key[r][j] == T) ? 1u : 0u;
    unsigned incl = c;
#pragma unroll
    for (int h = 1; h < 64; h <<= 1) {
      const unsigned v = __shfl_up(incl, h);
      if (lane >= h) incl += v;
    }
    wpre[r] = incl - c;
    if (lane == 63) s.wtot[par][r][w] = incl;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; r++) {
    unsigned before = eq_before + wpre[r], tot = 0;
#pragma unroll
    for (int w2 = 0; w2 < 4; w2++) {
      const unsigned v = s.wtot[par][r][w2];
      tot += v;
      if (w2 < w) before += v;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = cbase + r * 1024 + t * 4 + j;
      if (i < n) {
        const unsigned kk = key[r][j];
        if (kk > T) {
          const unsigned slot = atomicAdd(&s.sel[2], 1u);
          if (slot < g) s.buf[slot] = composite(kk, i);  // (there are exactly g such keys)
        } else if (kk == T) {
          if (before < need) s.buf[g + before] = composite(kk, i);
          before++;
        }
      }
    }
    eq_before += tot;
  }
}

// the k collected composites padded to P, sorted, and written out
__device__ __forceinline__ void sort_and_store(BlockLds &s, const TopkArgs &a, const long long row, const int P) {
  const int t = threadIdx.x;
  for (int i = a.k + t; i < P; i += 256) s.buf[i] = 0ull;
  sort_desc<256>(s.buf, P, t, true);
  for (int i = t; i < a.k; i += 256) store_result(a, row, i, s.buf[i]);
}

template <bool VEC>
__global__ void __launch_bounds__(256) topk_resident_kernel(const TopkArgs a) {
  constexpr int R = LH_SELECT_RESIDENT_N / 1024;
  __shared__ BlockLds s;
  const int t = threadIdx.x, n = a.n;
  int P = 1;
  while (P < a.k) P <<= 1;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const unsigned *x = a.x + row * a.xs;
    unsigned key[R][4];
#pragma unroll
    for (int r = 0; r < R; r++) {
      unsigned q[4] = {0u, 0u, 0u, 0u};
      if (r * 1024 < n) load4u<VEC>(x, r * 1024 + t * 4, n, q);
#pragma unroll
      for (int j = 0; j < 4; j++) key[r][j] = key_of(q[j], a.flip);
    }
    unsigned prefix = 0, mask = 0, need = (unsigned)a.k;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      s.hist[t] = 0;
      __syncthreads();
#pragma unroll
      for (int r = 0; r < R; r++) {
        if (r * 1024 < n) {
#pragma unroll
          for (int j = 0; j < 4; j++)
            hist_add(s.hist, r * 1024 + t * 4 + j < n && (key[r][j] & mask) == prefix, (key[r][j] >> shift) & 255u);
        }
      }
      __syncthreads();
      unsigned digit, rem;
      pick_digit(s, need, digit, rem);
      prefix |= digit << shift;
      mask |= 255u << shift;
      need = rem;
    }
    if (t == 0) s.sel[2] = 0;
    unsigned eq_before = 0;
    collect_chunk<R>(s, key, 0, n, prefix, need, (unsigned)a.k - need, 0, eq_before);
    sort_and_store(s, a, row, P);
    __syncthreads();  // the results are read before the next row's collection
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) topk_streaming_kernel(const TopkArgs a) {
  constexpr int R = LH_SELECT_COLLECT_CHUNK / 1024;
  __shared__ BlockLds s;
  const int t = threadIdx.x, n = a.n;
  int P = 1;
  while (P < a.k) P <<= 1;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const unsigned *x = a.x + row * a.xs;
    unsigned prefix = 0, mask = 0, need = (unsigned)a.k;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
      s.hist[t] = 0;
      __syncthreads();
#pragma unroll 1
      for (int cb = 0; cb < n; cb += LH_SELECT_COLLECT_CHUNK) {  // the trip count is the workgroup's: hist_add takes whole waves
        unsigned q[R][4];
#pragma unroll
        for (int r = 0; r < R; r++) load4u<VEC>(x, cb + r * 1024 + t * 4, n, q[r]);  // R loads in flight
#pragma unroll
        for (int r = 0; r < R; r++) {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const unsigned kk = key_of(q[r][j], a.flip);
            hist_add(s.hist, cb + r * 1024 + t * 4 + j < n && (kk & mask) == prefix, (kk >> shift) & 255u);
          }
        }
      }
      __syncthreads();
      unsigned digit, rem;
      pick_digit(s, need, digit, rem);
      prefix |= digit << shift;
      mask |= 255u << shift;
      need = rem;
    }
    if (t == 0) s.sel[2] = 0;
    unsigned eq_before = 0;
    int par = 0;
#pragma unroll 1
    for (int cb = 0; cb < n; cb += LH_SELECT_COLLECT_CHUNK, par ^= 1) {
      unsigned key[R][4];
#pragma unroll
      for (int r = 0; r < R; r++) {
        unsigned q[4];
        load4u<VEC>(x, cb + r * 1024 + t * 4, n, q);
#pragma unroll
        for (int j = 0; j < 4; j++) key[r][j] = key_of(q[j], a.flip);
      }
      collect_chunk<R>(s, key, cb, n, prefix, need, (unsigned)a.k - need, par, eq_before);
    }
    sort_and_store(s, a, row, P);
    __syncthreads();  // the results are read before the next row's collection
  }
}

// ---- argmax: one pass, the maximum of the composites ------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_max_u64(u64 m) {
#pragma unroll
  for (int h = 32; h >= 1; h /= 2) {
    const u64 o = __shfl_xor(m, h);
    m = o > m ? o : m;
  }
  return m;
}

__device__ __forceinline__ void store_argmax(const ArgmaxArgs &a, const long long row, const u64 c) {
  a.idx[row * a.is] = col_of(c);
  if (a.val) a.val[row * a.vs] = bits_of((unsigned)(c >> 32), a.flip);
}

template <bool VEC>
__global__ void __launch_bounds__(256) argmax_wave_kernel(const ArgmaxArgs a) {
  const int lane = threadIdx.x & 63;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < a.rows; row += (long long)gridDim.x * 4) {
    unsigned q[4];
    load4u<VEC>(a.x + row * a.xs, lane * 4, a.n, q);
    u64 m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u64 c = lane * 4 + j < a.n ? composite(key_of(q[j], a.flip), lane * 4 + j) : 0ull;
      m = c > m ? c : m;
    }
    m = wave_max_u64(m);
    if (lane == 0) store_argmax(a, row, m);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) argmax_block_kernel(const ArgmaxArgs a) {
  __shared__ u64 red[4];
  const int t = threadIdx.x, n = a.n;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const unsigned *x = a.x + row * a.xs;
    u64 m = 0;
#pragma unroll 4
    for (int base = t * 4; base < n; base += 1024) {
      unsigned q[4];
      load4u<VEC>(x, base, n, q);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const u64 c = base + j < n ? composite(key_of(q[j], a.flip), base + j) : 0ull;
        m = c > m ? c : m;
      }
    }
    m = wave_max_u64(m);
    __syncthreads();  // the last reader of red is done
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    if (t == 0) {
      const u64 m01 = red[0] > red[1] ? red[0] : red[1], m23 = red[2] > red[3] ? red[2] : red[3];
      store_argmax(a, row, m01 > m23 ? m01 : m23);
    }
  }
}

// ---- out[r, c] = src[r, j[r, c]], -1 where j[r, c] is outside [0, m) --------------------------------------------------------------
__global__ void __launch_bounds__(256) take_rows_kernel(int *out, const long long os, const int *src, const long long ss, const int *jj,
                                                        const long long js, const long long rows, const long long m,
                                                        const long long num) {
  const unsigned long long total = (unsigned long long)rows * (unsigned long long)num;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (unsigned long long)gridDim.x * 256) {
    const long long r = (long long)(i / (unsigned long long)num), c = (long long)(i - (unsigned long long)r * (unsigned long long)num);
    const long long j = jj[r * js + c];
    out[r * os + c] = j >= 0 && j < m ? src[r * ss + j] : -1;
  }
}

// 16-byte loads need the base and every applied row stride of the source on the alignment
bool vec_ok(const void *p, long long stride, long long rows) { return (uintptr_t)p % 16 == 0 && (rows <= 1 || stride % 4 == 0); }

}  // namespace

hipError_t launch_topk_rows_f32(float *vals, int64_t vs, int32_t *idx, int64_t is, const float *src, int64_t xs, int64_t rows, int64_t n,
                                int64_t k, int largest, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  long long p[3];
  if (lh_topk_plan(rows, n, k, vec_ok(src, xs, rows) ? 1 : 0, p) != 0) return hipErrorInvalidValue;
  TopkArgs a;
  a.vals = (unsigned *)vals;
  a.vs = vs;
  a.idx = idx;
  a.is = is;
  a.x = (const unsigned *)src;
  a.xs = xs;
  a.rows = rows;
  a.n = (int)n;
  a.k = (int)k;
  a.flip = largest ? 0u : 0xFFFFFFFFu;
  const dim3 grid((unsigned)p[1]);
  switch ((int)p[0]) {
    case 0: hipLaunchKernelGGL((topk_wave_kernel<true>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((topk_resident_kernel<true>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((topk_streaming_kernel<true>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((topk_wave_kernel<false>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((topk_resident_kernel<false>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((topk_streaming_kernel<false>), grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_topk_kernel = (int)p[0];
  return e;
}

hipError_t launch_argmax_rows_f32(int32_t *idx, int64_t is, float *val, int64_t vs, const float *src, int64_t xs, int64_t rows, int64_t n,
                                  int largest, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  long long p[3];
  if (lh_topk_plan(rows, n, 1, vec_ok(src, xs, rows) ? 1 : 0, p) != 0) return hipErrorInvalidValue;
  ArgmaxArgs a;
  a.idx = idx;
  a.is = is;
  a.val = (unsigned *)val;
  a.vs = vs;
  a.x = (const unsigned *)src;
  a.xs = xs;
  a.rows = rows;
  a.n = (int)n;
  a.flip = largest ? 0u : 0xFFFFFFFFu;
  const dim3 grid((unsigned)p[1]);
  switch ((int)p[0]) {
    case 0: hipLaunchKernelGGL((argmax_wave_kernel<true>), grid, dim3(256), 0, s, a); break;
    case 1:
    case 2: hipLaunchKernelGGL((argmax_block_kernel<true>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((argmax_wave_kernel<false>), grid, dim3(256), 0, s, a); break;
    case 5:
    case 6: hipLaunchKernelGGL((argmax_block_kernel<false>), grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) g_last_topk_kernel = (int)p[0] + 8;
  return e;
}

hipError_t launch_take_rows_i32(int32_t *out, int64_t os, const int32_t *src, int64_t ss, const int32_t *j, int64_t js, int64_t rows,
                                int64_t m, int64_t num, hipStream_t s) {
  if (rows == 0 || num == 0) return hipSuccess;
  const unsigned long long total = (unsigned long long)rows * (unsigned long long)num, want = (total + 255) / 256;
  const unsigned grid = (unsigned)std::min<unsigned long long>(want, LH_SELECT_MAX_WORKGROUPS);
  hipLaunchKernelGGL(take_rows_kernel, dim3(grid), dim3(256), 0, s, out, (long long)os, src, (long long)ss, j, (long long)js,
                     (long long)rows, (long long)m, (long long)num);
  return hipGetLastError();
}

}  // namespace laser_hip
