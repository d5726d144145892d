// laser_amd/csrc/reduce.hip -- reduce_sum / reduce_min / reduce_max over strided device views (include/laser_hip.h,
// "Reductions"): the device form of Laser's L4 primitives (laser/primitives/reductions.nim:48-116), precompiled for
// f32 / f64 / i32 / i64.
//
// The order of the operations is reduce_core.h's, shared with the run-time-compiled forEachReduce kernels (foreach.cpp):
// one workgroup per chunk of R*W*E elements writes the chunk's partial with a plain store; more than one chunk leaves an
// array of partials in stream-ordered scratch, which the next launch reduces by the same rule, until one value is left.
// No atomics.  Three traversals of the first level, picked per call like forEach's (last_reduce_variant):
//   0  C-contiguous and 16-byte aligned: one 16-byte vector per lane and step;
//   1  C-contiguous with a base off its 16-byte alignment: the same elements, one scalar load each;
//   2  strided (rank <= 6, any element strides, 0 included): logical index -> offset, 64-bit.
// Every traversal hands the visitor the same logical elements, so all three give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <limits>
#include <type_traits>

#include "../../include/laser_hip.h"
#include "capi_internal.h"
#include "common.h"
#include "reduce_core.h"

static_assert(LH_REDUCE_LANES == LASER_HIP_REDUCE_LANES && LH_REDUCE_STEPS == LASER_HIP_REDUCE_STEPS,
              "include/laser_hip.h states the order of reduce_core.h");

namespace laser_hip {

std::atomic<int> g_last_reduce_variant{-1};

namespace {

template <typename T, int N>
struct alignas(sizeof(T) * N) Vec {
  T v[N];
};

// the merges of the three reductions; integer sums wrap mod 2^n
template <typename T>
struct SumOp {
  static __device__ __forceinline__ void merge(T &a, const T b) {
    if constexpr (std::is_integral<T>::value) {
      typedef typename std::make_unsigned<T>::type U;
      a = (T)((U)a + (U)b);
    } else {
      a = a + b;
    }
  }
};
template <typename T>
struct MinOp {
  static __device__ __forceinline__ void merge(T &a, const T b) {
    if constexpr (std::is_integral<T>::value) a = b < a ? b : a;
    else a = lh_reduce_min(a, b);
  }
};
template <typename T>
struct MaxOp {
  static __device__ __forceinline__ void merge(T &a, const T b) {
    if constexpr (std::is_integral<T>::value) a = b > a ? b : a;
    else a = lh_reduce_max(a, b);
  }
};

struct RArgs {
  const void *p;
  long long n;
  long long rank;               // merged rank (strided traversal)
  long long shape[kMaxRank];    // merged extents
  long long st[kMaxRank];       // merged element strides
};

// the three traversals: how logical element i is found
template <typename T, int E, class M>
struct VecVisit {
  const T *p;
  __device__ __forceinline__ void group(long long i, T (&acc)[E]) {
    const Vec<T, E> x = ((const Vec<T, E> *)p)[i / E];
#pragma unroll
    for (int j = 0; j < E; j++) M::merge(acc[j], x.v[j]);
  }
  __device__ __forceinline__ void one(long long i, T &acc) { M::merge(acc, p[i]); }
};
template <typename T, int E, class M>
struct ScalarVisit {
  const T *p;
  __device__ __forceinline__ void group(long long i, T (&acc)[E]) {
#pragma unroll
    for (int j = 0; j < E; j++) M::merge(acc[j], p[i + j]);
  }
  __device__ __forceinline__ void one(long long i, T &acc) { M::merge(acc, p[i]); }
};
template <typename T, int E, class M>
struct StridedVisit {
  const T *p;
  const RArgs &a;
  // the index of logical element i along every merged dimension; returns its offset
  __device__ __forceinline__ long long locate(long long i, long long (&idx)[kMaxRank]) const {
    long long o = 0;
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      idx[d] = 0;
      if (d < a.rank) {
        const long long q = d ? i / a.shape[d] : 0;
        idx[d] = i - q * a.shape[d];
        o += idx[d] * a.st[d];
        i = q;
      }
    }
    return o;
  }
  // the next element in logical order: an odometer step, no division
  __device__ __forceinline__ void advance(long long (&idx)[kMaxRank], long long &o) const {
    bool carry = true;
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      if (d < a.rank && carry) {
        o += a.st[d];
        carry = ++idx[d] == a.shape[d];
        if (carry) {
          idx[d] = 0;
          o -= a.shape[d] * a.st[d];
        }
      }
    }
  }
  __device__ __forceinline__ void group(long long i, T (&acc)[E]) {
    long long idx[kMaxRank];
    long long o = locate(i, idx);
#pragma unroll
    for (int j = 0; j < E; j++) {
      M::merge(acc[j], p[o]);
      if (j + 1 < E) advance(idx, o);
    }
  }
  __device__ __forceinline__ void one(long long i, T &acc) {
    long long idx[kMaxRank];
    M::merge(acc, p[locate(i, idx)]);
  }
};

template <typename T, class M, int V>
__global__ void __launch_bounds__(256) reduce_kernel(const RArgs a, const T init, T *out) {
  constexpr int E = 16 / sizeof(T);
  __shared__ T lds[LH_REDUCE_LANES];
  T x;
  if constexpr (V == 0) {
    VecVisit<T, E, M> vis{(const T *)a.p};
    x = lh_reduce_chunk<T, E, M>(vis, blockIdx.x, a.n, init, lds);
  } else if constexpr (V == 1) {
    ScalarVisit<T, E, M> vis{(const T *)a.p};
    x = lh_reduce_chunk<T, E, M>(vis, blockIdx.x, a.n, init, lds);
  } else {
    StridedVisit<T, E, M> vis{(const T *)a.p, a};
    x = lh_reduce_chunk<T, E, M>(vis, blockIdx.x, a.n, init, lds);
  }
  if (threadIdx.x == 0) out[blockIdx.x] = x;
}

template <typename T, class M>
hipError_t run(const RArgs &a0, int variant, T init, T *out, hipStream_t s) {
  constexpr int E = 16 / sizeof(T);
  auto level0 = [&](int64_t blocks, void *dst) {
    if (variant == 0)
      hipLaunchKernelGGL((reduce_kernel<T, M, 0>), dim3((unsigned)blocks), dim3(256), 0, s, a0, init, (T *)dst);
    else if (variant == 1)
      hipLaunchKernelGGL((reduce_kernel<T, M, 1>), dim3((unsigned)blocks), dim3(256), 0, s, a0, init, (T *)dst);
    else
      hipLaunchKernelGGL((reduce_kernel<T, M, 2>), dim3((unsigned)blocks), dim3(256), 0, s, a0, init, (T *)dst);
    return hipGetLastError();
  };
  auto partials = [&](const void *in, int64_t n, int64_t blocks, void *dst) {
    RArgs a = {};
    a.p = in;
    a.n = n;
    hipLaunchKernelGGL((reduce_kernel<T, M, 0>), dim3((unsigned)blocks), dim3(256), 0, s, a, init, (T *)dst);
    return hipGetLastError();
  };
  return reduce_levels(a0.n, E, (int)sizeof(T), out, s, level0, partials);
}

}  // namespace

int merge_dims(int nops, const int64_t *strides, const int64_t *shape, int rank, int64_t (*st)[kMaxRank], int64_t *sh) {
  int r = 0;
  for (int d = 0; d < rank; d++) {
    if (shape[d] == 1) continue;
    bool merge = r > 0;
    for (int i = 0; i < nops && merge; i++) merge = st[i][r - 1] == strides[i * rank + d] * shape[d];
    if (merge) {
      sh[r - 1] *= shape[d];
      for (int i = 0; i < nops; i++) st[i][r - 1] = strides[i * rank + d];
    } else {
      sh[r] = shape[d];
      for (int i = 0; i < nops; i++) st[i][r] = strides[i * rank + d];
      r++;
    }
  }
  if (r == 0) {
    sh[0] = 1;
    for (int i = 0; i < nops; i++) st[i][0] = 1;
    r = 1;
  }
  return r;
}

hipError_t reduce_levels(int64_t n, int e0, int acc_size, void *out, hipStream_t s, const ReduceLevel0 &level0,
                         const ReducePartials &partials) {
  const int64_t lanes_steps = (int64_t)LH_REDUCE_LANES * LH_REDUCE_STEPS;
  const int64_t s0 = lanes_steps * e0, sp = lanes_steps * (16 / acc_size);
  int64_t count[64];
  int levels = 0;
  count[levels++] = std::max<int64_t>(1, (n + s0 - 1) / s0);  // partials the first level writes
  while (count[levels - 1] > 1) {
    count[levels] = (count[levels - 1] + sp - 1) / sp;
    levels++;
  }
  if (count[0] > 0x7fffffffLL) return hipErrorInvalidValue;
  if (levels == 1) return level0(1, out);
  // every level's partials in one stream-ordered allocation, each array 16-byte aligned for the vector loads
  size_t off[64], bytes = 0;
  for (int l = 0; l + 1 < levels; l++) {
    off[l] = bytes;
    bytes += ((size_t)count[l] * acc_size + 15) / 16 * 16;
  }
  char *buf = nullptr;
  hipError_t e = scratch_alloc_async((void **)&buf, bytes, s);
  if (e != hipSuccess) return e;
  e = level0(count[0], buf + off[0]);
  for (int l = 1; l < levels && e == hipSuccess; l++)
    e = partials(buf + off[l - 1], count[l - 1], count[l], l + 1 < levels ? (void *)(buf + off[l]) : out);
  const hipError_t f = scratch_free_async(buf, s);
  return e != hipSuccess ? e : f;
}

template <typename T>
hipError_t launch_reduce(int op, const T *src, const int64_t *strides, const int64_t *shape, int rank, T *out, hipStream_t s) {
  RArgs a = {};
  int64_t st[1][kMaxRank] = {}, sh[kMaxRank] = {};
  const int r = merge_dims(1, strides, shape, rank, st, sh);
  a.p = src;
  a.rank = r;
  a.n = 1;
  for (int d = 0; d < rank; d++) a.n *= shape[d];
  for (int d = 0; d < r; d++) {
    a.shape[d] = sh[d];
    a.st[d] = st[0][d];
  }
  const bool contiguous = r == 1 && a.st[0] == 1;
  const int variant = !contiguous ? 2 : (uintptr_t)src % 16 == 0 ? 0 : 1;
  typedef std::numeric_limits<T> L;
  hipError_t e;
  if (op == 0)
    e = run<T, SumOp<T>>(a, variant, T(0), out, s);
  else if (op == 1)
    e = run<T, MinOp<T>>(a, variant, L::has_infinity ? L::infinity() : L::max(), out, s);
  else
    e = run<T, MaxOp<T>>(a, variant, L::has_infinity ? -L::infinity() : L::min(), out, s);
  if (e == hipSuccess) g_last_reduce_variant = variant;
  return e;
}
#define LH_INST(T) template hipError_t launch_reduce<T>(int, const T *, const int64_t *, const int64_t *, int, T *, hipStream_t);
LH_INST(float)
LH_INST(double)
LH_INST(int32_t)
LH_INST(int64_t)
#undef LH_INST

}  // namespace laser_hip
