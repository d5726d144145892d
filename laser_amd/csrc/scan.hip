// laser_amd/csrc/scan.hip -- the row prefix sum, the sorted search and the inverse-CDF sampler of
// benchmarks/random_sampling/bench_multinomial_samplers.nim:49-61,143-214 on device rows (include/laser_hip.h "Row cumsum,
// searchsorted and the inverse-CDF sampler").  scan_core.h is the order, scan_plan.h picks the cumsum variant.
//
// scan_rows_kernel<T, L, VEC>   L lanes own a row (L = 64: four rows per workgroup; L = 256: one) and walk it in tiles of L R
//                               elements, R = LH_SCAN_RUN.  A lane owns one run of a tile: it loads its R elements (16-byte loads
//                               when VEC: the bases and strides allow them; the row's last, partial run element by element
//                               either way), forms loc in registers and puts the run's total into LDS.  One lane per row then
//                               walks the tile's chain, carry after carry, in the order of scan_core.h (128 bytes of totals at a time,
//                               turned into carries in registers) and leaves every run's carry in LDS; after the barrier every lane
//                               adds its carry and stores its run.  The loads of the
//                               next tile are issued before the chain and its local sums are formed while the chain runs, by
//                               every wave but the chain lane's.  A workgroup never waits on another: no flags, no spinning.
// search_kernel<T>              one lane per (row, value): lh_search.
// cdf_sample_kernel<U01>        one lane per (row, draw): lh_cdf_draw.  U01 is the caller's buffer or a Philox stream, as in
//                               sampler.hip.
// cdf_remove_round_kernel<U01>  round s of draw-and-remove: one lane per row draws from the row's fresh CDF, stores the index and
//                               sets the drawn weight to +0; round 0 also writes the -1 of the columns past min(k, n).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "philox_core.h"
#include "scan_plan.h"

static_assert(LH_SCAN_MAX_N == LASER_HIP_SCAN_MAX_N, "plan and header agree");
static_assert(LH_SCAN_RUN == 8 || LH_SCAN_RUN == 16 || LH_SCAN_RUN == 32, "a run is a whole number of 16-byte vectors");
static_assert(LH_SCAN_LANES == 256 && LH_SCAN_WAVE == 64, "the kernel below is written for 256 lanes and rows of 64 or 256 lanes");

namespace laser_hip {
namespace {

constexpr int kRun = LH_SCAN_RUN;
constexpr int kMaxGrid = 16384;  // the lane-per-item kernels walk their items with a grid-sized stride past this

template <class T>
struct alignas(16) Vec16 {
  T v[16 / sizeof(T)];
};

template <class T>
struct ScanArgs {
  T *dst;
  const T *src;
  long long ds, ss;  // row strides in elements
  long long rows, n;
  long long groups;  // groups of 256 / L rows
  int tiles;
};

// the run that starts at element `at` of a row of n: elements past n read as 0 (their sums are never stored).  Only the
// row's last run can be partial; every other one is loaded without a test per element
template <class T, bool VEC>
__device__ __forceinline__ void load_run(T x[kRun], const T *row, const long long at, const long long n, const bool live) {
  constexpr int E = 16 / sizeof(T);
  if (live && at + kRun <= n) {
    if (VEC) {
#pragma unroll
      for (int q = 0; q < kRun / E; q++) {
        const Vec16<T> f = *(const Vec16<T> *)(row + at + q * E);
#pragma unroll
        for (int j = 0; j < E; j++) x[q * E + j] = f.v[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < kRun; j++) x[j] = row[at + j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRun; j++) x[j] = (live && at + j < n) ? row[at + j] : T(0);
  }
}

template <class T, bool VEC>
__device__ __forceinline__ void store_run(const T x[kRun], T *row, const long long at, const long long n, const bool live) {
  constexpr int E = 16 / sizeof(T);
  if (!live) return;
  if (at + kRun <= n) {
    if (VEC) {
#pragma unroll
      for (int q = 0; q < kRun / E; q++) {
        Vec16<T> f;
#pragma unroll
        for (int j = 0; j < E; j++) f.v[j] = x[q * E + j];
        *(Vec16<T> *)(row + at + q * E) = f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kRun; j++) row[at + j] = x[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (at + j < n) row[at + j] = x[j];
  }
}

template <class T, int L, bool VEC>
__global__ void __launch_bounds__(256) scan_rows_kernel(const ScanArgs<T> a) {
#pragma clang fp contract(off)
  constexpr int G = 256 / L;        // rows of a workgroup
  constexpr int TILE = L * kRun;    // elements of a tile
  __shared__ __attribute__((aligned(16))) T tot[256];  // the runs' totals of the current tile
  __shared__ __attribute__((aligned(16))) T car[256];  // the runs' carries
  const int t = threadIdx.x, sub = t / L, l = t % L;
  for (long long g = blockIdx.x; g < a.groups; g += gridDim.x) {
    const long long row = g * G + sub;
    const bool live = row < a.rows;
    const T *src = a.src + (live ? row : 0) * a.ss;
    T *dst = a.dst + (live ? row : 0) * a.ds;
    T x[kRun], nx[kRun];
    T chain = T(0);  // the chain lane's: out of the last element of the previous tile
    load_run<T, VEC>(x, src, (long long)l * kRun, a.n, live);
    lh_scan_local<T, kRun>(x);
    __syncthreads();  // the readers of tot and car of the previous group of rows are done
    tot[t] = x[kRun - 1];
    for (int tile = 0; tile < a.tiles; tile++) {
      const long long at = (long long)tile * TILE + (long long)l * kRun;
      const bool more = tile + 1 < a.tiles;
      if (more) load_run<T, VEC>(nx, src, at + TILE, a.n, live);
      __syncthreads();  // the totals are in LDS
      if (l == 0) {
        // runs of this tile that hold an element of the row; the chain stops there
        const long long left = a.n - (long long)tile * TILE;
        const int runs = left >= TILE ? L : (int)((left + kRun - 1) / kRun);
        const T *tt = tot + sub * L;
        T *cc = car + sub * L;
        T c = chain;
        // CH totals at a time: read, turned into their runs' carries in the same registers, written back.  L is a multiple
        // of CH: a chunk may hold totals past `runs` (their carries are not used), never another row's
        constexpr int CH = 128 / (int)sizeof(T);
        for (int q0 = 0; q0 < runs; q0 += CH) {
          T v[CH];
#pragma unroll
          for (int j = 0; j < CH; j++) v[j] = tt[q0 + j];
#pragma unroll
          for (int j = 0; j < CH; j++) {
            const T total = v[j];
            v[j] = c;
            c = (tile == 0 && q0 + j == 0) ? total : c + total;  // run 0 of the row has no carry: its total is taken as it is
          }
#pragma unroll
          for (int j = 0; j < CH; j++) cc[q0 + j] = v[j];
        }
        chain = c;  // (past `runs` only zeros were added, and no later tile exists)
      }
      if (more) lh_scan_local<T, kRun>(nx);
      __syncthreads();  // the carries are in LDS; the chain lane is done with the totals
      if (tile != 0 || l != 0) lh_scan_add_carry<T, kRun>(x, car[t]);
      store_run<T, VEC>(x, dst, at, a.n, live);
      if (more) {
        tot[t] = nx[kRun - 1];
#pragma unroll
        for (int j = 0; j < kRun; j++) x[j] = nx[j];
      }
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) search_kernel(int *idx, const T *a, const long long as, const T *v, const long long rows,
                                                     const long long m, const int n, const bool right) {
  const long long total = rows * m;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
    idx[e] = lh_search<T>(a + (e / m) * as, n, v[e], right);
}

// where the uniform number of draw e comes from (as in sampler.hip)
struct U01Buffer {
  const float *u01;
  __device__ __forceinline__ float operator()(const long long e) const { return u01[e]; }
};
struct U01Philox {
  unsigned long long seed, subseq, offset;
  __device__ __forceinline__ float operator()(const long long e) const {
    return lh_u01_f32(lh_philox_word(seed, subseq, offset + (unsigned long long)e));
  }
};

template <class U01>
__global__ void __launch_bounds__(256) cdf_sample_kernel(int *idx, const float *cdf, const long long cs, const U01 u01,
                                                         const long long rows, const long long m, const int n) {
  const long long total = rows * m;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
    idx[e] = lh_cdf_draw(cdf + (e / m) * cs, n, u01(e));
}

template <class U01>
__global__ void __launch_bounds__(256) cdf_remove_round_kernel(int *idx, float *w, const long long ws, const float *cdf,
                                                               const long long cs, const U01 u01, const long long rows,
                                                               const long long k, const long long rounds, const long long s,
                                                               const int n) {
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long long)gridDim.x * 256) {
    const int i = lh_cdf_draw(cdf + row * cs, n, u01(row * k + s));
    idx[row * k + s] = i;
    if (i >= 0) w[row * ws + i] = 0.0f;
    if (s == 0)
      for (long long c = rounds; c < k; c++) idx[row * k + c] = -1;
  }
}

inline unsigned lane_grid(long long lanes) { return (unsigned)std::min<long long>((lanes + 255) / 256, kMaxGrid); }

template <class T>
inline bool vec_ok(const T *p, int64_t stride, int64_t rows) {
  return (uintptr_t)p % 16 == 0 && (rows == 1 || (stride * (int64_t)sizeof(T)) % 16 == 0);  // (a stride never applied does not count)
}

template <class T>
hipError_t scan_rows(T *dst, int64_t ds, const T *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  long long plan[4];
  if (lh_scan_plan(rows, n, (int)sizeof(T), 0, plan) != 0) return hipErrorInvalidValue;
  ScanArgs<T> a;
  a.dst = dst;
  a.src = src;
  a.ds = ds;
  a.ss = ss;
  a.rows = rows;
  a.n = n;
  a.groups = (rows + plan[1] - 1) / plan[1];
  a.tiles = (int)plan[3];
  const bool vec = vec_ok(dst, ds, rows) && vec_ok(src, ss, rows);
  const dim3 grid((unsigned)plan[2]);
  if (plan[0] == 0) {
    if (vec) hipLaunchKernelGGL((scan_rows_kernel<T, 64, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((scan_rows_kernel<T, 64, false>), grid, dim3(256), 0, s, a);
  } else {
    if (vec) hipLaunchKernelGGL((scan_rows_kernel<T, 256, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((scan_rows_kernel<T, 256, false>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

template <class T>
hipError_t search_rows(int32_t *idx, const T *a, int64_t as, const T *v, int64_t rows, int64_t n, int64_t m, int right, hipStream_t s) {
  if (rows == 0 || m == 0) return hipSuccess;
  hipLaunchKernelGGL(search_kernel<T>, dim3(lane_grid((long long)rows * m)), dim3(256), 0, s, idx, a, (long long)as, v, (long long)rows,
                     (long long)m, (int)n, right != 0);
  return hipGetLastError();
}

template <class U01>
hipError_t cdf_sample_from(int32_t *idx, const float *cdf, int64_t cs, const U01 &u01, int64_t rows, int64_t n, int64_t m, hipStream_t s) {
  if (rows == 0 || m == 0) return hipSuccess;
  hipLaunchKernelGGL(cdf_sample_kernel<U01>, dim3(lane_grid((long long)rows * m)), dim3(256), 0, s, idx, cdf, (long long)cs, u01,
                     (long long)rows, (long long)m, (int)n);
  return hipGetLastError();
}

template <class U01>
hipError_t cdf_remove_from(int32_t *idx, float *w, int64_t ws, float *cdf, int64_t cs, const U01 &u01, int64_t rows, int64_t n, int64_t k,
                           hipStream_t s) {
  if (rows == 0 || k == 0) return hipSuccess;
  const long long rounds = std::min<long long>(k, n);
  for (long long r = 0; r < rounds; r++) {
    hipError_t e = scan_rows<float>(cdf, cs, w, ws, rows, n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cdf_remove_round_kernel<U01>, dim3(lane_grid(rows)), dim3(256), 0, s, idx, w, (long long)ws, cdf, (long long)cs, u01,
                       (long long)rows, (long long)k, rounds, r, (int)n);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_cumsum_f32(float *dst, int64_t ds, const float *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s) {
  return scan_rows<float>(dst, ds, src, ss, rows, n, s);
}
hipError_t launch_cumsum_f64(double *dst, int64_t ds, const double *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s) {
  return scan_rows<double>(dst, ds, src, ss, rows, n, s);
}
// the integer sums wrap: they are formed in the unsigned type of the same width
hipError_t launch_cumsum_i32(int32_t *dst, int64_t ds, const int32_t *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s) {
  return scan_rows<uint32_t>((uint32_t *)dst, ds, (const uint32_t *)src, ss, rows, n, s);
}
hipError_t launch_cumsum_i64(int64_t *dst, int64_t ds, const int64_t *src, int64_t ss, int64_t rows, int64_t n, hipStream_t s) {
  return scan_rows<unsigned long long>((unsigned long long *)dst, ds, (const unsigned long long *)src, ss, rows, n, s);
}

hipError_t launch_searchsorted_f32(int32_t *idx, const float *a, int64_t as, const float *v, int64_t rows, int64_t n, int64_t m, int right,
                                   hipStream_t s) {
  return search_rows<float>(idx, a, as, v, rows, n, m, right, s);
}
hipError_t launch_searchsorted_f64(int32_t *idx, const double *a, int64_t as, const double *v, int64_t rows, int64_t n, int64_t m, int right,
                                   hipStream_t s) {
  return search_rows<double>(idx, a, as, v, rows, n, m, right, s);
}
hipError_t launch_searchsorted_i32(int32_t *idx, const int32_t *a, int64_t as, const int32_t *v, int64_t rows, int64_t n, int64_t m,
                                   int right, hipStream_t s) {
  return search_rows<int32_t>(idx, a, as, v, rows, n, m, right, s);
}
hipError_t launch_searchsorted_i64(int32_t *idx, const int64_t *a, int64_t as, const int64_t *v, int64_t rows, int64_t n, int64_t m,
                                   int right, hipStream_t s) {
  return search_rows<int64_t>(idx, a, as, v, rows, n, m, right, s);
}

hipError_t launch_cdf_sample_f32(int32_t *idx, const float *cdf, int64_t cs, const float *u01, int64_t rows, int64_t n, int64_t m,
                                 hipStream_t s) {
  return cdf_sample_from(idx, cdf, cs, U01Buffer{u01}, rows, n, m, s);
}
hipError_t launch_cdf_sample_rng_f32(int32_t *idx, const float *cdf, int64_t cs, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     int64_t rows, int64_t n, int64_t m, hipStream_t s) {
  return cdf_sample_from(idx, cdf, cs, U01Philox{seed, subseq, offset}, rows, n, m, s);
}
hipError_t launch_cdf_sample_remove_f32(int32_t *idx, float *w, int64_t ws, float *cdf, int64_t cs, const float *u01, int64_t rows,
                                        int64_t n, int64_t k, hipStream_t s) {
  return cdf_remove_from(idx, w, ws, cdf, cs, U01Buffer{u01}, rows, n, k, s);
}
hipError_t launch_cdf_sample_remove_rng_f32(int32_t *idx, float *w, int64_t ws, float *cdf, int64_t cs, uint64_t seed, uint64_t subseq,
                                            uint64_t offset, int64_t rows, int64_t n, int64_t k, hipStream_t s) {
  return cdf_remove_from(idx, w, ws, cdf, cs, U01Philox{seed, subseq, offset}, rows, n, k, s);
}

}  // namespace laser_hip
