// laser_amd/csrc/random.hip -- fills of device arrays with uniform and normal random numbers (include/laser_hip.h "Random
// numbers").  The generator and the uniform distributions are philox_core.h, the normal distribution is normal_core.h; which
// lane owns which block, and the grid, are random_plan.h.
//
// One lane computes one Philox4x32-10 block per step -- about forty 32-bit multiplies and as many xors and adds for 16 bytes of
// output -- and stores the elements that start in it: four 32-bit elements or two 64-bit ones, 16 contiguous bytes.  The lanes
// of a wave own consecutive blocks, so on the vector path a wave writes 1 KiB contiguous per step.  A block only partly
// inside [0, n) (the head when offset & 3 != 0, the tail) is stored element by element; so is everything when the runs do not
// start on 16-byte boundaries.  Block indices wrap mod 2^62 like the words they hold wrap mod 2^64.
// The normal fill is one word per element like the 32-bit uniform ones: a block is two Box-Muller pairs, (o[0], o[1]) and
// (o[2], o[3]), each giving its cosine and its sine branch, with the radius and the angle reduction computed once per pair.
#include <hip/hip_runtime.h>

#include "../../include/laser_hip.h"
#include "common.h"
#include "normal_core.h"
#include "philox_core.h"
#include "random_plan.h"

static_assert(LH_RANDOM_MAX_N == LASER_HIP_RANDOM_MAX_N, "plan and header agree");

namespace laser_hip {
namespace {

typedef unsigned long long u64;

// element i = op(x) of its word (WPE = 1) or of its pair of words, low word first (WPE = 2); BLOCK: op(o, v) turns the four
// words of a block into its four elements at once (WPE = 1)
struct BitsU32 {
  typedef uint32_t T;
  static constexpr int WPE = 1;
  static constexpr bool BLOCK = false;
  __device__ __forceinline__ T operator()(const unsigned int x) const { return x; }
};
struct UniformF32 {
  typedef float T;
  static constexpr int WPE = 1;
  static constexpr bool BLOCK = false;
  float lo, hi;
  __device__ __forceinline__ T operator()(const unsigned int x) const { return lh_uniform_f32(x, lo, hi); }
};
struct UniformI32 {
  typedef int32_t T;
  static constexpr int WPE = 1;
  static constexpr bool BLOCK = false;
  int32_t lo, hi;
  __device__ __forceinline__ T operator()(const unsigned int x) const { return lh_uniform_i32(x, lo, hi); }
};
struct UniformF64 {
  typedef double T;
  static constexpr int WPE = 2;
  static constexpr bool BLOCK = false;
  double lo, hi;
  __device__ __forceinline__ T operator()(const u64 x) const { return lh_uniform_f64(x, lo, hi); }
};
struct UniformI64 {
  typedef int64_t T;
  static constexpr int WPE = 2;
  static constexpr bool BLOCK = false;
  int64_t lo, hi;
  __device__ __forceinline__ T operator()(const u64 x) const { return (int64_t)lh_uniform_i64(x, lo, hi); }
};

struct NormalF32 {
  typedef float T;
  static constexpr int WPE = 1;
  static constexpr bool BLOCK = true;
  float mean, std;
  __device__ __forceinline__ void operator()(const unsigned int o[4], float v[4]) const {
    float z[4];
    lh_normal_pair(o[0], o[1], &z[0], &z[1]);
    lh_normal_pair(o[2], o[3], &z[2], &z[3]);
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = lh_normal_scale_f32(z[j], mean, std);
  }
};

template <typename T>
struct alignas(16) Run {
  T v[16 / sizeof(T)];
};

// b0: the block of word `offset`; head = offset & 3; blocks: lh_random_blocks.  VEC: every run starts on a 16-byte boundary.
template <class Op, bool VEC>
__global__ void __launch_bounds__(256) random_fill_kernel(typename Op::T *dst, const long long n, const u64 seed, const u64 subseq,
                                                          const u64 b0, const int head, const long long blocks, const Op op) {
  typedef typename Op::T T;
  constexpr int WPE = Op::WPE, EPB = 4 / WPE;
  const u64 mask62 = (1ull << 62) - 1;
  const int unit = WPE == 2 ? (head & 1) : 0;  // the word of the block at which the lane's run starts
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < blocks; k += (long long)gridDim.x * 256) {
    unsigned int o[4];
    lh_philox_block(seed, subseq, (b0 + (u64)k) & mask62, o);
    const long long e0 = (4 * k + unit - head) / WPE;  // the run's first element: may be < 0 (head) or end past n (tail); exact
    T v[EPB];
    if constexpr (Op::BLOCK) {
      op(o, v);
    } else if constexpr (WPE == 1) {
#pragma unroll
      for (int j = 0; j < 4; j++) v[j] = op(o[j]);
    } else {
      if (unit == 0) {
        v[0] = op((u64)o[0] | (u64)o[1] << 32);
        v[1] = op((u64)o[2] | (u64)o[3] << 32);
      } else {
        v[0] = op((u64)o[1] | (u64)o[2] << 32);
        unsigned int hi = 0;
        if (e0 + 1 < n) {  // the element at word 3 takes its high word from the next block
          unsigned int q[4];
          lh_philox_block(seed, subseq, (b0 + (u64)k + 1) & mask62, q);
          hi = q[0];
        }
        v[1] = op((u64)o[3] | (u64)hi << 32);
      }
    }
    if (VEC && e0 >= 0 && e0 + EPB <= n) {
      Run<T> r;
#pragma unroll
      for (int j = 0; j < EPB; j++) r.v[j] = v[j];
      *(Run<T> *)(dst + e0) = r;
    } else {
#pragma unroll
      for (int j = 0; j < EPB; j++)
        if (e0 + j >= 0 && e0 + j < n) dst[e0 + j] = v[j];
    }
  }
}

template <class Op>
hipError_t fill(typename Op::T *dst, int64_t n, uint64_t seed, uint64_t subseq, uint64_t offset, const Op &op, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const int mis = lh_random_dst_misaligned((u64)(uintptr_t)dst, Op::WPE, offset);
  long long plan[4];
  if (lh_random_plan(n, Op::WPE, offset, mis, 0, plan) != 0) return hipErrorInvalidValue;
  const long long blocks = lh_random_blocks(n, Op::WPE, offset);
  const dim3 grid((unsigned)plan[1]);
  if (plan[0] == 0)
    hipLaunchKernelGGL((random_fill_kernel<Op, true>), grid, dim3(256), 0, s, dst, (long long)n, (u64)seed, (u64)subseq, (u64)plan[3],
                       (int)(offset & 3), blocks, op);
  else
    hipLaunchKernelGGL((random_fill_kernel<Op, false>), grid, dim3(256), 0, s, dst, (long long)n, (u64)seed, (u64)subseq, (u64)plan[3],
                       (int)(offset & 3), blocks, op);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_random_bits_u32(uint32_t *dst, int64_t n, uint64_t seed, uint64_t subseq, uint64_t offset, hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, BitsU32{}, s);
}
hipError_t launch_random_uniform_f32(float *dst, int64_t n, float lo, float hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, UniformF32{lo, hi}, s);
}
hipError_t launch_random_uniform_f64(double *dst, int64_t n, double lo, double hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, UniformF64{lo, hi}, s);
}
hipError_t launch_random_uniform_i32(int32_t *dst, int64_t n, int32_t lo, int32_t hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, UniformI32{lo, hi}, s);
}
hipError_t launch_random_uniform_i64(int64_t *dst, int64_t n, int64_t lo, int64_t hi, uint64_t seed, uint64_t subseq, uint64_t offset,
                                     hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, UniformI64{lo, hi}, s);
}

hipError_t launch_random_normal_f32(float *dst, int64_t n, float mean, float std, uint64_t seed, uint64_t subseq, uint64_t offset,
                                    hipStream_t s) {
  return fill(dst, n, seed, subseq, offset, NormalF32{mean, std}, s);
}

}  // namespace laser_hip
