// laser_amd/csrc/pointwise.h -- the one elementwise traversal of lexp, llog, the activations with their gradients and
// lsin / lcos (exp_softmax.hip, log_softmax.hip, activation.hip, sincos.hip): a vector kernel, a strided kernel and their host
// launcher, templated on an Op that states
//   kIn, kOut                 how many float32 operands it reads and writes (1 or 2 each)
//   setup()                   once per workgroup, before the first element (PointwiseOp's does nothing; lexp's copies its
//                             table into LDS and keeps the pointer)
//   apply(x[kIn], y[kOut])    the rule for one element
// An Op is defined in its .hip file, where the file's `#pragma clang fp contract(off)` covers its arithmetic; this header
// holds no floating-point operation.  Operand arrays are sized by the Op's counts and every loop over them is unrolled, so a
// two-operand instance carries no third pointer or stride walk.
//   pointwise_vec_kernel      every operand merges to one unit-stride dimension and every base is 16-byte aligned: one
//                             16-byte vector per lane and step, then a scalar tail of n % 4 elements
//   pointwise_strided_kernel  anything else of rank <= 6: one element per lane and step, logical index -> per-operand
//                             offsets over the merged dimensions, 64-bit
// 256 lanes per workgroup, at most kMaxBlocks (2048) workgroups, which stride over the work.  An instance loads all its
// inputs of a step before it stores, so an output may be an input.  No workgroup waits on another; no atomics, no flags.
#ifndef LASER_HIP_POINTWISE_H
#define LASER_HIP_POINTWISE_H

#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "softmax_common.h"

namespace laser_hip {
namespace {

template <int IN, int OUT>
struct PointwiseOp {
  static constexpr int kIn = IN, kOut = OUT;
  __device__ __forceinline__ void setup() {}
};

template <class Op>
struct PointwisePtrs {
  float *out[Op::kOut];
  const float *in[Op::kIn];
};

template <class Op>
struct PointwiseArgs {
  PointwisePtrs<Op> p;
  long long n, rank;
  long long shape[kMaxRank], so[Op::kOut][kMaxRank], si[Op::kIn][kMaxRank];  // merged extents and element strides
};

template <class Op>
__global__ void __launch_bounds__(256) pointwise_vec_kernel(const PointwisePtrs<Op> p, const long long n) {
  Op op;
  op.setup();
  const long long nvec = n / 4, step = (long long)gridDim.x * 256;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long v = gid; v < nvec; v += step) {
    F4 x[Op::kIn], y[Op::kOut];
#pragma unroll
    for (int i = 0; i < Op::kIn; i++) x[i] = ((const F4 *)p.in[i])[v];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float xj[Op::kIn], yj[Op::kOut];
#pragma unroll
      for (int i = 0; i < Op::kIn; i++) xj[i] = x[i].v[j];
      op.apply(xj, yj);
#pragma unroll
      for (int o = 0; o < Op::kOut; o++) y[o].v[j] = yj[o];
    }
#pragma unroll
    for (int o = 0; o < Op::kOut; o++) ((F4 *)p.out[o])[v] = y[o];
  }
  const long long t = nvec * 4 + gid;  // the last n % 4 elements
  if (t < n) {
    float x[Op::kIn], y[Op::kOut];
#pragma unroll
    for (int i = 0; i < Op::kIn; i++) x[i] = p.in[i][t];
    op.apply(x, y);
#pragma unroll
    for (int o = 0; o < Op::kOut; o++) p.out[o][t] = y[o];
  }
}

template <class Op>
__global__ void __launch_bounds__(256) pointwise_strided_kernel(const PointwiseArgs<Op> a) {
  Op op;
  op.setup();
  const long long step = (long long)gridDim.x * 256;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.n; e += step) {
    long long rem = e, oo[Op::kOut] = {}, oi[Op::kIn] = {};
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      if (d < a.rank) {
        const long long q = d ? rem / a.shape[d] : 0, idx = rem - q * a.shape[d];
#pragma unroll
        for (int o = 0; o < Op::kOut; o++) oo[o] += idx * a.so[o][d];
#pragma unroll
        for (int i = 0; i < Op::kIn; i++) oi[i] += idx * a.si[i][d];
        rem = q;
      }
    }
    float x[Op::kIn], y[Op::kOut];
#pragma unroll
    for (int i = 0; i < Op::kIn; i++) x[i] = a.p.in[i][oi[i]];
    op.apply(x, y);
#pragma unroll
    for (int o = 0; o < Op::kOut; o++) a.p.out[o][oo[o]] = y[o];
  }
}

// out[o] with element strides ostrides[o][0 .. rank), in[i] with istrides[i][0 .. rank), all over `shape`
template <class Op>
hipError_t launch_pointwise(float *const (&out)[Op::kOut], const int64_t *const (&ostrides)[Op::kOut], const float *const (&in)[Op::kIn],
                            const int64_t *const (&istrides)[Op::kIn], const int64_t *shape, int rank, hipStream_t s) {
  constexpr int kOut = Op::kOut, kOps = Op::kOut + Op::kIn;
  int64_t all[kOps * kMaxRank], st[kOps][kMaxRank] = {}, sh[kMaxRank] = {};
  int64_t n = 1;
  for (int d = 0; d < rank; d++) {
    for (int i = 0; i < kOps; i++) all[i * rank + d] = i < kOut ? ostrides[i][d] : istrides[i - kOut][d];
    n *= shape[d];
  }
  if (n == 0) return hipSuccess;
  const int r = merge_dims(kOps, all, shape, rank, st, sh);
  PointwiseArgs<Op> a = {};
  bool vec = r == 1;
  for (int i = 0; i < kOps; i++) {
    if (i < kOut)
      a.p.out[i] = out[i];
    else
      a.p.in[i - kOut] = in[i - kOut];
    vec = vec && st[i][0] == 1 && (uintptr_t)(i < kOut ? out[i] : in[i - kOut]) % 16 == 0;
  }
  if (vec) {
    const int64_t blocks = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n / 4 + 255) / 256));
    hipLaunchKernelGGL(pointwise_vec_kernel<Op>, dim3((unsigned)blocks), dim3(256), 0, s, a.p, (long long)n);
    return hipGetLastError();
  }
  a.n = n;
  a.rank = r;
  for (int d = 0; d < r; d++) {
    a.shape[d] = sh[d];
    for (int i = 0; i < kOps; i++) (i < kOut ? a.so[i] : a.si[i - kOut])[d] = st[i][d];
  }
  const int64_t blocks = std::min<int64_t>(kMaxBlocks, (n + 255) / 256);
  hipLaunchKernelGGL(pointwise_strided_kernel<Op>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace laser_hip

#endif  // LASER_HIP_POINTWISE_H
