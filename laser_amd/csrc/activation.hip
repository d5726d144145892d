// laser_amd/csrc/activation.hip -- relu, ltanh and lsigmoid over strided device views, and their gradients from the forward
// OUTPUT (include/laser_hip.h, "Activations").  ltanh and lsigmoid are act_core.h's; relu is the fused GEMM / conv
// epilogue's rule.  All float32 operations of the gradients are rounded on their own, never fused:
//   relu      y = x > 0 ? x : +0 (NaN and -0 give +0)      dx = y > 0 ? dy : +0
//   tanh      y = ltanh(x)                                  t = y * y;  u = 1 - t;  dx = dy * u
//   sigmoid   y = lsigmoid(x)                               u = 1 - y;  v = y * u;  dx = dy * v
//   act_vec_kernel / act_strided_kernel             the shapes of log_vec_kernel / log_strided_kernel (log_softmax.hip): one
//   act_grad_vec_kernel / act_grad_strided_kernel   16-byte vector per lane and step for C-contiguous, 16-byte-aligned
//                                                   operands, otherwise one element per lane and step over the merged
//                                                   dimensions (rank <= 6).  At most 2048 workgroups, which stride over
//                                                   the elements.  No table in LDS: the 512 bytes of 2^(j/64) stay in four
//                                                   cache lines.
// The grid and vector choice is the log kernels'.  No workgroup waits on another; no atomics, no flags.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "act_core.h"
#include "common.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

namespace laser_hip {
namespace {

template <int ACT>
__device__ __forceinline__ float act_fwd(const float x) {
  if (ACT == LASER_HIP_ACT_RELU) return x > 0.0f ? x : 0.0f;
  if (ACT == LASER_HIP_ACT_TANH) return lh_act_tanh(x);
  return lh_act_sigmoid(x);
}

template <int ACT>
__device__ __forceinline__ float act_grad(const float dy, const float y) {
  if (ACT == LASER_HIP_ACT_RELU) return y > 0.0f ? dy : 0.0f;
  if (ACT == LASER_HIP_ACT_TANH) {
    const float t = y * y;
    const float u = 1.0f - t;
    return dy * u;
  }
  const float u = 1.0f - y;
  const float v = y * u;
  return dy * v;
}

template <int ACT>
__global__ void __launch_bounds__(256) act_vec_kernel(float *dst, const float *src, const long long n) {
  const long long nvec = n / 4, step = (long long)gridDim.x * 256;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long v = gid; v < nvec; v += step) {
    F4 x = ((const F4 *)src)[v];
#pragma unroll
    for (int j = 0; j < 4; j++) x.v[j] = act_fwd<ACT>(x.v[j]);
    ((F4 *)dst)[v] = x;
  }
  const long long t = nvec * 4 + gid;  // the last n % 4 elements
  if (t < n) dst[t] = act_fwd<ACT>(src[t]);
}

template <int ACT>
__global__ void __launch_bounds__(256) act_grad_vec_kernel(float *dx, const float *dy, const float *y, const long long n) {
  const long long nvec = n / 4, step = (long long)gridDim.x * 256;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long v = gid; v < nvec; v += step) {
    const F4 g = ((const F4 *)dy)[v], o = ((const F4 *)y)[v];
    F4 r;
#pragma unroll
    for (int j = 0; j < 4; j++) r.v[j] = act_grad<ACT>(g.v[j], o.v[j]);
    ((F4 *)dx)[v] = r;
  }
  const long long t = nvec * 4 + gid;
  if (t < n) dx[t] = act_grad<ACT>(dy[t], y[t]);
}

struct ActArgs {
  float *dst;
  const float *a, *b;  // forward: a = src; gradient: a = dy, b = y
  long long n, rank;
  long long shape[kMaxRank], sd[kMaxRank], sa[kMaxRank], sb[kMaxRank];  // merged extents and element strides
};

template <int ACT, bool GRAD>
__global__ void __launch_bounds__(256) act_strided_kernel(const ActArgs a) {
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += step) {
    long long rem = i, od = 0, oa = 0, ob = 0;
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      if (d < a.rank) {
        const long long q = d ? rem / a.shape[d] : 0, idx = rem - q * a.shape[d];
        od += idx * a.sd[d];
        oa += idx * a.sa[d];
        if (GRAD) ob += idx * a.sb[d];
        rem = q;
      }
    }
    a.dst[od] = GRAD ? act_grad<ACT>(a.a[oa], a.b[ob]) : act_fwd<ACT>(a.a[oa]);
  }
}

// nops = 2: dst, a; nops = 3: dst, a, b
template <int ACT>
hipError_t launch_act(int nops, float *dst, const int64_t *ds, const float *a, const int64_t *as, const float *b, const int64_t *bs,
                      const int64_t *shape, int rank, hipStream_t s) {
  int64_t all[3 * kMaxRank], st[3][kMaxRank] = {}, sh[kMaxRank] = {};
  int64_t n = 1;
  for (int d = 0; d < rank; d++) {
    all[d] = ds[d];
    all[rank + d] = as[d];
    if (nops == 3) all[2 * rank + d] = bs[d];
    n *= shape[d];
  }
  if (n == 0) return hipSuccess;
  const int r = merge_dims(nops, all, shape, rank, st, sh);
  const bool contiguous = r == 1 && st[0][0] == 1 && st[1][0] == 1 && (nops == 2 || st[2][0] == 1);
  if (contiguous && (uintptr_t)dst % 16 == 0 && (uintptr_t)a % 16 == 0 && (nops == 2 || (uintptr_t)b % 16 == 0)) {
    const int64_t blocks = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n / 4 + 255) / 256));
    if (nops == 2)
      hipLaunchKernelGGL(act_vec_kernel<ACT>, dim3((unsigned)blocks), dim3(256), 0, s, dst, a, (long long)n);
    else
      hipLaunchKernelGGL(act_grad_vec_kernel<ACT>, dim3((unsigned)blocks), dim3(256), 0, s, dst, a, b, (long long)n);
    return hipGetLastError();
  }
  ActArgs k = {};
  k.dst = dst;
  k.a = a;
  k.b = b;
  k.n = n;
  k.rank = r;
  for (int d = 0; d < r; d++) {
    k.shape[d] = sh[d];
    k.sd[d] = st[0][d];
    k.sa[d] = st[1][d];
    k.sb[d] = nops == 3 ? st[2][d] : 0;
  }
  const int64_t blocks = std::min<int64_t>(kMaxBlocks, (n + 255) / 256);
  if (nops == 2)
    hipLaunchKernelGGL((act_strided_kernel<ACT, false>), dim3((unsigned)blocks), dim3(256), 0, s, k);
  else
    hipLaunchKernelGGL((act_strided_kernel<ACT, true>), dim3((unsigned)blocks), dim3(256), 0, s, k);
  return hipGetLastError();
}

hipError_t launch_any(int act, int nops, float *dst, const int64_t *ds, const float *a, const int64_t *as, const float *b,
                      const int64_t *bs, const int64_t *shape, int rank, hipStream_t s) {
  switch (act) {
    case LASER_HIP_ACT_RELU:
      return launch_act<LASER_HIP_ACT_RELU>(nops, dst, ds, a, as, b, bs, shape, rank, s);
    case LASER_HIP_ACT_TANH:
      return launch_act<LASER_HIP_ACT_TANH>(nops, dst, ds, a, as, b, bs, shape, rank, s);
    case LASER_HIP_ACT_SIGMOID:
      return launch_act<LASER_HIP_ACT_SIGMOID>(nops, dst, ds, a, as, b, bs, shape, rank, s);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_act_f32(int act, float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s) {
  return launch_any(act, 2, dst, dstrides, src, sstrides, nullptr, nullptr, shape, rank, s);
}

hipError_t launch_act_grad_f32(int act, float *dx, const int64_t *dxstrides, const float *dy, const int64_t *dystrides, const float *y,
                               const int64_t *ystrides, const int64_t *shape, int rank, hipStream_t s) {
  return launch_any(act, 3, dx, dxstrides, dy, dystrides, y, ystrides, shape, rank, s);
}

}  // namespace laser_hip
