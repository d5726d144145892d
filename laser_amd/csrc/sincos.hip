// laser_amd/csrc/sincos.hip -- lsin, lcos and both at once over strided device views (include/laser_hip.h, "Sine and
// cosine").  The functions are sincos_core.h's; sincos shares one argument reduction between its two results, which have the
// bits of lsin and lcos.
//   sincos_vec_kernel      the shape of act_vec_kernel (activation.hip): one 16-byte vector per lane and step for C-contiguous,
//   sincos_strided_kernel  16-byte-aligned operands, otherwise one element per lane and step over the merged dimensions
//                          (rank <= 6).  At most 2048 workgroups, which stride over the elements.  The 36 bytes of 2/pi stay in
//                          one cache line and are read only by arguments of 2^20 and more.
// The grid and vector choice is the activation kernels'.  No workgroup waits on another; no atomics, no flags.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "sincos_core.h"
#include "softmax_common.h"

#pragma clang fp contract(off)

namespace laser_hip {
namespace {

enum { kSin = 0, kCos = 1, kBoth = 2 };

template <int FN>
__global__ void __launch_bounds__(256) sincos_vec_kernel(float *dst, float *dst2, const float *src, const long long n) {
  const long long nvec = n / 4, step = (long long)gridDim.x * 256;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  for (long long v = gid; v < nvec; v += step) {
    const F4 x = ((const F4 *)src)[v];
    F4 a, b;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (FN == kSin) a.v[j] = lh_sin(x.v[j]);
      if (FN == kCos) a.v[j] = lh_cos(x.v[j]);
      if (FN == kBoth) lh_sincos(x.v[j], &a.v[j], &b.v[j]);
    }
    ((F4 *)dst)[v] = a;
    if (FN == kBoth) ((F4 *)dst2)[v] = b;
  }
  const long long t = nvec * 4 + gid;  // the last n % 4 elements
  if (t < n) {
    const float x = src[t];
    if (FN == kSin) dst[t] = lh_sin(x);
    if (FN == kCos) dst[t] = lh_cos(x);
    if (FN == kBoth) {
      float s, c;
      lh_sincos(x, &s, &c);
      dst[t] = s;
      dst2[t] = c;
    }
  }
}

struct SinCosArgs {
  float *dst, *dst2;
  const float *src;
  long long n, rank;
  long long shape[kMaxRank], sd[kMaxRank], sd2[kMaxRank], ss[kMaxRank];  // merged extents and element strides
};

template <int FN>
__global__ void __launch_bounds__(256) sincos_strided_kernel(const SinCosArgs a) {
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += step) {
    long long rem = i, od = 0, od2 = 0, os = 0;
#pragma unroll
    for (int d = kMaxRank - 1; d >= 0; d--) {
      if (d < a.rank) {
        const long long q = d ? rem / a.shape[d] : 0, idx = rem - q * a.shape[d];
        od += idx * a.sd[d];
        if (FN == kBoth) od2 += idx * a.sd2[d];
        os += idx * a.ss[d];
        rem = q;
      }
    }
    const float x = a.src[os];
    if (FN == kSin) a.dst[od] = lh_sin(x);
    if (FN == kCos) a.dst[od] = lh_cos(x);
    if (FN == kBoth) {
      float s, c;
      lh_sincos(x, &s, &c);
      a.dst[od] = s;
      a.dst2[od2] = c;
    }
  }
}

// operands in merge order: dst, src and, for FN == kBoth, dst2
template <int FN>
hipError_t launch(float *dst, const int64_t *ds, float *dst2, const int64_t *ds2, const float *src, const int64_t *ss, const int64_t *shape,
                  int rank, hipStream_t s) {
  const int nops = FN == kBoth ? 3 : 2;
  int64_t all[3 * kMaxRank], st[3][kMaxRank] = {}, sh[kMaxRank] = {};
  int64_t n = 1;
  for (int d = 0; d < rank; d++) {
    all[d] = ds[d];
    all[rank + d] = ss[d];
    if (nops == 3) all[2 * rank + d] = ds2[d];
    n *= shape[d];
  }
  if (n == 0) return hipSuccess;
  const int r = merge_dims(nops, all, shape, rank, st, sh);
  const bool contiguous = r == 1 && st[0][0] == 1 && st[1][0] == 1 && (nops == 2 || st[2][0] == 1);
  if (contiguous && (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0 && (nops == 2 || (uintptr_t)dst2 % 16 == 0)) {
    const int64_t blocks = std::min<int64_t>(kMaxBlocks, std::max<int64_t>(1, (n / 4 + 255) / 256));
    hipLaunchKernelGGL(sincos_vec_kernel<FN>, dim3((unsigned)blocks), dim3(256), 0, s, dst, dst2, src, (long long)n);
    return hipGetLastError();
  }
  SinCosArgs k = {};
  k.dst = dst;
  k.dst2 = dst2;
  k.src = src;
  k.n = n;
  k.rank = r;
  for (int d = 0; d < r; d++) {
    k.shape[d] = sh[d];
    k.sd[d] = st[0][d];
    k.ss[d] = st[1][d];
    k.sd2[d] = nops == 3 ? st[2][d] : 0;
  }
  const int64_t blocks = std::min<int64_t>(kMaxBlocks, (n + 255) / 256);
  hipLaunchKernelGGL(sincos_strided_kernel<FN>, dim3((unsigned)blocks), dim3(256), 0, s, k);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_sin_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s) {
  return launch<kSin>(dst, dstrides, nullptr, nullptr, src, sstrides, shape, rank, s);
}
hipError_t launch_cos_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s) {
  return launch<kCos>(dst, dstrides, nullptr, nullptr, src, sstrides, shape, rank, s);
}
hipError_t launch_sincos_f32(float *sin_dst, const int64_t *sin_strides, float *cos_dst, const int64_t *cos_strides, const float *src,
                             const int64_t *sstrides, const int64_t *shape, int rank, hipStream_t s) {
  return launch<kBoth>(sin_dst, sin_strides, cos_dst, cos_strides, src, sstrides, shape, rank, s);
}

}  // namespace laser_hip
