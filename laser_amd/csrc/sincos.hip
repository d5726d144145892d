// laser_amd/csrc/sincos.hip -- lsin, lcos and both at once over strided device views (include/laser_hip.h, "Sine and
// cosine").  The functions are sincos_core.h's; sincos shares one argument reduction between its two results, which have the
// bits of lsin and lcos.  SinCosOp<FN> is the rule (kBoth: two outputs, sine then cosine); the kernels, the grid and the
// vector choice are pointwise.h's.  The 36 bytes of 2/pi stay in one cache line and are read only by arguments of 2^20 and
// more.
#include <hip/hip_runtime.h>

#include "../../include/laser_hip.h"
#include "common.h"
#include "pointwise.h"
#include "sincos_core.h"

#pragma clang fp contract(off)

namespace laser_hip {
namespace {

enum { kSin = 0, kCos = 1, kBoth = 2 };

template <int FN>
struct SinCosOp : PointwiseOp<1, FN == kBoth ? 2 : 1> {
  __device__ __forceinline__ void apply(const float (&x)[1], float (&y)[FN == kBoth ? 2 : 1]) const {
    if (FN == kSin) y[0] = lh_sin(x[0]);
    if (FN == kCos) y[0] = lh_cos(x[0]);
    if constexpr (FN == kBoth) lh_sincos(x[0], &y[0], &y[1]);
  }
};

}  // namespace

hipError_t launch_sin_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s) {
  return launch_pointwise<SinCosOp<kSin>>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
}
hipError_t launch_cos_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape, int rank,
                          hipStream_t s) {
  return launch_pointwise<SinCosOp<kCos>>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
}
hipError_t launch_sincos_f32(float *sin_dst, const int64_t *sin_strides, float *cos_dst, const int64_t *cos_strides, const float *src,
                             const int64_t *sstrides, const int64_t *shape, int rank, hipStream_t s) {
  return launch_pointwise<SinCosOp<kBoth>>({sin_dst, cos_dst}, {sin_strides, cos_strides}, {src}, {sstrides}, shape, rank, s);
}

}  // namespace laser_hip
