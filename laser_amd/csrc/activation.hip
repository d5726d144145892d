// laser_amd/csrc/activation.hip -- relu, ltanh and lsigmoid over strided device views, and their gradients from the forward
// OUTPUT (include/laser_hip.h, "Activations").  ltanh and lsigmoid are act_core.h's; relu is the fused GEMM / conv
// epilogue's rule.  All float32 operations of the gradients are rounded on their own, never fused:
//   relu      y = x > 0 ? x : +0 (NaN and -0 give +0)      dx = y > 0 ? dy : +0
//   tanh      y = ltanh(x)                                  t = y * y;  u = 1 - t;  dx = dy * u
//   sigmoid   y = lsigmoid(x)                               u = 1 - y;  v = y * u;  dx = dy * v
// ActOp<ACT> (one input) and ActGradOp<ACT> (dy and y; act_grad_core.h's lh_act_grad) are the rules; the kernels, the grid and the vector choice are
// pointwise.h's.  No table in LDS: the 512 bytes of 2^(j/64) stay in four cache lines.
#include <hip/hip_runtime.h>

#include "../../include/laser_hip.h"
#include "act_core.h"
#include "act_grad_core.h"
#include "common.h"
#include "pointwise.h"

#pragma clang fp contract(off)

namespace laser_hip {
namespace {

template <int ACT>
struct ActOp : PointwiseOp<1, 1> {
  __device__ __forceinline__ void apply(const float (&x)[1], float (&y)[1]) const {
    if (ACT == LASER_HIP_ACT_RELU) y[0] = x[0] > 0.0f ? x[0] : 0.0f;
    if (ACT == LASER_HIP_ACT_TANH) y[0] = lh_act_tanh(x[0]);
    if (ACT == LASER_HIP_ACT_SIGMOID) y[0] = lh_act_sigmoid(x[0]);
  }
};

// x[0] = dy, x[1] = the forward output y
template <int ACT>
struct ActGradOp : PointwiseOp<2, 1> {
  __device__ __forceinline__ void apply(const float (&x)[2], float (&dx)[1]) const {
    dx[0] = lh_act_grad<ACT>(x[0], x[1]);
  }
};

}  // namespace

hipError_t launch_act_f32(int act, float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s) {
  switch (act) {
    case LASER_HIP_ACT_RELU:
      return launch_pointwise<ActOp<LASER_HIP_ACT_RELU>>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
    case LASER_HIP_ACT_TANH:
      return launch_pointwise<ActOp<LASER_HIP_ACT_TANH>>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
    case LASER_HIP_ACT_SIGMOID:
      return launch_pointwise<ActOp<LASER_HIP_ACT_SIGMOID>>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_act_grad_f32(int act, float *dx, const int64_t *dxstrides, const float *dy, const int64_t *dystrides, const float *y,
                               const int64_t *ystrides, const int64_t *shape, int rank, hipStream_t s) {
  switch (act) {
    case LASER_HIP_ACT_RELU:
      return launch_pointwise<ActGradOp<LASER_HIP_ACT_RELU>>({dx}, {dxstrides}, {dy, y}, {dystrides, ystrides}, shape, rank, s);
    case LASER_HIP_ACT_TANH:
      return launch_pointwise<ActGradOp<LASER_HIP_ACT_TANH>>({dx}, {dxstrides}, {dy, y}, {dystrides, ystrides}, shape, rank, s);
    case LASER_HIP_ACT_SIGMOID:
      return launch_pointwise<ActGradOp<LASER_HIP_ACT_SIGMOID>>({dx}, {dxstrides}, {dy, y}, {dystrides, ystrides}, shape, rank, s);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace laser_hip
