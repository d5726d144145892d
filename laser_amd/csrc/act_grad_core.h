// laser_amd/csrc/act_grad_core.h -- the gradient rules of relu, ltanh and lsigmoid from the forward OUTPUT y (include/laser_hip.h,
// "Activations"): the one definition that laser_hip_act_grad_f32_dev (activation.hip) and laser_hip_bias_grad_f32_dev
// (dense_grad.hip) share.  Every float32 operation is rounded on its own, never fused:
//   relu      dx = y > 0 ? dy : +0
//   tanh      t = y * y;  u = 1 - t;  dx = dy * u
//   sigmoid   u = 1 - y;  v = y * u;  dx = dy * v
// LASER_HIP_ACT_NONE passes dy through (y is not read).
#ifndef LASER_HIP_ACT_GRAD_CORE_H
#define LASER_HIP_ACT_GRAD_CORE_H

#include "../../include/laser_hip.h"

template <int ACT>
__device__ __forceinline__ float lh_act_grad(const float dy, const float y) {
#pragma clang fp contract(off)
  if (ACT == LASER_HIP_ACT_RELU) return y > 0.0f ? dy : 0.0f;
  if (ACT == LASER_HIP_ACT_TANH) {
    const float t = y * y;
    const float u = 1.0f - t;
    return dy * u;
  }
  if (ACT == LASER_HIP_ACT_SIGMOID) {
    const float u = 1.0f - y;
    const float v = y * u;
    return dy * v;
  }
  return dy;
}

#endif  // LASER_HIP_ACT_GRAD_CORE_H
