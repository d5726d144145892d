// laser_amd/csrc/optim_core.h -- the arithmetic of the optimizer steps (include/laser_hip.h, "Optimizer steps"): the one
// definition that the kernels of optim.hip, laser_hip_adam_bias_correction and a host build for the tests share.  Every
// float32 operation below is rounded on its own, never fused: the pragma turns contraction off for the whole file, and a
// compiler that does not know the pragma needs -ffp-contract=off.  The divisions and the square root are the correctly
// rounded ones (hipcc's default for f32, IEEE on a host).
//
//   g1 = g * gscale                     (gscale == 1: the same bits)
//   g2 = g1 * c                         only with a clip factor (has_clip)
// SGD:
//   g3 = g2 + wd * w                    only when wd != 0
//   m' = mu * m + g3;  d = nesterov ? g3 + mu * m' : m'      with a momentum value;  d = g3 without
//   w' = w - lr * d
// Adam:
//   g3 = (!decoupled && wd != 0) ? g2 + wd * w : g2
//   m' = b1 * m + omb1 * g3
//   v' = b2 * v + (omb2 * g3) * g3
//   mh = m' / bc1;  vh = v' / bc2;  den = sqrt(vh) + eps;  u = mh / den
//   w1 = (decoupled && wd != 0) ? w - lrwd * w : w
//   w' = w1 - lr * u
// omb1 = 1 - b1, omb2 = 1 - b2 and lrwd = lr * wd are float32 values computed once on the host (lh_adam_rule_make).
//
// Plain C++ with no includes.  LH_OPTIM_FN: the function qualifiers (a HIP translation unit sets __host__ __device__).
#ifndef LASER_HIP_OPTIM_CORE_H
#define LASER_HIP_OPTIM_CORE_H

#pragma clang fp contract(off)

#ifndef LH_OPTIM_FN
#define LH_OPTIM_FN static inline
#endif

struct lh_sgd_rule {
  float lr, mu, wd, gscale;
  int nesterov, has_m, has_clip;
};
struct lh_adam_rule {
  float lr, b1, b2, omb1, omb2, eps, wd, lrwd, bc1, bc2, gscale;
  int decoupled, has_clip;
};

LH_OPTIM_FN lh_sgd_rule lh_sgd_rule_make(float lr, float mu, float wd, int nesterov, float gscale, int has_m, int has_clip) {
  lh_sgd_rule r;
  r.lr = lr;
  r.mu = mu;
  r.wd = wd;
  r.gscale = gscale;
  r.nesterov = nesterov != 0;
  r.has_m = has_m != 0;
  r.has_clip = has_clip != 0;
  return r;
}
LH_OPTIM_FN lh_adam_rule lh_adam_rule_make(float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                                           float gscale, int has_clip) {
  lh_adam_rule r;
  r.lr = lr;
  r.b1 = b1;
  r.b2 = b2;
  r.omb1 = 1.0f - b1;
  r.omb2 = 1.0f - b2;
  r.eps = eps;
  r.wd = wd;
  r.lrwd = lr * wd;
  r.bc1 = bc1;
  r.bc2 = bc2;
  r.gscale = gscale;
  r.decoupled = decoupled != 0;
  r.has_clip = has_clip != 0;
  return r;
}

// g2 of the rules: the gradient scaled by gscale and, with a clip factor, by c
LH_OPTIM_FN float lh_optim_grad(const float g, const float gscale, const int has_clip, const float c) {
  float x = g * gscale;
  if (has_clip) x = x * c;
  return x;
}

// one element of an SGD step: w and m are updated in place (m is neither read nor written without a momentum value)
LH_OPTIM_FN void lh_sgd_elem(const lh_sgd_rule &r, const float c, float &w, const float g, float &m) {
  float g3 = lh_optim_grad(g, r.gscale, r.has_clip, c);
  if (r.wd != 0.0f) {
    const float t = r.wd * w;
    g3 = g3 + t;
  }
  float d = g3;
  if (r.has_m) {
    const float t = r.mu * m;
    m = t + g3;
    d = m;
    if (r.nesterov) {
      const float s = r.mu * m;
      d = g3 + s;
    }
  }
  const float step = r.lr * d;
  w = w - step;
}

// one element of an Adam step: w, m and v are updated in place
LH_OPTIM_FN void lh_adam_elem(const lh_adam_rule &r, const float c, float &w, const float g, float &m, float &v) {
  float g3 = lh_optim_grad(g, r.gscale, r.has_clip, c);
  if (!r.decoupled && r.wd != 0.0f) {
    const float t = r.wd * w;
    g3 = g3 + t;
  }
  const float m0 = r.b1 * m;
  const float m1 = r.omb1 * g3;
  m = m0 + m1;
  const float v0 = r.b2 * v;
  const float v1 = r.omb2 * g3;
  const float v2 = v1 * g3;
  v = v0 + v2;
  const float mh = m / r.bc1;
  const float vh = v / r.bc2;
  const float den = __builtin_sqrtf(vh) + r.eps;
  const float u = mh / den;
  float w1 = w;
  if (r.decoupled && r.wd != 0.0f) {
    const float t = r.lrwd * w;
    w1 = w - t;
  }
  const float step = r.lr * u;
  w = w1 - step;
}

// norm and clip factor from the sum of the squares: norm = sqrt(total), clip = norm > max_norm ? max_norm / norm : 1
// (a NaN norm compares false: clip = 1, and the NaN is already in the gradients)
LH_OPTIM_FN void lh_optim_clip(const float total, const float max_norm, float &norm, float &clip) {
  norm = __builtin_sqrtf(total);
  clip = norm > max_norm ? max_norm / norm : 1.0f;
}

// 1 - beta^step for step >= 1, in double: beta^step by square-and-multiply from the low bit, then one subtraction, rounded
// to float32 once.  (With contraction on, 1.0 - r * b could become a fused multiply-add.)
LH_OPTIM_FN float lh_adam_bias_correction(const float beta, long long step) {
  double r = 1.0, b = (double)beta;
  while (step) {
    if (step & 1) r = r * b;
    b = b * b;
    step >>= 1;
  }
  const double one_minus = 1.0 - r;
  return (float)one_minus;
}

#endif  // LASER_HIP_OPTIM_CORE_H
